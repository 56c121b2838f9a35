"""GPU: the prediction rendering kernels (csrc/render.hip through mtt_amd.PredictionRenderer) against what the unmodified reference handed
to its file writers (tests/golden/render.*) and against the fp64 restatement tests/render_ref.py that the host suite pins to that fixture.

Bytes are judged by the rule of tests/render_ref.py: a pixel whose fp64 value lies within delta of an integer (whose two largest logits
lie within delta of each other) is left out and may differ by one level (to the runner-up class); everywhere else the bytes are equal.
The deltas are the ones tests/golden/render.json records, four times the reference's own fp32 error on inputs of the same distribution
(N(0, 3) on the fp16 grid), which every synthetic case below draws from as well.  Every output is written into the middle of a poisoned
buffer whose guard bands, and the gaps between packed images, must come back untouched."""
import functools
import inspect
import os
import sys
import warnings

import numpy as np
import pytest
import torch

import conftest
import render_ref as rr
from tests.golden import make_render_golden as mrg

GUARD, POISON = 64, 0xA5
CLASS_TASKS = ("semseg", "human_parts")
CHANNELS = {"sal": 2, "edge": 1, "normals": 3, "depth": 1}
GREY = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)       # a depth table that shows the index itself

# RENDER entry point -> the tests of this file that launch it (test_every_render_entry_point_is_covered)
COVERED = {
    "render_map": ["test_fixture_visualisation", "test_fixture_save_path", "test_small_shapes", "test_misaligned_views", "test_three_windows_in_one_batch",
                   "test_full_size_frames", "test_files_end_to_end", "test_no_synchronisation_and_graph_replay"],
    "render_minmax": ["test_fixture_visualisation", "test_minmax_is_exact_and_repeatable", "test_small_shapes", "test_files_end_to_end",
                      "test_no_synchronisation_and_graph_replay"],
}


def _need_gpu():
    if not conftest.has_gpu():
        pytest.fail("marked gpu but no HIP device is visible")


@functools.lru_cache(maxsize=None)
def _fixture():
    return conftest.load_golden("render")


def _logits_of(case):
    return _fixture()[1][case.get("logits_of", case["name"]) + "_logits"].astype(np.float32)


def _dev(a, skew=0):
    """a device copy; skew: the view starts that many elements past a 16-byte boundary"""
    a = np.ascontiguousarray(a)
    base = torch.empty(a.size + skew, dtype=torch.from_numpy(a).dtype, device="cuda:0")
    view = base[skew:].view(a.shape)
    view.copy_(torch.from_numpy(a))
    return view


@functools.lru_cache(maxsize=None)
def _renderer(db, grey=False):
    import mtt_amd
    return mtt_amd.PredictionRenderer(db, depth_lut=GREY if grey else None)


@functools.lru_cache(maxsize=None)
def _random_logits(task, C, h, w, B=2, seed=0):
    """the fixture's distribution (shared by the tests, never modified)"""
    case = dict(task=task, shape=[B, C, h, w])
    return mrg.make_logits(case, 900 + seed + 13 * h + w + 101 * C).astype(np.float32)


def _guarded(numel, dtype, skew):
    """a poisoned byte buffer and the contiguous view of `numel` elements that starts GUARD + skew bytes into it"""
    item = torch.empty(0, dtype=dtype).element_size()
    buf = torch.full((2 * GUARD + skew + numel * item + 16,), POISON, dtype=torch.uint8, device="cuda:0")
    return buf, buf[GUARD + skew:GUARD + skew + numel * item].view(dtype)


def _untouched(buf, skew, nbytes, written=None):
    host = buf.cpu().numpy()
    assert (host[:GUARD + skew] == POISON).all() and (host[GUARD + skew + nbytes:] == POISON).all(), "a guard band was written"
    if written is not None:
        body = host[GUARD + skew:GUARD + skew + nbytes]
        assert (body[~written] == POISON).all(), "a gap between packed images was written"


def _render(r, x, task, size, skew=0):
    B = x.shape[0]
    numel = B * size[0] * size[1] * (1 if task in ("sal", "edge") else 3)
    buf, view = _guarded(numel, torch.uint8, skew)
    out = r.render(x, task, size, out=view)
    assert out.data_ptr() == view.data_ptr() and out.dtype == torch.uint8
    assert tuple(out.shape) == ((B,) + tuple(size) if task in ("sal", "edge") else (B,) + tuple(size) + (3,))
    got = out.cpu().numpy()
    _untouched(buf, skew, numel)
    return got


def _raw(r, x, task, sizes, train_class=True, skew=0):
    rows, total = r.raw_layout(tuple(x.shape[2:]), sizes)
    dtype = torch.float32 if task == "depth" else torch.uint8
    item = 4 if task == "depth" else 1
    buf, view = _guarded(total, dtype, skew)
    maps = r.raw(x, task, sizes, semseg_save_train_class=train_class, out=view)
    got = [m.cpu().numpy() for m in maps]
    written = np.zeros(total * item, dtype=bool)
    for (_, _, hh, ww, off), m, s in zip(rows, got, sizes):
        assert m.shape == tuple(s) and m.dtype == (np.float32 if task == "depth" else np.uint8)
        written[off * item:(off + hh * ww) * item] = True
    _untouched(buf, skew, total * item, written)
    return got


def _judge_render(task, x, got, size, db="NYUD", what="", cap=True):
    """a rendered batch (depth: through GREY, so that channel 0 is the index) against the restatement.  cap=False: the caller pools the
    left-out share over its shapes (a share of a 30-pixel map moves in steps of 3 %) and receives the left-out count."""
    meta = _fixture()[0]
    case = dict(task=task, size=list(size), db=db)
    if task == "depth":
        assert (got[..., 0] == got[..., 1]).all() and (got[..., 0] == got[..., 2]).all()
        got = got[..., 0]
    left, mism, loose = rr.judge_vis(case, x, got, meta["delta"])
    print(f"{what or task} {tuple(x.shape)} -> {tuple(size)}: left out {left:.4f}, mismatches {mism}, loose {loose}")
    assert (mism, loose) == (0, 0) and (left <= rr.CAP or not cap), (what or task, x.shape, size, left, mism, loose)
    return left * x.shape[0] * size[0] * size[1]


# ---- 1. the fixture -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", [c["name"] for c in mrg.vis_cases()])
def test_fixture_visualisation(name):
    """every visualisation case through `render`: against the restatement under the rule, and equal to the reference's own bytes wherever
    the rule leaves nothing out.  Depth goes through a grey table (the stand-in recorded the index; OpenCV's colours are not pinned) and,
    once more, through the default table; its constant image holds index 0, where the reference divides 0 by 0."""
    _need_gpu()
    meta, arrs = _fixture()
    c = next(c for c in meta["vis"] if c["name"] == name)
    x, task, size = _logits_of(c), c["task"], c["size"]
    r = _renderer(c["db"], grey=task == "depth")
    got = _render(r, _dev(x), task, size)
    again = _render(r, _dev(x), task, size)
    assert (got == again).all(), "two calls, two results"
    _judge_render(task, x, got, size, db=c["db"], what=name)
    want = arrs[name + "_written"]
    want = want[..., ::-1] if want.ndim == 4 and task != "depth" else want        # cv2.imwrite was handed B, G, R
    differs = (got != want).reshape(got.shape[:3] + (-1,)).any(axis=-1)
    keep = ~rr.near_vis(c, x, meta["delta"])
    for b in c.get("constant_images", []):
        keep[b] = False
        assert (got[b] == 0).all()
    assert not (differs & keep).any(), (name, int((differs & keep).sum()))
    if task == "depth":
        jet = _render(_renderer(c["db"]), _dev(x), task, size)
        import mtt_amd
        assert (jet == mtt_amd.render.JET[got[..., 0]]).all(), "the default table, looked up with the same index"
        bgr = mtt_amd.PredictionRenderer(c["db"], bgr=True).render(_dev(x), task, size).cpu().numpy()
        assert (bgr == jet[..., ::-1]).all()
    if task in ("semseg", "normals"):
        import mtt_amd
        bgr = mtt_amd.PredictionRenderer(c["db"], bgr=True).render(_dev(x), task, size).cpu().numpy()
        assert (bgr == got[..., ::-1]).all(), "bgr=True is the reference's in-memory order"


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c["name"] for c in mrg.save_cases()])
def test_fixture_save_path(name):
    """every save-path case through `raw`: the centre crop of a padded prediction next to an uncropped one, the label-id table"""
    _need_gpu()
    meta, arrs = _fixture()
    c = next(c for c in meta["save"] if c["name"] == name)
    x, task = _logits_of(c), c["task"]
    got = _raw(_renderer(c["db"]), _dev(x), task, [tuple(s) for s in c["img_sizes"]], train_class=c["train_class"])
    for i in range(x.shape[0]):
        left, mism, loose = rr.judge_save(c, x, got[i], meta["delta"], i)
        assert (mism, loose) == (0, 0) and left <= rr.CAP, (name, i, left, mism, loose)
        for which in ("TP", "IP"):
            key = f"{name}_{which}_{i}"
            if key in arrs.files:
                differs = got[i] != arrs[key]
                if task in CLASS_TASKS:
                    assert not differs.any(), (key, int(differs.sum()))      # identity size: ==, nothing left out
                else:
                    y0, x0, hh, ww = rr.crop_window(x.shape[2:], c["img_sizes"][i])
                    vals = rr.values(x[i:i + 1], task, x.shape[2:])[0, y0:y0 + hh, x0:x0 + ww]
                    assert not (differs & ~rr.near_bytes(vals, meta["delta"][task])).any(), key


# ---- 2. the shapes at which the kernels can go wrong ----------------------------------------------------------------------------------------
SHAPES = [  # (h, w) -> (H, W)
    ((6, 1), (6, 1)), ((6, 3), (6, 3)), ((6, 5), (6, 5)), ((5, 67), (5, 67)), ((5, 68), (5, 68)), ((9, 260), (9, 260)),      # identity: scalar, vector, the seam
    ((7, 9), (11, 1)), ((7, 9), (11, 3)), ((7, 9), (11, 5)), ((7, 9), (11, 67)), ((7, 9), (11, 68)),                          # the same widths with taps
    ((1, 9), (6, 20)), ((7, 1), (10, 8)), ((1, 1), (5, 4)),                                                                  # a source of one row, of one column
    ((24, 48), (37, 101)), ((24, 48), (38, 264)), ((23, 37), (13, 17)), ((23, 37), (9, 20)), ((16, 24), (16, 40)), ((16, 24), (25, 24)),
]


@pytest.mark.gpu
@pytest.mark.parametrize("task", ["semseg", "sal", "edge", "normals", "depth"])
def test_small_shapes(task):
    """widths 1, 3, 5, 67 and 68 (one pixel per thread, four, and the seam between them), more than one workgroup along x and y, sources
    of one row and one column, up- and downscale by non-integer factors and along one axis only, identity"""
    _need_gpu()
    r = _renderer("NYUD", grey=task == "depth")
    C = 40 if task == "semseg" else CHANNELS[task]
    left = total = 0
    for (h, w), size in SHAPES:
        x = _random_logits(task, C, h, w)
        left += _judge_render(task, x, _render(r, _dev(x), task, size), size, cap=False)
        total += x.shape[0] * size[0] * size[1]
    assert left <= rr.CAP * total, (task, left, total)


@pytest.mark.gpu
@pytest.mark.parametrize("C", [1, 2, 3, 7, 19, 21, 40])
def test_class_counts(C):
    """the channel loop: one channel (no loop), fewer than its unrolling, a remainder, many; colours and the plain index"""
    _need_gpu()
    r = _renderer("NYUD")
    left = total = 0
    for (h, w), size in (((8, 12), (8, 12)), ((8, 12), (11, 20)), ((8, 13), (8, 13)), ((8, 13), (5, 9))):
        x = _random_logits("semseg", C, h, w)
        left += _judge_render("semseg", x, _render(r, _dev(x), "semseg", size), size, what=f"semseg C={C}", cap=False)
        total += x.shape[0] * size[0] * size[1]
        if tuple(size) == (h, w):                           # the index itself, through the save path
            got = _raw(r, _dev(x), "semseg", [size] * x.shape[0])
            case = dict(task="semseg", img_sizes=[list(size)] * x.shape[0])
            assert all(rr.judge_save(case, x, got[i], {}, i)[1] == 0 for i in range(x.shape[0]))
    assert left <= rr.CAP * total, (C, left, total)


@pytest.mark.gpu
def test_misaligned_views():
    """logits that start one element past a 16-byte boundary and outputs at an odd byte offset (fp32: 4 bytes past one) take the
    one-pixel path although the sizes would allow four; the bytes equal those of the aligned call"""
    _need_gpu()
    for task, C in (("semseg", 19), ("edge", 1), ("normals", 3), ("depth", 1)):
        r = _renderer("Cityscapes3D", grey=task == "depth")
        for (h, w), size in (((8, 16), (8, 16)), ((8, 16), (12, 24))):
            x = _random_logits(task, C, h, w)
            want = _render(r, _dev(x), task, size)
            for skew_in, skew_out in ((1, 0), (0, 1), (1, 3), (2, 2)):
                xs = _dev(x, skew=skew_in)
                assert xs.data_ptr() % 16 == 4 * skew_in
                assert (_render(r, xs, task, size, skew=skew_out) == want).all(), (task, size, skew_in, skew_out)
        if task != "normals":
            x = _random_logits(task, C, 8, 16)
            want = _raw(r, _dev(x), task, [(8, 16), (8, 16)])
            for skew_in, skew_out in ((1, 0), (0, 4 if task == "depth" else 1), (3, 12 if task == "depth" else 7)):
                got = _raw(r, _dev(x, skew=skew_in), task, [(8, 16), (8, 16)], skew=skew_out)
                assert all((a == b).all() for a, b in zip(got, want)), (task, skew_in, skew_out)


@pytest.mark.gpu
def test_three_windows_in_one_batch():
    """B = 3 with three different crop windows: odd ones (one pixel per thread) and ones whose origin, width and offset are multiples of 4"""
    _need_gpu()
    r = _renderer("Cityscapes3D")
    meta = _fixture()[0]
    for sizes in ([(17, 33), (24, 40), (20, 36)], [(24, 40), (16, 32), (8, 24)], [(1, 1), (24, 4), (3, 40)]):
        for task, C in (("semseg", 19), ("sal", 2), ("depth", 1)):
            x = _random_logits(task, C, 24, 40, B=3)
            got = _raw(r, _dev(x), task, sizes)
            case = dict(task=task, img_sizes=[list(s) for s in sizes])
            out = pixels = 0                                # the cap on the batch: one of the windows is a single pixel
            for i in range(3):
                left, mism, loose = rr.judge_save(case, x, got[i], meta["delta"], i)
                assert (mism, loose) == (0, 0), (task, sizes, i, left, mism, loose)
                out += left * got[i].size
                pixels += got[i].size
            assert out <= rr.CAP * pixels, (task, sizes, out, pixels)
    with pytest.raises(ValueError, match="does not fit"):
        r.raw(_dev(_random_logits("sal", 2, 24, 40, B=3)), "sal", [(24, 40), (25, 40), (8, 24)])


@pytest.mark.gpu
def test_minmax_is_exact_and_repeatable():
    """mtt_render_minmax: at identity size the bit patterns of torch's own minimum and maximum of the clamped map; with taps within the
    rounding of the three fp32 blends (values below 16: 6 x 2^-24 x 16 < 1e-5) of the fp64 restatement; twice the same bits; an all-negative
    image gives (0, 0)"""
    _need_gpu()
    import mtt_amd
    lib = mtt_amd._lib
    for (h, w), size in (((24, 48), (24, 48)), ((24, 47), (24, 47)), ((24, 48), (37, 101)), ((24, 48), (40, 264)), ((23, 37), (9, 20))):
        x = _random_logits("depth", 1, h, w, B=3).copy()
        x[2] = -np.abs(x[2]) - 1.0
        xd = _dev(x)
        runs = []
        for _ in range(2):
            buf, mm = _guarded(6, torch.int32, 0)
            assert lib.render_call("render_minmax", src=xd, minmax=mm, B=3, C=1, h=h, w=w, H=size[0], W=size[1]) == 0
            runs.append(mm.cpu().numpy().view(np.float32).reshape(2, 3))
            _untouched(buf, 0, 24)
        assert (runs[0].view(np.uint32) == runs[1].view(np.uint32)).all()
        v = rr.values(x, "depth", size)
        lo, hi = v.reshape(3, -1).min(axis=1), v.reshape(3, -1).max(axis=1)
        if tuple(size) == (h, w):
            assert (runs[0][0] == lo.astype(np.float32)).all() and (runs[0][1] == hi.astype(np.float32)).all()
        else:
            assert np.abs(runs[0][0] - lo).max() < 1e-5 and np.abs(runs[0][1] - hi).max() < 1e-5
        assert runs[0][0][2] == 0 and runs[0][1][2] == 0 and (runs[0].view(np.uint32)[:, 2] == 0).all()


# ---- 3. full size ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape,size,db", [((1, 19, 1024, 2048), (1024, 2048), "Cityscapes3D"), ((1, 21, 512, 512), (375, 500), "PASCALContext")],
                         ids=["cityscapes_identity", "pascal_resized"])
def test_full_size_frames(shape, size, db):
    """one frame at the size a user runs, judged on a strided sample of rows and columns plus the seams of the tiling (4 rows per
    workgroup, 256 columns per wave)"""
    _need_gpu()
    g = torch.Generator(device="cuda:0").manual_seed(11)
    x = torch.randn(shape, generator=g, device="cuda:0") * 3
    H, W = size
    rows = np.unique(np.concatenate([np.arange(0, H, 61), [3, 4, 5, H // 2 - 1, H // 2, H - 2, H - 1]]))
    cols = np.unique(np.concatenate([np.arange(0, W, 67), [3, 4, 255, 256, 257, W - 257, W - 256, W - 5, W - 4, W - 1]]))
    got = _render(_renderer(db), x, "semseg", size)
    if tuple(shape[2:]) == tuple(size):
        xs = x[:, :, torch.from_numpy(rows).cuda()][:, :, :, torch.from_numpy(cols).cuda()].cpu().numpy()
        idx, run, gap = rr.top2(xs.astype(np.float64))
        delta = 0.0
    else:
        idx, run, gap = rr.values(x.cpu().numpy(), "semseg", size, rows=rows, cols=cols)
        delta = _fixture()[0]["delta"]["semseg"]
    table = rr.full_table(rr.semseg_colormap(db))
    left, mism, loose = rr.judge_class(got[:, rows][:, :, cols], idx, run, gap, delta, lut=table)
    print(f"full size {shape} -> {size}: {idx.size} sampled pixels, left out {left:.5f}, mismatches {mism}, loose {loose}")
    assert (mism, loose) == (0, 0) and left <= rr.CAP
    colours = got.reshape(-1, 3).astype(np.uint32)
    assert len(np.unique(colours[:, 0] << 16 | colours[:, 1] << 8 | colours[:, 2])) == shape[1], "every class shows"


# ---- 4. files -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_files_end_to_end(tmp_path):
    """vis_pred_for_one_task and save_model_pred_for_one_task write the reference's file names; the PNGs read back equal the rendered
    bytes, the .mat the fp32 map; the all-ignore image has no file; both call orders of the save function"""
    _need_gpu()
    import mtt_amd
    import scipy.io as sio
    from PIL import Image
    meta, _ = _fixture()
    by = {c["name"]: c for c in meta["vis"] + meta["save"]}
    # the visualisation path, every task
    for name in ("semseg_cityscapes", "human_parts", "sal", "edge", "normals", "depth"):
        c = by[name]
        x, task = _dev(_logits_of(c)), c["task"]
        B = x.shape[0]
        names = [f"frame{i}" for i in range(B)]
        p = mtt_amd.factory.AttrDict(train_db_name=c["db"], ignore_index=255)
        sample = {"image": torch.zeros(B, 3, 4, 4), "meta": {"img_size": [tuple(c["size"])] * B, "img_name": names}}
        out_dir = tmp_path / ("vis_" + name)
        out_dir.mkdir()
        mtt_amd.vis_pred_for_one_task(p, sample, {task: x}, str(out_dir), task)
        assert sorted(os.listdir(out_dir)) == sorted(f"{n}_{task}.png" for n in names)
        want = _renderer(c["db"]).render(x, task, c["size"]).cpu().numpy()
        for i, n in enumerate(names):
            assert (np.array(Image.open(out_dir / f"{n}_{task}.png")) == want[i]).all(), (name, i)
    # the save path
    for name, which in (("save_padded_semseg", "TP"), ("save_label_ids", "TP"), ("save_padded_sal", "IP"), ("save_ignore_edge", "TP"), ("save_ignore_edge", "IP"),
                        ("depth", "TP")):
        c = by[name]
        task = c["task"]
        xh = _logits_of(c) if name != "depth" else _random_logits("depth", 1, 40, 56)
        sizes = c.get("img_sizes", [[33, 47], [40, 56]])
        x, B = _dev(xh), xh.shape[0]
        names = [f"{name}{i}" for i in range(B)]
        label = torch.zeros(B, 1, *xh.shape[2:], device="cuda:0")
        for i in c.get("ignored", []):
            label[i] = 255
        if which == "IP":
            label = label.cpu()                             # a loader's batch: the label still on the host
        p = mtt_amd.factory.AttrDict(train_db_name=c["db"], ignore_index=255, semseg_save_train_class=c.get("train_class", True))
        sample = {"image": torch.zeros(B, 3, 4, 4), task: label, "meta": {"img_size": torch.tensor(sizes), "img_name": names}}
        out_dir = tmp_path / f"save_{name}_{which}"
        out_dir.mkdir()
        if which == "TP":
            mtt_amd.save_model_pred_for_one_task(p, 0, sample, {task: x}, {task: str(out_dir)}, task, epoch=0)
        else:
            mtt_amd.save_model_pred_for_one_task(p, sample, {task: x}, {task: str(out_dir)}, task, epoch=0)
        kept = [i for i in range(B) if i not in c.get("ignored", [])]
        ext = ".mat" if task == "depth" else ".png"
        assert sorted(os.listdir(out_dir)) == sorted(names[i] + ext for i in kept), (name, which)
        want = _renderer(c["db"]).raw(x, task, [tuple(s) for s in sizes], semseg_save_train_class=c.get("train_class", True))
        for i in kept:
            if task == "depth":
                got = sio.loadmat(out_dir / (names[i] + ".mat"))["depth"]
                assert got.dtype == np.float32
            else:
                got = np.array(Image.open(out_dir / (names[i] + ".png")))
            assert got.shape == tuple(sizes[i]) and (got == want[i].cpu().numpy()).all(), (name, which, i)


# ---- 5. no host synchronisation, graph capture ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_no_synchronisation_and_graph_replay():
    """render and raw of every task: no host synchronisation after the warm-up call; captured once in a linear single-stream graph and
    replayed onto cleared outputs, the bytes are those of the direct calls"""
    _need_gpu()
    import mtt_amd
    r = mtt_amd.PredictionRenderer("PASCALContext")
    tasks = dict(semseg=21, human_parts=7, sal=2, edge=1, normals=3, depth=1)
    x = {t: _dev(_random_logits(t, C, 23, 37)) for t, C in tasks.items()}
    size, sizes = (50, 75), [(20, 37), (23, 30)]
    outs = {t: torch.zeros(2 * 50 * 75 * (1 if t in ("sal", "edge") else 3), dtype=torch.uint8, device="cuda:0") for t in tasks}
    total = r.raw_layout((23, 37), sizes)[1]
    raws = {t: torch.zeros(total, dtype=torch.float32 if t == "depth" else torch.uint8, device="cuda:0") for t in tasks if t != "normals"}

    def run():
        for t in tasks:
            r.render(x[t], t, size, out=outs[t])
            if t != "normals":
                r.raw(x[t], t, sizes, out=raws[t])

    run()                                                   # warm-up: library load, tables, windows and workspaces
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            run()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert not [str(w.message) for w in rec if "synchroniz" in str(w.message)]
    torch.cuda.synchronize()
    want = {k: v.clone() for k, v in list(outs.items()) + [("raw_" + k, v) for k, v in raws.items()]}
    for v in list(outs.values()) + list(raws.values()):
        v.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    assert not any(bool(v.any()) for v in outs.values()), "capture records the launches, it does not run them"
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    for t in tasks:
        assert torch.equal(outs[t], want[t]) and bool(outs[t].any()), t
        if t != "normals":
            assert torch.equal(raws[t].view(torch.uint8), want["raw_" + t].view(torch.uint8)), t


@pytest.mark.gpu
def test_a_device_tensor_as_the_host_copy_raises():
    """win_host is the copy the entry point reads on the host: a device tensor there is refused by the binding, before anything is launched"""
    _need_gpu()
    import mtt_amd
    win = torch.zeros(4, dtype=torch.int64, device="cuda:0")
    with pytest.raises(RuntimeError, match="must be a CPU tensor"):
        mtt_amd._lib.render_call("render_map", win_host=win)


# ---- 6. coverage of the binding table -----------------------------------------------------------------------------------------------------
def test_every_render_entry_point_is_covered():
    """the assertion tests/test_parity_comparator.py makes for DESCS | POSITIONAL | DESC_EXTRA, for the table of its own the rendering entry
    points are registered in: every entry is launched by a named test of this file"""
    import mtt_amd
    lib = mtt_amd._lib
    assert set(lib.RENDER) == set(COVERED)
    assert not set(lib.RENDER) & (set(lib.DESCS) | set(lib.POSITIONAL) | set(lib.DESC_EXTRA))
    assert all("mtt_" + n in lib.EXPORTS for n in lib.RENDER)
    here = sys.modules[__name__]
    map_src = inspect.getsource(mtt_amd.PredictionRenderer._map)
    assert '"render_map"' in map_src and '"render_minmax"' in map_src
    assert "self._map(" in inspect.getsource(mtt_amd.PredictionRenderer.render) and "self._map(" in inspect.getsource(mtt_amd.PredictionRenderer.raw)
    # what reaches PredictionRenderer._map (render: both entry points, the second for depth; raw: render_map) or the entry point itself
    launched_by = {"_render(": ["render_map", "render_minmax"], ".render(": ["render_map", "render_minmax"], "_raw(": ["render_map"], ".raw(": ["render_map"],
                   "vis_pred_for_one_task(": ["render_map", "render_minmax"], "save_model_pred_for_one_task(": ["render_map"],
                   'render_call("render_minmax"': ["render_minmax"]}
    for entry, tests in COVERED.items():
        assert tests
        for t in tests:
            fn = getattr(here, t)
            assert any(m.name == "gpu" for m in getattr(fn, "pytestmark", [])), t
            src = inspect.getsource(fn)
            assert any(h in src and entry in es for h, es in launched_by.items()), (entry, t)
            if entry == "render_minmax" and 'render_call("render_minmax"' not in src:
                assert "depth" in src, (entry, t)
