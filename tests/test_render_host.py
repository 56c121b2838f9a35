"""CPU (`-m "not gpu"`): the host side of the prediction rendering — the numpy restatement the GPU tests use equals what the unmodified
reference handed to its file writers (tests/golden/render.*) under the judging rule of tests/render_ref.py, the fixture holds the edge
cases it names, the colour tables and public signatures are the reference's, and the refusals."""
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import conftest
import render_ref as rr
from tests.golden import make_render_golden as mrg


def _fixture():
    return conftest.load_golden("render")


def _logits(case, arrs):
    return arrs[case.get("logits_of", case["name"]) + "_logits"].astype(np.float32)


def test_reference_regenerates_the_fixture(tmp_path):
    """the stand-ins + the unmodified reference functions reproduce tests/golden/render.* byte for byte (build container only; a child
    process, so that the stand-in modules never enter this interpreter)"""
    if not os.path.isfile(os.path.join(mrg.ref_import.REFERENCE_ROOT, "TaskPrompter", "utils", "visualization_utils.py")):
        pytest.skip("reference tree not present")
    r = subprocess.run([sys.executable, mrg.__file__, str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    for name in ("render.json", "render.npz"):
        assert open(tmp_path / name, "rb").read() == open(os.path.join(conftest.GOLDEN, name), "rb").read(), name


def test_fixture_covers_what_it_names():
    meta, arrs = _fixture()
    assert [c["name"] for c in meta["vis"]] == [c["name"] for c in mrg.vis_cases()]
    assert [c["name"] for c in meta["save"]] == [c["name"] for c in mrg.save_cases()]
    by = {c["name"]: c for c in meta["vis"] + meta["save"]}
    assert by["semseg_cityscapes"]["size"][1] % 2 == 1 and by["semseg_pascal"]["shape"][0] == 3 and by["human_parts"]["size"] < by["human_parts"]["shape"][2:]
    # exact ties at the maximum, with an earlier and with a later channel, at identity size
    x = _logits(by["semseg_nyud"], arrs)
    assert by["semseg_nyud"]["size"] == by["semseg_nyud"]["shape"][2:]
    idx, run, gap = rr.top2(x.astype(np.float64))
    assert (gap == 0).sum() >= 3 and (run[gap == 0] > idx[gap == 0]).all() and (idx[gap == 0] == 0).any() and (run[gap == 0] == 39).any()
    # all-zero normals, also after the interpolation
    n = rr.interpolate(_logits(by["normals"], arrs), by["normals"]["size"])
    zero = (n == 0).all(axis=1)
    assert zero.sum() > 20 and (arrs["normals_written"][zero] == 127).all()
    # depth: negatives in the varying image, the other one constant
    d = _logits(by["depth"], arrs)
    assert 0.02 < (d[0] < 0).mean() < 0.1 and (d[0] > 0).mean() > 0.9 and np.unique(d[1]).size == 1 and by["depth"]["constant_images"] == [1]
    assert (rr.values(d, "depth", by["depth"]["size"])[0] == 0).sum() > 0, "clamped pixels survive the interpolation"
    # the save path: a cropped and an uncropped image in one batch, an all-ignore label, the label-id table
    pad = by["save_padded_edge"]
    assert pad["img_sizes"] == [[33, 47], [40, 56]] and pad["shape_hw"] == [40, 56]
    assert arrs["save_padded_edge_TP_0"].shape == (33, 47) and arrs["save_padded_edge_TP_1"].shape == (40, 56)
    assert by["save_ignore_edge"]["ignored"] == [1] and "save_ignore_edge_TP_0" in arrs.files and "save_ignore_edge_TP_1" not in arrs.files
    ids = arrs["save_label_ids_TP_0"]
    assert set(np.unique(ids).tolist()) <= set(rr.label_ids()[:19].tolist()) and (ids != arrs["save_padded_semseg_TP_0"]).any()
    # the margins are the measured ones, and nothing comes near the cap
    for task, d in meta["delta"].items():
        assert d == 4.0 * meta["measured"][task] and 0 < d < 0.01
    assert all(0 <= c["left_out"] <= rr.CAP for c in by.values())
    for name in ("render.json", "render.npz"):
        assert os.path.getsize(os.path.join(conftest.GOLDEN, name)) < (1 << 20)


@pytest.mark.parametrize("case", [c["name"] for c in mrg.vis_cases()])
def test_restatement_equals_the_reference_visualisation(case):
    meta, arrs = _fixture()
    c = next(c for c in meta["vis"] if c["name"] == case)
    x, got = _logits(c, arrs), arrs[case + "_written"]
    assert got.dtype == np.uint8 and list(got.shape[:3]) == [x.shape[0]] + c["size"]
    if c["task"] == "depth":                                # the stand-in's stacked index; the constant image is the reference's 0 / 0
        keep = [b for b in range(x.shape[0]) if b not in c["constant_images"]]
        left, mism, loose = rr.judge_vis(c, x[keep], got[keep][..., 0], meta["delta"])
        idx, exact = rr.depth_index(rr.values(x, "depth", c["size"]))
        assert (idx[c["constant_images"]] == 0).all() and exact[c["constant_images"]].all()
    else:
        left, mism, loose = rr.judge_vis(c, x, got[..., ::-1] if got.ndim == 4 else got, meta["delta"])      # cv2.imwrite got B, G, R
    assert (mism, loose) == (0, 0) and left == c["left_out"] and left <= rr.CAP
    if list(x.shape[2:]) == c["size"]:
        assert left == 0.0


@pytest.mark.parametrize("which", ["TP", "IP"])
@pytest.mark.parametrize("case", [c["name"] for c in mrg.save_cases()])
def test_restatement_equals_the_reference_save_path(case, which):
    meta, arrs = _fixture()
    c = next(c for c in meta["save"] if c["name"] == case)
    if which == "IP" and not c["train_class"]:
        assert not any(k.startswith(case + "_IP_") for k in arrs.files), "InvPT has no label-id table"
        return
    x = _logits(c, arrs)
    for i, size in enumerate(c["img_sizes"]):
        label = np.full((1,) + tuple(x.shape[2:]), 255.0 if i in c["ignored"] else 0.0)
        key = f"{case}_{which}_{i}"
        if rr.skipped(label, 255):
            assert key not in arrs.files
            continue
        got = arrs[key]
        assert list(got.shape) == size and list(rr.crop(x[i, 0], size).shape) == size
        left, mism, loose = rr.judge_save(c, x, got, meta["delta"], i)
        assert (mism, loose) == (0, 0) and left <= c["left_out"] <= rr.CAP


def test_colour_tables_equal_the_reference():
    import mtt_amd
    _, arrs = _fixture()
    r = mtt_amd.render
    for name, ours, restated in (("labelcolormap_40", r.semseg_colormap("NYUD"), rr.semseg_colormap("NYUD")),
                                 ("labelcolormap_21", r.semseg_colormap("PASCALContext"), rr.semseg_colormap("PASCALContext")),
                                 ("labelcolormap_7", r.labelcolormap(7), rr.labelcolormap(7)),
                                 ("cityscapes", r.semseg_colormap("Cityscapes3D"), rr.cityscapes_colormap()),
                                 ("label_ids", r.cityscapes_label_ids(), rr.label_ids())):
        want = arrs["table_" + name]
        assert ours.dtype == np.uint8 and ours.shape == want.shape and (ours == want).all() and (restated == want).all(), name
    assert r.JET.shape == (256, 3) and r.JET.dtype == np.uint8 and tuple(r.JET[0]) == (0, 0, 127) and tuple(r.JET[255]) == (127, 0, 0)
    pr = mtt_amd.PredictionRenderer("NYUD", depth_lut=r.JET[::-1].copy(), bgr=True)
    assert (pr.tables["depth"] == r.JET[::-1]).all() and pr.bgr
    with pytest.raises(ValueError, match="depth_lut"):
        mtt_amd.PredictionRenderer("NYUD", depth_lut=np.zeros((255, 3), np.uint8))
    try:
        from matplotlib import colormaps
    except ImportError:
        return
    assert (r.JET == colormaps["jet"](np.arange(256), bytes=True)[:, :3]).all()


def test_public_signatures_equal_the_reference():
    import mtt_amd
    meta, _ = _fixture()
    r = mtt_amd.render
    assert str(inspect.signature(r.vis_pred_for_one_task)) == meta["signatures"]["vis_pred_for_one_task"]
    assert str(inspect.signature(r.save_model_pred_for_one_task)) == meta["signatures"]["save_model_pred_for_one_task"]
    assert str(inspect.signature(r.save_model_pred_for_one_task_invpt)) == meta["signatures"]["save_model_pred_for_one_task_invpt"]
    assert mtt_amd.vis_pred_for_one_task is r.vis_pred_for_one_task and mtt_amd.save_model_pred_for_one_task is r.save_model_pred_for_one_task
    assert mtt_amd.PredictionRenderer is r.PredictionRenderer
    p = mtt_amd.factory.make_p(["semseg"], (48, 64), train_db_name="PASCALContext")
    assert mtt_amd.PredictionRenderer.from_config(p).db_name == "PASCALContext"
    assert str(inspect.signature(mtt_amd.PredictionRenderer.__init__)) == "(self, db_name, depth_lut=None, bgr=False)"


def test_crop_and_layout_equal_the_restatement():
    import mtt_amd
    r = mtt_amd.PredictionRenderer("NYUD")
    for pred, img in (((40, 56), (33, 47)), ((40, 56), (40, 56)), ((40, 56), (39, 56)), ((41, 57), (40, 50)), ((5, 7), (1, 1))):
        assert mtt_amd.render.crop_window(pred, img) == rr.crop_window(pred, img)
    with pytest.raises(ValueError, match="does not fit"):
        mtt_amd.render.crop_window((40, 56), (41, 56))
    rows, total = r.raw_layout((40, 56), [(33, 47), (40, 56), (1, 1)])
    assert rows == [(3, 4, 33, 47, 0), (0, 0, 40, 56, 1552), (19, 27, 1, 1, 1552 + 2240)] and total == 1552 + 2240 + 4
    assert all(row[4] % 4 == 0 for row in rows), "every image starts on a 4-pixel boundary: the vector path stays open"


def test_cpu_tensors_and_other_dtypes_raise():
    import mtt_amd
    r = mtt_amd.PredictionRenderer("Cityscapes3D")
    x = torch.zeros(1, 19, 8, 8)
    with pytest.raises(RuntimeError, match="device memory"):
        r.render(x, "semseg", (8, 8))
    with pytest.raises(RuntimeError, match="device memory"):
        r.raw(x, "semseg", [(8, 8)])
    with pytest.raises(RuntimeError):
        mtt_amd._lib.render_call("render_map", src=x)
    p = {"train_db_name": "Cityscapes3D", "ignore_index": 255}
    sample = {"image": torch.zeros(1, 3, 8, 8), "semseg": torch.zeros(1, 1, 8, 8), "meta": {"img_size": [(8, 8)], "img_name": ["a"]}}
    with pytest.raises(RuntimeError, match="device memory"):
        mtt_amd.vis_pred_for_one_task(p, sample, {"semseg": x}, "/nonexistent", "semseg")
    with pytest.raises(RuntimeError, match="device memory"):
        mtt_amd.save_model_pred_for_one_task(p, 0, sample, {"semseg": x}, {"semseg": "/nonexistent"}, "semseg")

    class OnDevice(torch.Tensor):                           # the dtype test comes after the device test: a stand-in that claims the device
        is_cuda = True

    bf16 = torch.zeros(1, 19, 8, 8, dtype=torch.bfloat16).as_subclass(OnDevice)
    with pytest.raises(RuntimeError, match="fp32"):
        r.render(bf16, "semseg", (8, 8))
    with pytest.raises(RuntimeError, match="fp32"):
        r.raw(bf16, "semseg", [(8, 8)])
    with pytest.raises(ValueError, match="select one of"):
        r.render(x, "albedo", (8, 8))


def test_3ddet_and_normals_are_named_in_their_refusals():
    import mtt_amd
    r = mtt_amd.PredictionRenderer("Cityscapes3D")
    p = {"train_db_name": "Cityscapes3D", "ignore_index": 255}
    with pytest.raises(NotImplementedError, match="3ddet"):
        r.render(torch.zeros(1), "3ddet", (8, 8))
    with pytest.raises(NotImplementedError, match="3ddet"):
        mtt_amd.vis_pred_for_one_task(p, {}, {}, "/nonexistent", "3ddet")
    with pytest.raises(NotImplementedError, match="3ddet"):
        mtt_amd.save_model_pred_for_one_task(p, 0, {}, {}, {}, "3ddet")
    with pytest.raises(NotImplementedError, match="3ddet"):
        mtt_amd.save_model_pred_for_one_task(p, {}, {}, {}, "3ddet")           # InvPT's call order
    with pytest.raises(RuntimeError, match="normals"):
        mtt_amd.save_model_pred_for_one_task(p, 0, {}, {}, {}, "normals")
    with pytest.raises(RuntimeError, match="normals"):
        mtt_amd.render.save_model_pred_for_one_task_invpt(p, {}, {}, {}, "normals")


def test_render_table_is_its_own_and_exported():
    import mtt_amd
    lib = mtt_amd._lib
    assert set(lib.RENDER) == {"render_map", "render_minmax"} and all(st is lib.RenderDesc for st in lib.RENDER.values())
    others = set(lib.DESCS) | set(lib.POSITIONAL) | set(lib.DESC_EXTRA) | set(lib.POSTPROC) | set(lib.EVAL) | set(lib.AUGMENT) | set(lib.CS3D)
    assert not set(lib.RENDER) & others
    assert lib.ABI_VERSION == 17 and lib.load().mtt_abi_version() == 17
    for name in ["mtt_render_desc_size"] + ["mtt_" + n for n in lib.RENDER]:
        assert name in lib.EXPORTS and hasattr(lib.load(), name)
    assert lib.load().mtt_render_desc_size() == __import__("ctypes").sizeof(lib.RenderDesc)
    header = open(os.path.join(conftest.ROOT, "include", "mtt_hip.h")).read()
    modes = "enum { " + ", ".join(f"MTT_RENDER_{n} = {getattr(lib, 'RENDER_' + n)}" for n in ("CLASS", "SIGMOID255", "SOFTMAX1_255", "NORMALS", "DEPTH")) + " };"
    kinds = "enum { " + ", ".join(f"MTT_RENDER_OUT_{n} = {getattr(lib, 'RENDER_OUT_' + n)}" for n in ("U8", "LUT1", "LUT3", "RGB3", "F32")) + " };"
    assert modes in header and kinds in header and "} mtt_render_desc;" in header
    assert "render.hip" in __import__("importlib").import_module("multi-task-transformer_amd._build").SOURCES


def test_host_check_refuses_a_bad_descriptor_without_a_device():
    """the C entry points validate the descriptor and the HOST copy of the window table before anything touches the device: a refused
    descriptor returns a negative status even here, where no launch could succeed"""
    import mtt_amd
    lib = mtt_amd._lib
    win = torch.tensor([[3, 4, 33, 47, 0], [0, 0, 40, 56, 1552]], dtype=torch.int64)
    fake = win.data_ptr() & ~15                              # never dereferenced: every call below is refused by the host check

    def rmap(**kw):
        f = dict(src=fake, out=fake, B=2, C=19, h=40, w=56, H=40, W=56, mode=lib.RENDER_CLASS, out_kind=lib.RENDER_OUT_U8, out_pixels=1552 + 2240,
                 win=fake, win_host=win, stream=0)
        f.update(kw)
        return lib.render_call("render_map", **f)

    assert rmap(src=None) == lib.E_BADARG and rmap(out=None) == lib.E_BADARG and rmap(B=0) == lib.E_BADARG and rmap(C=0) == lib.E_BADARG
    assert rmap(h=0) == lib.E_BADARG and rmap(W=1 << 20) == lib.E_BADARG and rmap(mode=7) == lib.E_BADARG and rmap(out_kind=9) == lib.E_BADARG
    assert rmap(out_pixels=1552 + 2239) == lib.E_BADARG, "the last window ends one pixel past the output"
    assert rmap(H=39) == lib.E_BADARG and rmap(W=50) == lib.E_BADARG, "a window outside the grid"
    assert rmap(win_host=None) == lib.E_BADARG and rmap(win=None) == lib.E_BADARG, "the device table and its host copy come together"
    for col, val in ((0, -1), (1, -1), (2, 0), (3, 0), (4, -4), (2, 41), (3, 57)):
        bad = win.clone()
        bad[1, col] = val
        assert rmap(win_host=bad) == lib.E_BADARG, (col, val)
    assert rmap(win=None, win_host=None, out_pixels=2 * 40 * 56 - 1) == lib.E_BADARG
    assert rmap(src=fake + 2) == lib.E_ALIGN
    assert rmap(C=257) == lib.E_UNSUPPORTED and rmap(out_kind=lib.RENDER_OUT_LUT3) == lib.E_BADARG, "a table output without a table"
    assert rmap(out_kind=lib.RENDER_OUT_RGB3) == lib.E_BADARG and rmap(out_kind=lib.RENDER_OUT_F32) == lib.E_BADARG
    assert rmap(mode=lib.RENDER_SIGMOID255) == lib.E_BADARG and rmap(mode=lib.RENDER_SIGMOID255, C=1, out_kind=lib.RENDER_OUT_LUT1, table=fake) == lib.E_BADARG
    assert rmap(mode=lib.RENDER_SOFTMAX1_255, C=1) == lib.E_BADARG and rmap(mode=lib.RENDER_SOFTMAX1_255, C=3) == lib.E_UNSUPPORTED
    assert rmap(mode=lib.RENDER_NORMALS, C=3) == lib.E_BADARG and rmap(mode=lib.RENDER_NORMALS, C=2, out_kind=lib.RENDER_OUT_RGB3) == lib.E_BADARG
    assert rmap(mode=lib.RENDER_DEPTH, C=1) == lib.E_BADARG, "the depth index needs the minimum and maximum"
    assert rmap(mode=lib.RENDER_DEPTH, C=2, out_kind=lib.RENDER_OUT_F32) == lib.E_BADARG
    assert rmap(mode=lib.RENDER_DEPTH, C=1, out_kind=lib.RENDER_OUT_F32, out=fake + 2) == lib.E_ALIGN
    assert rmap(mode=lib.RENDER_DEPTH, C=1, minmax=fake + 1) == lib.E_ALIGN

    def minmax(**kw):
        f = dict(src=fake, minmax=fake, B=2, C=1, h=24, w=48, H=37, W=101, stream=0)
        f.update(kw)
        return lib.render_call("render_minmax", **f)

    assert minmax(minmax=None) == lib.E_BADARG and minmax(C=2) == lib.E_BADARG and minmax(H=0) == lib.E_BADARG and minmax(B=1 << 16) == lib.E_BADARG
    assert minmax(win=fake, win_host=win) == lib.E_BADARG, "windows of another grid"
