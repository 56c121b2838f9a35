"""GPU: the Cityscapes-3D preparation kernels (csrc/cs3d.hip through mtt_amd.Cityscapes3DPrepare) against the reference's own outputs
(tests/golden/cs3d.*) and against the numpy restatement tests/cs3d_ref.py that the host suite pins to that fixture and to Pillow.

Every comparison is BITWISE: the resample is 32-bit integer arithmetic on host-built tables and the normalisation two correctly rounded
fp32 divisions and one subtraction, so there is no tolerance to choose."""
import functools
import warnings

import numpy as np
import pytest
import torch

import conftest
import cs3d_ref
from tests.golden import make_cs3d_golden as mcg

TASKS = ["semseg", "depth"]
KEYS = ["image", "semseg", "depth"]


def _need_gpu():
    if not conftest.has_gpu():
        pytest.fail("marked gpu but no HIP device is visible")


def _fixture():
    meta, arrs = conftest.load_golden("cs3d")
    return meta, arrs, cs3d_ref.golden_sources(arrs)


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).to("cuda:0")             # a copy: the shared sources are read-only


def _samples(images, labels, disps, bgr):
    return [{"image": _dev(img[..., ::-1] if bgr else img), "semseg": _dev(lab), "depth": _dev(d)} for img, lab, d in zip(images, labels, disps)]


def _host(batch):
    torch.cuda.synchronize()
    return {k: batch[k].cpu().numpy() for k in KEYS + ["flags"] if k in batch}


def _assert_equal(got, want, keys, what):
    for k in keys:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k, got[k].shape, got[k].dtype, want[k].shape, want[k].dtype)
        bad = np.ascontiguousarray(got[k]).view(np.uint8) != np.ascontiguousarray(want[k]).view(np.uint8)
        if bad.any():
            bad = bad.reshape(got[k].shape + (-1,)).any(axis=-1)
            at = tuple(int(v) for v in np.argwhere(bad)[0])
            pytest.fail(f"{what}: '{k}' differs in {int(bad.sum())} of {bad.size} values, first at {at}: {got[k][at]!r} vs {want[k][at]!r}")


@functools.lru_cache(maxsize=None)
def _random_sources(B, H, W, seed=0):
    """B frames: random image; labels over every id 0..33 and 255; disparity with zeros and ones (shared by the tests, never modified)"""
    g = np.random.RandomState(1000 + seed + 7 * H + W)
    ids = np.array(mcg.VOID + mcg.VALID + [255], dtype=np.uint8)
    images = g.randint(0, 256, (B, H, W, 3)).astype(np.uint8)
    labels = ids[g.randint(0, len(ids), (B, H, W))]
    disps = g.randint(0, 1 << 16, (B, H, W)).astype(np.uint16)
    disps[g.rand(B, H, W) < 0.2] = 0
    disps[g.rand(B, H, W) < 0.2] = 1
    for a in (images, labels, disps):
        a.setflags(write=False)
    return images, labels, disps


# ---- 1. the reference's own outputs ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("bgr", [True, False], ids=["bgr", "rgb"])
@pytest.mark.parametrize("case", [c["name"] for c in mcg.cases()])
def test_matches_the_reference_fixture_bitwise(case, bgr):
    """non-integer downscale, upscale, each axis alone, x4 (9 taps), identity, image and labels at different sizes; a batch of two equal
    frames; the meta entries of cityscapes3d.py:140-144"""
    _need_gpu()
    import mtt_amd
    meta, arrs, srcs = _fixture()
    c = next(c for c in meta["cases"] if c["name"] == case)
    s = srcs[c["frame"]]
    prep = mtt_amd.Cityscapes3DPrepare(TASKS, c["img_size"], c["label_size"], mean=meta["mean"], std=meta["std"], bgr=bgr)
    samples = _samples([s["image"]] * 2, [s["semseg"]] * 2, [s["depth"]] * 2, bgr)
    samples[1]["det_label_number"] = 3
    samples[1]["meta"] = {"img_name": "b", "K_matrix": np.eye(3, dtype=np.float32)}
    batch = prep(samples)
    got = _host(batch)
    _assert_equal(got, {k: np.stack([arrs[f"{case}_{k}"]] * 2) for k in KEYS}, KEYS, case)
    assert got["flags"].tolist() == [0, 0]
    prep.check(batch)
    H, W = meta["frames"][c["frame"]]
    for m in batch["meta"]:
        assert m["img_size"] == (H, W) and m["dd_label_map_size"] == tuple(c["label_size"]) and m["scale_factor"].tolist() == c["scale_factor"]
    assert batch["det_label_number"] == [None, 3] and batch["meta"][1]["img_name"] == "b" and (batch["meta"][1]["K_matrix"] == np.eye(3)).all()


# ---- 2. shapes beyond the fixture ----------------------------------------------------------------------------------------------------------
TH, TW = 16, 64                  # the workgroup tile (MTT_CS3D_TILE_H / _W; asserted below)
SHAPES = {
    # name: (B, source, image size, label size)
    "batch3_odd_width": (3, (37, 53), (29, 41), (29, 41)),
    "tile_minus_one": (2, (40, 150), (TH - 1, TW - 1), (TH - 1, TW - 1)),
    "tile_exact": (2, (40, 150), (TH, TW), (TH, TW)),
    "tile_plus_one": (2, (40, 150), (TH + 1, TW + 1), (TH + 1, TW + 1)),
    "up_across_tiles": (2, (21, 50), (2 * TH + 1, 2 * TW + 4), (2 * TH + 1, 2 * TW + 4)),
    "x_only_two_tiles": (2, (40, 150), (40, 100), (40, 100)),
    "y_only_two_tiles": (2, (40, 150), (30, 150), (30, 150)),
    "source_rows_not_16_byte_multiples": (3, (33, 71), (20, 68), (20, 68)),
    "identity_vector": (3, (24, 32), (24, 32), (24, 32)),
    "identity_vector_three_blocks": (2, (80, 112), (80, 112), (80, 112)),      # 8960 pixels: two whole 4096-pixel blocks and a part of one
    "identity_scalar": (3, (23, 31), (23, 31), (23, 31)),
    "labels_keep_the_frame_size": (2, (24, 32), (18, 20), (1024, 2048)),       # dd_label_map_size == ori_img_size: no label resample
    "labels_keep_an_odd_frame_size": (2, (23, 31), (23, 31), (1024, 2048)),
    "full_size_frame": (1, (1024, 2048), (768, 1536), (512, 1024)),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_matches_the_restatement_bitwise(name):
    """a width that is no multiple of 4, output sizes one below / at / one above the workgroup tile, several tiles per axis, one axis
    only, source rows that start off a 16-byte boundary, both same-size kernels, label maps at the frame's size, one full-size frame"""
    _need_gpu()
    import mtt_amd
    assert (mtt_amd._lib.CS3D_TILE_H, mtt_amd._lib.CS3D_TILE_W) == (TH, TW)
    B, (H, W), img_size, label_size = SHAPES[name]
    images, labels, disps = _random_sources(B, H, W)
    for bgr in ((True,) if H >= 1024 else (True, False)):
        prep = mtt_amd.Cityscapes3DPrepare(TASKS, img_size, label_size, bgr=bgr)
        got = _host(prep(_samples(images, labels, disps, False)))
        want = cs3d_ref.prepare_batch(images, labels, disps, prep)
        _assert_equal(got, want, KEYS + ["flags"], f"{name} bgr={bgr}")
    assert (want["depth"] == -1).any() and (want["depth"] == 0).any() and (want["semseg"] == 255).any() and (want["semseg"] == 18).any()


@pytest.mark.gpu
def test_image_alone_and_semseg_without_depth():
    _need_gpu()
    import mtt_amd
    images, labels, disps = _random_sources(2, 40, 150)
    only = mtt_amd.Cityscapes3DPrepare([], (17, 65), (17, 65))
    batch = only([{"image": _dev(im)} for im in images])
    assert sorted(batch) == ["image", "meta"]
    want = cs3d_ref.prepare_batch(images, None, None, only)
    _assert_equal(_host(batch), want, ["image"], "image alone")
    seg = mtt_amd.Cityscapes3DPrepare(["semseg"], (17, 65), (17, 65))
    batch = seg([{"image": _dev(im), "semseg": _dev(lab)} for im, lab in zip(images, labels)])
    assert "depth" not in batch
    _assert_equal(_host(batch), cs3d_ref.prepare_batch(images, labels, None, seg), ["image", "semseg", "flags"], "semseg alone")


# ---- 3. stray writes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("offset", [64, 61], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("name", ["tile_plus_one", "batch3_odd_width", "identity_vector", "identity_vector_three_blocks", "identity_scalar", "x_only_two_tiles"])
def test_nothing_is_written_outside_the_outputs(name, offset):
    """each output lies `offset` elements inside a larger poisoned buffer (64: the 16-byte store paths stay available; 61: they do not),
    and the surround must be unchanged"""
    _need_gpu()
    import mtt_amd
    B, (H, W), img_size, label_size = SHAPES[name]
    images, labels, disps = _random_sources(B, H, W)
    prep = mtt_amd.Cityscapes3DPrepare(TASKS, img_size, label_size, bgr=False)
    h, w = prep.img_size
    lh, lw = prep.label_size((H, W))
    spec = {"image": ((B, 3, h, w), torch.float32, -7.0), "semseg": ((B, lh, lw), torch.int64, -7), "depth": ((B, 1, lh, lw), torch.float32, -7.0),
            "flags": ((B,), torch.int32, -7)}
    bufs, out = {}, {}
    for k, (shape, dtype, poison) in spec.items():
        n = int(np.prod(shape))
        bufs[k] = torch.full((n + 2 * offset + 67,), poison, dtype=dtype, device="cuda:0")
        out[k] = bufs[k][offset:offset + n].view(shape)
    batch = prep.run(prep.pack(_samples(images, labels, disps, False)), out=out)
    assert all(batch[k].data_ptr() == out[k].data_ptr() for k in spec)
    got = _host(batch)
    _assert_equal(got, cs3d_ref.prepare_batch(images, labels, disps, prep), KEYS + ["flags"], f"{name} at offset {offset}")
    for k, (shape, dtype, poison) in spec.items():
        n = int(np.prod(shape))
        assert bool((bufs[k][:offset] == poison).all()) and bool((bufs[k][offset + n:] == poison).all()), f"'{k}': a write outside the output"


# ---- 4. the validity flags ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_an_invalid_id_is_raised_for_its_image_only_and_only_when_it_survives_the_subsampling():
    _need_gpu()
    import mtt_amd
    B, H, W = 3, 40, 150
    images, labels, disps = _random_sources(B, H, W)
    prep = mtt_amd.Cityscapes3DPrepare(TASKS, (20, 75), (20, 75))
    yin, xin = prep.label_tables((H, W))
    kept_y, kept_x = int(yin[7]), int(xin[31])
    dropped_x = next(x for x in range(W) if x not in set(xin.tolist()))
    for what, (y, x), raised in (("kept", (kept_y, kept_x), True), ("dropped", (kept_y, dropped_x), False)):
        lab = labels.copy()
        lab[1, y, x] = 40                                    # neither void nor valid: encode_segmap keeps it, and 40 >= 19
        batch = prep(_samples(images, lab, disps, False))
        want = cs3d_ref.prepare_batch(images, lab, disps, prep)
        assert want["flags"].tolist() == [0, int(raised), 0], what
        _assert_equal(_host(batch), want, KEYS + ["flags"], what)
        if raised:
            with pytest.raises(ValueError, match="Segmentation map contained invalid class values") as e:
                prep.check(batch)
            assert e.value.images == [1] and (want["semseg"][1] == 40).sum() == 1
        else:
            prep.check(batch)
    # the flags are cleared by every call: a clean batch into the same tensors
    out = {"flags": torch.ones(B, dtype=torch.int32, device="cuda:0")}
    prep.check(prep.run(prep.pack(_samples(images, labels, disps, False)), out=out))


# ---- 5. the host check -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_bad_descriptor_is_refused_and_nothing_is_launched():
    _need_gpu()
    import mtt_amd
    L = mtt_amd._lib
    B, (H, W), (h, w) = 2, (40, 150), (17, 65)
    images, labels, disps = _random_sources(B, H, W)
    prep = mtt_amd.Cityscapes3DPrepare(TASKS, (h, w), (h, w), bgr=False)
    src, lab, disp = _dev(images), _dev(labels), _dev(disps)
    (yb_h, yc_h, xb_h, xc_h), (yb, yc, xb, xc) = prep._uploaded("image", (H, W), src.device)
    (yin_h, xin_h), (yin, xin) = prep._uploaded("labels", (H, W), src.device)
    out = torch.full((B, 3, h, w), -7.0, device="cuda:0")
    sem = torch.full((B, h, w), -7, dtype=torch.int64, device="cuda:0")
    dep = torch.full((B, 1, h, w), -7.0, device="cuda:0")
    flags = torch.full((B,), -7, dtype=torch.int32, device="cuda:0")

    def image(**kw):
        f = dict(src=src, out=out, xtab=xb, ytab=yb, xtab_host=xb_h, ytab_host=yb_h, xcoeff=xc, ycoeff=yc, B=B, H=H, W=W, h=h, w=w, xn=w, yn=h,
                 xk=xc.shape[1], yk=yc.shape[1], bgr=0, mean=prep.mean, std=prep.std)
        f.update(kw)
        return L.cs3d_call("cs3d_image", **f)

    def labels_(**kw):
        f = dict(src=lab, disp=disp, out=dep, semseg=sem, flags=flags, xtab=xin, ytab=yin, xtab_host=xin_h, ytab_host=yin_h, B=B, H=H, W=W, h=h, w=w,
                 xn=w, yn=h)
        f.update(kw)
        return L.cs3d_call("cs3d_labels", **f)

    assert image(xn=w - 1) == L.E_BADARG and image(yn=h + 1) == L.E_BADARG, "a table of another length than the output"
    assert image(h=0) == L.E_BADARG and image(B=0) == L.E_BADARG and image(W=W - 1) == L.E_BADARG
    assert image(xtab=None, ytab=None, xtab_host=None, ytab_host=None, xcoeff=None, ycoeff=None) == L.E_BADARG, "no tables: the sizes must agree"
    assert labels_(xn=w + 1) == L.E_BADARG and labels_(yn=h - 1) == L.E_BADARG and labels_(w=0) == L.E_BADARG and labels_(W=W - 10) == L.E_BADARG
    torch.cuda.synchronize()
    for t, poison in ((out, -7.0), (sem, -7), (dep, -7.0), (flags, -7)):
        assert bool((t == poison).all()), "a refused call wrote to its output"
    assert image() == 0 and labels_() == 0
    want = cs3d_ref.prepare_batch(images, labels, disps, prep)
    torch.cuda.synchronize()
    _assert_equal({"image": out.cpu().numpy(), "semseg": sem.cpu().numpy(), "depth": dep.cpu().numpy(), "flags": flags.cpu().numpy()}, want,
                  KEYS + ["flags"], "the accepted descriptor")


# ---- 6. reproducible, and no host synchronisation -----------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_call_is_reproducible_and_does_not_synchronise():
    """two calls are bitwise equal (integer arithmetic, integer atomics), and a call makes no host synchronisation and no device-to-host
    copy: the tables were uploaded by the first call, and only `check` reads the flags back"""
    _need_gpu()
    import mtt_amd
    images, labels, disps = _random_sources(3, 40, 150)
    samples = _samples(images, labels, disps, False)
    prep = mtt_amd.Cityscapes3DPrepare(TASKS, (30, 100), (20, 75))
    first = prep(samples)                                            # warm-up: library load, table upload
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            second = prep(samples)
            third = prep.run(prep.pack(samples))
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert not [str(w.message) for w in rec if "synchroniz" in str(w.message)]
    torch.cuda.synchronize()
    for k in KEYS + ["flags"]:
        assert torch.equal(first[k], second[k]) and torch.equal(first[k], third[k]), k
    _assert_equal(_host(second), cs3d_ref.prepare_batch(images, labels, disps, prep), KEYS + ["flags"], "second call")
