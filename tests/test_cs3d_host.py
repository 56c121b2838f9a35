"""CPU (`-m "not gpu"`): the host side of the Cityscapes-3D batch preparation — the numpy restatement the GPU tests use equals the
reference's own outputs (tests/golden/cs3d.*) and PIL.Image.resize bit for bit, the class builds the same tables, from_config covers
the three data sets, and the refusals."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import conftest
import cs3d_ref
from tests.golden import make_cs3d_golden as mcg

PAIRS = [((37, 53), (28, 40)), ((24, 32), (31, 45)), ((20, 30), (20, 23)), ((64, 96), (16, 24)), ((1024, 2048), (768, 1536))]


def _fixture():
    return conftest.load_golden("cs3d")


def test_reference_regenerates_the_fixture(tmp_path):
    """the stand-ins + the unmodified data/cityscapes3d.py reproduce tests/golden/cs3d.* byte for byte (build container only; a child
    process, so that the stand-in modules never enter this interpreter)"""
    if not os.path.isfile(os.path.join(mcg.REF, "TaskPrompter", "data", "cityscapes3d.py")):
        pytest.skip("reference tree not present")
    r = subprocess.run([sys.executable, mcg.__file__, str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    for name in ("cs3d.json", "cs3d.npz"):
        assert open(tmp_path / name, "rb").read() == open(os.path.join(conftest.GOLDEN, name), "rb").read(), name


def test_fixture_covers_what_it_names():
    meta, arrs = _fixture()
    assert [c["name"] for c in meta["cases"]] == [c["name"] for c in mcg.cases()] and len(meta["frames"]) >= 2
    sizes = {(tuple(meta["frames"][c["frame"]]), tuple(c["img_size"])) for c in meta["cases"]}
    assert {((37, 53), (28, 40)), ((24, 32), (31, 45)), ((64, 96), (16, 24)), ((37, 53), (37, 53))} <= sizes
    assert any(H == h and W != w for (H, W), (h, w) in sizes) and any(H != h and W == w for (H, W), (h, w) in sizes)
    for j in range(len(meta["frames"])):
        lab, disp = arrs[f"src{j}_semseg"], arrs[f"src{j}_depth"]
        assert set(mcg.VOID + mcg.VALID) <= set(np.unique(lab).tolist())
        assert (disp[lab == 10] > 1).any() and (disp == 0).any() and (disp == 1).any() and (disp[lab == 10] == 0).any()
    # the accumulated-addition index and the multiplied one part on a column of the upscale case, and the label map shows it
    acc, mul = cs3d_ref.nearest_axis(32, 45), cs3d_ref.nearest_axis_multiplied(32, 45)
    cols = np.nonzero(acc != mul)[0]
    assert len(cols) > 0
    lut = cs3d_ref.encode_lut()[arrs["src1_semseg"]]
    rows = cs3d_ref.nearest_axis(24, 31)
    assert (arrs["up_semseg"][:, cols] == lut[rows][:, acc[cols]]).all() and (lut[rows][:, acc[cols]] != lut[rows][:, mul[cols]]).any()
    assert os.path.getsize(os.path.join(conftest.GOLDEN, "cs3d.npz")) <= os.path.getsize(os.path.join(conftest.GOLDEN, "augment.npz"))


@pytest.mark.parametrize("case", [c["name"] for c in mcg.cases()])
def test_restatement_equals_the_reference_fixture_bitwise(case):
    meta, arrs = _fixture()
    c = next(c for c in meta["cases"] if c["name"] == case)
    src = cs3d_ref.golden_sources(arrs)[c["frame"]]
    for bgr in (False, True):
        image = src["image"][..., ::-1] if bgr else src["image"]
        got = cs3d_ref.prepare_frame(image, src["semseg"], src["depth"], c["img_size"], c["label_size"], meta["mean"], meta["std"], bgr=bgr)
        assert not got["flag"]
        for k in ("image", "semseg", "depth"):
            want = arrs[f"{case}_{k}"]
            assert cs3d_ref.bits_equal(got[k], want), (k, bgr, int((got[k] != want).sum()))


@pytest.mark.parametrize("pair", PAIRS, ids=[f"{a[0]}x{a[1]}_to_{b[0]}x{b[1]}" for a, b in PAIRS])
def test_restated_resize_equals_pillow(pair):
    """bilinear on random uint8 RGB images and nearest on random uint8 and float maps, as cityscapes3d.py's imresize calls them"""
    (H, W), (h, w) = pair
    g = np.random.RandomState(H * 7 + w)
    img = g.randint(0, 256, (H, W, 3)).astype(np.uint8)
    want = np.array(Image.fromarray(img).resize((w, h), Image.BILINEAR))
    assert cs3d_ref.bits_equal(cs3d_ref.resize_bilinear_u8(img, (h, w)), want)
    grey = np.ascontiguousarray(img[..., 0])
    assert cs3d_ref.bits_equal(cs3d_ref.resize_bilinear_u8(grey, (h, w)), np.array(Image.fromarray(grey).resize((w, h), Image.BILINEAR)))
    assert cs3d_ref.bits_equal(cs3d_ref.resize_nearest(grey, (h, w)), np.array(Image.fromarray(grey).resize((w, h), Image.NEAREST)))
    for arr in (g.randn(H, W).astype(np.float32), g.randint(0, 34, (H, W)).astype(float)):          # mode F, from float32 and from float64
        want = np.array(Image.fromarray(arr).resize((w, h), Image.NEAREST))
        assert want.dtype == np.float32
        assert cs3d_ref.bits_equal(cs3d_ref.resize_nearest(arr, (h, w)).astype(np.float32), want)


def test_nearest_is_not_the_multiplied_index():
    """what makes the tables necessary: (x + 0.5) * in / out lands on other pixels than Pillow's accumulated additions"""
    assert int((cs3d_ref.nearest_axis(2048, 1536) != cs3d_ref.nearest_axis_multiplied(2048, 1536)).sum()) > 0
    assert int((cs3d_ref.nearest_axis(32, 45) != cs3d_ref.nearest_axis_multiplied(32, 45)).sum()) > 0


@pytest.mark.parametrize("pair", PAIRS, ids=[f"{a[0]}x{a[1]}_to_{b[0]}x{b[1]}" for a, b in PAIRS])
def test_class_tables_equal_the_restatement(pair):
    import mtt_amd
    (H, W), (h, w) = pair
    prep = mtt_amd.Cityscapes3DPrepare(["semseg", "depth"], (h, w), (h, w))
    (yb, yc), (xb, xc) = prep.image_tables((H, W))
    for n_in, n_out, bounds, coeff in ((H, h, yb, yc), (W, w, xb, xc)):
        assert bounds.dtype == coeff.dtype == np.int32 and bounds.shape == (n_out, 2)
        if n_in == n_out:                                    # the identity table stands for the skipped axis
            assert coeff.shape == (n_out, 1) and (coeff == 1 << 22).all() and (bounds == np.stack([np.arange(n_out), np.ones(n_out)], 1)).all()
            continue
        xmin, cnt, kk = cs3d_ref.bilinear_axis(n_in, n_out)
        assert coeff.shape == kk.shape and (bounds[:, 0] == xmin).all() and (bounds[:, 1] == cnt).all() and (coeff == kk).all()
        assert (coeff.sum(axis=1) - (1 << 22)).__abs__().max() <= coeff.shape[1], "weights sum to one up to their rounding"
    yin, xin = prep.label_tables((H, W))
    assert yin.dtype == xin.dtype == np.int32
    assert (yin == cs3d_ref.nearest_axis(H, h)).all() and (xin == cs3d_ref.nearest_axis(W, w)).all()
    assert prep.image_tables((h, w)) is None
    same = mtt_amd.Cityscapes3DPrepare(["semseg"], (h, w), (1024, 2048))
    assert same.label_tables((H, W)) is None and same.label_size((H, W)) == (H, W), "the size test reads the constant, not the frame"


def test_from_config_covers_the_three_data_sets():
    import mtt_amd
    for db in ("NYUD", "PASCALContext"):
        p = mtt_amd.factory.make_p(["semseg", "depth"], (48, 64), train_db_name=db)
        assert mtt_amd.Cityscapes3DPrepare.from_config(p) == (None, None)
    p = mtt_amd.factory.make_p(["semseg", "depth"], (768, 1536), train_db_name="Cityscapes3D", dd_label_map_size=[512, 1024])
    p.TEST = mtt_amd.factory.AttrDict(SCALE=(1024, 2048))
    train, valid = mtt_amd.Cityscapes3DPrepare.from_config(p)
    assert train.img_size == (768, 1536) and valid.img_size == (1024, 2048)
    for prep in (train, valid):
        assert prep.tasks == ["semseg", "depth"] and prep.dd_label_map_size == (512, 1024) and prep.ori_img_size == (1024, 2048)
        assert prep.mean == (0.485, 0.456, 0.406) and prep.std == (0.229, 0.224, 0.225) and prep.bgr
    assert mtt_amd.DeviceAugment.from_config(p) == (None, None)
    assert mtt_amd.Cityscapes3DPrepare is mtt_amd.cs3d.Cityscapes3DPrepare


def test_depth_without_semseg_names_the_missing_key():
    import mtt_amd
    with pytest.raises(ValueError, match="semseg"):
        mtt_amd.Cityscapes3DPrepare(["depth"], (24, 32), (24, 32))
    mtt_amd.Cityscapes3DPrepare(["semseg"], (24, 32), (24, 32))
    mtt_amd.Cityscapes3DPrepare(["semseg", "depth", "3ddet"], (24, 32), (24, 32))


def test_cpu_tensors_raise():
    import mtt_amd
    prep = mtt_amd.Cityscapes3DPrepare(["semseg"], (24, 32), (24, 32))
    sample = {"image": torch.zeros(37, 53, 3, dtype=torch.uint8), "semseg": torch.zeros(37, 53, dtype=torch.uint8)}
    with pytest.raises(RuntimeError, match="device memory"):
        prep([sample])
    with pytest.raises(RuntimeError, match="device memory"):
        prep.run({"image": torch.zeros(1, 37, 53, 3, dtype=torch.uint8)})
    with pytest.raises(RuntimeError):
        mtt_amd._lib.cs3d_call("cs3d_image", src=torch.zeros(8, dtype=torch.uint8))


def test_abi_stays_17_and_exports_the_new_names():
    import mtt_amd
    lib = mtt_amd._lib
    assert lib.ABI_VERSION == 17 and lib.load().mtt_abi_version() == 17
    for name in ("mtt_cs3d_desc_size", "mtt_cs3d_image", "mtt_cs3d_labels"):
        assert name in lib.EXPORTS and hasattr(lib.load(), name)
    assert set(lib.CS3D) == {"cs3d_image", "cs3d_labels"} and not set(lib.CS3D) & (set(lib.DESCS) | set(lib.AUGMENT))
    header = open(os.path.join(conftest.ROOT, "include", "mtt_hip.h")).read()
    for name, val in (("TILE_H", lib.CS3D_TILE_H), ("TILE_W", lib.CS3D_TILE_W), ("MAX_ROWS", lib.CS3D_MAX_ROWS), ("MAX_COLS", lib.CS3D_MAX_COLS)):
        assert f"#define MTT_CS3D_{name} {val}\n" in header


def test_host_check_refuses_a_bad_descriptor_without_a_device():
    """the C entry points validate sizes and the HOST copies of the tables before anything touches the device: a refused descriptor
    returns a negative status even here, where no launch could succeed"""
    import mtt_amd
    lib = mtt_amd._lib
    prep = mtt_amd.Cityscapes3DPrepare(["semseg"], (28, 40), (28, 40))
    (yb, yc), (xb, xc) = [tuple(torch.from_numpy(a) for a in t) for t in prep.image_tables((37, 53))]
    fake = yb.data_ptr()                                     # never dereferenced: every call below is refused by the host check

    def image(**kw):
        f = dict(src=fake, out=fake, xtab=fake, ytab=fake, xcoeff=fake, ycoeff=fake, xtab_host=xb, ytab_host=yb, B=1, H=37, W=53, h=28, w=40,
                 xn=40, yn=28, xk=xc.shape[1], yk=yc.shape[1], mean=(0.5, 0.5, 0.5), std=(0.25, 0.25, 0.25), stream=0)
        f.update(kw)
        return lib.cs3d_call("cs3d_image", **f)

    assert image(h=0) == lib.E_BADARG and image(B=0) == lib.E_BADARG and image(W=0) == lib.E_BADARG and image(w=1 << 20) == lib.E_BADARG
    assert image(xn=39) == lib.E_BADARG and image(yn=29) == lib.E_BADARG, "a table of another length than the output"
    assert image(W=52) == lib.E_BADARG, "the last column's taps would end one pixel past the source row"
    assert image(xk=1) == lib.E_BADARG and image(yk=0) == lib.E_BADARG
    assert image(std=(0.25, 0.0, 0.25)) == lib.E_BADARG and image(out=None) == lib.E_BADARG and image(ycoeff=None) == lib.E_BADARG
    bad = xb.clone()
    bad[7, 0] = bad[6, 0] - 1
    assert image(xtab_host=bad) == lib.E_BADARG, "bounds that step backwards"
    assert image(src=fake + 1) == lib.E_ALIGN
    # a reduction whose tile window does not fit the LDS budget
    big = mtt_amd.Cityscapes3DPrepare([], (16, 40), (16, 40))
    (yb2, yc2), _ = [tuple(torch.from_numpy(a) for a in t) for t in big.image_tables((16 * 14, 53))]
    assert image(H=16 * 14, h=16, yn=16, ytab_host=yb2, yk=yc2.shape[1]) == lib.E_UNSUPPORTED
    yin, xin = [torch.from_numpy(a) for a in prep.label_tables((37, 53))]

    def labels(**kw):
        f = dict(src=fake, semseg=fake, flags=fake, xtab=fake, ytab=fake, xtab_host=xin, ytab_host=yin, B=1, H=37, W=53, h=28, w=40, xn=40, yn=28, stream=0)
        f.update(kw)
        return lib.cs3d_call("cs3d_labels", **f)

    assert labels(xn=41) == lib.E_BADARG and labels(yn=27) == lib.E_BADARG and labels(h=0) == lib.E_BADARG
    assert labels(H=36) == lib.E_BADARG, "the last index lies past the source"
    assert labels(xtab=None, xtab_host=None) == lib.E_BADARG, "no table stands for the identity, which needs equal sizes"
    assert labels(xtab_host=None) == lib.E_BADARG and labels(flags=None) == lib.E_BADARG and labels(disp=fake, out=None) == lib.E_BADARG
