"""CPU (`-m "not gpu"`): the host side of the batch augmentation — the fixture regenerates from the unmodified reference, the one-pass
restatement the GPU tests use equals the fixture bit for bit, `draw` keeps the reference's ranges, from_config mirrors
get_transformations, and the refusals (CPU tensors, cat_max_ratio without semseg)."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import augment_ref
import conftest
from tests.golden import make_augment_golden as mag


def _fixture():
    return conftest.load_golden("augment")


def test_reference_regenerates_the_fixture(tmp_path):
    """the cv2 stand-in + the unmodified data/transforms.py reproduce tests/golden/augment.* byte for byte (build container only; a child
    process, so that the stand-in `cv2` never enters this interpreter's modules)"""
    if not os.path.isfile(os.path.join(mag.REF, "TaskPrompter", "data", "transforms.py")):
        pytest.skip("reference tree not present")
    r = subprocess.run([sys.executable, mag.__file__, str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    for name in ("augment.json", "augment.npz"):
        assert open(tmp_path / name, "rb").read() == open(os.path.join(conftest.GOLDEN, name), "rb").read(), name


def test_fixture_covers_what_it_names():
    meta, arrs = _fixture()
    names = [c["name"] for c in meta["cases"]]
    assert names == [c["name"] for c in mag.cases()]
    assert any(k > 0 for c in meta["cases"] for k in c["chosen"]), "no case in which the reference redrew its crop"
    rows = [r for c in meta["cases"] for r in c["rows"]]
    assert {r["s"] for r in rows} >= {0.5, 1.0, 1.37, 2.0}
    assert {r["hue_delta"] for r in rows if r["hue"]} >= {-18, 17}
    assert {r["beta"] for r in rows if r["bright"]} >= {-32.0, 32.0} and {r["c_alpha"] for r in rows if r["contrast"]} >= {0.5, 1.5}
    assert any(not r["cands"] for r in rows), "no sample whose scaled size equals the crop size"
    assert os.path.getsize(os.path.join(conftest.GOLDEN, "augment.npz")) < os.path.getsize(os.path.join(conftest.GOLDEN, "mini_swin_pad.npz"))


@pytest.mark.parametrize("case", [c["name"] for c in mag.cases()])
def test_restatement_equals_the_reference_fixture_bitwise(case):
    """augment_ref (the composed inverse mapping, one pass per output pixel) == the reference's own chain of classes, every bit, and the
    crop candidate it settles on is the one the reference's draw-test-redraw loop stopped at"""
    import mtt_amd
    meta, arrs = _fixture()
    c = next(c for c in meta["cases"] if c["name"] == case)
    srcs = augment_ref.golden_sources(arrs)
    aug = mtt_amd.DeviceAugment(meta["tasks"], c["size"], train=c["mode"] == "train")
    P = augment_ref.params_from_rows(c["rows"], meta["shapes"], c["size"], c["mode"])
    got, chosen = augment_ref.augment_batch(srcs, P, aug)
    assert chosen == c["chosen"]
    for k in ["image"] + meta["tasks"]:
        want = arrs[f"{case}_{k}"]
        assert augment_ref.bits_equal(got[k], want), (k, int((got[k] != want).sum()))


def test_draw_keeps_the_references_ranges():
    import mtt_amd
    aug = mtt_amd.DeviceAugment(["semseg", "depth"], (24, 32))
    shapes = [(37, 53), (64, 48), (24, 32), (100, 17)] * 16
    P = aug.draw(shapes, random.Random(7))
    assert len(P) == len(shapes) and P.cand_y.shape == P.cand_x.shape == (len(shapes), 11)
    for i, (H, W) in enumerate(shapes):
        s = float(P.scale[i])
        assert 0.5 <= s <= 2.0 and bool(P.resized[i]) == (s != 1.0)
        assert P.scaled[i].tolist() == [int(H * s), int(W * s)]
        Sh, Sw = P.scaled[i].tolist()
        assert 0 <= P.cand_y[i].min() and P.cand_y[i].max() <= max(Sh - 24, 0)
        assert 0 <= P.cand_x[i].min() and P.cand_x[i].max() <= max(Sw - 32, 0)
        assert -18 <= P.hue_delta[i] <= 17 and -32 <= P.beta[i] <= 32
        assert 0.5 <= P.c_alpha[i] <= 1.5 and 0.5 <= P.s_alpha[i] <= 1.5
        assert P.n_test[i] == (0 if (Sh, Sw) == (24, 32) else 10)
    assert P.beta.dtype == P.c_alpha.dtype == P.s_alpha.dtype == np.float32
    assert len({tuple(r) for r in P.cand_y.tolist()}) > 1 and P.flip.any() and not P.flip.all() and P.hue.any() and P.f_mode.any()
    t = P.table()
    assert t.shape == (len(shapes), mtt_amd._lib.AUG_COLS) and t.dtype == np.int32
    assert (t[:, mtt_amd._lib.AUG_CHOSEN] == np.where(P.n_test == 10, 10, 0)).all()
    # the same seed gives the same table; an rng is consumed, not reseeded
    assert (aug.draw(shapes, random.Random(7)).table() == t).all()
    # without the class-share test no candidate is tested
    free = mtt_amd.DeviceAugment(["depth"], (24, 32), cat_max_ratio=1.0).draw(shapes, random.Random(7))
    assert not free.n_test.any()
    # valid mode: the identity row
    valid = mtt_amd.DeviceAugment(["depth"], (64, 64), train=False).draw([(37, 53)], random.Random(0))
    assert not valid.resized.any() and not valid.flip.any() and not valid.cand_y.any() and valid.scaled.tolist() == [[37, 53]]
    with pytest.raises(ValueError):
        mtt_amd.DeviceAugment(["depth"], (24, 32), train=False).draw([(37, 53)])


def test_from_config_reproduces_the_two_compositions():
    import mtt_amd
    for db in ("NYUD", "PASCALContext"):
        p = mtt_amd.factory.make_p(["semseg", "depth", "normals"], (48, 64), train_db_name=db)
        p.TEST = mtt_amd.factory.AttrDict(SCALE=(56, 72))
        train, valid = mtt_amd.DeviceAugment.from_config(p)
        assert train.train and train.size == (48, 64) and train.tasks == ["semseg", "depth", "normals"]
        assert (train.scale_factors, train.cat_max_ratio, train.flip_p, train.photometric) == ((0.5, 2.0), 0.75, 0.5, True)
        assert train.mean == (0.485, 0.456, 0.406) and train.std == (0.229, 0.224, 0.225) and train.depth_ignore_to_minus1
        assert not valid.train and valid.size == (56, 72) and valid.tasks == train.tasks and valid.mean == train.mean and valid.std == train.std
        for name in ("RandomScaling", "RandomCrop", "RandomHorizontalFlip", "PhotoMetricDistortion", "Normalize", "PadImage", "AddIgnoreRegions", "ToTensor"):
            assert name in repr(train)
            assert (name in repr(valid)) == (name in ("Normalize", "PadImage", "AddIgnoreRegions", "ToTensor"))
    p = mtt_amd.factory.make_p(["semseg"], (48, 64), train_db_name="Cityscapes3D")
    assert mtt_amd.DeviceAugment.from_config(p) == (None, None)


def test_cpu_tensors_raise():
    import mtt_amd
    aug = mtt_amd.DeviceAugment(["semseg"], (24, 32))
    sample = {"image": torch.zeros(37, 53, 3), "semseg": torch.zeros(37, 53, 1)}
    with pytest.raises(RuntimeError):
        aug([sample])
    with pytest.raises(RuntimeError):
        mtt_amd._lib.aug_call("aug_image", src=torch.zeros(8), table_host=torch.zeros(40, dtype=torch.int32))


def test_class_share_test_needs_semseg():
    import mtt_amd
    with pytest.raises(KeyError):
        mtt_amd.DeviceAugment(["depth", "normals"], (24, 32))
    mtt_amd.DeviceAugment(["depth", "normals"], (24, 32), cat_max_ratio=1.0)
    mtt_amd.DeviceAugment(["depth", "normals"], (24, 32), train=False)


def test_abi_stays_17_and_exports_the_new_names():
    import mtt_amd
    lib = mtt_amd._lib
    assert lib.ABI_VERSION == 17 and lib.load().mtt_abi_version() == 17
    for name in ("mtt_aug_desc_size", "mtt_aug_select", "mtt_aug_image", "mtt_aug_labels"):
        assert name in lib.EXPORTS and hasattr(lib.load(), name)
    assert set(lib.AUGMENT) == {"aug_select", "aug_image", "aug_labels"} and not set(lib.AUGMENT) & set(lib.DESCS)
    header = open(os.path.join(conftest.ROOT, "include", "mtt_hip.h")).read()
    assert f"#define MTT_AUG_COLS {lib.AUG_COLS}" in header and f"#define MTT_AUG_CANDS {lib.AUG_CANDS}" in header


def test_host_check_refuses_a_bad_table_without_a_device():
    """the C entry point validates the HOST copy of the table before anything touches the device: out-of-range rows return MTT_E_BADARG
    even here, where no launch could succeed"""
    import mtt_amd
    lib = mtt_amd._lib
    P = mtt_amd.AugParams.identity([(8, 8)])
    good = torch.from_numpy(P.table().copy())
    off = torch.zeros(1, dtype=torch.int64)
    fake = lambda t: t.data_ptr()                          # noqa: E731  (never dereferenced: every call below is refused by the host check)
    def call(table, numel=8 * 8 * 3, offset=0):
        off[0] = offset
        return lib.aug_call("aug_image", table_host=table, off_host=off, src=fake(good), off=fake(good), table=fake(good),
                            out=fake(good), src_numel=numel, B=1, h=8, w=8, C=3, stream=0)
    for col, val in ((lib.AUG_H, 9), (lib.AUG_W, 0), (lib.AUG_SH, 40000), (lib.AUG_CAND_Y + 3, 1), (lib.AUG_CAND_X, -1), (lib.AUG_CHOSEN, 11),
                     (lib.AUG_HDELTA, 18), (lib.AUG_FLIP, 2), (lib.AUG_NTEST, 5)):
        bad = good.clone()
        bad[0, col] = val
        assert call(bad) == lib.E_BADARG, col
    assert call(good, numel=8 * 8 * 3 - 1) == lib.E_BADARG
    assert call(good, offset=1) == lib.E_BADARG and call(good, offset=-1) == lib.E_BADARG
