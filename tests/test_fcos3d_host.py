"""CPU (`-m "not gpu"`): the FCOS3D criterion's host side — the fixture's regeneration from the unmodified reference, the plain-torch
restatement the GPU tests compare against (pinned to the fixture), the constructor contract and refusals, the cs parameters and stride
helper, the host-side label packing and the FusedMultiTaskLoss wiring."""
import json
import os

import numpy as np
import pytest
import torch

import conftest
import fcos3d_ref
from tests.golden import make_fcos3d_golden as mfg


def _fixture():
    with open(os.path.join(conftest.GOLDEN, "fcos3d.json")) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(conftest.GOLDEN, "fcos3d.npz"))


def _case(meta, arrs, name):
    c = meta["cases"][name]
    L = len(c["levels"])
    preds = [torch.from_numpy(arrs[f"{name}/pred{j}"]) for j in range(4 * L)]
    return c, mfg.load_labels(arrs, name, c["B"]), [preds[k * L:(k + 1) * L] for k in range(4)]


def _ref_layout(per_image, sizes):
    """[n, P, ...] -> the reference's get_targets layout: levels, then images"""
    offs = np.cumsum([0] + [h * w for h, w in sizes])
    return torch.cat([per_image[:, offs[l]:offs[l + 1]].reshape(-1, *per_image.shape[2:]) for l in range(len(sizes))])


def _dm():
    import mtt_amd
    return mtt_amd.det_model


def test_reference_regenerates_the_fixture(tmp_path):
    """the unmodified reference det_model.py / det_losses.py over import-only stand-ins reproduce tests/golden/fcos3d.* byte for byte
    (a child process, so that the stand-ins never enter this interpreter's modules)"""
    import subprocess
    import sys
    if not os.path.isdir(os.path.join(mfg.REF, "TaskPrompter", "detection_toolbox")):
        pytest.skip("reference tree not present")
    r = subprocess.run([sys.executable, mfg.__file__, str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    for name in ("fcos3d.json", "fcos3d.npz"):
        assert open(tmp_path / name, "rb").read() == open(os.path.join(conftest.GOLDEN, name), "rb").read(), name


def test_fixture_covers_the_edge_cases():
    meta, arrs = _fixture()
    a, b, c = (meta["cases"][k] for k in "abc")
    assert a["num_pos"] > 0 and b["num_pos"] == 0 and c["loss_keys"] == [] and c["loss_sum"] == 0.0
    assert int(arrs["a/num"][1]) == 0 and arrs["a/gt1/label"].shape[0] > 0           # an unlabelled image with gts in the middle
    assert all(v == 0.0 for k, v in b["loss"].items() if k != "loss_cls") and b["loss"]["loss_cls"] > 0
    for j in range(4 * len(a["levels"])):                                              # the dropped image gets zero gradient
        assert not arrs[f"a/grad{j}"][1].any()


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_restatement_reproduces_the_reference_fixture(name):
    """tests/fcos3d_ref.py: labels bit for bit, targets and centerness on positives, every component, loss_sum and every map gradient"""
    meta, arrs = _fixture()
    c, labels, preds = _case(meta, arrs, name)
    sizes = [tuple(l) for l in c["levels"]]
    keep, lab, tgt, cen = fcos3d_ref.assign(meta["params"], labels, sizes)
    if c.get("num_pos") is not None:
        lab_r = _ref_layout(lab, sizes)
        assert np.array_equal(lab_r.numpy(), arrs[f"{name}/labels"].astype(np.int64))
        pos = lab_r < 6
        assert int(pos.sum()) == c["num_pos"]
        assert torch.equal(_ref_layout(tgt, sizes)[pos], torch.from_numpy(arrs[f"{name}/pos_targets"]))
        assert np.allclose(_ref_layout(cen, sizes)[pos].numpy(), arrs[f"{name}/pos_ctr"], rtol=1e-6, atol=0)
    leaves = [[p.clone().requires_grad_(True) for p in lst] for lst in preds]
    ld, ls = fcos3d_ref.loss(meta["params"], leaves, labels)
    assert sorted(ld) == sorted(c["loss"])
    for k, v in ld.items():
        assert abs(float(v) - c["loss"][k]) <= 1e-6 * max(abs(c["loss"][k]), 1e-6), (k, float(v), c["loss"][k])
    assert abs(float(ls) - c["loss_sum"]) <= 1e-6 * max(abs(c["loss_sum"]), 1e-6)
    flat = [p for lst in leaves for p in lst]
    grads = torch.autograd.grad(ls, flat, allow_unused=True)
    for j, (p, g) in enumerate(zip(flat, grads)):
        ref = torch.from_numpy(arrs[f"{name}/grad{j}"]).double()
        g = torch.zeros_like(ref) if g is None else g.double()
        assert float((g - ref).abs().max()) <= 1e-6 * max(float(ref.abs().max()), 1e-30), j


def test_cs_params_and_strides_match_the_reference():
    """cs_det_model_params() is the reference's det_model_params; configure_3ddet scales the strides as config.py:157-160"""
    dm = _dm()
    meta, _ = _fixture()
    p = {"IMAGE_ORI_SIZE": (1024, 2048), "TRAIN": {"SCALE": (1024, 2048)}, "img_ds_ratio": 0.75}
    dm.configure_3ddet(p)
    got = json.loads(json.dumps({k: v for k, v in p["det_model_params"].items() if k != "test_cfg"}))
    assert got == meta["params"]
    assert isinstance(p["detmodel"], dm.DetModel) and p["detmodel"].strides == meta["params"]["strides"]
    assert dm.cs_det_model_params()["strides"] == [8, 16, 32, 32, 64]                  # the helper does not mutate the defaults
    q = {"IMAGE_ORI_SIZE": (1024, 2048), "TRAIN": {"SCALE": (512, 1024)}, "img_ds_ratio": 1.0}
    assert dm.configure_3ddet(q)["detmodel"].strides == [16, 32, 64, 64, 128]


def test_constructor_contract():
    dm = _dm()
    params = dm.cs_det_model_params()
    m = dm.DetModel(**params)
    assert m.strides == [8, 16, 32, 32, 64] and m.regress_ranges == params["regress_ranges"]
    assert m.group_reg_dims == [2, 1, 3, 3, 4] and m.code_weight == params["code_weight"]
    assert m.background_label == 6 and m.bbox_code_size == 9 and m.num_classes == 6
    assert "type" in params["loss_cls"]                                   # the config dicts are not consumed
    dm.DetModel(**params)                                                 # so one dict builds a second criterion
    assert isinstance(m, torch.nn.Module) and len(list(m.parameters())) == 0


@pytest.mark.parametrize("override,word", [
    (dict(pred_keypoints=True), "pred_keypoints"),
    (dict(center_sampling=False), "center_sampling"),
    (dict(use_direction_classifier=False), "use_direction_classifier"),
    (dict(pred_bbox2d=False), "pred_bbox2d"),
    (dict(loss_cls=dict(type='SmoothL1Loss', beta=1.0)), "loss_cls"),
    (dict(loss_centerness=dict(type='CrossEntropyLoss', use_sigmoid=False)), "use_sigmoid"),
    (dict(loss_dir=dict(type='CrossEntropyLoss', use_sigmoid=False, class_weight=[1.0, 2.0])), "class_weight"),
    (dict(loss_bbox=dict(type='SmoothL1Loss', beta=0.1, reduction='sum')), "reduction"),
    (dict(loss_bbox2d=dict(type='GIoULoss')), "loss_bbox2d"),
])
def test_unsupported_options_raise(override, word):
    dm = _dm()
    params = dm.cs_det_model_params()
    params.update(override)
    with pytest.raises(NotImplementedError, match=word):
        dm.DetModel(**params)


def test_giou_consistency_loss_is_accepted_and_ignored():
    dm = _dm()
    params = dm.cs_det_model_params()
    params["loss_consistency"] = dict(type='GIoULoss', eps=1e-7, loss_weight=3.0)
    dm.DetModel(**params)


def test_label_packing():
    """dropped images leave the batch, an image with zero gts stays labelled; the records carry box, label, centre, depth, size and
    rotation in the order of include/mtt_hip.h (ABI 15)"""
    dm = _dm()
    labels = dm.synthetic_det_labels(4, (128, 256), [3, 0, 2, 4], unlabelled=(2,), seed=3)
    assert labels["det_label_number"].tolist() == [3, 1, 0, 4]
    pk = dm.pack_det_labels(labels, "cpu")
    assert pk.B == 4 and pk.n_lab == 3 and pk.keep == [0, 1, 3] and pk.counts == [3, 0, 4]
    assert pk.img.dtype == torch.int32 and pk.img.tolist() == [0, 3, 3] + [3, 0, 4] + [0, 1, 3] + [0, 1, -1, 2]
    assert tuple(pk.gts.shape) == (7, 16)
    e = labels["det_labels"][3]
    rec = pk.gts[3:7]
    assert torch.equal(rec[:, 0:4], e["bbox_modal"]) and torch.equal(rec[:, 4], e["label"].float())
    assert torch.equal(rec[:, 5:8], e["center_I"]) and torch.equal(rec[:, 8:11], e["size_S"]) and torch.equal(rec[:, 11:14], e["rotation_S"])
    none = dm.pack_det_labels(dm.synthetic_det_labels(2, (64, 64), 2, unlabelled=(0, 1)), "cpu")
    assert none.n_lab == 0 and none.img.tolist() == [-1, -1] and tuple(none.gts.shape) == (1, 16)


def test_loss_refuses_cpu_and_non_fp32_predictions():
    dm = _dm()
    m = dm.DetModel(**dm.cs_det_model_params())
    labels = dm.synthetic_det_labels(1, (64, 128), 2)
    levels = ((4, 8), (2, 4), (1, 2), (1, 2), (1, 1))
    preds = [[torch.zeros(1, c, h, w) for h, w in levels] for c in (6, 13, 6, 1)]
    with pytest.raises(RuntimeError, match="GPU"):
        m.loss(preds, labels)


def test_fused_multitask_loss_takes_the_criterion_from_p():
    import mtt_amd
    dm = _dm()
    p = mtt_amd.factory.AttrDict(ignore_index=255)
    p.detmodel = dm.DetModel(**dm.cs_det_model_params())
    crit = mtt_amd.losses.FusedMultiTaskLoss(p, ['semseg', 'depth', '3ddet'], {'semseg': 100.0, 'depth': 1.0, '3ddet': 1.0})
    assert crit.detmodel is p.detmodel and set(crit.spec) == {'semseg', 'depth'}
    assert mtt_amd.losses.FusedMultiTaskLoss(p, ['semseg', '3ddet']).loss_weights == {'semseg': 1.0, '3ddet': 1.0}


# ---- the alt parameter set (tests/golden/fcos3d_alt.*): nothing coincides ----------------------------------------------------------------
def _alt_fixture():
    with open(os.path.join(conftest.GOLDEN, "fcos3d_alt.json")) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(conftest.GOLDEN, "fcos3d_alt.npz"))


def test_reference_regenerates_the_alt_fixture(tmp_path):
    """as test_reference_regenerates_the_fixture, for tests/golden/fcos3d_alt.*"""
    import subprocess
    import sys
    if not os.path.isdir(os.path.join(mfg.REF, "TaskPrompter", "detection_toolbox")):
        pytest.skip("reference tree not present")
    r = subprocess.run([sys.executable, mfg.__file__, str(tmp_path), "alt"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    size = 0
    for name in ("fcos3d_alt.json", "fcos3d_alt.npz"):
        assert open(tmp_path / name, "rb").read() == open(os.path.join(conftest.GOLDEN, name), "rb").read(), name
        size += os.path.getsize(os.path.join(conftest.GOLDEN, name))
    assert size < 512 * 1024


def test_alt_parameter_set_has_no_coincidences():
    meta, arrs = _alt_fixture()
    p = meta["params"]
    lw = [p[k]["loss_weight"] for k in ("loss_cls", "loss_bbox", "loss_dir", "loss_centerness", "loss_bbox2d")]
    assert len(set(lw)) == 5 and len(set(p["code_weight"])) == 13 and len(set(meta["gout"])) == 9 and all(meta["gout"])
    assert p["loss_cls"]["gamma"] not in (2.0,) and p["loss_cls"]["gamma"] >= 1 and p["loss_cls"]["alpha"] != 0.25
    assert p["loss_bbox"]["beta"] != p["loss_bbox2d"]["beta"] and p["dir_offset"] != 0 and p["centerness_alpha"] != 2.5
    assert p["center_sample_radius"] != 1.5 and p["num_classes"] != 6
    a, b = meta["cases"]["a"], meta["cases"]["b"]
    assert a["num_pos"] > 20 and b["num_pos"] == 0 and int(arrs["a/num"][1]) == 0
    assert int(arrs["a/labels"].max()) == p["num_classes"] and set(np.unique(arrs["a/labels"])) == set(range(p["num_classes"] + 1))


@pytest.mark.parametrize("name", ["a", "b"])
def test_restatement_reproduces_the_alt_fixture(name):
    """tests/fcos3d_ref.py under the alt set, at the bounds of test_restatement_reproduces_the_reference_fixture; the gradient is the
    fixture's one weighted set, d (sum_i w_i * component_i + w_8 * loss_sum)"""
    meta, arrs = _alt_fixture()
    C = meta["params"]["num_classes"]
    c, labels, preds = _case(meta, arrs, name)
    sizes = [tuple(l) for l in c["levels"]]
    keep, lab, tgt, cen = fcos3d_ref.assign(meta["params"], labels, sizes)
    lab_r = _ref_layout(lab, sizes)
    assert np.array_equal(lab_r.numpy(), arrs[f"{name}/labels"].astype(np.int64))
    pos = lab_r < C
    assert int(pos.sum()) == c["num_pos"]
    assert torch.equal(_ref_layout(tgt, sizes)[pos], torch.from_numpy(arrs[f"{name}/pos_targets"]))
    assert np.allclose(_ref_layout(cen, sizes)[pos].numpy(), arrs[f"{name}/pos_ctr"], rtol=1e-6, atol=0)
    leaves = [[p.clone().requires_grad_(True) for p in lst] for lst in preds]
    ld, ls = fcos3d_ref.loss(meta["params"], leaves, labels)
    assert sorted(ld) == sorted(c["loss"])
    for k, v in ld.items():
        assert abs(float(v) - c["loss"][k]) <= 1e-6 * max(abs(c["loss"][k]), 1e-6), (k, float(v), c["loss"][k])
    assert abs(float(ls) - c["loss_sum"]) <= 1e-6 * max(abs(c["loss_sum"]), 1e-6)
    w = meta["gout"]
    total = sum(w[i] * ld[k] for i, k in enumerate(fcos3d_ref.KEYS)) + w[8] * ls
    flat = [p for lst in leaves for p in lst]
    grads = torch.autograd.grad(total, flat, allow_unused=True)
    for j, (p, g) in enumerate(zip(flat, grads)):
        ref = torch.from_numpy(arrs[f"{name}/grad{j}"]).double()
        g = torch.zeros_like(ref) if g is None else g.double()
        assert float((g - ref).abs().max()) <= 1e-6 * max(float(ref.abs().max()), 1e-30), j
