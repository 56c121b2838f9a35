"""CPU (`-m "not gpu"`): the box-decoding restatement (tests/det_decode_ref.py) against the fixture of the unmodified reference
(tests/golden/decode.npz), the Cityscapes-3D test_cfg, and the refusal to decode CPU tensors."""
import json
import os

import numpy as np
import pytest
import torch

import conftest
import det_decode_ref as ddr
from tests.golden import make_decode_golden as mdg


def fixture():
    with open(os.path.join(conftest.GOLDEN, "decode.json")) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(conftest.GOLDEN, "decode.npz"))


@pytest.mark.parametrize("name", ["s", "t", "w", "n"])
def test_restatement_equals_the_reference_fixture(name):
    """kept labels, order and counts exact; every value to 1e-6 relative (fp32 restatement, the oracle's NMS)"""
    meta, arrs = fixture()
    c = meta["cases"][name]
    preds, label = mdg.load_inputs(arrs, meta, name)
    got = ddr.decode_batch(preds, meta["params"]["strides"], label, c["cfg"], ddr.oracle_nms, torch.float32)
    want = mdg.load_expected(arrs, meta, name)
    assert [int(g["labels_3d"].shape[0]) for g in got] == c["n_out"]
    for g, w in zip(got, want):
        assert g["labels_3d"].dtype == torch.int64 and torch.equal(g["labels_3d"], w["labels_3d"])
        for k in ddr.COLUMNS:
            assert g[k].shape == w[k].shape, k
            if w[k].numel():
                err = float(((g[k].double() - w[k].double()).abs() / w[k].double().abs().clamp_min(1e-30)).max())
                assert err <= 1e-6, (name, k, err)


def test_fixture_inputs_meet_the_decision_margins():
    meta, _ = fixture()
    for name, c in meta["cases"].items():
        for k, need in meta["margins_required"].items():
            assert c["margins"][k] >= need, (name, k, c["margins"][k])
    assert meta["cases"]["w"]["seeds_skipped"], "case w was expected to step its seed"


def test_cs_test_cfg_equals_the_reference():
    import mtt_amd
    meta, _ = fixture()
    assert mtt_amd.det_model.cs_det_model_params()["test_cfg"] == meta["test_cfg"]
    assert mtt_amd.det_model.cs_test_cfg() == meta["test_cfg"]
    for k, v in dict(use_rotate_nms=True, nms_pre=1000, nms_thr=0.3, score_thr=0.05, max_per_img=200).items():
        assert meta["test_cfg"][k] == v


def _crit(meta, cfg):
    import mtt_amd
    return mtt_amd.det_model.DetModel(**json.loads(json.dumps(meta["params"])), test_cfg=cfg)


def test_decoding_refuses_cpu_tensors_and_rescale():
    meta, arrs = fixture()
    preds, label = mdg.load_inputs(arrs, meta, "s")
    crit = _crit(meta, meta["cases"]["s"]["cfg"])
    with pytest.raises(RuntimeError):
        crit.get_results_from_bbox(preds, label)
    with pytest.raises(NotImplementedError):
        crit.get_results_from_bbox(preds, label, rescale=True)
    metas = [{k: v[b] for k, v in label["meta"].items()} for b in range(2)]
    with pytest.raises(RuntimeError):
        crit.get_bboxes(*preds, metas)
    with pytest.raises(RuntimeError):                       # non-fp32 maps: refused before anything touches a device
        crit.get_results_from_bbox(tuple([t.double() for t in lst] for lst in preds), label)


def test_candidate_and_class_limits_are_named_errors():
    import mtt_amd
    dd = mtt_amd.det_decode
    geo = dd.geometry([(96, 192), (48, 96)], [8.0, 16.0], 5000, True)
    assert geo["N"] == 5000 + 4608 and geo["cand_off"][:3] == [0, 5000, 9608] and geo["key_off"][2] == 96 * 192 + 48 * 96
    with pytest.raises(dd.DecodeLimitError):
        dd.check_limits(geo["N"], 6)
    with pytest.raises(dd.DecodeLimitError):
        dd.check_limits(100, 17)
    dd.check_limits(8192, 16)
    assert dd.geometry([(4, 5)], [8.0], -1, True)["N"] == 20 and dd.geometry([(4, 5)], [8.0], 20, True)["N"] == 20
    assert dd.geometry([(4, 5)], [8.0], 19, True)["N"] == 19


def test_test_cfg_may_be_a_dict_or_an_attribute_object():
    import types
    meta, _ = fixture()
    cfg = meta["cases"]["s"]["cfg"]
    a = _crit(meta, cfg)._test_cfg(None)
    b = _crit(meta, types.SimpleNamespace(**cfg))._test_cfg(None)
    assert a == b == {k: cfg[k] for k in ddr.CFG_KEYS}
    with pytest.raises(ValueError):
        _crit(meta, None)._test_cfg(None)
