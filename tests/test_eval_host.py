"""Host-side checks of mtt_amd.evaluation (no GPU): the fp64 restatement tests/eval_ref.py is pinned to the reference's recorded
results, get_score repeats the reference's host arithmetic, the interface keeps the reference's signatures, and nothing falls back to
the CPU."""
import inspect
import re

import numpy as np
import pytest
import torch

import eval_ref
import eval_util


@pytest.mark.parametrize("name", eval_util.case_names())
def test_restatement_pinned_to_reference(name):
    meta, arrs = eval_util.fixture()
    case = meta["cases"][name]
    x, gt = eval_util.inputs(name)
    assert list(x.shape) == case["shape"]
    m = eval_ref.map_ref(case["task"], x)
    got = arrs[name + ".map"]
    if m.dtype == np.int64:
        assert np.array_equal(m, got.astype(np.int64))
    else:
        assert got.dtype == np.float32 and got.shape == m.shape
        assert np.allclose(got, m, rtol=1e-5, atol=1e-4)
    if name == "semseg_cs":
        assert np.array_equal(eval_ref.map_ref("semseg", x, semseg_save_train_class=False), arrs[name + ".map_labelid"].astype(np.int64))
    # counts equal, the reference's own fp32 sums within 1e-5 relative of the fp64 restatement, after one and after two updates
    want1 = eval_ref.state_ref(case, x, gt)
    want2 = eval_ref.add_states(want1, eval_ref.state_ref(case, x[eval_util.SECOND], gt[eval_util.SECOND]))
    eval_ref.compare_states(case["state1"], want1, 1e-5)
    eval_ref.compare_states(case["state2"], want2, 1e-5)
    if case["task"] == "sal":                                     # no pixel is left out: every score keeps its distance from every threshold
        assert eval_ref.sal_margin(eval_ref.map_ref("sal", x), case["thresholds"]) >= 1e-4


def test_fixture_covers_the_edge_cases():
    meta, arrs = eval_util.fixture()
    x, gt = eval_util.inputs("semseg_pascal")
    top2 = np.sort(x, axis=1)[:, -2:]
    assert (top2[:, 0] == top2[:, 1]).sum() > 10                  # exact ties at the maximum
    assert (gt == 254).any() and (gt[1] == 255).all() and 0.02 < (gt[::2] == 255).mean() < 0.1
    x, gt = eval_util.inputs("depth_ignore")
    assert (x <= 0).any() and (gt <= 0).any() and (gt < 0.5).any() and ((gt > 8) & (gt != 255)).any()
    x, gt = eval_util.inputs("normals")
    assert ((x == 0).all(axis=1)).any() and ((gt == 0).all(axis=1)).any()
    assert {tuple(c["shape"]) for c in meta["cases"].values()} >= {(3, 21, 23, 37), (2, 40, 5, 7), (2, 19, 64, 80), (3, 7, 23, 37),
                                                                   (3, 2, 23, 37), (2, 2, 64, 80)}


@pytest.mark.parametrize("name", eval_util.case_names())
def test_get_score_repeats_reference_host_arithmetic(name, capsys):
    case = eval_util.fixture()[0]["cases"][name]
    meter = eval_util.make_meter(case)
    score = meter.score_from_state(eval_util.fixture_state_tensors(case, "state2"), False)
    assert set(score) == set(case["score"])
    for k, v in case["score"].items():
        assert float(score[k]) == v, (k, float(score[k]), v)
    assert capsys.readouterr().out == ""
    # before any update the state is zeros on the host, with the keys and lengths of the recorded one
    st = meter.state()
    for k, v in case["state2"].items():
        assert k in st and st[k].numel() == (len(v) if isinstance(v, list) else 1) and not st[k].any()


def _positional(sig):
    """signature string without keyword-only additions"""
    return re.sub(r",\s*\*,.*\)$", ")", sig)


def test_signatures_match_reference():
    import mtt_amd
    ev = mtt_amd.evaluation
    sigs = eval_util.fixture()[0]["signatures"]
    assert str(inspect.signature(ev.get_output)) == sigs["get_output"]
    assert str(inspect.signature(mtt_amd.get_output)) == sigs["get_output"]
    for key, want in sigs.items():
        if "." not in key:
            continue
        cls, fn = key.split(".")
        got = str(inspect.signature(getattr(getattr(ev, cls), fn)))
        if fn == "get_score":                                     # cat_names / **kw may follow the reference's parameters
            assert got.startswith(want[:-1]), (key, got, want)
        else:
            assert _positional(got) == want, (key, got, want)
    for cls in ("SemsegMeter", "HumanPartsMeter", "SaliencyMeter", "NormalsMeter", "DepthMeter", "EdgeMeter", "PerformanceMeter"):
        for fn in ("update", "update_from_logits", "reset", "get_score"):
            assert callable(getattr(getattr(ev, cls), fn))
        assert getattr(mtt_amd, cls) is getattr(ev, cls)


def test_no_cpu_fallback_and_argument_errors():
    import mtt_amd
    ev = mtt_amd.evaluation
    x = torch.zeros(2, 3, 4, 5)
    for task in ("semseg", "human_parts", "normals", "edge", "sal", "depth"):
        with pytest.raises(RuntimeError):
            ev.get_output(x, task)
    with pytest.raises(ValueError):
        ev.get_output(x, "flow")
    gt = torch.zeros(2, 1, 4, 5)
    for meter in (ev.SemsegMeter("NYUD"), ev.HumanPartsMeter("PASCALContext"), ev.NormalsMeter(), ev.SaliencyMeter(threshold_step=0.05),
                  ev.DepthMeter(8.0, 0.5), ev.DepthMeter(ignore_index=255), ev.EdgeMeter(0.95, 255)):
        with pytest.raises(RuntimeError):
            meter.update_from_logits(x, gt)
        with pytest.raises(RuntimeError):
            meter.update(torch.zeros(2, 4, 5), gt)
        with pytest.raises(RuntimeError):
            meter.to("cpu")
    with pytest.raises(NotImplementedError, match="pos_weight"):
        ev.EdgeMeter(None, 255)
    with pytest.raises(NotImplementedError):
        ev.SemsegMeter("KITTI")
    with pytest.raises(ValueError):
        ev.DepthMeter()


def test_get_output_3ddet_delegates():
    import mtt_amd

    class Det:
        def get_results_from_bbox(self, output, label, rescale):
            return ("det", output, label, rescale)

    p = mtt_amd.factory.AttrDict(detmodel=Det())
    assert mtt_amd.evaluation.get_output("boxes", "3ddet", p=p, label="sample") == ("det", "boxes", "sample", False)


def test_performance_meter_reads_the_reference_config_keys():
    import mtt_amd
    p = mtt_amd.factory.AttrDict(train_db_name="PASCALContext", ignore_index=255, edge_w=0.95, TASKS=mtt_amd.factory.AttrDict(depth_max=80.0, depth_min=0.0))
    tasks = ["semseg", "human_parts", "normals", "sal", "edge", "depth"]
    pm = mtt_amd.PerformanceMeter(p, tasks)
    assert [type(pm.meters[t]).__name__ for t in tasks] == ["SemsegMeter", "HumanPartsMeter", "NormalsMeter", "SaliencyMeter", "EdgeMeter", "DepthMeter"]
    assert pm.meters["semseg"].n_classes == 21 and pm.meters["depth"].max_depth == 80.0 and pm.meters["edge"].pos_weight == 0.95
    assert pm.meters["sal"].beta_squared == 0.3 and pm.meters["sal"].thresholds.numel() == 19
    pm.reset()


def test_eval_entries_in_a_table_of_their_own():
    import mtt_amd
    lib = mtt_amd._lib
    assert set(lib.EVAL) == {"eval_map", "eval_accum"}
    for table in (lib.DESCS, lib.POSITIONAL, lib.DESC_EXTRA, lib.POSTPROC):
        assert not set(lib.EVAL) & set(table)
    assert lib.ABI_VERSION == 17 and {"mtt_eval_map", "mtt_eval_accum", "mtt_eval_ws_floats", "mtt_eval_desc_size"} <= set(lib.EXPORTS)
    assert lib.eval_ws_floats(lib.EVAL_CONFUSION, 2, 1000) == 0 and lib.eval_ws_floats(lib.EVAL_DEPTH, 2, 1000) == 2 * 5 * 4 * 2
