"""GPU (`-m gpu`): get_output and the task meters on the HIP kernels of csrc/eval_ops.hip against the fixture the unmodified reference
wrote (tests/golden/eval.npz, eval.json) and the fp64 restatement tests/eval_ref.py.

Bounds.  int64 maps and every integer counter: exact.  Float maps: allclose(rtol=1e-5, atol=1e-4) — values are <= 255 and at most about
6 fp32 roundings from the exact one, each <= 1.5e-5.  Float sums: 1e-5 relative to the fp64 restatement — every accumulated term is
non-negative and about 20 fp32 operations deep (about 1.2e-6) and the partial sums are fp64.  The measured figures are reported through
parity_util.report.

Cases.  The fixture's shapes reach the four-pixel path (HW a multiple of 4, 16-byte aligned buffers) for semseg and saliency only, so
every check below also runs on ALIGNED: human_parts, normals, depth (both masks) and edge at 64 x 80 with inputs drawn here by the
generator's own make_inputs; their reference is the fp64 restatement (integer maps and counters exact, as tests/test_eval_host.py pins
it to the reference).  test_unaligned_buffers_take_the_scalar_path runs the same shapes from buffers 4 bytes off alignment.
"""
import functools

import numpy as np
import pytest
import torch

import eval_ref
import eval_util
import parity_util

SENTINEL = 0x5A5A5A5A5A5A5A5A
GUARD = 64              # 8-byte words on either side of a guarded buffer


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


ALIGNED = {  # name: task, (B, C, H, W), meter class, constructor kwargs, classes
    "aligned_human_parts": ("human_parts", (2, 7, 64, 80), "HumanPartsMeter", dict(database="PASCALContext", ignore_idx=255), 7),
    "aligned_normals": ("normals", (2, 3, 64, 80), "NormalsMeter", dict(ignore_index=255), None),
    "aligned_depth_range": ("depth", (2, 1, 64, 80), "DepthMeter", dict(max_depth=8.0, min_depth=0.5), None),
    "aligned_depth_ignore": ("depth", (2, 1, 64, 80), "DepthMeter_legacy", dict(ignore_index=255), None),
    "aligned_edge": ("edge", (3, 1, 64, 80), "EdgeMeter", dict(pos_weight=0.95, ignore_index=255), None),
}
CASES = eval_util.case_names() + list(ALIGNED)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(case record, logits, labels, the map to expect, states to expect after update 1 and 2 or None) as numpy"""
    if name in ALIGNED:
        task, shape, cls, kw, n = ALIGNED[name]
        x, gt = eval_util.make_inputs(task, shape, n, None, np.random.default_rng(sorted(ALIGNED).index(name) + 7))
        return eval_util.case_record(task, shape, cls, kw, n, None), x, gt, eval_ref.map_ref(task, x), None
    meta, arrs = eval_util.fixture()
    case = meta["cases"][name]
    x, gt = eval_util.inputs(name)
    return case, x, gt, arrs[name + ".map"], (case["state1"], case["state2"])


@functools.lru_cache(maxsize=None)
def _restated(name):
    """(state after update 1, after update 2) of the fp64 restatement: computed once per case"""
    case, x, gt = _case(name)[:3]
    s1 = eval_ref.state_ref(case, x, gt)
    return s1, eval_ref.add_states(s1, eval_ref.state_ref(case, x[eval_util.SECOND], gt[eval_util.SECOND]))


def _ev():
    import mtt_amd
    return mtt_amd.evaluation


# ---- 1. maps ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_maps_match_reference(name):
    _need_gpu()
    case, x, _, want, _ = _case(name)
    xd = _dev(x)
    out = _ev().get_output(xd, case["task"])
    assert tuple(out.shape) == want.shape
    if case["task"] in ("semseg", "human_parts"):
        assert out.dtype == torch.int64
        assert np.array_equal(out.cpu().numpy(), want.astype(np.int64))
        if name == "semseg_cs":
            ids = _ev().get_output(xd, "semseg", semseg_save_train_class=False)
            assert np.array_equal(ids.cpu().numpy(), eval_util.fixture()[1][name + ".map_labelid"].astype(np.int64))
    else:
        got = out.cpu().numpy()
        err = float(np.abs(got.astype(np.float64) - want).max())
        parity_util.report("eval_map", case=name, max_abs_err=err)
        assert out.dtype == torch.float32
        assert np.allclose(got, want, rtol=1e-5, atol=1e-4), err
    if case["task"] == "depth":                                    # clamped in place on the caller's tensor, returned as its permuted view
        assert out.data_ptr() == xd.data_ptr() and float(xd.min()) == 0.0
        assert np.array_equal(xd.cpu().numpy(), np.maximum(x, 0.0))
    else:
        assert np.array_equal(xd.cpu().numpy(), x)


# ---- 2. meters --------------------------------------------------------------------------------------------------------------------------
def _run(name, fused):
    case, x, gt = _case(name)[:3]
    ev = _ev()
    meter = eval_util.make_meter(case)
    states, raws = [], []
    for sl in (slice(0, None), eval_util.SECOND):
        xd, gd = _dev(x[sl]), _dev(gt[sl])
        if fused:
            meter.update_from_logits(xd, gd)
            assert np.array_equal(xd.cpu().numpy(), x[sl]) and np.array_equal(gd.cpu().numpy(), gt[sl])     # inputs are not modified
        else:
            meter.update(ev.get_output(xd, case["task"]), gd)
        states.append(meter.state())
        raws.append(meter._host())
    return meter, states, raws


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_counts_exact_and_sums_within_bound(name):
    """after update 1 (the whole batch) and update 2 (images [:-1]): integer counters equal the reference's, float sums within 1e-5
    relative of the fp64 restatement; get_score gives the reference's keys and values"""
    _need_gpu()
    case, _, _, _, recorded = _case(name)
    meter, states, _ = _run(name, fused=True)
    for i, (got, want) in enumerate(zip(states, _restated(name))):
        if recorded is not None:                                                          # the reference's counters, exactly
            for k in recorded[i]:
                if k in eval_ref.INT_KEYS:
                    eval_ref.compare_states({k: got[k]}, {k: recorded[i][k]}, 0.0)
        worst = eval_ref.compare_states(got, want, 1e-5)                                  # integer counters exact here too
        parity_util.report("eval_sums", case=name, update=i + 1, worst_rel_err=worst, bound=1e-5)
    score = meter.get_score(verbose=False)
    want = case["score"] if recorded is not None else meter.score_from_state(eval_util.fixture_state_tensors(dict(s=_restated(name)[1]), "s"), False)
    assert set(score) == set(want)
    for k, v in want.items():
        assert abs(float(score[k]) - float(v)) <= 1e-5 * abs(float(v)) + 1e-12, (k, float(score[k]), float(v))


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_two_paths_and_two_runs_are_bitwise_equal(name):
    _need_gpu()
    _, _, fused = _run(name, fused=True)
    _, _, again = _run(name, fused=True)
    _, _, mapped = _run(name, fused=False)
    for a, b, c in zip(fused, again, mapped):
        assert torch.equal(a, b), "two runs differ"
        assert torch.equal(a, c), "update(get_output(x)) and update_from_logits(x) differ"
    assert bool(fused[1].any())


# ---- 3. stray writes --------------------------------------------------------------------------------------------------------------------
def _guarded(words, dtype=torch.int64):
    """(whole int64 buffer of sentinels, the `words` 8-byte words in its middle viewed as dtype)"""
    whole = torch.full((words + 2 * GUARD,), SENTINEL, dtype=torch.int64, device="cuda:0")
    return whole, whole[GUARD:GUARD + words].view(dtype)


def _guards_intact(whole, words):
    return bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[GUARD + words:] == SENTINEL).all())


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_no_stray_writes(name):
    """guard bands around the map output, the accumulator and the workspace are untouched; the guarded run gives the meter's state"""
    _need_gpu()
    import mtt_amd
    lib = mtt_amd._lib
    case, x, gt = _case(name)[:3]
    B, C, H, W = x.shape
    HW = H * W
    meter = eval_util.make_meter(case)
    kind = meter._kind
    xd, gd = _dev(x), _dev(gt)
    per = 3 if kind == lib.EVAL_NORMALS else 1
    if kind == lib.EVAL_CONFUSION:
        map_words = B * HW
        mwhole, mview = _guarded(map_words)
    else:
        map_words = (B * HW * per + 1) // 2
        mwhole, mview = _guarded(map_words, torch.float32)
    lib.call("eval_map", pred=xd, out=mview, B=B, HW=HW, C=C, kind=kind)
    fields = meter._fields(xd.device)
    nws = lib.eval_ws_floats(kind, B, HW)
    results = []
    for source, pred in ((lib.EVAL_FROM_LOGITS, xd), (lib.EVAL_FROM_MAP, mview)):
        awhole, acc = _guarded(meter._slots)
        acc.zero_()
        wwhole, ws = _guarded(max(nws // 2, 1), torch.float64)
        lib.call("eval_accum", pred=pred, label=gd, acc=acc, ws=ws if nws else None, B=B, HW=HW, C=C if source == lib.EVAL_FROM_LOGITS else (meter._channels or 1),
                 Cl=meter._label_channels, kind=kind, source=source, **fields)
        torch.cuda.synchronize()
        assert _guards_intact(awhole, meter._slots), "accumulator guard band written"
        assert _guards_intact(wwhole, max(nws // 2, 1)), "workspace guard band written"
        if not nws:
            assert bool((ws.view(torch.int64) == SENTINEL).all()), "integer meters take no workspace"
        results.append(acc.cpu().clone())
    assert _guards_intact(mwhole, map_words), "map guard band written"
    if kind != lib.EVAL_CONFUSION and (B * HW * per) % 2:                 # the odd tail float of the last 8-byte word
        assert int(mview.view(torch.int32)[-1]) == SENTINEL & 0x7FFFFFFF
    assert torch.equal(results[0], results[1])
    meter.update_from_logits(xd, gd)
    assert torch.equal(meter._host(), results[0])


def _off_alignment(a):
    """a device copy of `a` whose storage starts 4 bytes past a 16-byte boundary"""
    flat = torch.empty(a.size + 1, dtype=torch.float32, device="cuda:0")
    view = flat[1:].view(*a.shape)
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["semseg_cs", "sal_big"] + list(ALIGNED))
@pytest.mark.parametrize("which", ["pred", "label"])
def test_unaligned_buffers_take_the_scalar_path(name, which):
    """HW is a multiple of 4 but the logits (or the labels) are not 16-byte aligned: one pixel per thread.  Same maps and integer
    counters as from aligned buffers, bit for bit; the fp64 sums are taken in another order and stay within the bound"""
    _need_gpu()
    case, x, gt = _case(name)[:3]
    assert (x.shape[2] * x.shape[3]) % 4 == 0
    ev = _ev()
    xa, ga = _dev(x), _dev(gt)
    xu = _off_alignment(x) if which == "pred" else _dev(x)
    gu = _off_alignment(gt) if which == "label" else _dev(gt)
    aligned, shifted = eval_util.make_meter(case), eval_util.make_meter(case)
    aligned.update_from_logits(xa, ga)
    shifted.update_from_logits(xu, gu)
    got, want = shifted.state(), aligned.state()
    for k in want:
        if k in eval_ref.INT_KEYS or k in ("pp_hist", "tp_hist"):
            assert torch.equal(got[k], want[k]), k
    eval_ref.compare_states(got, _restated(name)[0], 1e-5)
    assert torch.equal(ev.get_output(xu, case["task"]).contiguous(), ev.get_output(xa, case["task"]).contiguous())


# ---- 4. no host synchronisation, graph capture ------------------------------------------------------------------------------------------
def _pascal_batch(B, H, W, seed):
    import mtt_amd
    AttrDict = mtt_amd.factory.AttrDict
    tasks = ["semseg", "human_parts", "sal", "edge", "normals", "depth"]
    num = dict(semseg=21, human_parts=7, sal=2, edge=1, normals=3, depth=1)
    p = AttrDict(train_db_name="PASCALContext", ignore_index=255, edge_w=0.95,
                 TASKS=AttrDict(NAMES=tasks, NUM_OUTPUT=num, depth_max=8.0, depth_min=0.5))
    g = torch.Generator(device="cpu").manual_seed(seed)
    out = {t: (torch.randn(B, num[t], H, W, generator=g) * 2).to("cuda:0") for t in tasks}
    gt = mtt_amd.losses.synthetic_targets(p, B, H, W, "cuda:0", seed=seed + 1)
    return p, tasks, out, gt


def _raw(pm):
    return {t: pm.meters[t]._host() for t in pm.tasks}


@pytest.mark.gpu
def test_update_does_not_synchronise_and_replays_from_a_graph():
    """all-task update_from_logits: no host synchronisation; captured once in a linear single-stream graph and replayed three times, the
    integer counters are 3x those of one update (the fp64 sums 3x to rounding)"""
    _need_gpu()
    import warnings
    import mtt_amd
    p, tasks, out, gt = _pascal_batch(2, 23, 37, 5)
    pm = mtt_amd.PerformanceMeter(p, tasks).to("cuda:0")
    pm.update_from_logits(out, gt)                                   # warm-up: library load, thresholds and workspaces
    torch.cuda.synchronize()
    pm.reset()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            pm.update_from_logits(out, gt)
            pm.update({t: mtt_amd.get_output(out[t].clone(), t) for t in tasks}, gt)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert not [str(w.message) for w in rec if "synchroniz" in str(w.message)]
    twice = _raw(pm)
    pm.reset()
    pm.update_from_logits(out, gt)
    once = _raw(pm)
    for t in tasks:
        n_int = {"depth": 1, "normals": 1, "edge": 1}.get(t, once[t].numel())
        assert torch.equal(twice[t][:n_int], 2 * once[t][:n_int]) and bool(once[t][:n_int].any()), t
    pm.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pm.update_from_logits(out, gt)
    assert not any(bool(v.any()) for v in _raw(pm).values()), "capture records the launches, it does not run them"
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    thrice = _raw(pm)
    for t in tasks:
        n_int = {"depth": 1, "normals": 1, "edge": 1}.get(t, once[t].numel())
        assert torch.equal(thrice[t][:n_int], 3 * once[t][:n_int]), t
        a, b = thrice[t][n_int:].view(torch.float64), once[t][n_int:].view(torch.float64)
        assert torch.allclose(a, 3 * b, rtol=1e-14, atol=0.0), t


# ---- 5. full size -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_full_size_counts_match_torch_on_device():
    """(2, 21, 512, 512): more pixels per image than one sweep of the grid covers; counts against torch ops on the device"""
    _need_gpu()
    ev = _ev()
    B, C, H, W = 2, 21, 512, 512
    g = torch.Generator(device="cpu").manual_seed(11)
    x = (torch.randn(B, C, H, W, generator=g) * 2).to("cuda:0")
    gt = torch.randint(0, C, (B, 1, H, W), generator=g).float()
    gt[torch.rand(B, 1, H, W, generator=g) < 0.05] = 255
    gt[torch.rand(B, 1, H, W, generator=g) < 0.01] = 254
    gt = gt.to("cuda:0")
    meter = ev.SemsegMeter("PASCALContext")
    meter.update_from_logits(x, gt)
    st = meter.state()
    vals, pred = torch.max(x.permute(0, 2, 3, 1), dim=3)
    assert torch.equal(ev.get_output(x, "semseg"), pred)
    lab = gt.squeeze(1).long()
    valid = lab != 255
    hit = valid & (lab == pred)
    tp = torch.bincount(pred[hit], minlength=C)
    fp = torch.bincount(pred[valid & ~hit], minlength=C)
    fn = torch.bincount(lab[valid & ~hit & (lab < C)], minlength=C)
    assert torch.equal(st["tp"], tp.cpu()) and torch.equal(st["fp"], fp.cpu()) and torch.equal(st["fn"], fn.cpu())
    assert int(st["tp"].sum() + st["fp"].sum()) == int(valid.sum())
