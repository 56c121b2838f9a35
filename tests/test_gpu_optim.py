"""-m gpu: mtt_grad_sqnorm / mtt_adam_step and optim.FusedClipAdam on the device, judged per element against the fp64 Adam of
tests/optim_ref.py (reference, rounding counts, guard layout and cases are described there; tests/test_optim_host.py runs the same cases
on the emulator and shows that the judge rejects planted defects).

Part 1 calls the entry points through ops.call with hand-built pointer / numel / chunk tables, so that alignment and layout are the
test's choice.  Part 2 drives FusedClipAdam: parameter groups and step-count partitions, host run-ahead past the 4-deep pinned staging
rings, graph replay under a learning-rate schedule, state interchange with torch.optim.Adam, and a NaN gradient.

Not covered: tensors above 2^31 elements (the kernels' 64-bit chunk offsets cannot be reached at test sizes), denormal gradients, DDP.
"""
import copy
import math
import time
import warnings

import pytest
import torch

import optim_ref as R
import parity_util

ADAM_SPECS = R.adam_specs()
SQNORM_SPECS = R.sqnorm_specs()
_BUILT = {}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import mtt_amd
    assert mtt_amd.ops.adam_chunk() == R.CHUNK
    return mtt_amd


def _case(name):
    if name not in _BUILT:
        _BUILT[name] = R.build(next(s for s in ADAM_SPECS + SQNORM_SPECS if s["name"] == name))
    return _BUILT[name]


def _device_run(name, mtt_amd):
    """(the case on the CPU, the case after mtt_adam_step on the device); run once per case."""
    key = ("dev", name)
    if key not in _BUILT:
        after = R.run_adam(_case(name).to("cuda"), mtt_amd.ops.call)
        torch.cuda.synchronize()
        _BUILT[key] = after.to("cpu")
    return _case(name), _BUILT[key]


# ---------------------------------------------------------------------------------------------
# 1. the entry points
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("spec", ADAM_SPECS, ids=lambda s: s["name"])
def test_adam_step_case(spec):
    mtt_amd = _need_gpu()
    case, after = _device_run(spec["name"], mtt_amd)
    need, bad = R.judge_case(case, after)
    parity_util.report("optim_adam_step", case=spec["name"], need=need, count=R.COUNT)
    assert not bad, bad
    assert R.passes(need), (need, R.COUNT)
    if spec["hyper"]:                                       # the device pair gives the result of the same values passed as descriptor fields
        _, fields_run = _device_run("aligned", mtt_amd)
        for r in R.ROLES:
            assert torch.equal(after.buf[r].view(torch.int32), fields_run.buf[r].view(torch.int32)), r


@pytest.mark.gpu
@pytest.mark.parametrize("spec", SQNORM_SPECS, ids=lambda s: s["name"])
def test_grad_sqnorm_case(spec):
    mtt_amd = _need_gpu()
    case = _case(spec["name"])
    out, after = R.run_sqnorm(case.to("cuda"), mtt_amd.ops.call)
    ref = 3.0 + R.sumsq_ref([case.view("g", i) for i in range(len(R.SIZES))])          # out_sq was pre-filled with 3.0: accumulation
    need = R.norm_need(math.sqrt(out) if out >= 0 else float("nan"), math.sqrt(ref))
    parity_util.report("optim_grad_sqnorm", case=spec["name"], need=dict(norm=need), bound=R.NORM_TOL)
    assert need <= R.NORM_TOL, (out, ref)
    assert not R.guards_intact(case, after)
    for r in R.ROLES:                                        # nothing but out_sq and the workspace is written
        assert torch.equal(case.buf[r].view(torch.int32), after.buf[r].cpu().view(torch.int32)), r


# ---------------------------------------------------------------------------------------------
# 2. FusedClipAdam
# ---------------------------------------------------------------------------------------------
class _Totals:
    """ops.call wrapper that keeps a device copy of the sum of squares every mtt_adam_step launch clips by (no synchronisation)."""

    def __init__(self, real):
        self.real, self.totals = real, []

    def __call__(self, name, **kw):
        r = self.real(name, **kw)
        if name == "adam_step":
            t = kw["xargs"][0]
            self.totals.append(None if t is None else t.clone())
        return r

    def last(self):
        """The value of the latest step (every launch of one step reads the same tensor)."""
        t = self.totals[-1]
        return None if t is None else float(t.cpu()[0])


def _params(seed, scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter((torch.randn(n, generator=gen) * scale).cuda()) for n in R.SIZES]


def _grads(seed, scale):
    gen = torch.Generator().manual_seed(seed)
    return [(torch.randn(n, generator=gen) * scale).cuda() for n in R.SIZES]


def _state(opt, q):
    st = opt.state.get(q, {})
    if "exp_avg" not in st:
        return torch.zeros_like(q), torch.zeros_like(q), 0.0
    return st["exp_avg"].detach().clone(), st["exp_avg_sq"].detach().clone(), float(st["step"])


def _snapshot(opt, params):
    return [(q.detach().clone(),) + _state(opt, q) for q in params]


def _group_of(opt, q):
    return next(g for g in opt.param_groups if any(q is x for x in g["params"]))


def _judge_step(opt, params, grads, before, after, total_sq, hypers, label, step):
    """One optimizer step of every parameter against adam_ref from the parameter's own state before the step.
    before / after: _snapshot lists; hypers: per parameter dict(lr, betas, eps, weight_decay) as they stood when the step was taken."""
    worst = dict(m=0.0, v=0.0, dp=0.0)
    for q, g, (p0, m0, v0, t0), (p1, m1, v1, t1), h in zip(params, grads, before, after, hypers):
        if g is None:
            assert t1 == t0 and torch.equal(p0, p1) and torch.equal(m0, m1) and torch.equal(v0, v1), (label, step)
            continue
        assert t1 == t0 + 1, (label, step, t0, t1)
        f = R.fields(h["lr"], h["betas"], h["eps"], h["weight_decay"], opt.max_norm, t1)
        for k, n in R.judge(f, total_sq, g, p0, m0, v0, p1, m1, v1).items():
            worst[k] = max(worst[k], n)
    parity_util.report("optim_fused_clip_adam", case=label, step=step, need=worst, count=R.COUNT)
    assert R.passes(worst), (label, step, worst, R.COUNT)
    return worst


def _hypers(opt, params):
    return [{k: _group_of(opt, q)[k] for k in ("lr", "betas", "eps", "weight_decay")} for q in params]


def _judge_norm(norm, grads, label, step):
    n_ref = math.sqrt(R.sumsq_ref([g for g in grads if g is not None]))
    need = R.norm_need(float(norm), n_ref)
    parity_util.report("optim_fused_clip_adam_norm", case=label, step=step, need=dict(norm=need), bound=R.NORM_TOL)
    assert need <= R.NORM_TOL, (label, step, float(norm), n_ref)


@pytest.mark.gpu
@pytest.mark.parametrize("max_norm", [2.0, 0.0], ids=["clip", "max_norm_0"])
def test_groups_and_step_count_partitions(max_norm, monkeypatch):
    """Two parameter groups with different lr / betas / eps / weight_decay; two parameters of the first group receive their first gradient
    at step 3 (two step-count partitions in that group from then on).  p, m, v and the returned norm are judged after each of six steps;
    the gradients alternate between clipping (norm ~ 5.7) and not (norm ~ 0.57)."""
    mtt_amd = _need_gpu()
    rec = _Totals(mtt_amd.ops.call)
    monkeypatch.setattr(mtt_amd.ops, "call", rec)
    params = _params(40)
    first, second = params[0::2], params[1::2]
    late = [params[2], params[8]]                                  # sizes 4 and 65537, both in the first group
    opt = mtt_amd.optim.FusedClipAdam([dict(params=first), dict(params=second, lr=3e-3, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.05)],
                                      lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_norm=max_norm)
    label = "groups_partitions_" + ("clip" if max_norm > 0 else "max_norm_0")
    for step in range(1, 7):
        grads = _grads(50 + step, 1e-2 if step % 2 else 1e-3)
        if step < 3:
            grads = [None if any(q is x for x in late) else g for q, g in zip(params, grads)]
        for q, g in zip(params, grads):
            q.grad = g
        before, hy = _snapshot(opt, params), _hypers(opt, params)
        norm = opt.step()
        torch.cuda.synchronize()
        total = rec.last()
        assert (total is None) == (max_norm == 0.0)
        _judge_step(opt, params, grads, before, _snapshot(opt, params), total, hy, label, step)
        _judge_norm(norm, grads, label, step)
    assert [float(opt.state[q]["step"]) for q in params] == [4.0 if any(q is x for x in late) else 6.0 for q in params]


@pytest.mark.gpu
def test_host_runs_ahead_of_the_staging_rings(monkeypatch):
    """capturable=True under PolynomialLR, 12 steps with freshly allocated gradients and no host synchronisation while the device is
    still busy with earlier work: the host queues steps faster than the device takes them, three times round the 4-deep rings of pinned
    gradient-pointer tables and `hyper` pairs.  A slot rewritten before its copy ran would give a step another step's learning rate or
    gradients; every step is judged from device snapshots after one synchronisation at the end."""
    mtt_amd = _need_gpu()
    rec = _Totals(mtt_amd.ops.call)
    monkeypatch.setattr(mtt_amd.ops, "call", rec)
    params = _params(60)
    opt = mtt_amd.optim.FusedClipAdam(params, lr=1e-3, weight_decay=1e-2, max_norm=2.0, capturable=True)
    sched = mtt_amd.optim.PolynomialLR(opt, max_iterations=14, gamma=0.9)
    steps = 12
    gsets = [_grads(70 + k, 1e-2 if k % 2 else 1e-3) for k in range(steps)]
    a = torch.randn(4096, 4096, device="cuda")
    b = torch.empty_like(a)
    for q, g in zip(params, _grads(69, 1e-2)):                      # one step ahead of the loop: the first step builds the pointer tables
        q.grad = g                                                  # with blocking copies, which would drain the queue the loop is about
    opt.step()
    sched.step()
    snaps, hypers, norms, keep = [_snapshot(opt, params)], [], [], []
    first, c0, c1 = torch.cuda.Event(), torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    n0 = len(rec.totals)
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            c0.record()
            for _ in range(128):                                    # queued work ahead of the first step: ~0.1 s, the host needs a few ms for 4 steps
                torch.matmul(a, a, out=b)
            c1.record()
            t0 = time.perf_counter()
            for k in range(steps):
                fresh = [g.clone() for g in gsets[k]]               # new addresses every step: all of them stay alive in `keep`
                keep.append(fresh)
                for q, g in zip(params, fresh):
                    q.grad = g
                hypers.append(_hypers(opt, params))
                norms.append(opt.step())
                sched.step()
                snaps.append(_snapshot(opt, params))
                if k == 0:
                    first.record()
                if k == 3:
                    ahead = not first.query()                       # four steps queued, the first has not run yet
                    host_ms = 1e3 * (time.perf_counter() - t0)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    parity_util.report("optim_run_ahead", queued_work_ms=round(c0.elapsed_time(c1), 1), host_ms_for_4_steps=round(host_ms, 1), ahead=ahead)
    assert ahead, "the host did not run ahead of the device: the queued work ahead of the loop is too short for this machine"
    assert not [w for w in caught if "synchron" in str(w.message).lower()], [str(w.message) for w in caught]
    assert len({g.data_ptr() for fresh in keep for g in fresh}) == steps * len(params)
    assert len({h[0]["lr"] for h in hypers}) == steps                # the schedule moved the learning rate at every step
    for k in range(steps):
        assert all(torch.equal(g, f) for g, f in zip(gsets[k], keep[k]))
        total = float(rec.totals[n0 + k].cpu()[0])
        _judge_step(opt, params, gsets[k], snaps[k], snaps[k + 1], total, hypers[k], "run_ahead", k + 2)
        _judge_norm(norms[k], gsets[k], "run_ahead", k + 2)


@pytest.mark.gpu
def test_replay_under_a_schedule_equals_eager_steps():
    """opt.step() alone captured in a graph (static gradient buffers, after two eager steps on a side stream, as GraphedTrainStep does) and
    replayed six times under PolynomialLR, against an eager capturable=False twin taking the same steps: bitwise equal parameters and
    moments after every replay, equal step counts."""
    mtt_amd = _need_gpu()
    pg, pe = _params(80), _params(80)
    kw = dict(lr=2e-3, weight_decay=1e-2, max_norm=2.0)
    og = mtt_amd.optim.FusedClipAdam(pg, capturable=True, **kw)
    oe = mtt_amd.optim.FusedClipAdam(pe, **kw)
    sg, se = (mtt_amd.optim.PolynomialLR(o, max_iterations=10, gamma=0.9) for o in (og, oe))
    static = [torch.zeros_like(q) for q in pg]
    for q, g in zip(pg, static):
        q.grad = g

    def feed(k):
        new = _grads(90 + k, 1e-2 if k % 2 else 1e-3)
        for s, q, g in zip(static, pe, new):
            s.copy_(g)
            q.grad = g

    def same(k):
        for q, r in zip(pg, pe):
            assert torch.equal(q.detach(), r.detach()), k
            for key in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(og.state[q][key], oe.state[r][key]), (k, key)
            assert float(og.state[q]["step"]) == float(oe.state[r]["step"]) == float(k), k

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                               # torch's advice on the order of scheduler.step() and optimizer.step()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        for k in (1, 2):
            feed(k)
            sg.step(), se.step()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                og.step()
            torch.cuda.current_stream().wait_stream(side)
            oe.step()
            same(k)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            og.step()
        for k in range(3, 9):
            feed(k)
            sg.step(), se.step()
            og.prepare_replay()
            graph.replay()
            og.after_replay()
            oe.step()
            torch.cuda.synchronize()
            same(k)
    assert og.param_groups[0]["lr"] == oe.param_groups[0]["lr"] < kw["lr"]


EXACT = dict(lr=2.0 ** -9, betas=(0.875, 0.96875), eps=2.0 ** -27, weight_decay=2.0 ** -7)        # every value is an fp32 number


def _clone_params(params):
    return [torch.nn.Parameter(q.detach().clone()) for q in params]


@pytest.mark.gpu
def test_state_dict_resumes_bitwise_on_the_device():
    """After three steps the state_dict goes into a fresh FusedClipAdam on copies of the parameters: two more steps of the resumed run
    are bitwise equal to the uninterrupted one."""
    mtt_amd = _need_gpu()
    pa = _params(100)
    oa = mtt_amd.optim.FusedClipAdam(pa, lr=1e-3, weight_decay=1e-2, max_norm=2.0)
    for k in (1, 2, 3):
        for q, g in zip(pa, _grads(110 + k, 1e-2)):
            q.grad = g
        oa.step()
    pb = _clone_params(pa)
    ob = mtt_amd.optim.FusedClipAdam(pb, lr=1e-3, weight_decay=1e-2, max_norm=2.0)
    ob.load_state_dict(copy.deepcopy(oa.state_dict()))
    for k in (4, 5):
        for q, r, g in zip(pa, pb, _grads(110 + k, 1e-2 if k == 4 else 1e-3)):
            q.grad, r.grad = g, g.clone()
        na, nb = oa.step(), ob.step()
        assert torch.equal(na, nb)
        for q, r in zip(pa, pb):
            assert torch.equal(q.detach(), r.detach()), k
            for key in ("exp_avg", "exp_avg_sq", "step"):
                assert torch.equal(oa.state[q][key], ob.state[r][key]), (k, key)


def _torch_twin(opt, params, max_norm):
    """torch.optim.Adam on fp64 CPU copies of `params`, holding `opt`'s state (through state_dict / load_state_dict)."""
    twin = [torch.nn.Parameter(q.detach().double().cpu()) for q in params]
    ref = torch.optim.Adam(twin, **EXACT)
    ref.load_state_dict(copy.deepcopy(opt.state_dict()))
    for q, r in zip(params, twin):
        for key in ("exp_avg", "exp_avg_sq"):
            assert ref.state[r][key].dtype == torch.float64 and torch.equal(ref.state[r][key], opt.state[q][key].double().cpu()), key
        assert float(ref.state[r]["step"]) == float(opt.state[q]["step"])
    return twin, ref


def _step_against_torch(mtt_amd, rec, opt, params, twin, ref, grads, max_norm, label, step):
    """One step of FusedClipAdam and of clip_grad_norm_ + torch.optim.Adam from the SAME values, torch's result as the reference.
    torch keeps step_size and 1 / sqrt(bias_correction2) as doubles where the descriptor rounds each to fp32 once: two more roundings on
    the way to dp (one relative to dp, one relative to the denominator), none to m or v.  The gradients' norm is below max_norm: torch
    would clip by ITS fp64 norm, the kernel by the fp32 one (1e-5 apart), and the counts hold for one and the same coefficient only — the
    clipping formula is pinned to torch on the host, in fp64."""
    for q, r, g in zip(params, twin, grads):
        q.grad, r.grad = g, g.double().cpu()
    before = _snapshot(opt, params)
    norm = opt.step()
    n_ref = torch.nn.utils.clip_grad_norm_(twin, max_norm)
    ref.step()
    torch.cuda.synchronize()
    assert float(n_ref) < 0.5 * max_norm
    assert R.norm_need(float(norm), float(n_ref)) <= R.NORM_TOL
    worst = dict(m=0.0, v=0.0, dp=0.0)
    for q, r, g, (p0, m0, v0, t0) in zip(params, twin, grads, before):
        f = R.fields(max_norm=max_norm, t=t0 + 1, **EXACT)
        st = opt.state[q]
        assert float(st["step"]) == float(ref.state[r]["step"]) == t0 + 1
        need = R.judge(f, rec.last(), g, p0, m0, v0, q.detach(), st["exp_avg"], st["exp_avg_sq"],
                       ref=(r.detach(), ref.state[r]["exp_avg"], ref.state[r]["exp_avg_sq"]))
        for k, n in need.items():
            worst[k] = max(worst[k], n)
    extra = dict(dp=2)
    parity_util.report("optim_fused_clip_adam", case=label, step=step, need=worst, count={k: R.COUNT[k] + extra.get(k, 0) for k in R.COUNT})
    assert R.passes(worst, extra), (label, step, worst)


@pytest.mark.gpu
def test_state_interchange_with_torch_adam(monkeypatch):
    """FusedClipAdam's state after three steps goes into torch.optim.Adam on fp64 CPU copies (step 4 on both, judged), torch's state after
    that step goes back into a fresh FusedClipAdam on the device (moments cast to fp32 by the loader; step 5 against a torch twin of
    those values, judged).  Hyper-parameters that are exact in fp32, so that torch's doubles and the descriptor hold the same betas."""
    mtt_amd = _need_gpu()
    rec = _Totals(mtt_amd.ops.call)
    monkeypatch.setattr(mtt_amd.ops, "call", rec)
    max_norm = 2.0
    pa = _params(120)
    oa = mtt_amd.optim.FusedClipAdam(pa, max_norm=max_norm, **EXACT)
    for k in (1, 2, 3):
        for q, g in zip(pa, _grads(130 + k, 1e-2 if k == 1 else 1e-3)):
            q.grad = g
        oa.step()
    twin, ref = _torch_twin(oa, pa, max_norm)
    _step_against_torch(mtt_amd, rec, oa, pa, twin, ref, _grads(134, 1e-3), max_norm, "state_to_torch", 4)
    # ... and back: torch's fp64 state into a fresh FusedClipAdam
    pb = [torch.nn.Parameter(r.detach().float().cuda()) for r in twin]
    ob = mtt_amd.optim.FusedClipAdam(pb, max_norm=max_norm, **EXACT)
    ob.load_state_dict(copy.deepcopy(ref.state_dict()))
    for q, r in zip(pb, twin):
        for key in ("exp_avg", "exp_avg_sq"):
            got = ob.state[q][key]
            assert got.dtype == torch.float32 and got.is_cuda and torch.equal(got.cpu(), ref.state[r][key].float()), key
        assert float(ob.state[q]["step"]) == 4.0
    twin_b, ref_b = _torch_twin(ob, pb, max_norm)
    _step_against_torch(mtt_amd, rec, ob, pb, twin_b, ref_b, _grads(135, 1e-3), max_norm, "state_from_torch", 5)


@pytest.mark.gpu
def test_nan_gradient_is_reported_and_stays_in_its_element(monkeypatch):
    """One NaN element in one gradient.  The norm step() returns is not finite, so a caller can see it.  With a NaN norm the kernel's clamp
    `coef < 1 ? coef : 1` yields coef = 1 (torch's clip_grad_norm_ multiplies every gradient by NaN): only that element of p, m and v
    becomes NaN, every other element takes an UNCLIPPED Adam step, judged as such."""
    mtt_amd = _need_gpu()
    rec = _Totals(mtt_amd.ops.call)
    monkeypatch.setattr(mtt_amd.ops, "call", rec)
    params = _params(140)
    opt = mtt_amd.optim.FusedClipAdam(params, lr=1e-3, weight_decay=1e-2, max_norm=2.0)
    grads = _grads(141, 1.0)                                         # norm ~ 575: a finite norm would clip by ~0.0035
    which, pos = 7, 65535                                            # the last element of the exactly-one-chunk tensor
    grads[which][pos] = float("nan")
    for q, g in zip(params, grads):
        q.grad = g
    before, hy = _snapshot(opt, params), _hypers(opt, params)
    norm = opt.step()
    torch.cuda.synchronize()
    assert not math.isfinite(float(norm))
    assert math.isnan(rec.last())
    after = _snapshot(opt, params)
    worst = dict(m=0.0, v=0.0, dp=0.0)
    for i, (g, (p0, m0, v0, _), (p1, m1, v1, t1), h) in enumerate(zip(grads, before, after, hy)):
        skip = torch.zeros(g.numel(), dtype=torch.bool)
        if i == which:
            skip[pos] = True
        for x in (p1, m1, v1):
            assert torch.equal(~torch.isfinite(x).cpu(), skip), i      # non-finite exactly at the NaN's position
        f = R.fields(h["lr"], h["betas"], h["eps"], h["weight_decay"], opt.max_norm, t1)
        for k, n in R.judge(f, None, g, p0, m0, v0, p1, m1, v1, skip=skip).items():       # total_sq None: coef = 1
            worst[k] = max(worst[k], n)
    parity_util.report("optim_fused_clip_adam", case="nan_gradient", step=1, need=worst, count=R.COUNT)
    assert R.passes(worst), worst
