"""Host checks of tests/optim_ref.py: the fp64 reference is pinned to torch.optim.Adam + clip_grad_norm_, the CPU emulator of
mtt_grad_sqnorm / mtt_adam_step passes every case under the derived rounding counts, and the judge rejects planted defects (in the manner
of tests/test_parity_comparator.py).  tests/test_gpu_optim.py runs the same cases on the device."""
import math

import pytest
import torch

import optim_ref as R
from oracle import abi_emul

ADAM_SPECS = R.adam_specs()
SQNORM_SPECS = R.sqnorm_specs()
_BUILT = {}


def _case(name):
    """Cases are built once and never modified (run_adam / run_sqnorm work on copies)."""
    if name not in _BUILT:
        _BUILT[name] = R.build(next(s for s in ADAM_SPECS + SQNORM_SPECS if s["name"] == name))
    return _BUILT[name]


def _emulated(name):
    key = ("emu", name)
    if key not in _BUILT:
        _BUILT[key] = R.run_adam(_case(name), abi_emul.call)
    return _BUILT[key]


def test_reference_matches_torch_adam_in_fp64():
    """adam_ref + sumsq_ref vs clip_grad_norm_ + torch.optim.Adam on fp64 CPU parameters: three steps, the first one clipping,
    hyper-parameters that are exact in fp32, step_size and inv_sqrt_bc2 as doubles; 1e-12 relative on p, m and v."""
    lr, betas, eps, wd, max_norm = 2.0 ** -9, (0.875, 0.96875), 2.0 ** -27, 2.0 ** -7, 2.0
    gen = torch.Generator().manual_seed(5)
    shapes = [(1027,), (33, 17), (5,)]
    params = [torch.nn.Parameter(torch.randn(s, generator=gen, dtype=torch.float64)) for s in shapes]
    opt = torch.optim.Adam(params, lr=lr, betas=betas, eps=eps, weight_decay=wd)
    p = [q.detach().clone() for q in params]
    m = [torch.zeros_like(q) for q in p]
    v = [torch.zeros_like(q) for q in p]
    for t in (1, 2, 3):
        gs = [torch.randn(s, generator=gen, dtype=torch.float64) * (3.0 if t == 1 else 0.01) for s in shapes]
        for q, g in zip(params, gs):
            q.grad = g.clone()
        n_torch = float(torch.nn.utils.clip_grad_norm_(params, max_norm))
        opt.step()
        tsq = R.sumsq_ref(gs)
        assert abs(math.sqrt(tsq) - n_torch) <= 1e-12 * n_torch
        assert (math.sqrt(tsq) > max_norm) == (t == 1)                       # the first step clips, the others do not
        f = R.fields(lr, betas, eps, wd, max_norm, t, exact_step=True)
        assert (f["beta1"], f["beta2"], f["eps"], f["weight_decay"]) == (betas[0], betas[1], eps, wd)
        for i, q in enumerate(params):
            p[i], m[i], v[i] = R.adam_ref(f, tsq, gs[i], p[i], m[i], v[i])
            st = opt.state[q]
            for name, mine, ref in (("p", p[i], q.detach()), ("m", m[i], st["exp_avg"]), ("v", v[i], st["exp_avg_sq"])):
                err = float(((mine - ref).abs() / ref.abs().clamp_min(1e-300)).max())
                assert err <= 1e-12, (t, i, name, err)


def test_fields_are_the_fp32_descriptor_values():
    f = R.fields(1e-3, (0.9, 0.999), 1e-8, 0.1, 10.0, 3)
    assert f["beta2"] == R.f32(0.999) != 0.999 and f["omb2"] == 1.0 - R.f32(0.999)
    assert abs(f["omb2"] / 0.001 - 1.0 + 1.29e-5) < 1e-7                      # the rounded beta2 moves 1 - beta2 by -1.29e-5 relative
    assert f["step_size"] == R.f32(1e-3 / (1.0 - 0.9 ** 3)) and f["inv_sqrt_bc2"] == R.f32(1.0 / math.sqrt(1.0 - 0.999 ** 3))


@pytest.mark.parametrize("spec", ADAM_SPECS + SQNORM_SPECS, ids=lambda s: s["name"])
def test_layout_has_guards_and_the_chosen_alignment(spec):
    c = _case(spec["name"])
    for r in R.ROLES:
        end = 0
        for s, n in c.span[r]:
            assert s - end >= R.GUARD and s % 4 == spec["off"][r]
            end = s + n
        assert c.buf[r].numel() - end >= R.GUARD
    tab = c.tables()
    assert tab["n_chunks"] == sum(-(-n // R.CHUNK) for n in R.SIZES) == 13
    assert tab["numel"].tolist() == list(R.SIZES)


@pytest.mark.parametrize("spec", ADAM_SPECS, ids=lambda s: s["name"])
def test_emulator_passes_every_adam_case(spec):
    c = _case(spec["name"])
    need, bad = R.judge_case(c, _emulated(spec["name"]))
    assert not bad, bad
    assert R.passes(need), (need, R.COUNT)
    assert max(need.values()) <= 1.0, need                # fp64 arithmetic rounded once: within one rounding of the reference
    coef = R.clip_coef(c.fields(), c.total_sq())
    want = dict(clip=0.01, idle=1.0, null=1.0, eps=1.0).get(spec["regime"])
    if want is not None:
        assert abs(coef - want) <= 1e-3 * want, coef


def test_eps_regime_has_the_denominator_within_ten_of_eps():
    c = _case("eps_regime")
    f = c.fields()
    _, _, v1 = R.adam_ref(f, c.total_sq(), *(c.view(r, 7) for r in R.ROLES))
    ratio = (v1.sqrt() * f["inv_sqrt_bc2"] / f["eps"])
    inside = ((ratio > 0.1) & (ratio < 10.0)).double().mean()
    assert float(inside) > 0.85, float(inside)


def test_emulated_hyper_pair_equals_the_descriptor_fields():
    a, b = _emulated("aligned"), _emulated("hyper_pair")
    for r in R.ROLES:
        assert torch.equal(a.buf[r].view(torch.int32), b.buf[r].view(torch.int32)), r


@pytest.mark.parametrize("spec", SQNORM_SPECS, ids=lambda s: s["name"])
def test_emulator_passes_every_sqnorm_case(spec):
    c = _case(spec["name"])
    out, after = R.run_sqnorm(c, abi_emul.call)
    ref = 3.0 + R.sumsq_ref([c.view("g", i) for i in range(len(R.SIZES))])
    assert ref > 3.3                                                           # the pre-filled 3.0 is a visible share of the result
    assert R.norm_need(math.sqrt(out), math.sqrt(ref)) <= R.NORM_TOL
    assert R.norm_need(math.sqrt(out - 3.0), math.sqrt(ref)) > R.NORM_TOL      # an overwriting kernel would be seen
    assert not R.guards_intact(c, after)
    assert all(torch.equal(c.buf[r].view(torch.int32), after.buf[r].view(torch.int32)) for r in R.ROLES)


# ---------------------------------------------------------------------------------------------
# planted defects: the judge must fail each
# ---------------------------------------------------------------------------------------------
def _defective_formula(kind, f, tsq, g, p, m, v):
    """Adam with one deliberate error, fp64 -> (p', m', v')."""
    g, p, m, v = (x.double() for x in (g, p, m, v))
    coef = R.clip_coef(f, tsq)
    if kind == "coef_unclamped":
        coef = f["max_norm"] / (math.sqrt(tsq) + 1e-6)
    gh = coef * g + (0.0 if kind == "decay_dropped" else f["weight_decay"]) * p
    m1 = (f["beta2"] * m + f["omb2"] * gh) if kind == "beta2_for_m" else (f["beta1"] * m + f["omb1"] * gh)
    v1 = f["beta2"] * v + f["omb2"] * gh * gh
    isb = 1.0 if kind == "bias_correction_omitted" else f["inv_sqrt_bc2"]
    denom = (v1 * isb * isb + f["eps"]).sqrt() if kind == "eps_inside_sqrt" else v1.sqrt() * isb + f["eps"]
    return p - f["step_size"] * m1 / denom, m1, v1


FORMULA_DEFECTS = [("decay_dropped", "visible_decay"), ("beta2_for_m", "aligned"), ("eps_inside_sqrt", "eps_regime"),
                   ("bias_correction_omitted", "aligned"), ("coef_unclamped", "clip_idle")]


def _copy_of(after):
    c = after.to("cpu")
    c.buf = {r: b.clone() for r, b in after.buf.items()}
    return c


@pytest.mark.parametrize("kind,name", FORMULA_DEFECTS, ids=[k for k, _ in FORMULA_DEFECTS])
def test_judge_rejects_a_wrong_formula(kind, name):
    c = _case(name)
    bad = _copy_of(_emulated(name))
    for i in range(len(R.SIZES)):
        out = _defective_formula(kind, c.fields(), c.total_sq(), *(c.view(r, i) for r in R.ROLES))
        for r, x in zip(("p", "m", "v"), out):
            bad.view(r, i)[:] = x.float()
    need, guards = R.judge_case(c, bad)
    assert not guards
    assert not R.passes(need), (kind, need)
    # ... and in every tensor on its own, the 1-element one included
    for i in range(len(R.SIZES)):
        one = R.judge(c.fields(), c.total_sq(), *(c.view(r, i) for r in R.ROLES), *(bad.view(r, i) for r in ("p", "m", "v")))
        assert not R.passes(one), (kind, i, one)


@pytest.mark.parametrize("role", ["p", "m", "v"])
@pytest.mark.parametrize("tensor", [1, 3, 5, 8])                 # sizes 3, 5 (vector + tail), 1027, 65537 (one element into a second chunk)
def test_judge_rejects_a_tail_element_left_at_its_old_value(role, tensor):
    c = _case("aligned")
    bad = _copy_of(_emulated("aligned"))
    bad.view(role, tensor)[-1] = c.view(role, tensor)[-1]
    need, guards = R.judge_case(c, bad)
    assert not guards
    key = "dp" if role == "p" else role
    assert need[key] > R.COUNT[key], need
    assert all(need[k] <= R.COUNT[k] for k in need if k != key), need


@pytest.mark.parametrize("role", ["p", "m", "v"])
@pytest.mark.parametrize("where", ["before_first", "after_tail", "buffer_end"])
def test_judge_rejects_an_overwritten_sentinel(role, where):
    c = _case("aligned")
    bad = _copy_of(_emulated("aligned"))
    s, n = c.span[role][4]
    pos = {"before_first": c.span[role][0][0] - 1, "after_tail": s + n, "buffer_end": bad.buf[role].numel() - 1}[where]
    bad.buf[role][pos] = 0.0
    need, guards = R.judge_case(c, bad)
    assert R.passes(need) and len(guards) == 1 and guards[0].startswith(role), guards


def test_judge_rejects_a_written_gradient():
    c = _case("aligned")
    bad = _copy_of(_emulated("aligned"))
    bad.view("g", 6)[100] *= 1.0 + 2.0 ** -20
    assert R.guards_intact(c, bad) == ["g: the gradient buffer changed"]


def test_judge_rejects_the_emulators_former_second_moment():
    """Before it rounded the betas as the descriptor does, the emulator's exp_avg_sq was 1.3e-5 (relative, in the new term) off the device's."""
    c = _case("aligned")
    bad = _copy_of(_emulated("aligned"))
    for i in range(len(R.SIZES)):
        bad.view("v", i)[:] = (bad.view("v", i).double() * (1.0 - 1.3e-5)).float()
    need, _ = R.judge_case(c, bad)
    assert need["v"] > R.COUNT["v"] and need["m"] <= R.COUNT["m"] and need["dp"] <= R.COUNT["dp"], need
    # and the real thing: unrounded betas in the formula, zero starting moments (the first step, where the whole of v' is the new term)
    e = _case("eps_regime")
    f = dict(e.fields(), beta2=0.999, omb2=0.001)
    bad = _copy_of(_emulated("eps_regime"))
    for i in range(len(R.SIZES)):
        bad.view("v", i)[:] = R.adam_ref(f, e.total_sq(), *(e.view(r, i) for r in R.ROLES))[2].float()
    need, _ = R.judge_case(e, bad)
    assert need["v"] > R.COUNT["v"], need


def test_judge_rejects_non_finite_results():
    c = _case("aligned")
    bad = _copy_of(_emulated("aligned"))
    bad.view("m", 2)[1] = float("nan")
    need, _ = R.judge_case(c, bad)
    assert need["m"] == float("inf")
