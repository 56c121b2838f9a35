"""Reference, judge and cases of the fused clip + Adam entry points (mtt_grad_sqnorm, mtt_adam_step; optim.FusedClipAdam).

REFERENCE.  `adam_ref` is torch.optim.Adam (L2 weight decay added to the gradient, bias-corrected moments, no amsgrad) after
clip_grad_norm_, in fp64, written from those two formulas:

    coef = min(1, max_norm / (sqrt(total_sq) + 1e-6))            (1 when max_norm <= 0 or there is no total_sq)
    g^   = coef * g + wd * p
    m'   = b1 * m + (1 - b1) * g^
    v'   = b2 * v + (1 - b2) * g^ ** 2
    p'   = p - step_size * m' / (sqrt(v') * inv_sqrt_bc2 + eps)

`fields()` gives the scalars AS THE DESCRIPTOR HOLDS THEM (mtt_adam_desc: fp32), each rounded to fp32 and 1 - b formed from the rounded
b, so that only the rounding of the arithmetic separates a correct kernel from the reference.  tests/test_optim_host.py pins `adam_ref`
to torch.optim.Adam + clip_grad_norm_ on fp64 parameters (1e-12 relative).

JUDGE.  Per element |got - ref| <= count * 2^-24 * scale, the scale being the element's OWN magnitude sum (never the tensor's rms:
the update of p is 1e-3 of p, an rms bound cannot see it).  u = 2^-24 bounds the relative error of one fp32 rounding.  The counts are
the number of fp32 roundings on the way to each output in a straightforward fp32 evaluation of the formula above, every operation
rounded once, division and square root correctly rounded; a compiler that contracts a multiply and an add into an fma removes
roundings and never adds one.  First order in u (the second-order terms are below 1e-5 of the bound).

    coef   sqrt(total_sq), + 1e-6, max_norm / (.)                                         3      relative, of coef
    g^     coef * g (1), + wd * p (1; one rounding if fused, counted as one for the sum)   3 + 2 = 5
           relative to G = |coef * g| + |wd * p|.  G, not |g^|: the two terms may cancel, and the error of the sum stays
           proportional to the terms.  Without decay, or with terms of one sign, G = |g^|.
    m'     1 - b1 (1: exact only for b1 >= 0.5), (1 - b1) * g^ (1), b1 * m + (.) (1)         5 + 3 = 8
           relative to Sm = b1 |m| + (1 - b1) G: the g^ errors enter through the second term only, the last rounding is of the sum.
    v'     g^ ** 2 doubles g^'s 5; 1 - b2 (1), two products (2), b2 * v + (.) (1)           10 + 4 = 14
           relative to Sv = b2 v + (1 - b2) G ** 2.
    dp     dp = p' - p = -step_size * m' / denom, denom = sqrt(v') * inv_sqrt_bc2 + eps:
           m' (8); sqrt halves v' (7) and rounds (1); * inv_sqrt_bc2 (1); + eps (1): all three relative to denom or less, its terms
           are positive; m' / denom (1); step_size * (.) (1)                                8 + 7 + 5 = 20
           relative to Sp = step_size * Sm / denom, plus the final rounding of p' itself: half an ulp of p'.
           (The v share assumes Sv / v' = 1, true unless the two terms of g^ cancel.  Where they do, the share is
           |dp| * 5 u G / |g^| with |dp| <= step_size * (b1 |m| + (1 - b1) |g^|) / denom: still within 7 u Sp when m = v = 0, and when v
           is of the order of G ** 2 or more.  The cases start both moments at zero or v at the gradient's scale.)

COUNT = dict(m=8, v=14, dp=20).  `judge` also returns, per output, the smallest count that would have passed (the "need").

NORM.  |n - n_ref| <= 1e-5 * n_ref.  Depth of the fp32 summation: at most 256 additions per lane (64 float4 of a 65536-element chunk,
4 additions each), 9 in the workgroup (6 wave levels + 3), ceil(chunks / 256) + 8 in the second stage, one to accumulate into out_sq:
at most 256 + 9 + 9 + 1 = 275 roundings for up to 256 chunks, halved by the square root: 138 u = 8.2e-6.  More than 256 chunks need
their own count; no case here has more than 16.

GUARDS.  `build` carves every gradient, parameter and moment tensor of a case out of ONE flat fp32 buffer per role, with at least
GUARD sentinel floats (a NaN bit pattern) between neighbours and at both ends and a start offset per role (floats past a 16-byte
boundary).  `guards_intact` compares the sentinels bitwise; the gradient buffer must be bitwise unchanged as a whole.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
COUNT = dict(m=8, v=14, dp=20)
NORM_TOL = 1e-5
CHUNK = 65536                     # mtt_adam_chunk(); the device module asserts that the library agrees
SIZES = (1, 3, 4, 5, 255, 1027, 65535, 65536, 65537, 131073)
GUARD = 8
SENTINEL_BITS = 0x7FC5A5A5        # a quiet NaN: a kernel that READS a guard poisons its result as well
ROLES = ("g", "p", "m", "v")


def f32(x):
    return float(np.float32(x))


def fields(lr, betas, eps, weight_decay, max_norm, t, exact_step=False):
    """The scalars of one launch as mtt_adam_desc holds them (fp32 values, as Python floats); `t` is the step count AFTER this step.
    exact_step: step_size and inv_sqrt_bc2 stay doubles (the torch pin)."""
    b1, b2 = betas
    step_size, isb = lr / (1.0 - b1 ** t), 1.0 / math.sqrt(1.0 - b2 ** t)
    r1, r2 = f32(b1), f32(b2)
    return dict(max_norm=f32(max_norm), step_size=step_size if exact_step else f32(step_size),
                inv_sqrt_bc2=isb if exact_step else f32(isb), beta1=r1, beta2=r2, omb1=1.0 - r1, omb2=1.0 - r2,
                eps=f32(eps), weight_decay=f32(weight_decay))


def sumsq_ref(gs):
    """fp64 sum of squares of a list of tensors."""
    return float(sum(float(g.detach().double().cpu().square().sum()) for g in gs))


def clip_coef(f, total_sq):
    if f["max_norm"] > 0 and total_sq is not None:
        return min(1.0, f["max_norm"] / (math.sqrt(float(total_sq)) + 1e-6))
    return 1.0


def _parts(f, total_sq, g, p, m, v):
    g, p, m, v = (x.detach().double().cpu() for x in (g, p, m, v))
    coef = clip_coef(f, total_sq)
    cg, dp = coef * g, f["weight_decay"] * p
    gh = cg + dp
    m1 = f["beta1"] * m + f["omb1"] * gh
    v1 = f["beta2"] * v + f["omb2"] * gh * gh
    denom = v1.sqrt() * f["inv_sqrt_bc2"] + f["eps"]
    p1 = p - f["step_size"] * m1 / denom
    G = cg.abs() + dp.abs()
    Sm = f["beta1"] * m.abs() + f["omb1"] * G
    Sv = f["beta2"] * v + f["omb2"] * G * G
    return p1, m1, v1, dict(Sm=Sm, Sv=Sv, Sp=f["step_size"] * Sm / denom, p0=p)


def adam_ref(f, total_sq, g, p, m, v):
    """-> (p', m', v') in fp64.  f: fields(); total_sq: the sum of squares the clip coefficient is formed from (None: no clipping)."""
    return _parts(f, total_sq, g, p, m, v)[:3]


def _ulp32(x):
    """Spacing of fp32 numbers at |x| (fp64 tensor), normal range."""
    _, e = torch.frexp(x.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(x), e - 24)


def _need(d, scale, slack=None):
    """Smallest count with d <= count * U * scale (+ slack) everywhere; inf where got is not finite or a zero scale is missed."""
    if slack is not None:
        d = (d - slack).clamp_min(0)
    r = torch.where(d == 0, torch.zeros_like(d), d / (U * scale))          # 0 / 0 -> 0, x / 0 -> inf
    r = torch.where(torch.isfinite(d), r, torch.full_like(r, float("inf")))
    return float(r.max()) if r.numel() else 0.0


def judge(f, total_sq, g, p0, m0, v0, got_p, got_m, got_v, ref=None, skip=None):
    """One tensor.  -> dict(m=need, v=need, dp=need): passes iff need[k] <= COUNT[k] for every k.
    ref: (p', m', v') of another fp64 implementation (torch.optim.Adam) to judge against instead of adam_ref, under the same scales;
    skip: bool mask of elements that are not judged."""
    p1, m1, v1, s = _parts(f, total_sq, g, p0, m0, v0)
    if ref is not None:
        p1, m1, v1 = (x.detach().double().cpu().reshape(p1.shape) for x in ref)
    got_p, got_m, got_v = (x.detach().double().cpu() for x in (got_p, got_m, got_v))
    if skip is not None:
        keep = ~skip
        p1, m1, v1, got_p, got_m, got_v = (x[keep] for x in (p1, m1, v1, got_p, got_m, got_v))
        s = {k: x[keep] for k, x in s.items()}
    half_ulp = 0.5 * _ulp32(p1.abs() + COUNT["dp"] * U * s["Sp"])
    return dict(m=_need((got_m - m1).abs(), s["Sm"]), v=_need((got_v - v1).abs(), s["Sv"]),
                dp=_need(((got_p - s["p0"]) - (p1 - s["p0"])).abs(), s["Sp"], half_ulp))


def judge_many(f, total_sq, tensors):
    """tensors: iterable of (g, p0, m0, v0, got_p, got_m, got_v).  -> worst need per output over all of them."""
    worst = dict(m=0.0, v=0.0, dp=0.0)
    for t in tensors:
        for k, n in judge(f, total_sq, *t).items():
            worst[k] = max(worst[k], n)
    return worst


def passes(need, extra=None):
    """extra: further roundings per output that a comparison adds by its construction (stated where it is used)."""
    return all(need[k] <= COUNT[k] + (extra or {}).get(k, 0) for k in COUNT)


def norm_need(n, n_ref):
    """|n - n_ref| / n_ref (inf if n is not finite); passes iff <= NORM_TOL."""
    n, n_ref = float(n), float(n_ref)
    return abs(n - n_ref) / n_ref if math.isfinite(n) else float("inf")


# ---------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------
HYPER = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8)


def _spec(name, regime, off=(0, 0, 0, 0), hyper=False, wd=1e-2, t=3, seed=0):
    return dict(name=name, regime=regime, off=dict(zip(ROLES, off)), hyper=hyper, wd=wd, t=t, seed=seed)


def adam_specs():
    """Every mtt_adam_step case: the regimes (all roles 16-byte aligned), then exactly one role 4 / 8 / 12 bytes past a 16-byte boundary."""
    specs = [_spec("aligned", "base"), _spec("clip_engaged", "clip"), _spec("clip_idle", "idle"), _spec("no_clip_null_total", "null"),
             _spec("visible_decay", "decay", wd=0.1), _spec("eps_regime", "eps", wd=0.0, t=1), _spec("cancelling_moments", "cancel", wd=0.0),
             _spec("hyper_pair", "base", hyper=True)]
    for i, role in enumerate(ROLES):
        for k in (1, 2, 3):
            off = [0, 0, 0, 0]
            off[i] = k
            specs.append(_spec(f"misaligned_{role}_{4 * k}B", "base", off=tuple(off), seed=1 + 3 * i + k))
    return specs


def sqnorm_specs():
    return [_spec(f"sqnorm_g_{4 * k}B", "base", off=(k, 0, 0, 0), seed=20 + k) for k in (0, 1, 2, 3)]


class Case:
    """buf[role]: the flat fp32 buffer; span[role]: [(start, n)] per tensor; everything on the CPU until `.to(device)`."""

    def view(self, role, i, buf=None):
        s, n = self.span[role][i]
        return (self.buf if buf is None else buf)[role][s:s + n]

    def to(self, device):
        c = Case()
        c.__dict__.update(self.__dict__)
        c.buf = {r: b.to(device).contiguous() for r, b in self.buf.items()}
        c.total = None if self.total is None else self.total.to(device)
        c.hyper = None if self.hyper is None else self.hyper.to(device)
        return c

    def tables(self):
        """Pointer / numel / chunk tables as FusedClipAdam._group_tables builds them, on the buffers' device."""
        dev = self.buf["g"].device
        ct, co = [], []
        for i, n in enumerate(SIZES):
            for o in range(0, n, CHUNK):
                ct.append(i)
                co.append(o)
        tab = {}
        for role, key in zip(ROLES, ("grads", "params", "exp_avg", "exp_avg_sq")):
            base = self.buf[role].data_ptr()
            assert base % 16 == 0, "the role buffers must start on a 16-byte boundary"
            addr = [base + 4 * s for s, _ in self.span[role]]
            assert all(a % 16 == 4 * self.spec["off"][role] for a in addr)
            tab[key] = torch.from_numpy(np.array(addr, dtype=np.int64)).to(dev)
        tab.update(numel=torch.tensor(SIZES, dtype=torch.int64, device=dev), chunk_tensor=torch.tensor(ct, dtype=torch.int32, device=dev),
                   chunk_off=torch.tensor(co, dtype=torch.int64, device=dev), n_chunks=len(ct))
        return tab

    def adam_kw(self):
        h = dict(HYPER, weight_decay=self.spec["wd"])
        b1, b2 = h["betas"]
        t = self.spec["t"]
        step_size, isb = h["lr"] / (1.0 - b1 ** t), 1.0 / math.sqrt(1.0 - b2 ** t)
        if self.hyper is not None:                   # the pair replaces the fields: a kernel that still read them would take these
            step_size, isb = 7.0, 0.5
        return dict(hyper=self.hyper, max_norm=self.max_norm, step_size=step_size, beta1=b1, beta2=b2, eps=h["eps"],
                    weight_decay=h["weight_decay"], inv_sqrt_bc2=isb, xargs=[self.total], **self.tables())

    def fields(self):
        return fields(HYPER["lr"], HYPER["betas"], HYPER["eps"], self.spec["wd"], self.max_norm, self.spec["t"])

    def total_sq(self):
        return None if self.total is None else float(self.total.cpu()[0])


def _layout(off):
    """[(start, n)] per tensor and the buffer length: >= GUARD sentinels before, between and after; start = off mod 4 floats."""
    spans, pos = [], 0
    for n in SIZES:
        start = (pos + GUARD + 3) // 4 * 4 + off
        spans.append((start, n))
        pos = start + n
    return spans, pos + GUARD + 4


def sentinel(n):
    return torch.full((n,), SENTINEL_BITS, dtype=torch.int32).view(torch.float32)


def build(spec):
    """The case on the CPU.  Regimes: base (clip engaged at ~0.17, small decay, moments of the gradient's sign and scale), clip (coef ~0.01),
    idle (norm below max_norm, |p| ~ 1e-3 so that the update is not hidden below the ulp of p), null (max_norm 0, NULL total_sq), decay (wd 0.1, |p| ~ |g|), eps (g ~ 1e-8, zero moments, first step:
    sqrt(v') * inv_sqrt_bc2 = |g| ~ eps), cancel (b1 * m ~ -(1 - b1) * g)."""
    c = Case()
    c.spec, c.span, c.buf = spec, {}, {}
    gen = torch.Generator().manual_seed(1000 + spec["seed"])
    regime = spec["regime"]
    gs = {"base": 1e-2, "clip": 1.0, "idle": 1e-2, "null": 1e-2, "decay": 1.0, "eps": 1e-8, "cancel": 1e-2}[regime]
    vals = {r: [] for r in ROLES}
    for n in SIZES:
        g = torch.randn(n, generator=gen) * gs
        p = torch.randn(n, generator=gen) * (1e-3 if regime == "idle" else 1.0)      # idle: |dp| ~ |p|, far above the ulp of p
        if regime == "eps":
            m, v = torch.zeros(n), torch.zeros(n)
        elif regime == "cancel":
            m = -g * (0.1 / 0.9) * (0.9 + 0.2 * torch.rand(n, generator=gen))
            v = g * g * (0.5 + torch.rand(n, generator=gen))
        else:
            m = g * (0.5 + torch.rand(n, generator=gen))
            v = (gs * gs) * (0.5 + torch.rand(n, generator=gen))
        for r, x in zip(ROLES, (g, p, m, v)):
            vals[r].append(x.float())
    for r in ROLES:
        c.span[r], length = _layout(spec["off"][r])
        buf = sentinel(length).clone()
        for (s, n), x in zip(c.span[r], vals[r]):
            buf[s:s + n] = x
        c.buf[r] = buf
    sq = np.float32(sumsq_ref(vals["g"]))
    norm = math.sqrt(float(sq))
    c.max_norm = {"base": norm * 0.17, "clip": norm * 0.01, "idle": norm * 4.0, "null": 0.0, "decay": norm * 0.5, "eps": 0.0,
                  "cancel": norm * 0.5}[regime]
    c.total = None if regime == "null" else torch.tensor([float(sq)], dtype=torch.float32)
    c.hyper = None
    if spec["hyper"]:                           # the pair the descriptor fields would carry
        c.hyper = torch.tensor([HYPER["lr"] / (1.0 - HYPER["betas"][0] ** spec["t"]), 1.0 / math.sqrt(1.0 - HYPER["betas"][1] ** spec["t"])],
                               dtype=torch.float32)
    return c


def guards_intact(before, after):
    """before / after: Case (any device).  -> list of violations: a sentinel that changed (bitwise) or a changed gradient buffer."""
    bad = []
    for r in ROLES:
        b, a = before.buf[r].cpu().view(torch.int32), after.buf[r].cpu().view(torch.int32)
        mask = torch.ones(b.numel(), dtype=torch.bool)
        for s, n in before.span[r]:
            mask[s:s + n] = False
        assert bool((b[mask] == SENTINEL_BITS).all())
        if not torch.equal(a[mask], b[mask]):
            bad.append(f"{r}: sentinel at float {int(torch.nonzero(mask & (a != b))[0])} overwritten")
    if not torch.equal(before.buf["g"].cpu().view(torch.int32), after.buf["g"].cpu().view(torch.int32)):
        bad.append("g: the gradient buffer changed")
    return bad


def run_adam(case, call):
    """Run mtt_adam_step of `case` through `call` (ops.call or abi_emul.call) on a copy of its buffers -> the Case after the call."""
    after = case.to(case.buf["g"].device)
    after.buf = {r: b.clone() for r, b in case.buf.items()}
    call("adam_step", **after.adam_kw())
    return after


def judge_case(case, after):
    """-> (worst need per output over the case's tensors, guard violations)."""
    f, tsq = case.fields(), case.total_sq()
    need = judge_many(f, tsq, ((case.view("g", i), case.view("p", i), case.view("m", i), case.view("v", i),
                               after.view("p", i), after.view("m", i), after.view("v", i)) for i in range(len(SIZES))))
    return need, guards_intact(case, after)


def run_sqnorm(case, call, prefill=3.0):
    """mtt_grad_sqnorm of `case` with out_sq pre-filled -> (out_sq after, the Case after the call)."""
    after = case.to(case.buf["g"].device)
    after.buf = {r: b.clone() for r, b in case.buf.items()}
    dev = after.buf["g"].device
    out = torch.full((1,), prefill, dtype=torch.float32, device=dev)
    ws = torch.full((64,), float("nan"), dtype=torch.float32, device=dev)        # scratch: n_chunks partials, fully written before they are read
    tab = after.tables()
    assert tab["n_chunks"] <= ws.numel()
    call("grad_sqnorm", ws=ws, xargs=[out], max_norm=0.0, step_size=0.0, beta1=0.0, beta2=0.0, eps=0.0, weight_decay=0.0, inv_sqrt_bc2=0.0, **tab)
    return float(out.cpu()[0]), after
