"""-m gpu: one training step on the MI355X against the SAME step on the exact emulator (oracle/abi_emul.py: the kernels' operand rounding,
fp64 sums), per parameter, with no cosine escape (train_check.DIFF_PER_PARAM).  The oracle bound of the bf16-arithmetic backward
(train_check.PER_PARAM) has to allow bf16-vs-fp32 differences and so lets a gradient scaled by 1.1 through; this one does not
(tests/test_host_grad_differential.py proves both on injected errors).

Every leg also declares the GEMM kernels (mtt_gemm_variant codes) its device step must reach, and the recorded census must contain them: a
leg whose calls quietly fall back to the general kernel fails instead of testing nothing.  Across the file the census covers
0 (general), 3 (DMA 256), 4 (DMA 128), 6 (gemm_tn weight gradients), 8 / 9 (split planes, ring3 / its 3x3 conv form), 11 (f32n) and
12 (ringc 3x3 conv).

Not run here: the bf16 mode.  A per-op replay of the bf16 step (every call's inputs replayed on the emulator) showed attn_fwd / attn_bwd
as the only ops whose outputs differed in a third of their elements: the flash kernels take P (and dS) as bf16 MFMA operands.  The
emulator now restates that.  The bf16 forward heads then measured 8.8e-3 - 1.2e-2 against the emulator (1.2e-2 - 2.1e-2 against the
oracle) and the worst gradient 1.6e-2 (mini_win) to 0.37 (mini8), median 1e-2 - 0.1: still bf16-noise-sized, so a differential bound
under the 2e-2 ceiling is not possible until the remaining difference is found.  bf16 gradients stay on the oracle bound
(tests/test_gpu_train.py, tests/test_gpu_fullsize.py); the kernels of the bf16 legs (3, 4, 6, 12) are reached here by the x3f legs, whose
backward is the same bf16 arithmetic.

TaskPrompter-Swin x3f: named per-parameter allowances, train_check.DIFF_ALLOW.

Not run here: InvPT (`mini8`) at PITCH32_FROM = 33.  Its training path needs decoder widths that are their own channel pitch
(invpt_autograd._check8: 56 -> 64 is refused with NotImplementedError), so the wide-pitch leg of InvPT is the forward only
(tests/test_gpu_model.py under MTT_TEST_PITCH32_FROM); the wide-pitch gradient leg runs on `mini_ctr`."""
import pytest
import torch

import parity_util as pu
import train_check

pytestmark = pytest.mark.gpu

FWD_TOL = {"x3": 5e-5, "x3f": 5e-5}

TP = ["mini_ctr", "mini_win", "mini_deconv", "mini_p32", "mini_skip"]
# (family, config, mode, gemm_variant, pitch32_from, tasks) -> GEMM variants the device step must resolve calls to (derived from the
# census of each leg: mtt_gemm_variant is a pure host function of the descriptor)
LEGS = {}
for _n in TP:
    LEGS[("taskprompter", _n, "x3", None, None, None)] = {0}
    LEGS[("taskprompter", _n, "x3f", None, None, None)] = {0, 8} | ({11} if _n in ("mini_ctr", "mini_deconv") else set()) | ({9} if _n == "mini_p32" else set())
LEGS.update({
    ("invpt", "mini8", "x3f", None, None, None): {0, 4, 8, 9},
    ("swin", "mini_swin", "x3f", None, None, None): {0, 8, 11},
    ("swin", "mini_swin_pad", "x3f", None, None, None): {0, 8, 11},
    ("swin", "mini_swin", "x3f", 1, None, None): {0, 8},
    ("swin", "mini_swin", "x3f", 3, None, None): {3, 6, 8},
    ("swin", "mini_swin", "x3f", 4, None, None): {4, 8},
    # forced kernels (ops.GEMM_VARIANT: every call that leaves its descriptor at AUTO); 1 = the general kernel everywhere it applies
    ("taskprompter", "mini_ctr", "x3f", 1, None, None): {0, 8},
    ("taskprompter", "mini_ctr", "x3f", 3, None, None): {3, 6, 8},
    ("taskprompter", "mini_ctr", "x3f", 4, None, None): {4, 8},
    ("invpt", "mini8", "x3f", 1, None, None): {0, 8, 9},
    ("invpt", "mini8", "x3f", 3, None, None): {3, 6, 8, 9, 12},
    ("invpt", "mini8", "x3f", 4, None, None): {4, 8, 9},
    # every ragged channel count of the miniature on the multiple-of-32 pitch (44 -> 64, 52 -> 64): the split-plane 3x3 conv (9) joins
    ("taskprompter", "mini_ctr", "x3f", None, 33, None): {0, 8, 9, 11},
    # partial losses: one head in the loss, the other heads' parameters get no gradient on either side
    ("taskprompter", "mini_ctr", "x3f", None, None, ("semseg",)): {0, 8, 11},
    ("invpt", "mini8", "x3f", None, None, ("depth",)): {0, 4, 8, 9},
})


def _leg_id(leg):
    family, name, mode, variant, pitch, tasks = leg
    return "-".join([name, mode] + ([f"v{variant}"] if variant else []) + ([f"p{pitch}"] if pitch else []) + (list(tasks) if tasks else []))


@pytest.mark.parametrize("leg", list(LEGS), ids=[_leg_id(k) for k in LEGS])
def test_gradients_match_the_emulator(leg, monkeypatch):
    import mtt_amd
    family, name, mode, variant, pitch, tasks = leg
    torch.manual_seed(0)
    seen = []
    inner = mtt_amd.ops.call
    call = lambda n, **kw: (seen.append((n, kw.get("mfma"))), inner(n, **kw))[1]
    key = ()
    if family == "swin":
        # the switches of test_host_cpu.check_swin_x3f_split_planes: the miniature takes Swin-B's split-plane stage Linears / task features
        # and the matrix-core window attention (mtt_winattn_desc.mfma)
        monkeypatch.setattr(mtt_amd.autograd_path, "AUTO_SPLIT_MIN_ROWS", 64)
        key = ("split_min_rows", 64)
    r = train_check.device_vs_emulator(family, name, mode, "cuda:0", gemm_variant=variant, pitch32_from=pitch, tasks=tasks, call=call, key=key)
    rel = sorted(train_check.rel_errors({k: v for k, v in r.errs.items()
                                         if v.ref / v.numel ** 0.5 >= train_check.DIFF_PER_PARAM[mode]["floor"] *
                                         max(e.ref / e.numel ** 0.5 for e in r.errs.values())}).items(), key=lambda kv: -kv[1])
    pu.report("grad_diff", config=name, family=family, mode=mode, gemm_variant=variant, pitch32_from=pitch, tasks=tasks,
              fwd_worst=max(r.fwd.values()), fwd_oracle_worst=max(r.fwd_oracle.values()),
              worst=rel[0], p90=rel[len(rel) // 10][1], median=rel[len(rel) // 2][1], checked=len(rel), dead=len(r.dead),
              rel_max=train_check.DIFF_PER_PARAM[mode]["rel_max"], oracle_worst=_oracle_worst(r.oracle_errs),
              census={str(k): v for k, v in sorted(r.census.items())})
    assert max(r.fwd.values()) <= FWD_TOL[mode], r.fwd
    train_check.assert_diff_per_param(r.errs, mode, name)
    assert LEGS[leg] <= set(r.census), (LEGS[leg], r.census)
    assert all(v >= 0 for v in r.census), r.census
    if family == "swin":
        assert all(m == 1 for n, m in seen if n in ("winattn_fwd", "winattn_bwd")) and any(n == "winattn_bwd" for n, _ in seen)
    if tasks is not None:
        assert r.dead, "a partial loss leaves the other heads' parameters without a gradient"


def _oracle_worst(oerrs):
    """(worst relative error vs the oracle, parameter) over the parameters above PER_PARAM's floor"""
    rms = {k: v.ref / v.numel ** 0.5 for k, v in oerrs.items()}
    top = max(rms.values())
    return max(((v.err / v.ref, k) for k, v in oerrs.items() if rms[k] >= train_check.PER_PARAM["x3f"]["floor"] * top), default=None)
