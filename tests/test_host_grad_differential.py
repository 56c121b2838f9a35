"""CPU: the device-vs-emulator gradient check (train_check.device_vs_emulator + DIFF_PER_PARAM, run on the MI355X by
tests/test_gpu_grad_differential.py) has teeth.  The "device" leg here is the emulator itself with one injected kernel error; the oracle's
per-parameter bound of the bf16 backward (PER_PARAM["x3f"]) does not see either error, the differential bound names exactly the mutated
parameter."""
import pytest

import train_check
from oracle import abi_emul

OP_R = 1                         # MTT_OP_R: the token-major operand of a weight-gradient GEMM (reduction over the rows)


def _mutant(shape, which, edit):
    """abi_emul.call, except for the `which`-th weight-gradient gemm (a_op = MTT_OP_R) whose output is `shape`: its descriptor goes through
    `edit` first.  -> (call, hits: the K of every mutated call)"""
    hits, seen = [], [0]

    def call(n, **kw):
        if n == "gemm" and kw.get("a_op") == OP_R and tuple(kw["D"].shape[-2:]) == shape:
            if which is None or seen[0] == which:
                hits.append(kw["K"])
                kw = edit(dict(kw))
            seen[0] += 1
        return abi_emul.call(n, **kw)
    return call, hits


def _scale(kw):                  # (a) the weight gradient 10 % too large
    kw["alpha"] = kw.get("alpha", 1.0) * 1.10
    return kw


def _drop_k_tail(kw):            # (b) the reduction's ragged tail (rows past the last whole 8-row chunk) never accumulated
    kw["K"] = kw["K"] // 8 * 8
    return kw


def test_emulator_against_itself_is_exact():
    r = train_check.device_vs_emulator("taskprompter", "mini_ctr", "x3f", "cpu", call=abi_emul.call)
    assert all(v == 0.0 for v in r.fwd.values()), r.fwd
    assert r.errs and all(v.err == 0.0 for v in r.errs.values())
    assert r.census and sum(r.census.values()) > 0 and 8 in r.census, r.census
    train_check.assert_diff_per_param(r.errs, "x3f")


@pytest.mark.parametrize("shape,which,edit,mutated", [
    # every weight-gradient call of the patch embedding (one: its [128, 3 * 16 * 16] shape is unique in the model)
    ((128, 768), None, _scale, "backbone.patch_embed.proj.weight"),
    # the first qkv weight gradient of the backward = the last encoder block's; K = 2 x 30 tokens = 60, a ragged tail of 4 rows
    ((384, 128), 0, _drop_k_tail, "backbone.blocks.3.attn.qkv.weight"),
], ids=["wgrad_scaled_1.1", "wgrad_k_tail_dropped"])
def test_differential_bound_catches_what_the_oracle_bound_misses(shape, which, edit, mutated):
    call, hits = _mutant(shape, which, edit)
    r = train_check.device_vs_emulator("taskprompter", "mini_ctr", "x3f", "cpu", call=call)
    assert len(hits) == 1 and (edit is _scale or hits[0] % 8), hits
    # the hole: the oracle's bound of the bf16 backward passes the mutant
    train_check.assert_per_param(r.oracle_errs, "x3f")
    # the differential bound fails, naming exactly the mutated parameter
    bad, checked, below = train_check.diff_violations(r.errs, "x3f")
    assert [k for k, *_ in bad] == [mutated], bad
    with pytest.raises(AssertionError):
        train_check.assert_diff_per_param(r.errs, "x3f")


@pytest.mark.parametrize("family,name,task", [("taskprompter", "mini_ctr", "semseg"), ("invpt", "mini8", "depth")])
@pytest.mark.parametrize("prec", ["x3", "x3f"])
def test_partial_loss_gradients_on_emulator(family, name, task, prec):
    """Only one head in the loss: the backward nodes that see no gradient for the other heads (set_materialize_grads(False) hands them None)
    must still give the oracle's gradients, and no gradient where the oracle has none."""
    r = train_check.device_vs_emulator(family, name, prec, "cpu", call=abi_emul.call, tasks=(task,))
    assert r.dead and not any(task in k for k in r.dead if "fea_fuse" in k or "heads" in k), r.dead[:5]
    assert max(r.fwd_oracle.values()) < 5e-5, r.fwd_oracle
    if prec == "x3":
        worst, med = train_check.summarize(r.oracle_errs)
        assert worst[0] < 1e-3, worst
    else:
        train_check.assert_per_param(r.oracle_errs, "x3f")
