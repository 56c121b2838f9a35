"""Host tests of the call recorder (tests/replay_util.py), no GPU: every leg that tests/test_gpu_replay.py replays on the device is
recorded here too, and each snapshot, re-run through the emulator, must reproduce bit for bit what the original call wrote (so it
captured every input and the aliasing) and pass the comparator with a zero worst element.  Every recorded entry is replayed or is in
the closed list NOT_REPLAYABLE; every replayed call has a tolerance derived from the hand-written cases; and the comparator still
fails the planted defects D1 - D4 at those derived tolerances (the body of tests/test_parity_comparator.py over the replayed calls of
one leg)."""
import pytest
import torch

import gpu_cases
import replay_util as ru
import test_parity_comparator as tpc
from oracle import abi_emul


def _host_replay(s):
    """Re-run a snapshot through the emulator on two copies -> what gpu_cases.compare takes, the second copy standing in for the device"""
    kw, store = s.fresh()
    kw_d, store_d = s.fresh()
    pre = {gpu_cases.skey(f): f.clone() for f in store.values()}
    with abi_emul.tracking() as written:
        abi_emul.call(s.entry, **kw)
    abi_emul.call(s.entry, **kw_d)
    emu = {gpu_cases.skey(f): f for f in store.values()}
    dev = {gpu_cases.skey(store[k]): store_d[k] for k in store}
    skip = {gpu_cases.skey(t) for _, t in gpu_cases._arg_tensors(kw) if getattr(t, "_mtt_scratch", False)}
    return kw, store, pre, emu, written, dev, skip


@pytest.mark.parametrize("leg", list(ru.LEGS))
def test_leg_is_closed_and_self_consistent(leg):
    rec = ru.record_leg(leg)
    assert rec.snaps, "nothing recorded"
    # closure: every call the leg made belongs to a snapshotted signature or to an entry of the closed exclusion list
    replayed = {s.entry for s in rec.snaps}
    assert set(rec.entries) == replayed | set(rec.not_replayed()), set(rec.entries) - replayed
    assert {s.sig for s in rec.snaps} == set(rec.signatures)
    bad = []
    for s in rec.snaps:
        tol = ru.tolerance(s.entry, s.kw)
        if tol is None:
            bad.append((s.entry, s.site, "no precision class", ru.precision_class(s.entry, s.kw, any(ru.split_outputs(s.entry, s.kw)))))
            continue
        kw, store, pre, emu, written, dev, skip = _host_replay(s)
        if {gpu_cases.skey(store[k]) for k in s.written} != set(written) - skip:
            bad.append((s.entry, s.site, "the replay writes other storages than the call did"))
            continue
        for k, m in s.written.items():
            f = store[k]
            if not torch.equal(written[gpu_cases.skey(f)], m) or not torch.equal(gpu_cases._bits(f[m]), gpu_cases._bits(s.wrote[k])):
                bad.append((s.entry, s.site, "the replay does not reproduce what the call wrote"))
                break
        else:
            r = gpu_cases.compare(kw, tol, pre, emu, written, dev, skip, None, True)
            if not r["ok"] or r["errs"]["worst_elem"][0] != 0.0 or r["errs"]["worst_norm"] != 0.0:
                bad.append((s.entry, s.site, r["errs"]))
    assert not bad, bad
    nomatch = sum(ru.matching_case(s.sig) is None for s in rec.snaps)
    print(f"replay {leg}: {sum(rec.entries.values())} calls, {len(rec.snaps)} signatures, {nomatch} without an exactly matching hand-written case")


def test_a_recording_does_not_depend_on_uninitialised_memory():
    """two recordings of one leg, the allocator's free blocks filled with other values in between, give bitwise the same snapshots: what the
    product allocates with torch.empty and no kernel writes (pitch padding of an output) would otherwise differ from run to run, and sit
    in the norm of the storage the device is judged on.  torch's allocation functions are back in place afterwards."""
    empties = [torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty]
    recs = []
    for fill in (3.0e7, -5.0e9):
        junk = [torch.full((1 << 18,), fill) for _ in range(8)] + [torch.full((n,), fill) for n in (64, 512, 4096, 32768) for _ in range(16)]
        del junk
        recs.append(ru.record_leg("invpt-mini-bf16-eval"))
    a, b = recs
    assert [s.sig for s in a.snaps] == [s.sig for s in b.snaps]
    for s, t in zip(a.snaps, b.snaps):
        sa, sb = s.fresh()[1], t.fresh()[1]
        assert len(sa) == len(sb)
        for x, y in zip(sa.values(), sb.values()):
            assert torch.equal(gpu_cases._bits(x), gpu_cases._bits(y)), (s.entry, s.site)
    assert empties == [torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty]


def test_exclusion_list_is_closed():
    """NOT_REPLAYABLE is exactly the pointer-table entries, each checked on the device by a test of its own"""
    assert set(ru.NOT_REPLAYABLE) == {"adam_step", "grad_sqnorm", "segcopy"}
    assert set(ru.NOT_REPLAYABLE) <= set(gpu_cases.COVERED_ELSEWHERE)


@pytest.mark.parametrize("prec", ["x3f", "bf16"])
def test_det_train_leg_launches_the_real_criterion(prec):
    """the 3ddet train legs run _DetLossFn on the head's outputs: fcos3d_loss_fwd and fcos3d_loss_bwd are recorded once each, with one
    image unlabelled and more than 20 positive points"""
    rec = ru.record_leg(f"det_head-mini-{prec}-train")
    assert rec.entries["fcos3d_loss_fwd"] == 1 and rec.entries["fcos3d_loss_bwd"] == 1
    fwd = next(s for s in rec.snaps if s.entry == "fcos3d_loss_fwd")
    kw, _ = fwd.fresh()
    assert kw["B"] == 2 and kw["n_lab"] == 1
    abi_emul.call("fcos3d_loss_fwd", **kw)
    assert float(kw["stats"][0]) > 20, float(kw["stats"][0])
    assert "fcos3d_loss_fwd" not in ru.record_leg(f"det_head-mini-{prec}-eval").entries
    # positives on every level, so that the first (kept) call of every backward signature carries a gradient: no snapshot of the leg writes
    # only zeros, and none reads an all-zero gradient
    lab = kw["label"].view(-1)
    lo = 0
    for l in range(kw["nlev"]):
        n = kw["H"][l] * kw["W"][l]
        assert int((lab[lo:lo + n] < kw["C"]).sum()) > 0, f"no positive on level {l}"
        lo += n
    for s in rec.snaps:
        assert s.wrote and all(bool(v.double().abs().max() > 0) for v in s.wrote.values() if v.numel()), f"{s.entry} at {s.site} writes only zeros"
        if s.entry.endswith("_bwd"):
            skw, _ = s.fresh()
            for name in ("dy", "dout", "dcol", "gout"):
                if isinstance(skw.get(name), torch.Tensor):
                    assert bool(skw[name].double().abs().max() > 0), f"{s.entry} at {s.site}: {name} is all zero"


def test_workspace_table_covers_the_scratch_arguments_of_the_cases():
    for cname, entry, kw, _ in tpc.CASES:
        for lbl, t in gpu_cases._arg_tensors(kw):
            if getattr(t, "_mtt_scratch", False):
                assert lbl in ru.WORKSPACE_ARGS.get(entry, ()), (cname, lbl)
    for entry in gpu_cases.WS_QUERY:
        assert "ws" in ru.WORKSPACE_ARGS[entry], entry


def test_signature_separates_configurations_not_sizes():
    g = torch.Generator().manual_seed(0)

    def gemm(M, N, K, adt, ddt, **extra):
        kw = dict(A=gpu_cases.rnd(g, M, K, dtype=gpu_cases.DT[adt]), B=gpu_cases.rnd(g, N, K, dtype=torch.bfloat16),
                  D=torch.full((M, N), 7.0, dtype=gpu_cases.DT[ddt]), M=M, N=N, K=K, a_op=0, b_op=0, a_dtype=adt, b_dtype=1, d_dtype=ddt, prec=0,
                  lda=K, ldb=K, ldd=N, batch=1, batch_inner=1, alpha=1.0)
        kw.update(extra)
        return kw
    base = ru.signature("gemm", gemm(64, 64, 64, 1, 1))
    assert base == ru.signature("gemm", gemm(72, 64, 64, 1, 1, resid=None, variant=0))            # a size, an absent pointer
    others = [gemm(64, 64, 64, 0, 1), gemm(64, 64, 64, 1, 0), gemm(64, 64, 64, 1, 1, act=1), gemm(64, 64, 64, 1, 1, colshift=torch.zeros(64)),
              gemm(64, 64, 64, 1, 1, d_mb=32, d_bs=32 * 64), gemm(64, 64, 64, 1, 1, batch=2, batch_inner=2), gemm(64, 64, 64, 1, 1, variant=4)]
    sigs = {ru.signature("gemm", kw) for kw in others}
    assert len(sigs) == len(others) and base not in sigs


def test_tolerances_come_from_the_hand_written_cases():
    """every hand-written case is in a class whose merged bound is at least its own, and equal to it where the class has one bound"""
    classes = {}
    for cname, entry, kw, tol in tpc.CASES:
        t = ru.tolerance(entry, kw)
        assert t is not None, cname
        for k in ("f32", "bf16", "split"):
            assert (k in t) >= (k in tol) and (k not in tol or t[k] >= tol[k]), (cname, k)
        if "elem" in tol:
            assert t["elem"] >= tol["elem"], cname
        assert [tuple(p) for p in t.get("split_pairs", ())] == [tuple(p) for p in tol.get("split_pairs", ())], cname
        assert t.get("split_args") == tol.get("split_args"), cname
        key = ru.precision_class(entry, kw, "split_pairs" in tol or "split_args" in tol)
        classes.setdefault(key, []).append((tol, t))
    for key, lst in classes.items():
        for k in ("f32", "bf16"):
            assert lst[0][1][k] == max(tol[k] for tol, _ in lst), (key, k)
    assert ru.tolerance("gemm", dict(prec=1, A=torch.zeros(2, dtype=torch.float64))) is None


def test_comparator_fails_planted_defects_over_the_replayed_calls():
    """D1 - D4 and the one-ulp moves of tests/test_parity_comparator.py over the calls of one training step (mini_ctr, x3f), at the derived
    tolerances: a class merged too loose to see a wrong element fails here.  No output storage keeps a zero outside the written set unless
    the snapshot names it as read."""
    rec = ru.record_leg(ru.PLANTED_LEG)
    unrefilled = {}
    for i, s in enumerate(rec.snaps):
        names = {}
        for lbl, t in gpu_cases._arg_tensors(s.kw):
            names.setdefault(gpu_cases.skey(t), lbl)
        slack = {names[k]: v for k, v in ru.allowance(s).items()}
        # only the named zero-sum outputs have an allowance (and D1 enlarged by it): everywhere else D1 must fail at the class bound alone
        assert all((s.entry, lbl) in ru.ZERO_SUM_OUTPUTS for lbl in slack), (s.entry, slack)
        tpc.check_comparator(f"{s.entry}#{i}({s.site})", s.entry, s.kw, ru.tolerance(s.entry, s.kw), zeros_allowed=s.unrefilled, slack_of=slack,
                             split_moves=False)
        if s.unrefilled:
            unrefilled[f"{s.entry}#{i}({s.site})"] = s.unrefilled
    print(f"replay {ru.PLANTED_LEG}: zeros left in place because the emulator reads them: {unrefilled or 'none'}")
