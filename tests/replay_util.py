"""Replay of the product's own kernel calls through the device parity suite.  `record` runs a piece of the product on the CPU with
every C-ABI call forwarded to the emulator (oracle/abi_emul.py) and snapshots the first call of each distinct `signature` (the kernel
configuration: dtypes, optional pointers, layouts, epilogue pieces, row groups, batches, the GEMM kernel the library would dispatch) on
fresh storages with the call's own sharing, views and pitches.  Each snapshot is a parity case: gpu_cases.run_case judges it on the
device against the emulator (tests/test_gpu_replay.py), with the bound the hand-written cases of the same precision class set
(`tolerance`).  tests/test_replay_host.py checks the recorder itself without a GPU.  LEGS names what is recorded: one training step
(the second, after the optimizer ran) and one eval forward of every miniature, per arithmetic mode.

What a snapshot changes about the call: workspaces (WORKSPACE_ARGS) are marked as scratch, and a zero outside the emulator's written set
of a storage the emulator writes becomes the sentinel 7.0 where the emulator's outputs do not depend on it (a stray zero-write would be
invisible on a zero); positions it does depend on keep their value and are counted in Snapshot.unrefilled.  Memory the product leaves
uninitialised (torch.empty) reads as zero while recording, so that a snapshot is the same in every run; a NaN or a value from 2^64 that
no call writes is replaced like a zero all the same."""
import collections
import contextlib
import functools
import os
import traceback

import torch

import conftest
import gpu_cases
import mtt_amd
from oracle import abi_emul, configs, weights  # noqa: F401

SENTINEL = 7.0

# entry points whose arguments carry raw addresses inside tensors: a host snapshot cannot be re-run on the device (each has its own device
# test, gpu_cases.COVERED_ELSEWHERE)
NOT_REPLAYABLE = {
    "adam_step": "the gradient / parameter / moment tables are int64 tensors of raw addresses",
    "grad_sqnorm": "the gradient table is an int64 tensor of raw addresses",
    "segcopy": "the segment table is an int64 tensor of raw source and destination addresses",
}
# int64 tensor arguments that are data (indices, labels), not addresses: every other int64 argument of a recorded call is refused
INT64_DATA = {"nms_bev": {"args[4]"}, "detloss_fwd": {"target"}, "detloss_bwd": {"target"}}

# which argument of which entry is a kernel workspace (contents unspecified before and after the call; the emulator ignores it): labels
# as gpu_cases._arg_tensors gives them.  The entries of gpu_cases.WS_QUERY get a workspace of run_case's own on the device.
WORKSPACE_ARGS = {
    "gemm": {"colsum_ws"}, "layernorm_bwd": {"ws"}, "chan_logits": {"ws"}, "modulate_bwd": {"xargs[4]"}, "ctr_dw": {"xargs[2]"},
    "rowscale_cast_colsum": {"args[12]"}, "bn_stats": {"xargs[0]"}, "bn_bwd_reduce": {"xargs[0]"}, "colsum": {"args[6]"},
    "colsum_batched": {"args[9]"}, "detloss_fwd": {"ws"}, "attn_msg_bwd": {"xargs[5]"}, "chanattn_bwd": {"xargs[5]"},
    "loss_label_stats": {"ws"}, "loss_fwd": {"ws"}, "nms_bev": {"args[6]"},
    "groupnorm_fwd": {"ws"}, "groupnorm_bwd": {"ws"}, "dcn_col2im_bwd": {"ws"}, "fcos_bbox_post_bwd": {"ws"},
    "fcos3d_targets": {"ws"}, "fcos3d_loss_fwd": {"ws"}, "fcos3d_loss_bwd": {"ws"},       # (the assignment and the backward take a ws and do not use it)
}

# enum-like descriptor fields (0 = absent) and the enum-like positions of the positional entry points
ENUM_FIELDS = {"a_op", "b_op", "prec", "act", "a_act", "store_mode", "kind", "out_nchw", "fused", "accumulate", "dtype", "g_dtype", "mfma",
               "relu", "bbox2d", "mask_sigmoid", "wmode", "skip_neg", "stride", "variant"}
POS_ENUMS = {"cast2d": (6, 7, 8), "pixshuf2": (8, 9), "colsum": (5,), "colsum_batched": (5,), "add_rows": (6,), "rowscale_cast": (6, 7),
             "rowscale_cast_colsum": (6, 7), "patchify16": (5,), "patchify": (7,), "nms_bev": (3,)}
POS_FLAGS = {"rowscale_cast": (9, 10), "rowscale_cast_colsum": (9, 10)}          # sizes that switch a path on when > 0 (row groups, prompt rows)
FLAG_FIELDS = {"a_mb": "rowgroups(A)", "d_mb": "rowgroups(D)", "r_mb": "rowgroups(resid)", "n_prompt": "n_prompt>0", "T": "T>0",
               "skip_mb": "rowgroups(skip)"}


def _dt(t):
    return str(t.dtype).replace("torch.", "")


def signature(entry, kw):
    """The kernel configuration of a call, for de-duplication: entry, dtype of every tensor argument (so also which optional pointers are
    there), the enum-like fields that are not zero, conv.dil / conv.flip, whether row groups / an inner batch / prompt rows are on, and for
    mtt_gemm the kernel the library dispatches these fields to (a host query) in place of the `variant` request."""
    parts = [entry]
    for lk in ("args", "xargs"):
        for i, a in enumerate(kw.get(lk) or ()):
            if isinstance(a, torch.Tensor):
                parts.append((f"{lk}[{i}]", _dt(a)))
            elif lk == "args" and a is not None and i in POS_ENUMS.get(entry, ()):
                parts.append((f"{lk}[{i}]", int(a)))
            elif lk == "args" and a is not None and i in POS_FLAGS.get(entry, ()) and a > 0:
                parts.append((f"{lk}[{i}]", ">0"))
    for k in sorted(kw):
        v = kw[k]
        if k in ("args", "xargs") or v is None:
            continue
        if isinstance(v, torch.Tensor):
            parts.append((k, _dt(v)))
        elif isinstance(v, (list, tuple)):
            ts = tuple(_dt(a) for a in v if isinstance(a, torch.Tensor))
            if ts:
                parts.append((k, ts))
        elif k == "conv":
            if kw.get("a_op") in (gpu_cases.OP_CONV_K, gpu_cases.OP_CONV_R) or kw.get("b_op") in (gpu_cases.OP_CONV_K, gpu_cases.OP_CONV_R):
                parts.append(("conv", int(v.get("dil", 1)), int(v.get("flip", 0))))
        elif isinstance(v, bool) or not isinstance(v, int):
            continue
        elif k in FLAG_FIELDS:
            if v > 0:
                parts.append(FLAG_FIELDS[k])
        elif k == "batch_inner":
            if v > 1:
                parts.append("batch_inner>1")
        elif k == "variant" and entry == "gemm":
            continue
        elif (k in ENUM_FIELDS or k.endswith("_dtype")) and v != 0:
            parts.append((k, v))
    if entry == "gemm":
        parts.append(("kernel", mtt_amd._lib.gemm_variant(**kw)))
    return tuple(parts)


def _site():
    pkg = os.path.join(conftest.ROOT, "multi-task-transformer_amd")
    for fr in reversed(traceback.extract_stack()[:-3]):
        if fr.filename.startswith(pkg):
            return f"{os.path.basename(fr.filename)}:{fr.lineno}"
    return "?"


class Snapshot:
    """One recorded call as a parity case.  kw: the arguments on fresh storages (refilled, workspaces marked); written / wrote: {storage key
    of kw: mask of the positions the original call wrote / the bytes it wrote there}; refilled: zeros replaced by the sentinel;
    unrefilled: {argument label: count} of zeros left in place because the emulator's outputs depend on them."""

    def __init__(self, entry, sig, kw, written, wrote, refilled, unrefilled, site):
        self.entry, self.sig, self.kw, self.written, self.wrote = entry, sig, kw, written, wrote
        self.refilled, self.unrefilled, self.site = refilled, unrefilled, site

    def fresh(self):
        """(a copy of the arguments on storages of their own, {storage key of self.kw: the copy's flat storage})"""
        return gpu_cases.clone_storages(self.kw)


class Recording:
    def __init__(self):
        self.snaps, self.entries, self.signatures = [], collections.Counter(), collections.Counter()

    def not_replayed(self):
        return sorted(e for e in self.entries if e in NOT_REPLAYABLE)


def _check_no_addresses(entry, kw):
    for lbl, t in gpu_cases._arg_tensors(kw):
        if t.dtype == torch.int64 and lbl not in INT64_DATA.get(entry, ()):
            raise AssertionError(f"{entry}: {lbl} is an int64 tensor: if it holds raw addresses the entry belongs in NOT_REPLAYABLE, "
                                 f"if it holds data, in INT64_DATA")


def _workspace_keys():
    ops = mtt_amd.ops
    return {gpu_cases.skey(b) for b in list(ops._ws_cache.values()) + list(ops._ws_retired)}


def _snapshot(entry, sig, kw, forward):
    """Snapshot the arguments, forward the call itself (under write tracking), then refill the snapshot's stray zeros."""
    labels = gpu_cases._arg_tensors(kw)
    ws_keys = _workspace_keys()
    for lbl, t in labels:
        if gpu_cases.skey(t) in ws_keys and lbl not in WORKSPACE_ARGS.get(entry, ()):
            raise AssertionError(f"{entry}: {lbl} is the product's kernel workspace but WORKSPACE_ARGS does not list it")
    snap_kw, store = gpu_cases.clone_storages(kw)
    for lbl, t in gpu_cases._arg_tensors(snap_kw):
        if lbl in WORKSPACE_ARGS.get(entry, ()):
            t._mtt_scratch = True
    skip = {gpu_cases.skey(t) for _, t in gpu_cases._arg_tensors(snap_kw) if getattr(t, "_mtt_scratch", False)}
    live = {}
    for _, t in labels:
        live.setdefault(gpu_cases.skey(t), abi_emul.flat(t)[0])
    with abi_emul.tracking() as tracked:
        forward(entry, **kw)
    flats = {gpu_cases.skey(f): f for f in store.values()}
    written, wrote = {}, {}
    for okey, m in tracked.items():
        k = gpu_cases.skey(store[okey])
        if k in skip:
            continue
        written[k] = m.clone()
        wrote[k] = live[okey][m].clone()
    names = {}
    for lbl, t in gpu_cases._arg_tensors(snap_kw):
        names.setdefault(gpu_cases.skey(t), lbl)
    cand = {k: ((flats[k] == 0) | (flats[k].abs() >= 2.0 ** 64 if flats[k].is_floating_point() else False)) & ~m for k, m in written.items()}
    # uninitialised memory (torch.empty) the call never writes: a NaN there fails compare's finiteness check, and a value of 2^64 in an output
    # storage drowns its norm-wise error
    for k, f in flats.items():
        if k not in skip and f.is_floating_point():
            junk = ~torch.isfinite(f) & ~written.get(k, torch.zeros(f.numel(), dtype=torch.bool))
            cand[k] = cand[k] | junk if k in cand else junk
    cand = {k: z for k, z in cand.items() if z.any()}
    refilled, unrefilled = 0, {}
    if cand:
        def harmless(keys):
            trial, tstore = gpu_cases.clone_storages(snap_kw)
            for k in keys:
                tstore[k][cand[k]] = SENTINEL
            abi_emul.call(entry, **trial)
            return all(torch.equal(gpu_cases._bits(tstore[k][m]), gpu_cases._bits(wrote[k])) for k, m in written.items())
        keys = list(cand)
        ok = keys if harmless(keys) else [k for k in keys if harmless([k])]
        if ok != keys and len(ok) > 1 and not harmless(ok):
            ok = []
        for k in keys:
            if k in ok:
                flats[k][cand[k]] = SENTINEL
                refilled += int(cand[k].sum())
            else:
                unrefilled[names[k]] = int(cand[k].sum())
    return Snapshot(entry, sig, snap_kw, written, wrote, refilled, unrefilled, _site())


def record(run, keep_per_signature=1, warmup=None, forward=None):
    """Run `run(state)` with mtt_amd.ops.call forwarded to the emulator (`forward`, default abi_emul.call) and snapshot the first
    `keep_per_signature` calls of every signature.  warmup: run first under the same routing without recording; what it returns is
    `state`.  Returns a Recording (snaps, entries: calls per entry, signatures: calls per signature)."""
    ops = mtt_amd.ops
    forward = forward or abi_emul.call
    rec = Recording()
    on = [False]

    def call(entry, **kw):
        if ops.GEMM_VARIANT is not None and entry == "gemm" and not kw.get("variant"):
            kw["variant"] = ops.GEMM_VARIANT
        if not on[0]:
            return forward(entry, **kw)
        rec.entries[entry] += 1
        if entry in NOT_REPLAYABLE:
            return forward(entry, **kw)
        _check_no_addresses(entry, kw)
        sig = signature(entry, kw)
        rec.signatures[sig] += 1
        if rec.signatures[sig] > keep_per_signature:
            return forward(entry, **kw)
        rec.snaps.append(_snapshot(entry, sig, kw, forward))

    saved = ops.call
    ops.call = call
    ops.clear_pack_cache()
    try:
        with _zeroed_empty() if keep_per_signature > 0 else contextlib.nullcontext():          # only a snapshot needs it (launch_census.py)
            state = warmup() if warmup is not None else None
            on[0] = True
            run(state)
    finally:
        ops.call = saved
        ops.clear_pack_cache()
    return rec


class _zeroed_empty:
    """While recording, memory the product allocates without initialising it (torch.empty and its kin) reads as zero: what no kernel
    writes (pitch padding of an output) is then the same in every run, so a snapshot and the errors measured on it are reproducible, and
    in an output storage it falls under the sentinel refill like any other zero."""
    NAMES = ((torch, "empty"), (torch, "empty_like"), (torch, "empty_strided"), (torch.Tensor, "new_empty"))

    def __enter__(self):
        self.saved = [(o, n, getattr(o, n)) for o, n in self.NAMES]
        for o, n, f in self.saved:
            setattr(o, n, (lambda f: lambda *a, **k: f(*a, **k).zero_())(f))

    def __exit__(self, *exc):
        for o, n, f in self.saved:
            setattr(o, n, f)


# ---- tolerances: from the hand-written cases of the same precision class -------------------------------------------------------------------
# fields besides `prec` and the dtypes that put a call into a rounding regime of its own in the hand-written cases: column sums of rounded
# values (TOL_CS), the matrix-core window attention (TOL_WINATTN_BWD_MFMA), the flash / plain attention forward
CLASS_FIELDS = {"gemm": ("colsum_out",), "winattn_fwd": ("mfma",), "winattn_bwd": ("mfma",), "attn_fwd": ("variant",), "attn_bwd": ("variant",)}


@functools.lru_cache(maxsize=None)
def _case_tables():
    """({precision class: merged tolerance}, {entry: split-plane output pairs}, {signature: case name}) of gpu_cases.all_cases()"""
    pairs = collections.defaultdict(set)
    cases = gpu_cases.all_cases()
    for _, entry, kw, tol in cases:
        for p in tol.get("split_pairs", ()):
            pairs[entry].add(tuple(p))
        if "split_args" in tol:
            pairs[entry].add(("args",) + tuple(tol["split_args"]))
    groups, sigs = collections.defaultdict(list), {}
    for cname, entry, kw, tol in cases:
        groups[precision_class(entry, kw, "split_pairs" in tol or "split_args" in tol)].append(tol)
        sigs.setdefault(signature(entry, kw), cname)
    merged = {}
    for key, tols in groups.items():
        t = dict(f32=max(c["f32"] for c in tols), bf16=max(c["bf16"] for c in tols))
        if any("split" in c for c in tols):
            t["split"] = max(c["split"] for c in tols if "split" in c)
        if any("elem" in c for c in tols):
            t["elem"] = max(c.get("elem", 10 * c["f32"]) for c in tols)
        merged[key] = t
    return merged, dict(pairs), sigs


def precision_class(entry, kw, split_out):
    """(entry, prec, the storage dtypes of the floating-point arguments, the CLASS_FIELDS that are set, split-plane output)"""
    dts = frozenset(_dt(t) for _, t in gpu_cases._arg_tensors(kw) if t.is_floating_point() and not getattr(t, "_mtt_scratch", False))
    extra = tuple(k for k in CLASS_FIELDS.get(entry, ()) if kw.get(k) is not None and not (isinstance(kw.get(k), int) and kw.get(k) == 0))
    return (entry, kw.get("prec") or 0, dts, extra, bool(split_out))


def split_outputs(entry, kw):
    """(split_pairs, split_args) of a call: the hi / lo output planes the hand-written cases of the entry name, where the call has them"""
    pairs, args = [], None
    for p in _case_tables()[1].get(entry, ()):
        if p[0] == "args":
            args = (p[1], p[2])
        elif isinstance(kw.get(p[1]), torch.Tensor):
            pairs.append(p)
    return pairs, args


def tolerance(entry, kw):
    """The bound of a replayed call: the loosest f32 / bf16 / split / elem among the hand-written cases of its precision class (the split
    pairs are the call's own).  None when no hand-written case defines the class."""
    pairs, args = split_outputs(entry, kw)
    t = _case_tables()[0].get(precision_class(entry, kw, bool(pairs) or args is not None))
    if t is None:
        return None
    t = dict(t)
    if pairs:
        t["split_pairs"] = pairs
    if args is not None:
        t["split_args"] = args
    return t


def matching_case(sig):
    """name of a hand-written case with exactly this signature, or None"""
    return _case_tables()[2].get(sig)


# ---- the legs ---------------------------------------------------------------------------------------------------------------------------------
def _model_leg(family, name, prec, mode, pitch32=None, drop=False):
    import train_check
    from tests.golden.make_golden import loss_of
    ops = mtt_amd.ops

    def go():
        cfg, sd, x, strict = train_check._family_setup(family, name, 0)
        model = conftest.build_product_model(cfg, prec, "cpu", drop_path_rate=0.3 if drop else 0.0)
        model.load_state_dict(sd, strict=strict)
        if drop:            # the masks of test_host_cpu.test_training_with_injected_droppath_masks
            g = torch.Generator().manual_seed(3)
            model.backbone._drop_override = [(torch.bernoulli(torch.full((4, 2), 0.6), generator=g) / 0.6) for _ in range(4)]
        if mode == "eval":
            model.eval()

            def run(_):
                with torch.no_grad():
                    model(x)
            return record(run)
        model.train()
        opt = mtt_amd.optim.FusedClipAdam(model.parameters(), lr=1e-4, max_norm=10.0)

        def step(_=None):
            opt.zero_grad()
            out = model(x)
            sel = {k: v for k, v in out.items() if k != "inter_preds"}
            if "inter_preds" in out:
                sel["inter_preds"] = dict(out["inter_preds"])
            loss_of(sel).backward()
            opt.step()
        return record(step, warmup=step)          # the second step is the steady state (packs rebuilt after the optimizer ran)

    if pitch32 is None:
        return go()
    saved = ops.PITCH32_FROM
    ops.clear_pack_cache()
    ops.PITCH32_FROM = pitch32
    try:
        return go()
    finally:
        ops.PITCH32_FROM = saved
        ops.clear_pack_cache()


DET_LEVELS = ((32, 12, 20), (48, 6, 10), (64, 3, 5), (64, 3, 5))      # the level maps of tests/test_gpu_det_head.py


DET_GTS, DET_LABEL_SEED = 8, 3


def _det_leg(prec, mode):
    import det_ref
    head = mtt_amd.det_head.FCOS3DHead(**det_ref.mini_head_params())
    det_ref.randomize(head, 0)
    head.set_prec(prec)
    g = torch.Generator().manual_seed(5)
    feats = [torch.randn(2, c, h, w, generator=g) for c, h, w in DET_LEVELS]
    # the train legs run the real criterion on the head's outputs (cs parameters, the strides of img_ds_ratio 0.75: a 128 x 213 image over
    # the 12 x 20 level); image 1 is unlabelled, DET_LABEL_SEED gives num_pos > 20 (tests/test_replay_host.py asserts it)
    dm = mtt_amd.det_model
    crit = dm.configure_3ddet({"IMAGE_ORI_SIZE": (1024, 2048), "TRAIN": {"SCALE": (1024, 2048)}, "img_ds_ratio": 0.75})["detmodel"]
    labels = dm.synthetic_det_labels(2, (128, 213), DET_GTS, unlabelled=(1,), seed=DET_LABEL_SEED)
    # synthetic_det_labels draws boxes below level 0's range end, so every positive would sit on level 0 and the head's backward would see
    # all-zero gradients on the other levels (whose kernels run first, and the recorder keeps the first call of a signature).  One more gt
    # per higher level, a box around the image centre whose half size is 8 px past the level's range start, puts positives on every level
    e, c = labels["det_labels"][0], torch.tensor([106.0, 64.0])
    half = torch.tensor([[float(r[0]) + 8.0] for r in crit.regress_ranges[1:]])
    n = half.shape[0]
    e["bbox_modal"] = torch.cat([e["bbox_modal"], torch.cat([c - half, c + half], 1)])
    e["center_I"] = torch.cat([e["center_I"], torch.cat([c.expand(n, 2), torch.full((n, 1), 20.0)], 1)])
    e["label"] = torch.cat([e["label"], torch.arange(n) % crit.num_classes])
    for k in ("center_S", "size_S", "rotation_S"):
        e[k] = torch.cat([e[k], e[k][:n] * 0.5 + 0.25])
    labels["det_label_number"][0] += n

    def run(_):
        if mode == "eval":
            head.eval()
            with torch.no_grad():
                head(feats)
        else:
            maps = [m.contiguous() for lst in head(feats) for m in lst]
            sizes = [tuple(m.shape[-2:]) for m in maps[:len(maps) // 4]]
            dm._DetLossFn.apply(crit, crit.pack_labels(labels, "cpu"), crit._geometry(sizes), *maps)[8].backward()
    return record(run)


def _legs():
    legs = {}
    for fam, names in (("taskprompter", ("mini_ctr", "mini_win", "mini_deconv", "mini_p32", "mini_skip")), ("invpt", ("mini", "mini8")),
                       ("swin", ("mini_swin", "mini_swin_pad", "mini_swin_sp"))):
        for name in names:
            for prec in ("x3f", "bf16") + (("x3",) if name == "mini_ctr" else ()):
                for mode in ("train", "eval"):
                    if (fam, name, mode) == ("invpt", "mini", "train"):
                        continue          # the InvPT training path refuses widths that are not their own channel pitch (_check8): mini8 trains
                    legs[f"{fam}-{name}-{prec}-{mode}"] = functools.partial(_model_leg, fam, name, prec, mode)
    legs["taskprompter-mini_ctr-x3f-train-pitch32"] = functools.partial(_model_leg, "taskprompter", "mini_ctr", "x3f", "train", pitch32=33)
    legs["taskprompter-mini_ctr-x3f-train-droppath"] = functools.partial(_model_leg, "taskprompter", "mini_ctr", "x3f", "train", drop=True)
    for prec in ("x3f", "bf16"):
        for mode in ("train", "eval"):
            legs[f"det_head-mini-{prec}-{mode}"] = functools.partial(_det_leg, prec, mode)
    return legs


LEGS = _legs()
PLANTED_LEG = "taskprompter-mini_ctr-x3f-train"


def record_leg(leg):
    return LEGS[leg]()


# ---- conditioning ---------------------------------------------------------------------------------------------------------------------------------
# The comparator bounds an error by the size of the output (coef * rms of the emulator's values).  The models' own data makes a few
# outputs ill-conditioned: the bias gradient in front of a train-mode BatchNorm or of a softmax is a column sum that is zero in exact
# arithmetic, so what the emulator's fp64 leaves is the residue of the inputs' own rounding, and any fp32 summation is "wrong" by many
# times that.  A backward-stable fp32 kernel is exact for inputs moved by a few fp32 roundings, so the emulator is asked how far its
# output moves under one: every value it reads is scaled by 1 +- 2^-24 (half an fp32 ulp, random signs); the unit is the rms of that
# movement over the written set, less the movement that is only the output's own fp32 quantisation (2^-23 of its rms): zero for a
# well-conditioned call.  Only the outputs named here get an allowance, of so many units on top of both bounds of their class; every
# other replayed call is judged at its class bound alone.  The need is the smallest number of units with which every replayed call of
# the entry passes on the MI355X (all legs); the coefficient is at most twice that.
ZERO_SUM_OUTPUTS = {
    # (entry, output label): (units allowed, why the output can be a zero sum)
    ("colsum_batched", "args[1]"): (16.0, "the bias gradient of a Linear / conv in front of a train-mode BatchNorm or a softmax over the summed "
                                          "axis: need 11.33 units (per element; 1.9 norm-wise), mini_ctr x3 train"),
    ("attn_msg_bwd", "xargs[4]"): (6.0, "dbias of fuse_attn, whose output feeds a softmax over the keys, summed over all of them: need 3.51 units "
                                        "(per element; 2.5 norm-wise), InvPT mini8 x3f train"),
}


def sensitivity(s):
    """{storage key of s.kw: one unit of allowance per written element} for the outputs of Snapshot s that ZERO_SUM_OUTPUTS names"""
    names = {}
    for lbl, t in gpu_cases._arg_tensors(s.kw):
        names.setdefault(gpu_cases.skey(t), lbl)
    named = {k for k in s.written if (s.entry, names[k]) in ZERO_SUM_OUTPUTS}
    if not named:
        return {}
    kw1, st1 = s.fresh()
    kw2, st2 = s.fresh()
    abi_emul.call(s.entry, **kw1)
    g = torch.Generator().manual_seed(len(s.entry))
    rd = abi_emul._rd

    def noisy(t, idx, valid=None):
        v = rd(t, idx, valid)
        return v * (1.0 + 2.0 ** -24 * (2.0 * torch.bernoulli(torch.full(v.shape, 0.5, dtype=torch.float64), generator=g) - 1.0))
    abi_emul._rd = noisy
    try:
        abi_emul.call(s.entry, **kw2)
    finally:
        abi_emul._rd = rd
    out = {}
    for k in named:
        m = s.written[k]
        assert st1[k].dtype == torch.float32, (s.entry, names[k])
        if not m.any():
            continue
        e = st1[k][m].double()
        move = float((e - st2[k][m].double()).square().mean().sqrt())
        excess = move - 2.0 ** -23 * float(e.square().mean().sqrt())
        if excess > 0:
            out[k] = excess
    return out


def allowance(s):
    """{storage key of s.kw: compare's slack} of Snapshot s: ZERO_SUM_OUTPUTS' units of `sensitivity`, nothing for any other output"""
    names = {}
    for lbl, t in gpu_cases._arg_tensors(s.kw):
        names.setdefault(gpu_cases.skey(t), lbl)
    return {k: ZERO_SUM_OUTPUTS[(s.entry, names[k])][0] * u for k, u in sensitivity(s).items()}


# ---- judging -------------------------------------------------------------------------------------------------------------------------------------
def ratios(errs):
    """(worst norm-wise error / the bound applied to it, worst per-element error / the bound applied to it) of a gpu_cases.compare result"""
    return errs["worst_norm"], errs["worst_elem"][0]


def replay(rec, runner=None):
    """Every snapshot of a Recording through `runner` (default gpu_cases.run_case: the device against the emulator) on a copy of its
    storages.  -> (failures [(entry, signature, site, errs)], rows [(entry, norm ratio, element ratio)])"""
    runner = runner or gpu_cases.run_case
    failures, rows = [], []
    for s in rec.snaps:
        kw, store = s.fresh()
        tol = tolerance(s.entry, kw)
        if tol is None:
            failures.append((s.entry, s.sig, s.site, "no hand-written case defines this precision class: "
                             f"{precision_class(s.entry, kw, any(split_outputs(s.entry, kw)))} (add one to gpu_cases.py)"))
            continue
        slack = {gpu_cases.skey(store[k]): v for k, v in allowance(s).items()}
        r = runner(s.entry, kw, None, tol, slack, True)          # written_norm: the sentinels must not carry a small output's norm
        rows.append((s.entry,) + ratios(r["errs"]))
        if not r["ok"]:
            failures.append((s.entry, s.sig, s.site, r["errs"]))
    return failures, rows
