"""The launch plan of the backward GEMM plumbing (autograd_path: the sliced weight gradients, the stacked input gradients), pinned
against tests/golden/bwd_gemm_plan.json without a GPU.  A plan is the list of C-ABI calls a helper issues: `ops.call` is replaced by a
recorder that computes nothing and stores, per call, the entry name, every scalar field and (dtype, shape, strides, storage offset) of
every tensor; the helpers run on `device="meta"` tensors, so the full-size shapes of the benchmark cost nothing.  Equal plans mean equal
launches: the same kernels on the same descriptors, so the same speed.

What the recorder normalises: a keyword field that is None or 0 is left out (a descriptor starts zeroed and None leaves a pointer NULL:
`b_zi=0` and no `b_zi` are the same descriptor); positional `args` / `xargs` are kept as they are.

Shapes: oracle/configs.py at the benchmark's batch (ns6: 126 images, 32 x 32 patches, 6 tasks; cfg4_6: 64; cs_swinB: 16), and the small
shapes of tests/test_gpu_bwd_gemm.py under lowered thresholds.  Run as a script, the module writes the golden file:
    python tests/test_bwd_gemm_plan.py
"""
import json
import os
import sys

import pytest
import torch

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conftest
import mtt_amd
from oracle import configs

ops, ap = mtt_amd.ops, mtt_amd.autograd_path
OP_R, OP_CONV_R = mtt_amd._lib.OP_R, mtt_amd._lib.OP_CONV_R
GOLDEN = os.path.join(conftest.GOLDEN, "bwd_gemm_plan.json")
F32, B16 = torch.float32, torch.bfloat16

DEFAULTS = dict(SPLITK_MIN_ROWS=4096, SPLIT_ROW_UNIT=512, SPLIT_TARGET_WGS=1024, FAST_MIN_DIM=256, FAST_MIN_ROWS=1024, FAST_BWD=True,
                WGRAD_MAX_SLICES=192, WGRAD_TARGET_WGS=512, N_CUS=256)
LOWERED = dict(DEFAULTS, SPLITK_MIN_ROWS=64, SPLIT_ROW_UNIT=8, FAST_MIN_DIM=8, FAST_MIN_ROWS=8)


def _enc(v):
    if isinstance(v, torch.Tensor):
        return ["tensor", str(v.dtype).replace("torch.", ""), list(v.shape), list(v.stride()), v.storage_offset()]
    if isinstance(v, ops.Split):
        return ["split", _enc(v.hi), _enc(v.lo)]
    if isinstance(v, dict):
        return {k: _enc(v[k]) for k in sorted(v)}
    if isinstance(v, (list, tuple)):
        return [_enc(e) for e in v]
    assert v is None or isinstance(v, (bool, int, float, str)), type(v)
    return v


def _t(*shape, dtype):
    return torch.empty(*shape, dtype=dtype, device="meta")


class _Ctx:
    """what a Function.backward reads from its ctx"""

    def __init__(self, saved, meta, grad_dtype=None):
        self.saved_tensors, self.meta = tuple(saved), meta
        if grad_dtype is not None:
            self.grad_dtype = grad_dtype


def record(run, consts):
    """-> the plan of run(): [{entry, field: value ...}] with ops.call replaced by a recorder and the pack / unpack helpers by meta stand-ins"""
    plan = []

    def call(entry, **kw):
        plan.append(dict({k: _enc(v) for k, v in kw.items() if k in ("args", "xargs") or not (v is None or (not isinstance(v, torch.Tensor) and v == 0))},
                         entry=entry))

    def pack_conv3(weights, prec, tag, transpose=False, split=None):
        Co, Ci = weights[0].shape[:2]
        R, Cin = (Ci, Co) if transpose else (Co, Ci)
        return _t(len(weights), R, 9 * ops.pitch(Cin), dtype=prec.adt)

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ops, "PITCH32_FROM", 160)
        mp.setattr(ops, "GEMM_VARIANT", None)
        mp.setattr(ops, "call", call)
        mp.setattr(ops, "pack_conv3", pack_conv3)
        mp.setattr(ops, "pack_linear_T", lambda w, dtype, tag: _t(w.numel() // w.shape[0], w.shape[0], dtype=dtype))
        mp.setattr(ops, "unpack_grads", lambda src, key, shapes, rows_of, partial=False: [_t(*sh, dtype=F32) for sh in shapes])
        mp.setattr(ops, "colsum_batched", lambda x3d, cols, Z, src_zs, col_off=0: _t(Z, cols, dtype=F32))
        mp.setattr(ops, "stack_vec", lambda vs, tag: _t(len(vs), vs[0].numel(), dtype=F32))
        for k, v in consts.items():
            mp.setattr(ap, k, v)
        run()
    return plan


# ---- the cases: name -> (kind of helper, thresholds, thunk) ---------------------------------------------------------------------------------
def _prec(name):
    return ops.Prec(name)


def _adt(pn):
    return B16 if pn == "bf16" else F32


def _wgrad_case(rows, N, Kp, pn):
    dt = _adt(pn)
    return lambda: ap._wgrad(_t(rows, ops.pitch(N), dtype=dt), _t(rows, Kp, dtype=dt), N, Kp, _prec(pn))


def _enc_wgrad_case(rows, N, Kp):
    return lambda: ap._enc_wgrad(_t(rows, N, dtype=B16), _t(rows, Kp, dtype=B16), N, Kp, _prec("bf16"), bias=False)


def _batched_case(Z, M, N, Kp, pn, catpair=None):
    """catpair = 0 / 1: the half of a [Z, M, 2 * pitch(N)] gradient whose columns start at pitch(N) * half, on x[2 z + half]"""
    dt, Np = _adt(pn), ops.pitch(N)
    if catpair is None:
        return lambda: ap._wgrad_batched(_t(Z, M, Np, dtype=dt), _t(Z, M, Kp, dtype=dt), N, Kp, M, _prec(pn), Z, Np, Kp, M * Np, M * Kp)
    return lambda: ap._wgrad_batched(_t(Z, M, 2 * Np, dtype=dt), _t(2 * Z, M, Kp, dtype=dt), N, Kp, M, _prec(pn), Z, 2 * Np, Kp, M * 2 * Np,
                                     2 * M * Kp, a0=catpair * Np, b0=catpair * M * Kp)


def _conv_case(Z, B, H, W, Ci, Co, pn):
    dt = _adt(pn)
    ctx = _Ctx([_t(Z, B * H * W, ops.pitch(Ci), dtype=dt)] + [_t(Co, Ci, 3, 3, dtype=F32) for _ in range(Z)],
               ((B, H, W, Co, Ci, 1), _prec(pn), "c", Z, True, dt))
    return lambda: ap.Conv3x3Fn.backward(ctx, _t(Z, B * H * W, ops.pitch(Co), dtype=dt))


def _blinear_case(Z, M, N, K, pn, layout="plain", kmap=None, dy=None, x=None, w=None, grad_dtype=None):
    """pn 'x3f': bf16 hi planes saved unless the dtypes say otherwise (dy / x / w: the dtypes of the gradient, the saved input and pack)"""
    dt = B16 if pn in ("bf16", "x3f") else F32
    Kp, Np = (kmap[0] if kmap else ops.pitch(K)), ops.pitch(N)
    xs = _t(Z, M, Kp, dtype=x or dt)
    ctx = _Ctx([xs, _t(Z, N, Kp, dtype=w or dt)], (Z, N, layout, kmap, _prec(pn), [(N, K)] * Z, xs.dtype), grad_dtype)
    g = _t(Z // 2, M, 2 * Np, dtype=dy or dt) if layout == "catpair" else _t(Z, M, Np, dtype=dy or dt)
    return lambda: ap.BLinearFn.backward(ctx, g)


def _upconv_case(Z, B, h, w, Ci, Co, pn):
    dt = B16 if pn in ("bf16", "x3f") else F32
    ctx = _Ctx([_t(Z, B * h * w, ops.pitch(Ci), dtype=dt), _t(Z, 9 * ops.pitch(Co), ops.pitch(Ci), dtype=dt)], ((B, h, w, Co, Ci), _prec(pn), Z, dt))
    return lambda: ap.UpConv3x3Fn.backward(ctx, _t(Z, B * 16 * h * w, ops.pitch(Co), dtype=dt))


def cases():
    ns6, c4, sw = configs.taskprompter("ns6"), configs.invpt("cfg4_6"), configs.swin("cs_swinB")
    B, T = 126, len(ns6["tasks"])
    h, w = ns6["img_size"][0] // 16, ns6["img_size"][1] // 16
    C = configs.VIT[ns6["backbone"]][0]
    tar, F = ns6["embed_dim"], ns6["final_embed_dim"]
    Fp, M = ops.pitch(F), B * h * w
    out = {}

    def add(name, kind, thunk, consts=DEFAULTS):
        assert name not in out
        out[name] = (kind, consts, thunk)

    for N, Kp in ((C, C), (3 * C, C), (C, 4 * C), (4 * C, C)):
        add(f"enc_wgrad-{N}x{Kp}-bf16", "flat", _enc_wgrad_case(B * (T + h * w), N, Kp))
    for pn in ("bf16", "x3"):
        for _, n in ns6["tasks"]:
            if f"pred_wgrad-n{n}-{pn}" not in out:
                add(f"pred_wgrad-n{n}-{pn}", "flat", _wgrad_case(B * 16 * h * w, n, Fp, pn))
        add(f"prompt_wgrad-{pn}", "flat", _wgrad_case(B * T, C, C, pn))
        for half in (0, 1):
            add(f"fea_decode-half{half}-{pn}", "stack", _batched_case(T, M, tar, C, pn, catpair=half))
        add(f"fea_fuse0-{pn}", "stack", _batched_case(T, M, F, 2 * ops.pitch(tar), pn))
        add(f"fea_fuse4-{pn}", "stack", _batched_case(T, M, F, Fp, pn))
        add(f"head9-{pn}", "stack", _batched_case(T, M, 9 * Fp, Fp, pn))
        add(f"conv-fea_fuse1-{pn}", "stack", _conv_case(T, B, h, w, F, F, pn))
        E = c4["embed_dim"] + c4["pred_const"]
        add(f"conv-invpt{E}-{pn}", "stack", _conv_case(len(c4["tasks"]), 64, 128, 128, E, E, pn))
        Fs = sw["final_embed_dim"]
        hs, ws = (int(s * sw["img_ds_ratio"]) // 8 for s in sw["img_size"])
        add(f"conv-swin_msf-{pn}", "stack", _conv_case(len(sw["tasks"]), 16, hs, ws, Fs, Fs, pn))
    kmap = (2 * ops.pitch(tar), [(0, 0, tar), (ops.pitch(tar), tar, tar)])
    for pn in ("bf16", "x3f", "x3"):
        add(f"blinear-fea_decode-{pn}", "dgrad", _blinear_case(2 * T, M, tar, C, pn, layout="catpair"))
        add(f"blinear-fea_fuse0-{pn}", "dgrad", _blinear_case(T, M, F, 2 * tar, pn, kmap=kmap))
        add(f"blinear-fea_fuse4-{pn}", "dgrad", _blinear_case(T, M, F, F, pn, dy=F32 if pn == "x3f" else None, grad_dtype=_prec(pn).bwd.adt))
        add(f"upconv-head-{pn}", "dgrad", _upconv_case(T, B, h, w, F, F, pn))
    # x3f on a layer nobody split (fp32 rows and pack saved), one task: the flat weight gradient behind a stacked input gradient
    add("blinear-z1-fp32saved-x3f", "dgrad", _blinear_case(1, M, F, F, "x3f", dy=F32, x=F32, w=F32))
    # ---- the small shapes of tests/test_gpu_bwd_gemm.py, thresholds lowered ---------------------------------------------------------------
    add("small-wgrad-x3", "flat", _wgrad_case(1001, 21, 64, "x3"), LOWERED)
    add("small-batched-x3", "stack", _batched_case(2, 1001, 44, 64, "x3"), LOWERED)
    for half in (0, 1):
        add(f"small-batched-half{half}-x3", "stack", _batched_case(2, 1001, 44, 64, "x3", catpair=half), LOWERED)
    add("small-batched-bf16", "stack", _batched_case(2, 4296, 256, 256, "bf16"), LOWERED)
    add("small-enc_wgrad-bf16", "flat", _enc_wgrad_case(16392, 256, 256), LOWERED)
    for pn in ("bf16", "x3"):
        add(f"small-conv-{pn}", "stack", _conv_case(2, 3, 6, 6, 16, 16, pn), LOWERED)
        add(f"small-blinear-{pn}", "dgrad", _blinear_case(2, 1001, 44, 64, pn), LOWERED)
        add(f"small-blinear-catpair-{pn}", "dgrad", _blinear_case(4, 1001, 44, 64, pn, layout="catpair"), LOWERED)
        add(f"small-upconv-{pn}", "dgrad", _upconv_case(2, 3, 6, 6, 16, 16, pn), LOWERED)
    return out


def record_all():
    return {name: record(thunk, consts) for name, (_, consts, thunk) in cases().items()}


def dumps(plans):
    return "{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(plans[k], sort_keys=True)}" for k in sorted(plans)) + "\n}\n"


# ---- what kind of plan a case is -----------------------------------------------------------------------------------------------------------
def _wgrad_calls(plan):
    return [c for c in plan if c["entry"] == "gemm" and c.get("a_op") == OP_R and c.get("b_op") in (OP_R, OP_CONV_R) and c["D"][1] == "float32"]


def kinds(kind, plan):
    """the kinds of plan a case covers (the names of test_golden_covers_every_kind_of_plan)"""
    found = set()
    wg = _wgrad_calls(plan)
    if kind in ("flat", "stack") and wg:
        m = wg[0]
        sliced = len(m["D"][2]) == (3 if kind == "flat" else 4)
        rem = len(wg) > 1
        if not sliced:
            found.add("unsliced")
        elif kind == "flat":
            assert m.get("batch_inner", 1) == 1 and m["a_zo"] == m["K"] * m["lda"] and m["d_zo"] == m["N"] * m["M"]
            found.add("one-level slabs + remainder" if rem else "one-level slabs")
        else:
            assert m["batch_inner"] > 1 and m["a_zi"] == m["K"] * m["lda"] and m["batch"] == m["batch_inner"] * m["D"][2][0]
            found.add("two-level slabs + remainder" if rem else "two-level slabs")
        if sliced and m["b_op"] == OP_CONV_R and m["K"] % (m["conv"]["H"] * m["conv"]["W"]) == 0:
            found.add("whole-image conv slabs")
        if sliced and m["b_op"] == OP_R and m["K"] % 64 == 0 and m["K"] >= 512 and m["A"][1] == m["B"][1] == "bfloat16":
            found.add("token-major slabs")
    if kind == "dgrad":
        d = [c for c in plan if c["entry"] == "gemm" and "n_store" in c and c.get("a_op", 0) == 0]
        assert d, "no input-gradient GEMM in the plan"
        found.add("dgrad on the transposing stager" if d[0].get("b_op") == OP_R else "dgrad on a transposed bf16 copy")
    return found


KINDS = ("unsliced", "one-level slabs + remainder", "two-level slabs", "two-level slabs + remainder", "token-major slabs",
         "whole-image conv slabs", "dgrad on the transposing stager", "dgrad on a transposed bf16 copy")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_every_plan_equals_the_golden(golden):
    plans = json.loads(dumps(record_all()))
    assert sorted(plans) == sorted(golden)
    for name in sorted(plans):
        assert plans[name] == golden[name], name


def test_golden_covers_every_kind_of_plan(golden):
    table = cases()
    found = set()
    for name, plan in golden.items():
        found |= kinds(table[name][0], plan)
    assert not set(KINDS) - found, set(KINDS) - found


def _slices(plan):
    """(batch, batch_inner, rows per slice, remainder batch, remainder rows) of a case's first weight gradient"""
    wg = _wgrad_calls(plan)
    m, r = wg[0], (wg[1] if len(wg) > 1 else {})
    return m["batch"], m.get("batch_inner", 1), m["K"], r.get("batch", 1 if r else 0), r.get("K", 0)


def test_anchor_plans(golden):
    """slice counts of five benchmark launches, worked out by hand from the policies: they check the recorder, not the product"""
    assert _slices(golden["fea_fuse0-bf16"]) == (42, 7, 18432, 0, 0)
    assert _slices(golden["fea_fuse4-bf16"]) == (60, 10, 12864, 6, 384)
    assert _slices(golden["fea_decode-half0-bf16"]) == (30, 5, 25792, 6, 64)
    assert _slices(golden["pred_wgrad-n21-bf16"]) == (170, 1, 12143, 1, 74)
    assert _slices(golden["enc_wgrad-3072x1024-bf16"]) == (5, 1, 25920, 1, 180)
    assert _slices(golden["small-wgrad-x3"]) == (2, 1, 500, 1, 1)
    assert _slices(golden["small-batched-x3"]) == (32, 16, 56, 2, 105)
    assert _slices(golden["small-batched-bf16"]) == (32, 16, 264, 2, 72)
    assert _slices(golden["small-enc_wgrad-bf16"]) == (32, 1, 512, 1, 8)
    assert _slices(golden["small-conv-x3"]) == (6, 3, 36, 0, 0)


if __name__ == "__main__":
    with open(GOLDEN, "w") as f:
        f.write(dumps(record_all()))
    print("wrote", GOLDEN)
