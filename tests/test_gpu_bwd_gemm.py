"""-m gpu: the sliced weight gradients of autograd_path (one launcher, _slab_gemm, behind _wgrad / _wgrad_batched / _enc_wgrad /
Conv3x3Fn.backward) on the device, at the smallest shapes at which each path can go wrong: a remainder launch of one row, a remainder
longer than a slice, element offsets into a pair-concatenated gradient, a map off the 8-pixel granule.

Each case compares the helper's dW with dy.double().T @ x.double() computed on the host from the same (already rounded) inputs, and
launches the same product UNSLICED, as one mtt_gemm call with a_op = b_op = MTT_OP_R.  Criterion: the relative Frobenius error of the
sliced result is at most twice the unsliced launch's error against the same fp64 reference, + 1e-7: slabs only reorder the fp32
accumulation and add one fp32 add per slab, and the factor 2 is that allowance.  The slicing each case is there for is asserted too
(main launch: batch / batch_inner / rows per slice; remainder rows), so that a changed policy cannot quietly turn a case into an
unsliced one.  tests/test_bwd_gemm_plan.py pins the same plans, and the benchmark's, field by field without a GPU.

(The bf16 `_wgrad_batched` case runs on the token-major kernel, which mtt_gemm picks for bf16 row-major operands; its 16 slices of 264
rows come from the general rule with SPLIT_ROW_UNIT = 8, because the token-major rule wants at least 512 rows per slice and
declines at 4296 rows.)"""
import pytest
import torch
import torch.nn.functional as Fn

import mtt_amd

ops, ap = mtt_amd.ops, mtt_amd.autograd_path
OP_R, OP_CONV_R = mtt_amd._lib.OP_R, mtt_amd._lib.OP_CONV_R
DEV = "cuda"


def _rel(got, ref):
    return float((got.double().cpu() - ref).norm() / ref.norm())


def _judge(name, sliced, unsliced, ref):
    e_s, e_u = _rel(sliced, ref), _rel(unsliced, ref)
    print(f"{name}: sliced {e_s:.3e}, unsliced {e_u:.3e}")
    assert e_s <= 2.0 * e_u + 1e-7, (name, e_s, e_u)


def _spy(monkeypatch):
    """-> the list that collects (batch, batch_inner, K) of every weight-gradient GEMM launched from here on"""
    seen, real = [], ops.call

    def call(entry, **kw):
        if entry == "gemm" and kw.get("a_op") == OP_R and kw.get("b_op") in (OP_R, OP_CONV_R):
            seen.append((kw.get("batch", 1), kw.get("batch_inner", 1), kw["K"]))
        return real(entry, **kw)
    monkeypatch.setattr(ops, "call", call)
    return seen


def _rand(shape, dtype, seed, cols=None):
    """values of `dtype` in the first `cols` columns, zeros in the channel padding"""
    t = torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dtype)
    if cols is not None:
        t[..., cols:] = 0
    return t


def _unsliced(A, B, N, Kp, rows, prec, lda, ldb, Z=None, **zs):
    D = torch.empty((N, Kp) if Z is None else (Z, N, Kp), dtype=torch.float32, device=A.device)
    batch = {} if Z is None else dict(batch=Z, d_zo=N * Kp, **zs)
    return ap._gemm(A, B, D, N, Kp, rows, prec, a_op=OP_R, b_op=OP_R, lda=lda, ldb=ldb, ldd=Kp, **batch)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.mark.gpu
def test_wgrad_two_slices_and_a_one_row_remainder(monkeypatch):
    _need_gpu()
    monkeypatch.setattr(ap, "SPLITK_MIN_ROWS", 64)
    rows, N, Kp, prec = 1001, 21, 64, ops.Prec("x3")
    dy, x = _rand((rows, 24), torch.float32, 1, N), _rand((rows, Kp), torch.float32, 2)
    ref = dy[:, :N].double().T @ x.double()
    dy, x = dy.to(DEV), x.to(DEV)
    seen = _spy(monkeypatch)
    got = ap._wgrad(dy, x, N, Kp, prec)
    assert seen == [(2, 1, 500), (1, 1, 1)], seen
    _judge("wgrad-x3", got, _unsliced(dy, x, N, Kp, rows, prec, 24, Kp), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("catpair", (False, True), ids=("plain", "catpair"))
def test_wgrad_batched_general_rule_with_a_long_remainder(monkeypatch, catpair):
    """Z = 2, 16 slices of 56 rows and 105 rows left over; catpair: the second half of a [Z, M, 2 * pitch(N)] gradient (a0 = pitch(N),
    lda = 2 * pitch(N)) against every second map of x, starting at the second (b0 = one task stride)"""
    _need_gpu()
    monkeypatch.setattr(ap, "SPLIT_ROW_UNIT", 8)
    Z, M, N, Kp, prec = 2, 1001, 44, 64, ops.Prec("x3")
    Np = ops.pitch(N)
    if catpair:
        dy, x = _rand((Z, M, 2 * Np), torch.float32, 3), _rand((2 * Z, M, Kp), torch.float32, 4)
        ref = torch.stack([dy[z][:, Np:Np + N].double().T @ x[2 * z + 1].double() for z in range(Z)])
        geo = dict(lda=2 * Np, ldb=Kp, a_zo=M * 2 * Np, b_zo=2 * M * Kp)
        a0, b0 = Np, M * Kp
    else:
        dy, x = _rand((Z, M, Np), torch.float32, 3, N), _rand((Z, M, Kp), torch.float32, 4)
        ref = torch.stack([dy[z][:, :N].double().T @ x[z].double() for z in range(Z)])
        geo = dict(lda=Np, ldb=Kp, a_zo=M * Np, b_zo=M * Kp)
        a0 = b0 = 0
    dy, x = dy.to(DEV), x.to(DEV)
    seen = _spy(monkeypatch)
    got = ap._wgrad_batched(dy, x, N, Kp, M, prec, Z, geo["lda"], geo["ldb"], geo["a_zo"], geo["b_zo"], a0=a0, b0=b0)
    assert seen == [(32, 16, 56), (2, 1, 105)], seen
    uns = _unsliced(dy.reshape(-1)[a0:], x.reshape(-1)[b0:], N, Kp, M, prec, geo["lda"], geo["ldb"], Z, a_zo=geo["a_zo"], b_zo=geo["b_zo"])
    _judge("wgrad_batched-x3-" + ("catpair" if catpair else "plain"), got, uns, ref)


@pytest.mark.gpu
def test_wgrad_batched_on_the_token_major_kernel(monkeypatch):
    _need_gpu()
    monkeypatch.setattr(ap, "SPLIT_ROW_UNIT", 8)
    Z, M, N, Kp, prec = 2, 4296, 256, 256, ops.Prec("bf16")
    dy, x = _rand((Z, M, N), torch.bfloat16, 5), _rand((Z, M, Kp), torch.bfloat16, 6)
    ref = torch.stack([dy[z].double().T @ x[z].double() for z in range(Z)])
    dy, x = dy.to(DEV), x.to(DEV)
    seen = _spy(monkeypatch)
    got = ap._wgrad_batched(dy, x, N, Kp, M, prec, Z, N, Kp, M * N, M * Kp)
    assert seen == [(32, 16, 264), (2, 1, 72)], seen
    _judge("wgrad_batched-bf16", got, _unsliced(dy, x, N, Kp, M, prec, N, Kp, Z, a_zo=M * N, b_zo=M * Kp), ref)


@pytest.mark.gpu
def test_enc_wgrad_at_the_first_row_count_its_policy_slices(monkeypatch):
    """16392 rows of a 256 x 256 weight: the smallest row count at which _tn_splits' slices reach 512 rows (32 of them, 8 rows over)"""
    _need_gpu()
    rows, N, Kp, prec = 16392, 256, 256, ops.Prec("bf16")
    dy, x = _rand((rows, N), torch.bfloat16, 7), _rand((rows, Kp), torch.bfloat16, 8)
    ref = dy.double().T @ x.double()
    dy, x = dy.to(DEV), x.to(DEV)
    seen = _spy(monkeypatch)
    got, _ = ap._enc_wgrad(dy, x, N, Kp, prec, bias=False)
    assert seen == [(32, 1, 512), (1, 1, 8)], seen
    _judge("enc_wgrad-bf16", got, _unsliced(dy, x, N, Kp, rows, prec, N, Kp), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("pn", ("x3", "bf16"))
def test_conv3x3_weight_gradient_in_whole_image_slices(monkeypatch, pn):
    """Z = 2 convs 16 -> 16 on 3 images of 6 x 6 (a map off the 8-pixel granule): three slices of one image each, against the fp64 im2col
    product; the unsliced launch reads the im2col matrix of the same inputs"""
    _need_gpu()
    Z, B, H, W, C, prec = 2, 3, 6, 6, 16, ops.Prec(pn)
    rows, Cp = B * H * W, ops.pitch(C)
    assert Cp == C
    x, dy = _rand((Z, rows, Cp), prec.adt, 9), _rand((Z, rows, Cp), prec.adt, 10)
    ws = [torch.nn.Parameter(_rand((C, C, 3, 3), torch.float32, 11 + z).to(DEV)) for z in range(Z)]
    bs = [torch.nn.Parameter(torch.zeros(C).to(DEV)) for z in range(Z)]

    def nchw(t):
        return t.double().view(B, H, W, Cp).permute(0, 3, 1, 2)
    cols = [Fn.unfold(nchw(x[z]), 3, padding=1) for z in range(Z)]                                   # [B, C * 9, H * W], k = ci * 9 + tap
    ref = torch.stack([torch.einsum("bnp,bkp->nk", nchw(dy[z]).reshape(B, C, H * W), cols[z]).view(C, C, 3, 3) for z in range(Z)])
    # the unsliced launch's B operand: rows = pixels, k = tap * Cp + ci (the implicit GEMM's order), in the operands' dtype (exact: a gather)
    im2col = torch.stack([c.view(B, C, 9, H * W).permute(0, 3, 2, 1).reshape(rows, 9 * Cp) for c in cols]).to(prec.adt)
    seen = _spy(monkeypatch)
    xd = x.to(DEV).requires_grad_(True)
    ap.Conv3x3Fn.apply(xd, (B, H, W, C, C), prec, "bwd_gemm_test", *ws, *bs).backward(dy.to(DEV))
    assert seen == [(6, 3, H * W)], seen
    got = torch.stack([w.grad for w in ws])
    uns = _unsliced(dy.to(DEV), im2col.to(DEV), C, 9 * Cp, rows, prec.bwd, Cp, 9 * Cp, Z, a_zo=rows * Cp, b_zo=rows * 9 * Cp)
    uns = uns.view(Z, C, 9, Cp)[..., :C].permute(0, 1, 3, 2).reshape(Z, C, C, 3, 3)
    _judge("conv3x3-" + pn, got, uns, ref)
