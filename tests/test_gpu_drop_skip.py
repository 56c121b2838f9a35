"""-m gpu: DropPath work skipping (mtt_gemm_desc.skip_scale / mtt_attn_desc.skip_scale).  A skipped tile stores exactly what the unskipped
kernel stores for zero input rows, so every case compares `torch.equal` (whole buffers, guard bands included) against THE SAME entry point
without the table on inputs whose dead rows are zeroed — while the skipping run gets NaN wherever it must not read."""
import pytest
import torch

import train_check
from gpu_cases import pkg

F32, BF16, SPLIT = 0, 1, 2
OP_K, OP_R = 0, 1
MB, NP, NS = 600, 6, 4                # rows per sample, prompt rows, samples
M = MB * NS                           # 2400 = nine 256-row tiles + one of 96 rows
K = 128
KEEP = 1.0 / 0.85
GUARD = 8                             # guard rows before and after every output


def _table(kind):
    t = torch.full((NS, 2), KEEP)
    if kind == "b":
        t[:, 1] = 0.0
    elif kind == "c":
        t[:] = 0.0
    elif kind == "d":                 # tile [1792, 2048) straddles the 2 | 3 sample boundary and is wholly dead
        t[0, 1] = t[2, 1] = 0.0
        t[3] = 0.0
    return t


def _dead_rows(table, rows=M, mb=MB, n_prompt=NP, row0=0):
    r = torch.arange(row0, row0 + rows)
    return table[r // mb, ((r % mb) >= n_prompt).long()] == 0.0


def _dead_tiles(dead, step):
    """rows lying in a `step`-row tile (counted from row 0 of `dead`) whose rows are all dead"""
    out = torch.zeros_like(dead)
    for r0 in range(0, dead.numel(), step):
        if bool(dead[r0:r0 + step].all()):
            out[r0:r0 + step] = True
    return out


class Guarded:
    """an output [rows, ld] inside a sentinel-filled buffer with GUARD rows on either side (and ld - ncols pad columns per row)"""

    def __init__(self, rows, ld, ncols, dtype, fill=7.0, init=None):
        self.buf = torch.full((rows + 2 * GUARD, ld), fill, dtype=dtype, device="cuda")
        self.t = self.buf[GUARD:GUARD + rows]
        if init is not None:
            self.t[:, :init.shape[1]] = init
        self.before = self.buf.clone()
        self.ncols = ncols

    def guards_untouched(self):
        b, a = self.buf, self.before
        return (torch.equal(b[:GUARD], a[:GUARD]) and torch.equal(b[-GUARD:], a[-GUARD:]) and
                torch.equal(b[:, self.ncols:], a[:, self.ncols:]))


def _rnd(g, *shape, dtype=torch.float32):
    return torch.randn(*shape, generator=g).to(dtype).cuda()


def _planes(g, rows, cols):
    x = torch.randn(rows, cols, generator=g)
    hi = x.to(torch.bfloat16)
    return hi.cuda(), (x - hi.float()).to(torch.bfloat16).cuda()


def _run_gemm(kw, outs):
    lib = pkg()._lib
    lib.call("gemm", **kw)
    torch.cuda.synchronize()
    return {k: v.buf.clone() for k, v in outs.items()}


GEMM_FORMS = ["ring3_gelu_daux_split", "ring3_f32_resid_rowscale", "ring3_edge_n300", "dma_bf16", "dma_mulaux_colsum"]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["a", "b", "c", "d"])
@pytest.mark.parametrize("form", GEMM_FORMS)
def test_gemm_tile_skip_equals_unskipped_on_zero_rows(form, kind):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    lib = pkg()._lib
    g = torch.Generator().manual_seed(21)
    table = _table(kind)
    dead = _dead_rows(table)
    nan_rows = _dead_tiles(dead, 256).cuda()
    dead, tab = dead.cuda(), table.cuda()
    ring3 = form.startswith("ring3")
    N = {"ring3_gelu_daux_split": 512, "ring3_f32_resid_rowscale": 256, "ring3_edge_n300": 300}.get(form, 512)
    B_hi, B_lo = _planes(g, N, K)
    A_hi, A_lo = _planes(g, M, K)
    A_hi[dead] = 0
    A_lo[dead] = 0
    bias = _rnd(g, N)

    def build(skipping):
        ah, al = A_hi.clone(), A_lo.clone()
        if skipping:
            ah[nan_rows] = float("nan")
            al[nan_rows] = float("nan")
        outs = {}
        kw = dict(A=ah, B=B_hi, M=M, N=N, K=K, a_op=OP_K, b_op=OP_K, lda=K, ldb=K, batch=1, batch_inner=1, alpha=1.0, colshift=bias)
        if ring3:
            kw.update(A_lo=al, B_lo=B_lo, a_dtype=SPLIT, b_dtype=SPLIT, prec=1)
        else:
            kw.update(a_dtype=BF16, b_dtype=BF16, prec=0, variant=3)
        if form == "ring3_gelu_daux_split":
            outs = dict(D=Guarded(M, N + 8, N, torch.bfloat16), D_lo=Guarded(M, N + 8, N, torch.bfloat16), aux=Guarded(M, N + 16, N, torch.bfloat16, 3.0))
            kw.update(D=outs["D"].t, D_lo=outs["D_lo"].t, d_dtype=SPLIT, ldd=N + 8, n_store=N, act=5, aux_out=outs["aux"].t, aux_dtype=BF16, ldaux=N + 16)
        elif form == "ring3_f32_resid_rowscale":
            outs = dict(D=Guarded(M, N + 8, N, torch.float32))
            resid = torch.randn(M, N, generator=torch.Generator().manual_seed(5)).cuda()
            kw.update(D=outs["D"].t, d_dtype=F32, ldd=N + 8, n_store=N, d_mb=MB, d_bs=MB * (N + 8), resid=resid, ldr=N, r_mb=MB, r_bs=MB * N,
                      rowscale=tab, n_prompt=NP)
        elif form == "ring3_edge_n300":
            outs = dict(D=Guarded(M, 312, 304, torch.bfloat16), D_lo=Guarded(M, 312, 304, torch.bfloat16))
            kw.update(D=outs["D"].t, D_lo=outs["D_lo"].t, d_dtype=SPLIT, ldd=312, n_store=304)
        elif form == "dma_bf16":
            outs = dict(D=Guarded(M, N + 8, N, torch.bfloat16))
            kw.update(D=outs["D"].t, d_dtype=BF16, ldd=N + 8, n_store=N)
        else:
            aux = torch.randn(M, N + 8, generator=torch.Generator().manual_seed(6)).to(torch.bfloat16).cuda()
            outs = dict(D=Guarded(M, N + 8, N, torch.bfloat16), cs=Guarded(1, N + 8, N, torch.float32, 9.0))
            ws = torch.full((((M + 127) // 128) * N,), float("nan"), device="cuda")
            kw.pop("colshift")
            kw.update(D=outs["D"].t, d_dtype=BF16, ldd=N + 8, n_store=N, act=6, aux_in=aux, aux_dtype=BF16, ldaux=N + 8,
                      colsum_out=outs["cs"].t, colsum_ws=ws)
        if skipping:
            kw.update(skip_scale=tab, skip_mb=MB, skip_prompt=NP)
        return kw, outs

    kw_ref, outs_ref = build(False)
    assert lib.gemm_variant(**kw_ref) == (8 if ring3 else 3)
    ref = _run_gemm(kw_ref, outs_ref)
    kw, outs = build(True)
    assert lib.gemm_variant(**kw) == (8 if ring3 else 3)
    got = _run_gemm(kw, outs)
    for k in ref:
        assert outs_ref[k].guards_untouched() and outs[k].guards_untouched(), (k, "guard band written")
        assert not bool(torch.isnan(got[k].float()).any()), (k, "a dead tile's input was read")
        assert torch.equal(got[k], ref[k]), (k, int((got[k] != ref[k]).sum()))


# ---------------------------------------------------------------------------------------------------------------------------------
ATTN_SHAPES = [(3, 200, 2, 6), (2, 1030, 1, 6)]


def _attn_table(B, kind):
    t = torch.full((B, 2), KEEP)
    if kind in ("patch", "whole"):
        t[1, 1] = 0.0
    if kind == "whole":
        t[1, 0] = 0.0
    return t


def _fwd_dead_rows(table, B, N, T):
    """rows of the forward's skipped 128-row blocks: blocks past the prompt rows' of images whose patch rows are dead"""
    first = -(-T // 128) * 128
    dead = torch.zeros(B, N, dtype=torch.bool)
    for b in range(B):
        if float(table[b, 1]) == 0.0:
            dead[b, first:] = True
    return dead.reshape(-1)


def _attn_fwd(qkv, qkv_lo, B, N, nH, T, table):
    lib = pkg()._lib
    C = nH * 64
    out = Guarded(B * N, C, C, torch.bfloat16)
    out_lo = Guarded(B * N, C, C, torch.bfloat16) if qkv_lo is not None else None
    lse = Guarded(B * nH, N, N, torch.float32)
    rawlog = Guarded(B * nH * T, N, N, torch.float32)
    kw = dict(qkv=qkv, out=out.t, rawlog=rawlog.t, lse=lse.t, B=B, N=N, nH=nH, T=T, scale=0.125, dtype=BF16, prec=0)
    if qkv_lo is not None:
        kw.update(qkv_lo=qkv_lo, out_lo=out_lo.t, dtype=SPLIT, prec=1)
    if table is not None:
        kw.update(skip_scale=table.cuda())
    lib.call("attn_fwd", **kw)
    torch.cuda.synchronize()
    return dict(out=out, out_lo=out_lo, lse=lse, rawlog=rawlog)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["none", "patch", "whole"])
@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("B,N,nH,T", ATTN_SHAPES)
def test_attention_forward_block_skip(B, N, nH, T, split, kind):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    g = torch.Generator().manual_seed(23)
    C = nH * 64
    if split:
        qkv, qkv_lo = _planes(g, B * N, 3 * C)
    else:
        qkv, qkv_lo = _rnd(g, B * N, 3 * C, dtype=torch.bfloat16), None
    table = _attn_table(B, kind)
    ref = _attn_fwd(qkv, qkv_lo, B, N, nH, T, None)
    got = _attn_fwd(qkv, qkv_lo, B, N, nH, T, table)
    dead = _fwd_dead_rows(table, B, N, T).cuda()
    assert bool(dead.any()) == (kind != "none")
    for k in ("out", "out_lo"):
        if got[k] is None:
            continue
        assert got[k].guards_untouched(), k
        assert torch.equal(got[k].t[~dead], ref[k].t[~dead]), k
        assert not bool((got[k].t[dead] != 0).any()), k
    dl = dead.view(B, 1, N).expand(B, nH, N).reshape(B * nH, N)
    assert got["lse"].guards_untouched() and got["rawlog"].guards_untouched()
    assert torch.equal(got["lse"].t[~dl], ref["lse"].t[~dl])
    assert bool((got["lse"].t[dl] == 0).all())
    assert torch.equal(got["rawlog"].buf, ref["rawlog"].buf)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["none", "patch", "whole"])
@pytest.mark.parametrize("B,N,nH,T", ATTN_SHAPES)
def test_attention_backward_block_skip(B, N, nH, T, kind):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    lib = pkg()._lib
    g = torch.Generator().manual_seed(24)
    C = nH * 64
    qkv = _rnd(g, B * N, 3 * C, dtype=torch.bfloat16)
    table = _attn_table(B, kind)
    fw = _attn_fwd(qkv, None, B, N, nH, T, None)
    out, lse = fw["out"].t.contiguous(), fw["lse"].t.contiguous().view(B, nH, N)
    r = torch.arange(N)
    dead_rows = torch.stack([table[b, (r >= T).long()] == 0.0 for b in range(B)]).reshape(-1).cuda()      # where the DropPath scale zeroes dout
    dout = _rnd(g, B * N, C, dtype=torch.bfloat16)
    dout[dead_rows] = 0
    drawlog = _rnd(g, B, nH, T, N) * 0.05
    fdead = _fwd_dead_rows(table, B, N, T).cuda()

    def run(skipping):
        o, l = out.clone(), lse.clone()
        if skipping:                                        # what the skipping forward never wrote must not be read
            o[fdead] = float("nan")
            l.view(B, nH, N)[fdead.view(B, 1, N).expand(B, nH, N)] = float("nan")
        dqkv = Guarded(B * N, 3 * C, 3 * C, torch.bfloat16)
        stat = torch.full((B, nH, 2, (N + 3) // 4 * 4), float("nan"), device="cuda")
        kw = dict(qkv=qkv, out=o, rawlog=None, lse=l, B=B, N=N, nH=nH, T=T, dtype=BF16, prec=0, scale=0.125, xargs=[dout, drawlog, dqkv.t, stat])
        if skipping:
            kw.update(skip_scale=table.cuda())
        lib.call("attn_bwd", **kw)
        torch.cuda.synchronize()
        return dqkv

    ref, got = run(False), run(True)
    assert ref.guards_untouched() and got.guards_untouched()
    assert not bool(torch.isnan(got.buf.float()).any())
    assert torch.equal(got.buf, ref.buf), int((got.buf != ref.buf).sum())


# ---------------------------------------------------------------------------------------------------------------------------------
def drop_override(depth=4, B=2):
    """[4, B] mask / keep tables per block (rows: attention patch, MLP patch, attention prompt, MLP prompt draws) with dead draws of each of
    the four kinds, whole-batch dead branches (the only wholly dead row tiles at the miniature's 60 token rows) and an untouched block"""
    k = 1.0 / 0.7
    d = [torch.full((4, B), k) for _ in range(depth)]
    d[0][0, 1] = 0.0                   # attention patch rows of image 1
    d[0][3, 0] = 0.0                   # MLP prompt rows of image 0
    d[1][0] = 0.0
    d[1][2] = 0.0                      # attention branch: everything dead
    d[2][1] = 0.0
    d[2][3] = 0.0                      # MLP branch: everything dead
    d[3][1, 0] = 0.0                   # MLP patch rows of image 0
    d[3][2, 1] = 0.0                   # attention prompt rows of image 1
    return d


def model_step(prec, device, call_fn, drop_skip, training=True, gemm_variant=None):
    """one mini_ctr training step under drop_override() -> (heads, loss, grads) as CPU tensors"""
    import conftest
    import mtt_amd
    from oracle import configs, weights
    ops, ap = mtt_amd.ops, mtt_amd.autograd_path
    cfg = configs.taskprompter("mini_ctr")
    contract = conftest.load_golden("mini_ctr")[0]["contract"]
    sd = weights.synth_state_dict(contract, 0)
    saved = ops.call, ap.DROP_SKIP, ops.GEMM_VARIANT
    ops.call, ap.DROP_SKIP, ops.GEMM_VARIANT = call_fn, drop_skip, gemm_variant
    ops.clear_pack_cache()
    try:
        model = conftest.build_product_model(cfg, prec, device, drop_path_rate=0.3)
        model.load_state_dict({k: v.to(device) for k, v in sd.items()}, strict=True)
        model.train(training)
        model.backbone._drop_override = drop_override()
        x = weights.synth_images(2, cfg["img_size"], 2).to(device)
        if not training:
            with torch.no_grad():
                return {k: v.cpu() for k, v in model(x).items()}, None, None
        out = {k: v.cpu() for k, v in model(x).items()}
        loss = train_check.loss_of(out)
        loss.backward()
        return ({k: v.detach() for k, v in out.items()}, loss.detach(),
                {k: (None if p.grad is None else p.grad.detach().cpu()) for k, p in model.named_parameters()})
    finally:
        ops.call, ap.DROP_SKIP, ops.GEMM_VARIANT = saved
        ops.clear_pack_cache()


def assert_steps_equal(a, b):
    (ha, la, ga), (hb, lb, gb) = a, b
    for k in ha:
        assert torch.equal(ha[k], hb[k]), k
    assert torch.equal(la, lb)
    assert set(ga) == set(gb)
    for k in ga:
        assert (ga[k] is None) == (gb[k] is None), k
        if ga[k] is not None:
            assert torch.isfinite(ga[k]).all(), k
            assert torch.equal(ga[k], gb[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("gemm_variant", [None, 3])
@pytest.mark.parametrize("prec", ["x3f", "bf16"])
def test_model_step_equal_with_and_without_skipping(prec, gemm_variant):
    """gemm_variant 3 puts the miniature's GEMMs on the 256-row LDS-DMA kernels, where the whole-batch dead branches are dead tiles"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import mtt_amd
    call = mtt_amd.ops.call
    on = model_step(prec, "cuda", call, True, gemm_variant=gemm_variant)
    off = model_step(prec, "cuda", call, False, gemm_variant=gemm_variant)
    assert_steps_equal(on, off)
