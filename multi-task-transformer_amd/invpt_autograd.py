"""InvPT's forward (InvPT/models/transformers/vit.py, transformer_decoder.py, invpt.py, InvPT/models/transformer_net.py), stated once
for inference and training: the ViT (vit_taps), the decoder (decoder_forward) and TransformerNet.forward (net_forward).  `keep` = somebody
will differentiate the result: the launches then run inside torch.autograd.Functions whose backward runs on the libmtt_hip.so kernels
too; otherwise the same launch bodies run alone.

A launch body (convt3x3s2, dwconv_s2, avgpool_ceil, scores, attn_msg, softmax, pv, resize_add) is written once, for padded widths (Dp,
hdp, Kp: any channel count); its Function calls it and saves what the backward needs.  Only the backward kernels need widths that are
their own pitch (_check8, raised under `keep` alone: true for every published config, 576/288/144, heads 2).  Where the two schedules
really differ — BatchNorm folded into the conv epilogue in eval, the row-group projections, layernorm_mt, the skip add, the block's MLP,
the head node, the mix projections — decoder_forward / _block say so at the branch.

Shared with the TaskPrompter training path (autograd_path.py): LayerNormFn, AttnHalfFn (no prompt rows), MlpHalfFn, BLinearFn,
Conv3x3Fn (dilated, bias-free), BnActStackFn, BilinearFn, ConvHeadFn, TaskHeadsFn.  With gradients torch ops are plumbing between
Functions only (permuted copies between task-major and batch-major token order, fp32 residual adds).
"""
import torch
from torch.autograd import Function

from . import bn as bn_mod
from . import ops
from ._lib import ACT_GELU, ACT_NONE, ACT_RELU, F32, OP_R, dtype_code
from . import autograd_path
from .autograd_path import (MlpHalfFn, BLinearFn, BilinearFn, Conv3x3Fn, ConvHeadFn, LayerNormFn, TaskHeadsFn, _bn_act,
                            _colsum, _dgrad, _gemm, _pad_last, _wgrad, block_attn, block_mlp, patch_embed)

pitch = ops.pitch


# =================================================================================================
def vit_embed(img, Wpe, bpe, pos, cls, geo, prec):
    """VitEmbedFn's launches -> (XT, patch columns): autograd_path.patch_embed with the class token + its position in row 0"""
    B, N, hw = geo
    return patch_embed(img, Wpe, bpe, pos, cls + pos[:, :1], (B, N, 1, hw), prec, 'vpe')


class VitEmbedFn(Function):
    """patchify + k=s=16 conv as GEMM + pos-embed add, class token in row 0 (vit.py:326-333)."""

    @staticmethod
    def forward(ctx, img, Wpe, bpe, pos, cls, geo, prec):
        XT, cols = vit_embed(img, Wpe, bpe, pos, cls, geo, prec)
        ctx.save_for_backward(cols)
        ctx.geo, ctx.prec, ctx.wshape = geo, prec, Wpe.shape
        return XT

    @staticmethod
    def backward(ctx, dXT):
        (cols,) = ctx.saved_tensors
        B, N, hw = ctx.geo
        C = ctx.wshape[0]
        d3 = dXT.contiguous().view(B, N, C)
        dpatch = d3[:, 1:].reshape(B * hw, C)
        dW = _wgrad(dpatch, cols, C, 768, ctx.prec.bwd).view(ctx.wshape)
        db = _colsum(dpatch, C)
        dpos = d3.sum(0, keepdim=True)
        return None, dW, db, dpos, d3[:, :1].sum(0, keepdim=True), None, None


def _run(keep, Fn, body, *args):
    """a launch body as an autograd node (keep) or alone"""
    return Fn.apply(*args) if keep else body(*args)


def _convt_wall(weight, prec):
    """ConvTranspose2d weight [C, Co, 3, 3] -> its nine tap matrices stacked as one Linear [1, 9*pitch(Co), pitch(C)] (cached)"""
    C, Co = weight.shape[0], weight.shape[1]
    Cop = pitch(Co)

    def build():
        with torch.no_grad():
            buf = torch.zeros(9, Cop, C, dtype=torch.float32, device=weight.device)
            buf[:, :Co] = weight.detach().permute(2, 3, 1, 0).reshape(9, Co, C)           # [ci, co, ky, kx] -> [tap, co, ci]
            return ops.pack_matrix(buf.reshape(9 * Cop, C), prec)[None]
    return ops._cached(('se0', prec.name, id(weight)), [weight], build)


def convt3x3s2(x, weight, bias, geo, prec):
    """ConvTranspose2d(k=3, s=2, p=1, output_padding=1) (transformer_decoder.py:60): one GEMM producing the 9 tap
    products per input pixel, then a gather (+bias) into the 2x map.  x [B*H*W, C] -> [B*2H*2W, pitch(Co)]."""
    B, H, W = geo
    Co = weight.shape[1]
    Cop = pitch(Co)
    yall = ops.linear(x, _convt_wall(weight, prec), 9 * Cop, prec, ldd=9 * Cop)[0]
    bpad = ops._cached(('se0b', id(bias)), [bias], lambda: torch.cat([bias.detach(), bias.detach().new_zeros(Cop - Co)]).contiguous())
    out = torch.empty(B * 4 * H * W, Cop, dtype=prec.adt, device=x.device)
    ops.call("convt3x3s2_gather", yall=yall, out=out, bias=bpad, B=B, H=H, W=W, Cop=Cop, dtype=dtype_code(yall),
             out_dtype=dtype_code(out))
    return out


class ConvT3x3s2Fn(Function):
    @staticmethod
    def forward(ctx, x, weight, bias, geo, prec):
        ctx.save_for_backward(x, _convt_wall(weight, prec))
        ctx.meta = (geo, prec, weight.shape[0], weight.shape[1], pitch(weight.shape[1]))
        return convt3x3s2(x, weight, bias, geo, prec)

    @staticmethod
    def backward(ctx, dout):
        x, wall = ctx.saved_tensors
        (B, H, W), prec, C, Co, Cop = ctx.meta
        prec = prec.bwd
        dout = dout.contiguous()
        dyall = torch.empty(B * H * W, 9 * Cop, dtype=dout.dtype, device=dout.device)
        ops.call("convt3x3s2_gather_bwd", yall=None, out=None, bias=None, B=B, H=H, W=W, Cop=Cop, dtype=dtype_code(dyall),
                 out_dtype=dtype_code(dout), xargs=[dout, dyall])
        dWall = _wgrad(dyall, x, 9 * Cop, x.shape[1], prec)                                  # [9*Cop, C]
        dweight = dWall.view(9, Cop, -1)[:, :Co, :C].permute(2, 1, 0).reshape(C, Co, 3, 3)
        dx = _dgrad(dyall, wall[0], B * H * W, x.shape[1], 9 * Cop, prec, x.dtype)
        return dx, dweight, _colsum(dout, Co), None, None


def _dw_pack(ws, Dp):
    """T depthwise weights [D, 1, 3, 3] -> fp32 [T, 9, Dp], zero padded (cached: a parameter update hands out a fresh tensor, so a
    backward may save it)"""
    def build():
        with torch.no_grad():
            out = torch.zeros(len(ws), 9, Dp, dtype=torch.float32, device=ws[0].device)
            for z, wt in enumerate(ws):
                out[z, :, :wt.shape[0]] = wt.detach().reshape(wt.shape[0], 9).t()
            return out
    return ops._cached(('dwq', tuple(id(w) for w in ws)), list(ws), build)


def dwconv_s2(x, geo, *ws, scale=None, shift=None):
    """Per-task depthwise 3x3 stride-2 conv, bias-free (invpt.py:44-52 conv_proj_q), optionally * scale + shift [T, Dp] (a folded
    BatchNorm).  x [T, B*H*W, Dp] -> [T, B*Ho*Wo, Dp]."""
    B, H, W = geo
    T, _, Dp = x.shape
    y = torch.empty(T, B * ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1), Dp, dtype=x.dtype, device=x.device)
    ops.call("dwconv3x3s2", x=x, w=_dw_pack(ws, Dp), y=y, scale=scale, shift=shift, Z=T, B=B, H=H, W=W, ld=Dp, dtype=dtype_code(x))
    return y


class DwConvS2Fn(Function):
    @staticmethod
    def forward(ctx, x, geo, *ws):
        ctx.save_for_backward(x, _dw_pack(ws, x.shape[-1]))
        ctx.geo = geo
        return dwconv_s2(x, geo, *ws)

    @staticmethod
    def backward(ctx, dy):
        x, wq = ctx.saved_tensors
        B, H, W = ctx.geo
        T, _, D = x.shape
        dy = dy.contiguous()
        dx, dw = torch.empty_like(x), torch.empty_like(wq)
        ops.call("dwconv3x3s2_bwd", x=x, w=wq, y=None, scale=None, shift=None, Z=T, B=B, H=H, W=W, ld=D, dtype=dtype_code(x),
                 xargs=[dy, dx, dw])
        return (dx, None) + tuple(dw[t].t().reshape(D, 1, 3, 3) for t in range(T))


def avgpool_ceil(x, geo):
    """AvgPool2d(k, stride k, ceil_mode=True) on NHWC maps (invpt.py:54-66): x [Z, B*H*W, Dp] -> [Z, B*Ho*Wo, Dp]."""
    B, H, W, k = geo
    Z, _, Dp = x.shape
    y = torch.empty(Z, B * -(-H // k) * -(-W // k), Dp, dtype=x.dtype, device=x.device)
    ops.call("avgpool_ceil", x=x, y=y, B=Z * B, H=H, W=W, k=k, ld=Dp, dtype=dtype_code(x))
    return y


class AvgPoolFn(Function):
    @staticmethod
    def forward(ctx, x, geo):
        ctx.meta = (geo, x.shape)
        return avgpool_ceil(x, geo)

    @staticmethod
    def backward(ctx, dy):
        (B, H, W, k), xshape = ctx.meta
        dy = dy.contiguous()
        dx = torch.empty(xshape, dtype=dy.dtype, device=dy.device)
        ops.call("avgpool_ceil_bwd", x=None, y=None, B=xshape[0] * B, H=H, W=W, k=k, ld=xshape[2], dtype=dtype_code(dy), xargs=[dy, dx])
        return dx, None


def _heads_kw(B, heads):
    return dict(batch=B * heads, batch_inner=heads)


def scores(q, k, heads, hdp, alpha, prec):
    """S[b, h] = alpha * q[b, :, h] k[b, :, h]^T on batch-major q [B, Q, heads*hdp], k [B, K, heads*hdp] (heads = column blocks of
    width hdp); fp32 scores [B, heads, Q, pitch(K)] (invpt.py:205)."""
    B, Q, Dh = q.shape
    K = k.shape[1]
    Kp = pitch(K)
    S = torch.empty(B, heads, Q, Kp, dtype=torch.float32, device=q.device)
    return _gemm(q, k, S, Q, K, hdp, prec, lda=Dh, ldb=Dh, ldd=Kp, a_zo=Q * Dh, a_zi=hdp, b_zo=K * Dh, b_zi=hdp, d_zo=heads * Q * Kp,
                 d_zi=Q * Kp, alpha=alpha, n_store=Kp, **_heads_kw(B, heads))


class ScoresFn(Function):
    @staticmethod
    def forward(ctx, q, k, heads, hdp, alpha, prec):
        ctx.save_for_backward(q, k)
        ctx.meta = (heads, alpha, prec)
        return scores(q, k, heads, hdp, alpha, prec)

    @staticmethod
    def backward(ctx, dS):
        q, k = ctx.saved_tensors
        heads, alpha, prec = ctx.meta
        prec = prec.bwd
        B, Q, D = q.shape
        K = k.shape[1]
        hd, Kp = D // heads, pitch(K)
        dS = dS.contiguous()
        dq, dk = torch.empty_like(q), torch.empty_like(k)
        zs = dict(a_zo=heads * Q * Kp, a_zi=Q * Kp, **_heads_kw(B, heads))
        _gemm(dS, k, dq, Q, hd, K, prec, b_op=OP_R, lda=Kp, ldb=D, ldd=D, b_zo=K * D, b_zi=hd, d_zo=Q * D, d_zi=hd, alpha=alpha,
              n_store=hd, **zs)
        _gemm(dS, q, dk, K, hd, Q, prec, a_op=OP_R, b_op=OP_R, lda=Kp, ldb=D, ldd=D, b_zo=Q * D, b_zi=hd, d_zo=K * D, d_zi=hd,
              alpha=alpha, n_store=hd, **zs)
        return dq, dk, None, None, None, None


def softmax(S, K, prec):
    """Row softmax over the K valid columns of fp32 scores [B, heads, Q, pitch(K)] -> P (activation dtype)."""
    P = torch.empty(S.shape, dtype=prec.adt, device=S.device)
    ops.call("softmax_fwd", S=S, P=P, rows=S.numel() // S.shape[-1], cols=K, ld=S.shape[-1], s_dtype=F32, p_dtype=dtype_code(P),
             scale=1.0)
    return P


class SoftmaxFn(Function):
    @staticmethod
    def forward(ctx, S, K, prec):
        P = softmax(S, K, prec)
        ctx.save_for_backward(P)
        ctx.K = K
        return P

    @staticmethod
    def backward(ctx, dP):
        (P,) = ctx.saved_tensors
        dP = dP.contiguous().float()
        dS = torch.zeros_like(dP)
        ops.call("softmax_bwd", P=P, dP=dP, dS=dS, extra=None, rows=P.numel() // P.shape[-1], cols=ctx.K, ld=P.shape[-1], s_dtype=F32,
                 p_dtype=dtype_code(P), scale=1.0, rows_per_mat=P.shape[-2], extra_rows=0, extra_ld=0)
        if P.shape[-1] != ctx.K:
            dS[..., ctx.K:] = 0
        return dS, None, None


def pv(P, v, hdp, prec):
    """o[b, :, h] = P[b, h] v[b, :, h]  -> [B, Q, heads*hdp] (heads concatenated along channels, invpt.py:234-235)."""
    B, heads, Q, Kp = P.shape
    K, Dh = v.shape[1], v.shape[2]
    o = torch.empty(B, Q, Dh, dtype=prec.adt, device=P.device)
    return _gemm(P, v, o, Q, hdp, K, prec, b_op=OP_R, lda=Kp, ldb=Dh, ldd=Dh, a_zo=heads * Q * Kp, a_zi=Q * Kp, b_zo=K * Dh, b_zi=hdp,
                 d_zo=Q * Dh, d_zi=hdp, n_store=hdp, **_heads_kw(B, heads))


class PVFn(Function):
    @staticmethod
    def forward(ctx, P, v, hdp, prec):
        ctx.save_for_backward(P, v)
        ctx.prec = prec
        return pv(P, v, hdp, prec)

    @staticmethod
    def backward(ctx, do):
        P, v = ctx.saved_tensors
        prec = ctx.prec.bwd
        B, heads, Q, Kp = P.shape
        K, D = v.shape[1], v.shape[2]
        hd = D // heads
        do = do.contiguous()
        dP = torch.empty(B, heads, Q, Kp, dtype=torch.float32, device=P.device)
        _gemm(do, v, dP, Q, K, hd, prec, lda=D, ldb=D, ldd=Kp, a_zo=Q * D, a_zi=hd, b_zo=K * D, b_zi=hd, d_zo=heads * Q * Kp,
              d_zi=Q * Kp, n_store=Kp, **_heads_kw(B, heads))
        dv = torch.empty_like(v)
        _gemm(P, do, dv, K, hd, Q, prec, a_op=OP_R, b_op=OP_R, lda=Kp, ldb=D, ldd=D, a_zo=heads * Q * Kp, a_zi=Q * Kp, b_zo=Q * D,
              b_zi=hd, d_zo=K * D, d_zi=hd, n_store=hd, **_heads_kw(B, heads))
        return dP, dv, None, None


def attn_msg(S, prev, weight, bias, geo):
    """Attention message passing (invpt.py:208-229): the previous stage's scores, bilinearly upsampled x2 over each task's query grid,
    and the current scores are mixed over heads by the 1x1 conv `fuse_attn` — one fused kernel (mtt_attn_msg)."""
    B, heads, T, qh, qw, K = geo
    out = torch.empty_like(S)
    ops.call("attn_msg", cur=S, prev=prev, out=out, w=weight.detach().reshape(heads, 2 * heads).contiguous(), bias=bias.detach(), B=B,
             heads=heads, T=T, qh=qh, qw=qw, K=K, ldk=S.shape[-1], ldkp=prev.shape[-1])
    return out


class FuseAttnFn(Function):
    """attn_msg with its one fused kernel backward (mtt_attn_msg_bwd: dcur, the upsampled-space gradient, dW, dbias) + the
    bilinear-backward gather for dprev."""

    @staticmethod
    def forward(ctx, S, prev, weight, bias, geo):
        S, prev = S.contiguous(), prev.contiguous()
        ctx.save_for_backward(S, prev, weight.detach().reshape(geo[1], 2 * geo[1]).contiguous())
        ctx.geo, ctx.wshape = geo, weight.shape
        return attn_msg(S, prev, weight, bias, geo)

    @staticmethod
    def backward(ctx, dout):
        S, prev, w2 = ctx.saved_tensors
        B, heads, T, qh, qw, K = ctx.geo
        dout = dout.contiguous()
        dcur, dup = torch.empty_like(S), torch.empty_like(S)
        if S.shape[-1] > K:                                            # padded key columns carry no gradient
            dcur[..., K:] = 0
            dup[..., K:] = 0
        dw = torch.empty(heads, 2 * heads, dtype=torch.float32, device=S.device)
        db = torch.empty(heads, dtype=torch.float32, device=S.device)
        ops.call("attn_msg_bwd", cur=S, prev=prev, out=None, w=w2, bias=None, B=B, heads=heads, T=T, qh=qh, qw=qw, K=K,
                 ldk=S.shape[-1], ldkp=prev.shape[-1],
                 xargs=[dout, dcur, dup, dw, db, ops.ws_for("attn_msg_bwd", S.device, B=B, heads=heads, T=T, qh=qh, qw=qw, K=K)])
        Kp = prev.shape[-1]
        dprev = torch.zeros_like(prev)
        ops.call("bilinear_bwd", **{"in": dup}, out=dprev, B=B * heads * T, C=min(Kp, S.shape[-1]), Hin=qh // 2, Win=qw // 2, Hout=qh, Wout=qw,
                 ld_in=Kp, ld_out=S.shape[-1], in_dtype=F32, out_dtype=F32, out_nchw=0, accumulate=1)
        return dcur, dprev, dw.view(ctx.wshape), db, None


# =================================================================================================
def resize_add(y, acc, B, size, target, accumulate):
    """acc (+)= bilinear(y -> target) for a task stack y [T, B*gh*gw, ld] and fp32 acc [T, B*th*tw, ld]: the sum happens inside the
    kernel (mtt_resize_desc.accumulate)."""
    T, _, ld = y.shape
    assert acc.shape[0] == T and acc.shape[2] == ld and y.is_contiguous()
    ops.call("bilinear_fwd", **{"in": y}, out=acc, B=T * B, C=ld, Hin=size[0], Win=size[1], Hout=target[0], Wout=target[1], ld_in=ld,
             ld_out=ld, in_dtype=dtype_code(y), out_dtype=F32, out_nchw=0, accumulate=accumulate)


class MultiScaleSumFn(Function):
    """acc = sum_i bilinear(y_i -> (th, tw)) over the InvPT stages' task stacks y_i [T, B*gh_i*gw_i, ld] (invpt.py:531-536: every stage's
    normalised features resized to the target resolution and summed) as ONE node: the first resize writes the fp32 sum buffer, the others
    accumulate into it inside the kernel — no separate [T, B*th*tw, ld] tensor per stage and no add passes
    (2 x 21.6 GB of traffic at the cfg4 batch); a stage that already has the target resolution is added / differentiated as the identity
    it is (its backward hands the incoming gradient through instead of running the adjoint resize)."""

    @staticmethod
    def forward(ctx, geo, *ys):
        B, C, th, tw, sizes = geo
        T, _, ld = ys[0].shape
        acc = torch.empty(T, B * th * tw, ld, dtype=torch.float32, device=ys[0].device)
        for i, (y, size) in enumerate(zip(ys, sizes)):
            resize_add(y, acc, B, size, (th, tw), 1 if i else 0)
        ctx.meta = (geo, [(tuple(y.shape), y.dtype) for y in ys])
        return acc

    @staticmethod
    def backward(ctx, dacc):
        (B, C, th, tw, sizes), metas = ctx.meta
        dacc = dacc.contiguous()
        outs = []
        for (shape, dtype), (gh, gw) in zip(metas, sizes):
            ld = shape[2]
            if (gh, gw) == (th, tw):
                outs.append(dacc if dtype == torch.float32 else ops.cast2d(dacc.view(-1, ld), dacc.numel() // ld, ld, ld, dtype, ldd=ld).view(shape))
                continue
            din = torch.zeros(shape, dtype=torch.float32, device=dacc.device)
            ops.call("bilinear_bwd", **{"in": dacc}, out=din, B=shape[0] * B, C=ld, Hin=gh, Win=gw, Hout=th, Wout=tw, ld_in=ld, ld_out=ld,
                     in_dtype=F32, out_dtype=F32, out_nchw=0, accumulate=1)
            outs.append(din if dtype == torch.float32 else ops.cast2d(din.view(-1, ld), din.numel() // ld, ld, ld, dtype, ldd=ld).view(shape))
        return (None,) + tuple(outs)


def _check8(*dims):
    if any(d != pitch(d) for d in dims):
        raise NotImplementedError("InvPT training path needs channel / head dims that are their own channel pitch (multiples of 8; of 32 from "
                                  f"{ops.PITCH32_FROM} channels on), got {dims}")


def vit_taps(vit, img, keep):
    """VisionTransformer.forward_taps (vit.py:326-349): the ViT's one forward.  keep: somebody will differentiate it (autograd nodes around
    the launches); otherwise the same launches alone (autograd_path.block_attn / block_mlp).  x3f: the four big Linears of a block on the
    split-plane LDS-DMA kernel, operands written as hi / lo planes by LayerNorm, the qkv / fc1 epilogues and the attention kernel."""
    prec = vit.prec
    B = img.shape[0]
    C, nH = vit.embed_dim, vit.num_heads
    hw = vit.patch_embed.num_patches
    N = hw + 1
    embed = (img, vit.patch_embed.proj.weight, vit.patch_embed.proj.bias, vit.pos_embed, vit.cls_token, (B, N, hw), prec)
    XT = VitEmbedFn.apply(*embed) if keep else vit_embed(*embed)[0]
    taps = []
    for i, blk in enumerate(vit.blocks):
        a = blk.attn
        XT = block_attn(keep, None, XT, blk.norm1.weight, blk.norm1.bias, blk.norm1.eps, a.qkv.weight, a.qkv.bias, a.proj.weight, a.proj.bias,
                        None, None, None, None, None, (B, N, nH, 0, 0, 0, 1), prec, ('vblk', i))[0]
        XT = block_mlp(keep, None, XT, blk.norm2.weight, blk.norm2.bias, blk.norm2.eps, blk.mlp.fc1.weight, blk.mlp.fc1.bias,
                       blk.mlp.fc2.weight, blk.mlp.fc2.bias, None, (B, N, 0), prec, ('vblk', i))
        if (i + 1) in vit.select_list:
            taps.append(XT.view(B, N, C)[:, 1:].to(prec.adt).reshape(B * hw, C))
    xf = autograd_path.layernorm(XT, vit.norm.weight, vit.norm.bias, vit.norm.eps, prec, None, keep)
    taps.append(xf.view(B, N, C)[:, 1:].reshape(B * hw, C))
    return taps


# =================================================================================================
def _ln_padded(Xf, norm, D, prec):
    """LayerNorm over the D valid channels of fp32 [T, rows, Dp] -> activation dtype [T, rows, Dp] with zero padding."""
    T, rows, Dp = Xf.shape
    y = (torch.zeros if Dp != D else torch.empty)(T * rows, Dp, dtype=prec.adt, device=Xf.device)
    if D % 4 == 0:
        ops.call("layernorm_fwd", x=Xf, y=y, gamma=norm.weight.detach(), beta=norm.bias.detach(), mean=None, rstd=None,
                 rows=T * rows, C=D, ldx=Dp, ldy=Dp, y_dtype=dtype_code(y), eps=norm.eps)
    else:   # odd channel counts (miniature configs): the multi-task LN kernel with T = 1 handles any D
        ops.call("layernorm_mt", x=Xf, y=y, gamma=norm.weight.detach(), beta=norm.bias.detach(), rows=T * rows, T=1, D=D, ldx=Dp, ldy=Dp,
                 y_dtype=dtype_code(y), eps=norm.eps)
    return y.view(T, rows, Dp)


def _proj_in(src, lin, geo, tag, prec):
    """A shared-weight Linear on task-major maps src [T, B*n, Dp] -> batch-major [B, T*n, heads*hdp] through the GEMM's row-group output
    mapping; the weight rows re-laid as heads padded to hdp (a layout of this schedule alone: cached, not in the pack registry)."""
    B, T, n, D, heads, hdp = geo
    hd, Dh, Dp = D // heads, heads * hdp, src.shape[-1]

    def build():
        with torch.no_grad():
            Wt = torch.zeros(Dh, D, dtype=torch.float32, device=lin.weight.device)
            bt = torch.zeros(Dh, dtype=torch.float32, device=lin.weight.device)
            for hh in range(heads):
                Wt[hh * hdp:hh * hdp + hd] = lin.weight.detach()[hh * hd:(hh + 1) * hd]
                if lin.bias is not None:
                    bt[hh * hdp:hh * hdp + hd] = lin.bias.detach()[hh * hd:(hh + 1) * hd]
            return ops.pack_matrix(Wt, prec), bt
    wpk, bpk = ops._cached(tag + (prec.name, id(lin.weight)), [lin.weight] + ([lin.bias] if lin.bias is not None else []), build)
    out = torch.empty(B, T * n, Dh, dtype=prec.adt, device=src.device)
    return _gemm(src, wpk, out, B * n, Dh, wpk.shape[-1], prec, lda=Dp, ldb=wpk.shape[-1], ldd=Dh, d_mb=n, d_bs=T * n * Dh, batch=T,
                 a_zo=B * n * Dp, b_zo=0, d_zo=n * Dh, colshift=bpk, n_store=Dh)


def _proj_out(o, lin, geo, tag, prec):
    """The output projection of batch-major o [B, T*n, heads*hdp] back to task-major maps [T, B*n, pitch(D)] (row-group input mapping)."""
    B, T, n, D, heads, hdp = geo
    hd, Dh, Dp = D // heads, heads * hdp, pitch(D)

    def build():
        with torch.no_grad():
            Wt = torch.zeros(D, Dh, dtype=torch.float32, device=lin.weight.device)
            for hh in range(heads):
                Wt[:, hh * hdp:hh * hdp + hd] = lin.weight.detach()[:, hh * hd:(hh + 1) * hd]
            return ops.pack_matrix(Wt, prec)
    wpo = ops._cached(tag + (prec.name, id(lin.weight)), [lin.weight], build)
    om = torch.empty(T, B * n, Dp, dtype=prec.adt, device=o.device)
    return _gemm(o, wpo, om, B * n, D, Dh, prec, lda=Dh, ldb=wpo.shape[-1], ldd=Dp, a_mb=n, a_bs=T * n * Dh, batch=T, a_zo=n * Dh, b_zo=0,
                 d_zo=B * n * Dp, colshift=lin.bias.detach(), n_store=Dp)


def _to_batch_major(x, T, B, n):
    """[1, T*B*n, D] task-major rows -> [B, T*n, D]."""
    D = x.shape[-1]
    return x.view(T, B, n, D).permute(1, 0, 2, 3).reshape(B, T * n, D)


def _block(dec, blk, si, Xf, B, T, D, gh, gw, prev_score, keep):
    """InvPTBlock (invpt.py:290-312) on task-major fp32 tokens Xf [T, B*g*g, pitch(D)].  Returns (new Xf, attention scores)."""
    prec, at = dec.prec, blk.attn
    heads = at.num_heads
    Dp, hdp = Xf.shape[-1], pitch(D // heads)
    rows = B * gh * gw
    qh, qw = (gh - 1) // 2 + 1, (gw - 1) // 2 + 1
    kk = 2 ** (si + 1)
    nq, nk = qh * qw, -(-gh // kk) * -(-gw // kk)
    K = T * nk
    tag = ('ipb', si)
    # norm1 / norm2 / MLP: LayerNormFn and MlpHalfFn have the backward; without gradients odd widths need _ln_padded's layernorm_mt fallback
    if keep:
        xn = LayerNormFn.apply(Xf.view(T * rows, D), blk.norm1.weight, blk.norm1.bias, blk.norm1.eps, prec, None).view(T, rows, D)
    else:
        xn = _ln_padded(Xf, blk.norm1, D, prec)
    # queries: depthwise 3x3 stride-2 conv + BN per task; keys / values: ceil-mode average pooling
    wdw, bns = [m.conv.weight for m in at.conv_proj_q], [m.bn for m in at.conv_proj_q]
    if keep or dec.training:
        qmap = _bn_act(_run(keep, DwConvS2Fn, dwconv_s2, xn, (B, gh, gw), *wdw), bns, D, ACT_NONE, dec.training)
    else:   # BatchNorm in eval without gradients: folded into the depthwise conv's epilogue
        sc, sh = bn_mod.fold(bns, None, ('dwqbn', si))
        qmap = dwconv_s2(xn, (B, gh, gw), *wdw, scale=_pad_last(sc, Dp), shift=_pad_last(sh, Dp))
    kvmap = _run(keep, AvgPoolFn, avgpool_ceil, xn, (B, gh, gw, kk))

    def proj(src, lin, n, name):
        if not keep:    # q / k / v / output projections: the row-group mapping writes batch-major tensors directly, but has no backward
            return _proj_in(src, lin, (B, T, n, D, heads, hdp), tag + (name,), prec)
        y = BLinearFn.apply(src.reshape(1, -1, D), D, 'plain', None, None, prec, tag + (name,), None, lin.weight, lin.bias)
        return _to_batch_major(y, T, B, n).contiguous()
    q, k, v = proj(qmap, at.proj_q, nq, 'q'), proj(kvmap, at.proj_k, nk, 'k'), proj(kvmap, at.proj_v, nk, 'v')
    S = _run(keep, ScoresFn, scores, q, k, heads, hdp, float(D) ** -0.5, prec)                     # scale = full dim (invpt.py:92)
    if prev_score is not None:
        ph, pw = (gh // 2 - 1) // 2 + 1, (gw // 2 - 1) // 2 + 1                                   # previous stage's query grid
        assert prev_score.shape[2] == T * ph * pw and prev_score.shape[-1] == S.shape[-1]
        S = _run(keep, FuseAttnFn, attn_msg, S, prev_score, at.fuse_attn.weight, at.fuse_attn.bias, (B, heads, T, qh, qw, K))
    P = _run(keep, SoftmaxFn, softmax, S, K, prec)
    o = _run(keep, PVFn, pv, P, v, hdp, prec)                                                     # [B, T*nq, heads*hdp]
    mlp = blk.mlp
    if keep:                    # the resize as a node + an fp32 add autograd differentiates; without gradients the kernel adds into a copy
        o_tm = o.view(B, T, nq, D).permute(1, 0, 2, 3).reshape(1, T * B * nq, D)
        om = BLinearFn.apply(o_tm, D, 'plain', None, None, prec, tag + ('po',), None, at.proj.weight, at.proj.bias).view(T, B * nq, D)
        X2 = Xf + BilinearFn.apply(om, (B, D, qh, qw, gh, gw), torch.float32, False)
        X3 = MlpHalfFn.apply(X2.view(T * rows, D), blk.norm2.weight, blk.norm2.bias, blk.norm2.eps, mlp.fc1.weight, mlp.fc1.bias,
                             mlp.fc2.weight, mlp.fc2.bias, None, (1, T * rows, 0), prec, tag)
        return X3.view(T, rows, D), S
    # bilinear upsample of the attention output to the stage grid + residual (invpt.py:300-307), summed inside the kernel
    X2 = Xf.clone()
    resize_add(_proj_out(o, at.proj, (B, T, nq, D, heads, hdp), tag + ('po',), prec), X2, B, (qh, qw), (gh, gw), 1)
    xn2 = _ln_padded(X2, blk.norm2, D, prec)
    Hd = mlp.fc1.weight.shape[0]
    hmid = ops.linear(xn2.view(T * rows, Dp), ops.pack_linear([mlp.fc1.weight], prec, tag + ('fc1',)), Hd, prec,
                      bias=mlp.fc1.bias.detach()[None], act=ACT_GELU)[0]
    X3 = torch.empty(T * rows, Dp, dtype=torch.float32, device=Xf.device)
    ops.linear(hmid, ops.pack_linear([mlp.fc2.weight], prec, tag + ('fc2',)), D, prec, bias=mlp.fc2.bias.detach()[None],
               out=X3, resid=X2.view(T * rows, Dp), n_store=Dp)
    return X3.view(T, rows, Dp), S


_zeros = {}


def _zero_bias(n, device):
    """the bias of a BLinearFn that has none; kept outside the pack cache, because its identity is part of a registry key"""
    key = (n, str(device))
    if key not in _zeros:
        _zeros[key] = torch.zeros(n, dtype=torch.float32, device=device)
    return _zeros[key]


def _conv_bn(x, geo, prec, tag, ws, bs, bns, training, keep):
    """Task-stacked conv3x3 (geo = (B, H, W, Co, Ci[, dilation]); bs: its biases or None) -> BatchNorm -> ReLU."""
    B, H, W, Co, Ci = geo[:5]
    if keep or training:        # batch statistics, or a backward: the Functions (under no_grad their conv / bn_stats / bn_apply launches alone)
        y = Conv3x3Fn.apply(x, geo, prec, tag, *ws, *(bs or [None] * len(ws)))
        return _bn_act(y, bns, Co, ACT_RELU, training)
    # BatchNorm in eval without gradients: folded into the conv's epilogue (colscale / bias / act)
    sc, sh = bn_mod.fold(bns, bs, tag + 'bn' if isinstance(tag, str) else (tag[0] + 'bn',) + tag[1:])
    return ops.conv3x3(x, ops.pack_conv3(ws, prec, tag), Co, Ci, B, H, W, prec, dil=geo[5] if len(geo) > 5 else 1, bias=sh, colscale=sc,
                       act=ACT_RELU)


def decoder_forward(dec, taps, B, keep, heads=None):
    """TransformerDecoder + InvPT.forward (transformer_decoder.py:18-98, invpt.py:502-544), the one statement.  taps: 4 contiguous
    [B*hw, C] maps; keep: somebody will differentiate the result.  -> (features [T, B*8mh*8mw, pitch(E)], {task: inter_pred
    [1, B*mh*mw, pitch(n)] fp32}); heads (the MLPHeads, in task order): -> (their predictions [1, B*8mh*8mw, pitch(n)] fp32 per task,
    inter_preds) instead of the features."""
    p, prec = dec.p, dec.prec
    names = p.TASKS.NAMES
    T = len(names)
    h, w = p.spatial_dim[-1]
    mh, mw = p.mtt_resolution
    C = p.backbone_channels[-1]
    Ed = dec.embed_dim
    E = Ed + p.PRED_OUT_NUM_CONSTANT
    dims = [E, E // 2, E // 4]
    stages = dec.invpt.invpt_stages
    if keep:                    # the backward kernels need widths that are their own pitch; the forward bodies do not
        _check8(C, Ed, *dims, *[d // st.blocks[0].attn.num_heads for d, st in zip(dims, stages)])
    training = dec.training
    dev = taps[0].device
    # ---- multi-scale skip features (scale_embed[2] is dead in the reference: skipped) -------------------
    se0, se1 = dec.scale_embed[0], dec.scale_embed[1]
    back0 = _run(keep, ConvT3x3s2Fn, convt3x3s2, taps[0], se0.weight, se0.bias, (B, h, w), prec)   # [B*4hw, pitch(dims[2])]
    back1 = Conv3x3Fn.apply(taps[1][None], (B, h, w, dims[1], C), prec, 'se1', se1.weight, se1.bias)[0]

    # ---- preliminary decoder + intermediate heads (transformer_decoder.py:85-95) --------------------------
    x = BilinearFn.apply(taps[3][None], (B, C, h, w, mh, mw), prec.adt, False)                   # [1, B*mh*mw, C]
    pd = [dec.preliminary_decoder[t] for t in names]
    y = x.repeat(T, 1, 1) if keep else x.expand(T, -1, -1)                                        # (a conv backward reads a materialised stack)
    y = _conv_bn(y, (B, mh, mw, C, C), prec, 'pd0', [m[0].conv.weight for m in pd], None, [m[0].bn1 for m in pd], training, keep)
    y = _conv_bn(y, (B, mh, mw, Ed, C), prec, 'pd1', [m[1].conv.weight for m in pd], None, [m[1].bn1 for m in pd], training, keep)
    inter, xs = {}, []
    y = y.unbind(0)                                                                        # backward = one stack (no per-slice zero fill + add)
    for i, t in enumerate(names):
        n_out = p.TASKS.NUM_OUTPUT[t]
        ih = dec.intermediate_head[t]
        mp = dec.invpt.mix_proj[t][0]                                                      # 1x1 on cat([feature, inter_pred]) (invpt.py:509-513)
        kma, kmb = (pitch(Ed), [(0, 0, Ed)]), (pitch(n_out), [(0, Ed, n_out)])             # its two column ranges as two GEMMs
        if keep:                # ih / mix_proj with gradients: BLinearFn, the two products added by torch
            inter[t] = BLinearFn.apply(y[i][None], n_out, 'plain', None, torch.float32, prec, ('ih', t), None, ih.weight, ih.bias)
            part = BLinearFn.apply(y[i][None], E, 'plain', kma, torch.float32, prec, ('mixa', t), None, mp.weight, mp.bias)
            second = BLinearFn.apply(inter[t].to(prec.adt), E, 'plain', kmb, torch.float32, prec, ('mixb', t), None, mp.weight, _zero_bias(E, dev))
            xs.append(part[0] + second[0])
        else:                   # without: the second GEMM accumulates into the first's output (resid), its fp32 A operand converted while staging
            inter[t] = ops.linear(y[i], ops.pack_linear([ih.weight], prec, ('ih', t)), n_out, prec, bias=ih.bias.detach()[None],
                                  out_dtype=torch.float32)
            part = ops.linear(y[i], ops.pack_kmap([mp.weight], E, *kma, prec, ('mixa', t)), E, prec, bias=mp.bias.detach()[None],
                              out_dtype=torch.float32)[0]
            xs.append(ops.linear(inter[t], ops.pack_kmap([mp.weight], E, *kmb, prec, ('mixb', t)), E, prec, resid=part)[0])
    Xf = torch.stack(xs, 0).float()                                                        # fp32 [T, rows0, pitch(E)]

    # ---- InvPT stages --------------------------------------------------------------------------------------
    th, tw = mh * 8, mw * 8
    acc = None if keep else torch.zeros(T, B * th * tw, pitch(E), dtype=torch.float32, device=dev)
    scales, scale_sizes = [], []
    prev_score = None
    gh, gw = mh, mw
    for i in range(3):
        D, Dp = dims[i], pitch(dims[i])
        if i > 0:
            ue = [m.proj for m in stages[i].patch_embed]
            Din = dims[i - 1]
            # (with gradients the tokens are rounded to the activation dtype before the resize, without by it)
            up = BilinearFn.apply(Xf.to(prec.adt) if keep else Xf, (B, Din, gh, gw, 2 * gh, 2 * gw), prec.adt, False)
            gh, gw = 2 * gh, 2 * gw
            yy = _conv_bn(up, (B, gh, gw, D, Din, 2), prec, ('ue1', i), [m[1].weight for m in ue], None, [m[2] for m in ue], training, keep)
            yy = _conv_bn(yy, (B, gh, gw, D, D, 2), prec, ('ue2', i), [m[4].weight for m in ue], None, [m[5] for m in ue], training, keep)
            skip = back1 if i == 1 else back0                                              # invpt.py:406-411
            if keep:            # the skip add: fp32 torch adds autograd differentiates; without gradients the cast and add kernels
                Xf = yy.float() + skip.float()[None]
            else:
                Xf = torch.empty(T, B * gh * gw, Dp, dtype=torch.float32, device=dev)
                for t in range(T):
                    ops.call("cast2d", args=[yy[t], Xf[t], B * gh * gw, Dp, Dp, Dp, dtype_code(yy), F32, 0])
                    ops.call("add_rows", args=[skip, Xf[t], B * gh * gw, Dp, Dp, Dp, dtype_code(skip), 1.0])
        rows = B * gh * gw
        Xf, prev_score = _block(dec, stages[i].blocks[0], i, Xf, B, T, D, gh, gw, prev_score, keep)
        # LayerNorm over all tasks' channels (invpt.py:526-530), redu_chan (i > 0), resize to the target grid and sum
        nm = dec.invpt.norm_mts[i]
        if keep:                # the all-task LayerNorm: layernorm_mt has no backward — LayerNormFn on the permuted rows [rows, T*D]
            cat = Xf.permute(1, 0, 2).reshape(rows, T * D)
            yn = LayerNormFn.apply(cat, nm.weight, nm.bias, nm.eps, prec, None).view(rows, T, D).permute(1, 0, 2).contiguous()
        else:
            yn = torch.empty(T, rows, Dp, dtype=prec.adt, device=dev)
            ops.call("layernorm_mt", x=Xf, y=yn, gamma=nm.weight.detach(), beta=nm.bias.detach(), rows=rows, T=T, D=D, ldx=Dp, ldy=Dp,
                     y_dtype=dtype_code(yn), eps=nm.eps)
        if i > 0:
            rc = dec.invpt.redu_chan[i]
            if keep:            # (BLinearFn's own split pass would change the launches of a forward without gradients from 2048 rows on)
                yn = BLinearFn.apply(yn, E, 'plain', None, None, prec, ('rc', i), None, *[m.weight for m in rc], *[m.bias for m in rc])
            else:
                yn = ops.linear(yn, ops.pack_linear([m.weight for m in rc], prec, ('rc', i)), E, prec,
                                bias=ops.stack_vec([m.bias for m in rc], (('rc', i), 'b')))
        if keep:                # one node for the whole sum (MultiScaleSumFn); without gradients each stage is added and freed at once
            scales.append(yn)
            scale_sizes.append((gh, gw))
        else:
            resize_add(yn, acc, B, (gh, gw), (th, tw), 1)
    if keep:
        acc = MultiScaleSumFn.apply((B, E, th, tw, tuple(scale_sizes)), *scales)
    # ---- mt_proj: 3x3 conv + BN + ReLU at the target resolution (invpt.py:538-541), the MLPHeads' 1x1 predictions -----------------
    mps = [dec.invpt.mt_proj[t] for t in names]
    cw, cb, bns = [m[0].weight for m in mps], [m[0].bias for m in mps], [m[1] for m in mps]
    pwb = [hd.linear_pred.weight for hd in heads] + [hd.linear_pred.bias for hd in heads] if heads is not None else None
    if keep and heads is not None and autograd_path.FUSE_HEAD_NODE:
        # mt_proj + heads with gradients: ONE node, the 128 x 128 gradient maps of the six tasks stay in the backward's dtype (ConvHeadFn)
        preds = ConvHeadFn.apply(acc.to(prec.adt), ('conv', (B, th, tw, E, E), 'mtp', E, ACT_RELU, 'iph'), prec, training, bns,
                                 *cw, *cb, *[bn.weight for bn in bns], *[bn.bias for bn in bns], *pwb)
        return preds, inter
    if keep or prec.adt == torch.float32:
        accq = acc.to(prec.adt)
    else:                       # (without gradients the cast kernel)
        accq = ops.cast2d(acc.view(-1, acc.shape[-1]), acc.shape[0] * acc.shape[1], acc.shape[-1], acc.shape[-1], prec.adt,
                          ldd=acc.shape[-1]).view(acc.shape)
    f = _conv_bn(accq, (B, th, tw, E, E), prec, 'mtp', cw, cb, bns, training, keep)
    if heads is not None:       # (under no_grad: one GEMM per head)
        return TaskHeadsFn.apply(f, prec, 'iph', *pwb), inter
    return f, inter


def net_forward(net, x, keep):
    """TransformerNet.forward (transformer_net.py:25-38), the one statement; keep as in vit_taps / decoder_forward."""
    img_size = tuple(x.shape[-2:])
    B = x.shape[0]
    hds = [net.heads[t] for t in net.tasks]
    preds, inter = decoder_forward(net.multi_task_decoder, vit_taps(net.backbone, x, keep), B, keep, heads=hds)
    mh, mw = net.p.mtt_resolution
    out = {}
    for t, hd, pred in zip(net.tasks, hds, preds):
        out[t] = BilinearFn.apply(pred, (B, hd.linear_pred.weight.shape[0], 8 * mh, 8 * mw, img_size[0], img_size[1]), torch.float32, True)
    out['inter_preds'] = {t: BilinearFn.apply(inter[t], (B, net.p.TASKS.NUM_OUTPUT[t], mh, mw, img_size[0], img_size[1]),
                                              torch.float32, True) for t in net.tasks}
    return out
