"""TaskPrompterSwin's forward and the autograd nodes of its training path.

`backbone_forward` states the forward of taskprompter_swin.py once — preamble, level loop, task features, multi-scale fusion — for inference
and training.  `keep` (somebody will differentiate it) picks where there really are two schedules: the block and the patch merging (the
autograd graph `_block` / `_merge` below, or the in-place TaskPrompterSwin._block / _merge), the patch embed's form, the cast in front of the
fusion conv and, in eval without gradients, the BatchNorm fold of the task features' tail.  Everything else is a Function applied in both
cases: under `no_grad` it launches and saves nothing.

The heavy operators are the HIP building blocks of the ViT variant (LayerNormFn, BLinearFn, MlpHalfFn, ModulateFn, Conv3x3Fn,
BnActStackFn, BilinearFn, MultiScaleSumFn) plus the Functions here: window gather (forward and adjoint through the same mtt_gather_rows
kernel with the inverse tables), window attention (mtt_winattn_fwd / mtt_winattn_bwd; the relative-position-bias gradient is the window
sum of the kernel's dS, index-added into the table), channel attention (mtt_chanattn_fwd / _bwd), chan_kv as three GEMMs on the
token-major rows (ChanKvFn), the block's residual as one node (BlockResidualFn) and the 3x3 stride-2 convolution of the attention maps.
Prompt / pixel row concatenations are torch ops in the autograd schedule (the in-place one has none).  DropPath: the block's four
independent per-sample draws (taskprompter_swin.py:408-413) scale the attention branch (pixels / prompts) and, through MlpHalfFn's
row-scale epilogue, the MLP branch.
"""
import math
from functools import partial

import torch
from torch.autograd import Function

from . import bn as bn_mod
from . import ops
from . import taskprompter_swin as sw
from ._lib import ACT_GELU, F32, OP_K, OP_R, dtype_code
from .autograd_path import (BilinearFn, BLinearFn, Conv3x3Fn, LayerNormFn, MlpHalfFn, ModulateFn, _bn_act, layernorm)
from .invpt_autograd import MultiScaleSumFn
from .taskprompter_swin import _gather


CHAN_KV_FN = True          # A/B switch: False = chan_kv through BLinearFn on a transposed copy of the pixel rows (rounds 2-5)
WINATTN_BIAST = True       # A/B switch: the transposed bias table for the key-owner pass of the matrix-core window-attention backward (ABI 13)
WINATTN_MFMA = True        # A/B switch: False = the exact fp32 VALU window-attention kernels on fp32 storage (rounds 2-5)


class WindowGatherFn(Function):
    """to_windows=True : image token rows [B*N, C] -> window tokens [B*nW*Nw, C] (shift, zero padding, the T prompts joined to every window)
       to_windows=False: window rows -> image rows [B*N, C]; the T prompt rows are the MEAN over the windows (taskprompter_swin.py:208).
    Each direction's adjoint is the other direction's gather (prompt rows summed / spread by hand)."""

    @staticmethod
    def forward(ctx, x, to_windows, part, rev, geo):
        B, N, T, nW, Nw, C = geo
        ctx.tables, ctx.geo, ctx.to_windows = (part, rev), geo, to_windows
        if to_windows:
            out = torch.empty(B * nW * Nw, C, dtype=x.dtype, device=x.device)
            _gather(x, out, part, nW * Nw, C, C, C, B, N * C, nW * Nw * C)
        else:
            out = torch.empty(B * N, C, dtype=x.dtype, device=x.device)
            _gather(x, out.view(B, N, C)[:, T:], rev, N - T, C, C, C, B, nW * Nw * C, N * C)
            out.view(B, N, C)[:, :T] = x.view(B, nW, Nw, C)[:, :, :T].float().mean(1).to(x.dtype)
        return out

    @staticmethod
    def backward(ctx, dy):
        B, N, T, nW, Nw, C = ctx.geo
        part, rev = ctx.tables
        dy = dy.contiguous()
        if ctx.to_windows:                       # dy: window rows -> d image rows
            dx = torch.empty(B * N, C, dtype=dy.dtype, device=dy.device)
            _gather(dy, dx.view(B, N, C)[:, T:], rev, N - T, C, C, C, B, nW * Nw * C, N * C)
            dx.view(B, N, C)[:, :T] = dy.view(B, nW, Nw, C)[:, :, :T].float().sum(1).to(dy.dtype)
        else:                                    # dy: image rows -> d window rows (padding positions get zero)
            dx = torch.empty(B * nW * Nw, C, dtype=dy.dtype, device=dy.device)
            _gather(dy, dx, part, nW * Nw, C, C, C, B, N * C, nW * Nw * C)
            dx.view(B, nW, Nw, C)[:, :, :T] *= 1.0 / nW
        return dx, None, None, None, None


class MergeGatherFn(Function):
    """PatchMerging's 2x2 concatenation (taskprompter_swin.py:450-456): pixel rows of XT [B*N, C] fp32 -> [B*(N2-T), 4C]."""

    @staticmethod
    def forward(ctx, XT, tables, inv_tables, geo):
        B, N, N2, T, C = geo
        ctx.inv, ctx.geo = inv_tables, geo
        cat = torch.empty(B * (N2 - T), 4 * C, dtype=torch.float32, device=XT.device)
        for k, idx in enumerate(tables):
            _gather(XT, cat[:, k * C:], idx, N2 - T, C, C, 4 * C, B, N * C, (N2 - T) * 4 * C)
        return cat

    @staticmethod
    def backward(ctx, dcat):
        B, N, N2, T, C = ctx.geo
        dcat = dcat.contiguous()
        dXT = torch.zeros(B * N, C, dtype=torch.float32, device=dcat.device)
        for k, inv in enumerate(ctx.inv):        # every pixel receives from exactly one (row, column block): 4 disjoint scatter-style gathers
            _gather(dcat[:, k * C:], dXT.view(B, N, C)[:, T:], inv, N - T, C, 4 * C, C, B, (N2 - T) * 4 * C, N * C, skip_neg=1)
        return dXT, None, None, None


class BlockResidualFn(Function):
    """out = XT + rowscale * branch, prompt rows additionally + s_prompt * tt1 (taskprompter_swin.py:404-413: the attention branch's residual,
    the prompts' channel-attention update and the block's first two DropPath draws) as ONE node: the row concatenations / slices it
    replaces cost a zero-fill, a copy and an accumulate of a token-map-sized gradient each in the backward.
    XT, branch fp32 [B*N, C]; tt1 fp32 [B*T, C] or None; s_pix, s_prompt fp32 [B] per-sample DropPath scales or None (= 1)."""

    @staticmethod
    def forward(ctx, XT, branch, tt1, s_pix, s_prompt, geo):
        B, N, T, C = geo
        rs = None
        if s_pix is not None or s_prompt is not None:
            rs = torch.ones(B, N, 1, dtype=torch.float32, device=XT.device)
            if s_pix is not None:
                rs[:, T:, 0] = s_pix[:, None]
            if s_prompt is not None:
                rs[:, :T, 0] = s_prompt[:, None]
        out = XT + branch if rs is None else torch.addcmul(XT.view(B, N, C), branch.view(B, N, C), rs).view(B * N, C)
        if tt1 is not None:
            t3 = tt1.view(B, T, C)
            out.view(B, N, C)[:, :T] += t3 if s_prompt is None else t3 * s_prompt[:, None, None]
        ctx.geo, ctx.has_tt1 = geo, tt1 is not None
        ctx.save_for_backward(rs, s_prompt)
        return out

    @staticmethod
    def backward(ctx, dout):
        B, N, T, C = ctx.geo
        rs, s_prompt = ctx.saved_tensors
        dout = dout.contiguous()
        dbranch = dout if rs is None else (dout.view(B, N, C) * rs).view(B * N, C)
        dtt1 = None
        if ctx.has_tt1:
            dtt1 = dout.view(B, N, C)[:, :T]
            dtt1 = (dtt1 if s_prompt is None else dtt1 * s_prompt[:, None, None]).reshape(B * T, C)
        return dout, dbranch, dtt1, None, None, None


class WinAttnFn(Function):
    @staticmethod
    def forward(ctx, qkv, table, rel_index, mask, pix, geo, prec=None):
        B, nW, nH, T, ws2, N = geo
        bias = table.detach()[rel_index.view(-1)].view(ws2, ws2, nH).permute(2, 0, 1).contiguous().float()
        # fp32 storage: the backward of the x3f mode is the bf16 one (matrix cores), x3's the exact fp32 kernel
        out, rawlog = sw.winattn_fwd(qkv, bias, mask, pix, geo, WINATTN_MFMA)
        # tensors go through save_for_backward — an OUTPUT kept on ctx directly is a reference cycle (node -> ctx -> out -> grad_fn = node) that
        # is never collected: the step leaked a block's qkv + out (GBs per step at the Swin-B shape) until round 6
        ctx.scalars = dict(nwin=B * nW, nW=nW, nH=nH, T=T, ws2=ws2, dtype=dtype_code(qkv), scale=32 ** -0.5, map_ld=N, map_off=T,
                           mfma=1 if (qkv.dtype == torch.float32 and prec is not None and prec.bwd.name == "bf16" and WINATTN_MFMA) else 0)
        ctx.geo, ctx.has_mask = geo, mask is not None
        biasT = bias.transpose(1, 2).contiguous() if (WINATTN_BIAST and (ctx.scalars["mfma"] or qkv.dtype == torch.bfloat16)) else bias.new_empty(0)
        ctx.save_for_backward(table, qkv, out, bias, pix, rel_index, biasT, *([mask] if mask is not None else []))
        return out, rawlog

    @staticmethod
    def backward(ctx, dout, drawlog):
        B, nW, nH, T, ws2, N = ctx.geo
        table, qkv, out, bias, pix, rel_index, biasT = ctx.saved_tensors[:7]
        kw = dict(ctx.scalars, qkv=qkv, out=out, bias=bias, pix=pix, mask=ctx.saved_tensors[7] if ctx.has_mask else None,
                  biasT=biasT if biasT.numel() else None)
        dqkv = torch.empty_like(qkv)
        dS = torch.empty(B * nW, nH, ws2, ws2, dtype=torch.float32, device=qkv.device)
        dout = dout.contiguous()
        ops.call("winattn_bwd", rawmap=None, xargs=[dout, drawlog.contiguous() if drawlog is not None else None, dqkv, dS], **kw)
        dbias = dS.sum(0).permute(1, 2, 0).reshape(ws2 * ws2, nH)
        dtable = torch.zeros_like(table).index_add_(0, rel_index.view(-1), dbias)
        return dqkv, dtable, None, None, None, None, None


def _chan_split(t, B, nh, nw, wh, ww):          # [B, X, ce] -> [B, nwin, X, wh*ww]   ('b t (nh h nw w) -> b (nh nw) t (h w)')
    return t.view(B, t.shape[1], nh, wh, nw, ww).permute(0, 2, 4, 1, 3, 5).reshape(B, nh * nw, t.shape[1], wh * ww)


class ChanAttnFn(Function):
    """q [B*T, ce] fp32, kv [B, C, 2ce] fp32 (k | v per channel, biases included) -> rawchan [B, T, nwin, C], cx [B*T, ce]."""

    @staticmethod
    def forward(ctx, q, kv, geo):
        B, T, C, ce, nwin = geo
        Cp = ops.pitch(C)
        kvT = torch.zeros(B, 2 * ce, Cp, dtype=torch.float32, device=q.device)
        kvT[:, :, :C] = kv.transpose(1, 2)
        rawchan = torch.empty(B, T, nwin * nwin, C, dtype=torch.float32, device=q.device)
        cx = torch.empty(B * T, ce, dtype=torch.float32, device=q.device)
        ops.call("chanattn_fwd", q=q, kvT=kvT, rawchan=rawchan, cx=cx, B=B, T=T, C=C, ce=ce, nh=nwin, nw=nwin, kv_dtype=0, ldk=Cp,
                 scale=ce ** -0.5, kvbias=None)
        ctx.save_for_backward(q, kvT, rawchan)
        ctx.geo = geo
        return rawchan, cx

    @staticmethod
    def backward(ctx, drawchan, dcx):
        q, kvT, rawchan = ctx.saved_tensors
        B, T, C, ce, nwin = ctx.geo
        Cp = kvT.shape[-1]
        dq = torch.empty(B * T, ce, dtype=torch.float32, device=q.device)
        dkvT = torch.empty(B, 2 * ce, Cp, dtype=torch.float32, device=q.device)
        kw = dict(B=B, T=T, C=C, ce=ce, nh=nwin, nw=nwin)
        ops.call("chanattn_bwd", q=q, kvT=kvT, rawchan=rawchan, cx=None, kv_dtype=0, ldk=Cp, scale=ce ** -0.5, kvbias=None,
                 xargs=[drawchan.contiguous() if drawchan is not None else None, dcx.contiguous(), dq, dkvT, Cp,
                        ops.ws_for("chanattn_bwd", q.device, **kw)], **kw)
        return dq, dkvT[:, :, :C].transpose(1, 2), None


class ChanKvFn(Function):
    """kv[b] = chan_kv(x_attn[b]^T) (taskprompter_swin.py:393-397): W [2ce, HW] applied to the TRANSPOSED pixel rows of the attention branch, i.e.
    kvT[b] = W x_b + bias with the pixels as the reduction axis (73 728 at Swin-B's first stage).  As three GEMMs on the token-major rows
    themselves — no transposed copy of the map: forward = split-K over the pixels (slabs summed; the BLinearFn form ran K = HW on 16-32
    workgroups: 3.9 ms per block of stage 0 at the benchmark shape), dx_b = W^T dkvT_b written into the pixel rows of the token buffer,
    dW = sum_b dkvT_b x_b^T as one batch of B GEMMs with fp32 slabs.  po [B*N, C] (activation dtype) -> kv fp32 [B, C, 2ce]."""

    @staticmethod
    def forward(ctx, po, weight, bias, geo, prec, tag):
        C = geo[3]
        Wkv = ops.pack_linear([weight], prec, tag)                               # [1, 2ce, pitch(HW)]
        kvT = sw.chan_kv_gemm(po, Wkv, geo, prec)
        if bias is not None:
            kvT = kvT + bias.detach()[None, :, None]
        ctx.save_for_backward(po, Wkv)
        ctx.meta = (geo, prec, weight.shape, bias is not None)
        return kvT[:, :, :C].transpose(1, 2)

    @staticmethod
    def backward(ctx, dkv):
        po, Wkv = ctx.saved_tensors
        (B, N, T, C, HW), prec, wshape, has_bias = ctx.meta
        prec = prec.bwd
        ce2 = wshape[0]
        ldw = Wkv.shape[-1]
        dkvT = dkv.transpose(1, 2).contiguous().float()                          # [B, 2ce, C] (small)
        # dx_b [HW, C] = W^T dkvT_b -> the pixel rows of the token-buffer gradient (prompt rows: no gradient through chan_kv)
        dpo = torch.empty(B * N, C, dtype=po.dtype, device=po.device)
        dpo.view(B, N, C)[:, :T].zero_()
        ops.call("gemm", A=Wkv, B=dkvT, D=dpo.view(B, N, C)[:, T:], M=HW, N=C, K=ce2, a_op=OP_R, b_op=OP_R, a_dtype=dtype_code(Wkv), b_dtype=F32,
                 d_dtype=dtype_code(dpo), prec=prec.code, lda=ldw, ldb=C, ldd=C, batch=B, batch_inner=1, a_zo=0, b_zo=ce2 * C, d_zo=N * C,
                 alpha=1.0, n_store=C)
        # dW = sum_b dkvT_b [2ce, C] x_b^T [C, HW]: B GEMMs (reduction over the C channels of one image each), fp32 slabs summed
        slabs = torch.empty(B, ce2, ldw, dtype=torch.float32, device=po.device)
        ops.call("gemm", A=dkvT, B=po.view(B, N, C)[:, T:], D=slabs, M=ce2, N=HW, K=C, a_op=OP_K, b_op=OP_K, a_dtype=F32, b_dtype=dtype_code(po),
                 d_dtype=F32, prec=prec.code, lda=C, ldb=C, ldd=ldw, batch=B, batch_inner=1, a_zo=ce2 * C, b_zo=N * C, d_zo=ce2 * ldw, alpha=1.0,
                 n_store=ldw)
        dW = slabs.sum(0)[:, :HW].reshape(wshape)
        dbias = dkvT.sum((0, 2)) if has_bias else None
        return dpo, dW, dbias, None, None, None


class Conv3s2Fn(Function):
    """PatchMerging.spa_attn_ds on the raw prompt-logit maps [B, nH, T, T + H*W] -> [B, nH, T, T + H*W/4]."""

    @staticmethod
    def forward(ctx, rawlog, weight, bias, geo):
        B, nH, T, H, W = geo
        N, N2 = T + H * W, T + (H // 2) * (W // 2)
        raw2 = torch.zeros(B, nH, T, N2, dtype=torch.float32, device=rawlog.device)
        ops.call("conv3s2_nchw", x=rawlog, w=weight.detach().contiguous(), bias=bias.detach(), y=raw2, B=B, Ci=nH * T, Co=nH * T, H=H, W=W,
                 x_bs=nH * T * N, x_cs=N, x_off=T, y_bs=nH * T * N2, y_cs=N2, y_off=T)
        ctx.save_for_backward(rawlog, weight, bias)
        ctx.geo = geo
        return raw2

    @staticmethod
    def backward(ctx, draw2):
        rawlog, weight, bias = ctx.saved_tensors
        B, nH, T, H, W = ctx.geo
        N, N2 = T + H * W, T + (H // 2) * (W // 2)
        draw2 = draw2.contiguous()
        dl = torch.zeros_like(rawlog)                       # the first T columns (prompt <-> prompt logits) take no gradient here
        gw, gb = torch.empty_like(weight), torch.empty_like(bias)
        ops.call("conv3s2_nchw_bwd", x=rawlog, w=weight.detach().contiguous(), bias=None, y=None, B=B, Ci=nH * T, Co=nH * T, H=H, W=W,
                 x_bs=nH * T * N, x_cs=N, x_off=T, y_bs=nH * T * N2, y_cs=N2, y_off=T, xargs=[draw2, dl, gw, gb])
        return dl, gw, gb, None


_zero_bias = {}


def _lin(model, x, layer, tag, out_dtype=None):
    """x [M, K] (activation dtype) @ layer.weight^T + bias through BLinearFn (bias-free layers get a constant zero vector)."""
    bias = layer.bias
    if bias is None:
        key = (layer.weight.shape[0], str(x.device))
        if key not in _zero_bias:
            _zero_bias[key] = torch.zeros(layer.weight.shape[0], dtype=torch.float32, device=x.device)
        bias = _zero_bias[key]
    if x.shape[-1] != ops.pitch(x.shape[-1]):              # reduction length off the channel pitch (chan_kv on a 6 x 9 map): zero columns
        x = torch.nn.functional.pad(x, (0, ops.pitch(x.shape[-1]) - x.shape[-1]))
    y = BLinearFn.apply(x, layer.weight.shape[0], 'plain', None, out_dtype, model.prec, tag, None, layer.weight, bias).squeeze(0)
    return y if y.shape[1] == layer.weight.shape[0] else y[:, :layer.weight.shape[0]]     # (views: a select / full-range slice would cost a zero-fill + copy in the backward)


def _inverse_merge_tables(res, T, device):
    """For k = (dy, dx) in PatchMerging's order: table over ALL H*W pixels, the merged row that holds the pixel in column block k, -1 else."""
    H, W = res
    yy = torch.arange(H)[:, None]
    xx = torch.arange(W)[None, :]
    row = (yy // 2) * (W // 2) + xx // 2
    out = []
    for dy, dx in ((0, 0), (1, 0), (0, 1), (1, 1)):
        ok = ((yy % 2) == dy) & ((xx % 2) == dx)
        out.append(torch.where(ok, row, torch.full_like(row, -1)).reshape(-1).to(torch.int32).to(device))
    return out


def backbone_forward(model, img, keep):
    """TaskPrompterSwin's forward -> [T, B*h0*w0, pitch(F)] task features.  keep: somebody will differentiate it — blocks and patch mergings
    then run as the autograd graph of this file, otherwise as the model's in-place `_block` / `_merge`."""
    p, prec = model.p, model.prec
    adt = prec.adt
    dev = img.device
    B = img.shape[0]
    assert tuple(img.shape[-2:]) == model.full_img_size, "input size must equal img_size"
    img = img.float().contiguous()
    if model.img_ds_ratio != 1:                                              # :666-667
        Hs, Ws = model.patch_embed.img_size
        small = torch.empty(B, 3, Hs, Ws, dtype=torch.float32, device=dev)
        ops.call("resize_nchw", args=[img, small, B * 3, img.shape[-2], img.shape[-1], Hs, Ws])
        img = small
    T = model.prompts_len
    ps = model.patch_embed.patch_size[0]
    gh, gw = model.patch_grid
    C = model.embed_dim
    N = T + gh * gw
    # ---- patch embed (+ patch_norm) into the token buffer, prompts first ------------------------------------------------------------
    Kp = ops.pitch(3 * ps * ps)
    cols = torch.empty(B * gh * gw, Kp, dtype=adt, device=dev)
    ops.call("patchify", args=[img, cols, B, img.shape[-2], img.shape[-1], ps, Kp, dtype_code(cols)])
    nm = model.patch_embed.norm if isinstance(model.patch_embed.norm, torch.nn.LayerNorm) else None
    if keep:
        pe = _lin(model, cols, model.patch_embed.proj, 'pe', torch.float32)
        if nm is not None:
            pe = LayerNormFn.apply(pe.contiguous(), nm.weight, nm.bias, nm.eps, prec, torch.float32)
        XT = torch.cat([model.task_prompts[None].expand(B, T, C), pe.reshape(B, gh * gw, C)], 1).reshape(B * N, C)
    else:                                                                    # the GEMM writes the pixel rows of the token buffer itself
        XT = torch.empty(B * N, C, dtype=torch.float32, device=dev)
        pe = XT if nm is None else torch.zeros(B * N, C, dtype=torch.float32, device=dev)    # prompt rows: zeros (normalised, then overwritten)
        model._lin(cols, model.patch_embed.proj, 'pe', out=pe.view(B, N, C)[:, T:], d_rows=(gh * gw, N * C, C), M=B * gh * gw)
        if nm is not None:
            ops.call("layernorm_fwd", x=pe, y=XT, gamma=nm.weight.detach(), beta=nm.bias.detach(), mean=None, rstd=None, rows=B * N, C=C,
                     ldx=C, ldy=C, y_dtype=F32, eps=nm.eps)
        XT.view(B, N, C)[:, :T] = model.task_prompts.detach()
    block, merge = (partial(_block, model), partial(_merge, model)) if keep else (model._block, model._merge)
    fea_levels = []
    rawlog = rawchan = None
    for il, layer in enumerate(model.layers):
        res = layer.input_resolution
        nH = layer.blocks[0].num_heads
        for ib, blk in enumerate(layer.blocks):
            XT, rawlog, rawchan = block(blk, (il, ib), XT, B, T, res)
        if layer.downsample is not None:
            XT, rawlog, rawchan = merge(layer.downsample, il, XT, rawlog, rawchan, B, T, res, nH)
            fea_levels.append(_task_features(model, XT, rawlog, rawchan, il, B, (res[0] // 2, res[1] // 2), 2 * layer.dim, 2 * layer.dim // nH, keep))
    last = model.layers[-1]
    xf = layernorm(XT, model.norm.weight, model.norm.bias, model.norm.eps, prec, torch.float32, keep)
    fea_levels.append(_task_features(model, xf, rawlog, rawchan, model.num_layers - 1, B, last.input_resolution, last.dim,
                                     last.dim // last.blocks[0].num_heads, keep))
    # multi-scale fusion (:699-709): every level resized to the first one's grid and summed as ONE node (inside the kernel), then a 3x3 conv
    h0, w0 = model.feature_hw
    Fp = fea_levels[0].shape[-1]
    sizes = [(2 * model.resolution[i][0], 2 * model.resolution[i][1]) for i in range(len(fea_levels))]
    acc = MultiScaleSumFn.apply((B, Fp, h0, w0, sizes), *[f.contiguous() for f in fea_levels])
    if adt != torch.float32:
        acc = acc.to(adt) if keep else ops.cast2d(acc.view(-1, Fp), acc.shape[0] * acc.shape[1], Fp, Fp, adt, ldd=Fp).view(acc.shape[0], -1, Fp)
    names = list(model.all_tasks)
    F = p.final_embed_dim
    return Conv3x3Fn.apply(acc, (B, h0, w0, F, F), prec, 'msf', *[model.multi_scale_fuse[t].weight for t in names],
                           *[model.multi_scale_fuse[t].bias for t in names])


def _drop_scales(model, blk, tag, B, device):
    """The block's 4 independent per-sample DropPath draws (taskprompter_swin.py:412-413, 408-409), already mask / keep: [4, B] in the
    reference's call order x-attention, x-mlp, prompt-attention, prompt-mlp; None when inactive.  Tests inject the oracle's masks
    through model._drop_override[(layer, block)]."""
    override = getattr(model, "_drop_override", None)
    if override is not None:
        return override[tag].to(device)
    rate = blk.drop_path_rate
    if not model.training or rate <= 0.0:
        return None
    keep = 1.0 - rate
    return torch.bernoulli(torch.full((4, B), keep, device=device)) / keep


def _block(model, blk, tag, XT, B, T, res):
    drops = _drop_scales(model, blk, tag, B, XT.device)
    prec = model.prec
    adt = prec.adt
    dev = XT.device
    H, W = res
    C, nH, ws, shift = blk.dim, blk.num_heads, blk.window_size, blk.shift_size
    Hp, Wp = blk.padded
    N, ws2 = T + H * W, ws * ws
    Nw, nW = T + ws2, (Hp // ws) * (Wp // ws)
    part, pix, rev = sw.window_tables(res, ws, shift, Hp, Wp, T, dev)
    tag = ('sw',) + tag
    a = blk.attn
    xn = LayerNormFn.apply(XT, blk.norm1.weight, blk.norm1.bias, blk.norm1.eps, prec, None)
    prompts = XT.view(B, N, C)[:, :T].reshape(B * T, C)
    chan_p = _lin(model, prompts.to(adt), blk.token_trans, tag + ('tt',), torch.float32)              # [B*T, ce]
    wtok = WindowGatherFn.apply(xn, True, part, rev, (B, N, T, nW, Nw, C))
    qkv = _lin(model, wtok, a.qkv, tag + ('qkv',)).contiguous()
    ao, rawlog = WinAttnFn.apply(qkv, a.relative_position_bias_table, a.relative_position_index, blk.attn_mask, pix, (B, nW, nH, T, ws2, N), prec)
    ao_img = WindowGatherFn.apply(ao, False, part, rev, (B, N, T, nW, Nw, C))
    po = _lin(model, ao_img, a.proj, tag + ('proj',))                                                 # [B*N, C] activation dtype
    branch = po.float()
    # channel attention: kv = chan_kv(x_attn^T) per image (taskprompter_swin.py:393-397)
    ce = model.p.chan_embed_dim
    nwin = int(math.isqrt(model.p.chan_nheads))
    q = _lin(model, chan_p.to(adt), blk.chan_q, tag + ('cq',), torch.float32)
    if CHAN_KV_FN and (H * W) % 8 == 0 and C % 8 == 0:
        kv = ChanKvFn.apply(po, blk.chan_kv.weight, blk.chan_kv.bias, (B, N, T, C, H * W), prec, tag + ('ckv',))
    else:                                        # a pixel count off the 8-element granule (6 x 9 maps of the miniatures): the transposed-copy form
        xT = po.view(B, N, C)[:, T:].transpose(1, 2).reshape(B * C, H * W)
        kv = _lin(model, xT.contiguous(), blk.chan_kv, tag + ('ckv',), torch.float32).reshape(B, C, 2 * ce)
    rawchan, cx = ChanAttnFn.apply(q.contiguous(), kv.contiguous(), (B, T, C, ce, nwin))
    tt1 = None
    if not blk.last_block:
        cp = _lin(model, cx.to(adt), blk.chan_proj, tag + ('cpj',), torch.float32)
        tt1 = _lin(model, cp.to(adt), blk.token_trans1, tag + ('tt1',), torch.float32)                # [B*T, C]
    # residual: pixels + draw0 * branch; prompts + draw2 * (branch + channel term) — the last block's prompt output is not used downstream
    # (its prompt rows take the unscaled branch, no channel term)
    XT2 = BlockResidualFn.apply(XT, branch, tt1, None if drops is None else drops[0],
                                None if (drops is None or blk.last_block) else drops[2], (B, N, T, C))
    rs_mlp = None if drops is None else torch.stack([drops[3], drops[1]], 1).contiguous()            # [B, 2]: prompt rows, pixel rows
    XT3 = MlpHalfFn.apply(XT2.contiguous(), blk.norm2.weight, blk.norm2.bias, blk.norm2.eps, blk.mlp.fc1.weight, blk.mlp.fc1.bias,
                          blk.mlp.fc2.weight, blk.mlp.fc2.bias, rs_mlp, (B, N, T), prec, tag)
    return XT3, rawlog, rawchan


def _merge(model, ds, il, XT, rawlog, rawchan, B, T, res, nH):
    prec = model.prec
    adt = prec.adt
    dev = XT.device
    H, W = res
    C = ds.dim
    N, N2 = T + H * W, T + (H // 2) * (W // 2)
    tag = ('swm', il)
    cat = MergeGatherFn.apply(XT, sw.merge_tables(res, T, dev), _inverse_merge_tables(res, T, dev), (B, N, N2, T, C))
    catn = LayerNormFn.apply(cat, ds.norm.weight, ds.norm.bias, ds.norm.eps, prec, None)
    red = _lin(model, catn, ds.reduction, tag + ('red',), torch.float32)                              # [B*(N2-T), 2C]
    prompts = XT.view(B, N, C)[:, :T].reshape(B * T, C)
    pr = _lin(model, prompts.to(adt), ds.task_prompts_up, tag + ('tpu',), torch.float32)
    XT2 = torch.cat([pr.reshape(B, T, 2 * C), red.reshape(B, N2 - T, 2 * C)], 1).reshape(B * N2, 2 * C)
    raw2 = Conv3s2Fn.apply(rawlog, ds.spa_attn_ds.weight, ds.spa_attn_ds.bias, (B, nH, T, H, W))
    nwin2 = rawchan.shape[2]
    rc2 = _lin(model, rawchan.reshape(B * T * nwin2, C).to(adt), ds.process_chan_attn, tag + ('pca',), torch.float32)
    return XT2.contiguous(), raw2, rc2.reshape(B, T, nwin2, 2 * C).contiguous()


def _task_features(model, xsrc, rawlog, rawchan, il, B, res, C, hg, keep):
    """cal_task_feature (taskprompter_swin.py:715-777) of one level, all tasks -> [T, B*2h*2w, pitch(F)] activation dtype.  One statement for
    both paths, except that a forward in eval mode that nobody differentiates folds the BatchNorm into the first 3x3 conv's epilogue."""
    p, prec = model.p, model.prec
    names = list(model.all_tasks)
    T = len(names)
    h, w = res
    N = T + h * w
    tar, F = p.level_embed_dim, p.final_embed_dim
    tarp = ops.pitch(tar)
    nwin = int(math.isqrt(p.chan_nheads))
    sp = model._decoder_split(C)         # x3f: modulate and the fea_decode epilogue write hi / lo planes, both GEMMs on the split-plane kernel
    mod = ModulateFn.apply(xsrc.contiguous(), rawlog, rawchan, (B, N, T, C, h, w, nwin, hg), prec, sp)
    mod, mod_lo = mod if sp else (mod, None)
    dec_w, dec_b = [], []
    for t in names:
        dec_w += [model.fea_decode_spa[il][t][0].weight, model.fea_decode_chan[il][t][0].weight]
        dec_b += [model.fea_decode_spa[il][t][0].bias, model.fea_decode_chan[il][t][0].bias]
    cat = BLinearFn.apply(mod, tar, 'catpair', None, "split" if sp else None, prec, ('swdec', il), mod_lo, *dec_w, *dec_b)
    cat, cat_lo = cat if sp else (cat, None)
    del mod, mod_lo
    ff = [model.fea_fuse[il][t] for t in names]
    kmap = (2 * tarp, [(0, 0, tar), (tarp, tar, tar)])
    y0 = BLinearFn.apply(cat, F, 'plain', kmap, None, prec, ('swf0', il), cat_lo, *[m[0].weight for m in ff], *[m[0].bias for m in ff])
    del cat, cat_lo
    y0 = BilinearFn.apply(y0, (B, y0.shape[-1], h, w, 2 * h, 2 * w), prec.adt, False)        # :737 / :765
    geo = (B, 2 * h, 2 * w, F, F)
    bns = [m[2] for m in ff]
    if keep or model.training:
        y1 = Conv3x3Fn.apply(y0, geo, prec, ('swf1', il), *[m[1].weight for m in ff], *[m[1].bias for m in ff])
        y1 = _bn_act(y1, bns, F, ACT_GELU, model.training)
    else:
        sc, sh = bn_mod.fold(bns, [m[1].bias for m in ff], ('swf2', il))
        y1 = ops.conv3x3(y0, ops.pack_conv3([m[1].weight for m in ff], prec, ('swf1', il)), F, F, *geo[:3], prec, bias=sh, colscale=sc, act=ACT_GELU)
    return Conv3x3Fn.apply(y1, geo, prec, ('swf4', il), *[m[4].weight for m in ff], *[m[4].bias for m in ff])
