"""FCOS3D detection head + FPN neck of the 3ddet task (TaskPrompter/detection_toolbox/det_head.py:128-457, fpn.py), on the HIP kernels.

Drop-in for the reference's `FCOS3DHead(**p.det_head_params)`: same constructor, same `init_weights()`, same state-dict names and shapes as
the reference built on mmcv 1.6.2 (ConvModule -> `.conv` / `.gn`; the DCNv2 layer -> `.conv.weight`, `.conv.bias`, `.conv.conv_offset.*`),
and the same forward contract: `forward([4 NCHW maps])` -> (cls_scores, bbox_preds, dir_cls_preds, centernesses), four lists of 5 fp32
NCHW tensors.

Compute: 3x3 convs on the implicit-GEMM conv (autograd_path.Conv3x3Fn), 1x1 convs on mtt_gemm (BLinearFn), GroupNorm + ReLU
(mtt_groupnorm_*), the modulated deformable conv and the FPN's stride-2 extra conv as sampled im2col (mtt_dcn_*) + mtt_gemm, the FPN's
nearest top-down add (mtt_nearest_add*) and the per-level bbox tail + NCHW store (mtt_fcos_bbox_post*).  Activations are NHWC rows
[B*H*W, pitch(C)] between layers.  No torch conv / group_norm / interpolate on this path.

The mmcv layer semantics used here are restated, not imported (mmcv is not a dependency): ConvModule = conv -> norm -> ReLU with the conv
bias kept under a norm when bias=True; ModulatedDeformConv2dPack = `o1, o2, m = chunk(conv_offset(x), 3)`, offset = cat(o1, o2),
mask = sigmoid(m), deform_groups = groups = 1 (the sampling rule is in include/mtt_hip.h, mtt_dcn_im2col).
"""
import numpy as np
import torch
import torch.nn as nn
from torch.autograd import Function

from . import ops
from .autograd_path import BLinearFn, Conv3x3Fn, _dgrad, _to_bwd, _wgrad
from .ops import DEFAULT_PREC, Prec, pitch

GN_EPS = 1e-5


def _dt(t):
    return ops.dtype_code(t)


# =====================================================================================================================
# autograd Functions
# =====================================================================================================================
class GroupNormActFn(Function):
    """x [Z*B*HW, ld] (Z stacked layers) -> act(GroupNorm(x)) in `out_dtype`; gamma / beta [Z*C]."""

    @staticmethod
    def forward(ctx, x, gamma, beta, geo, out_dtype):
        Z, B, HW, C, G, relu = geo
        ld = x.shape[-1]
        x2 = x.reshape(-1, ld)
        y = torch.empty(x2.shape, dtype=out_dtype, device=x.device)
        stats = torch.empty(2, Z * B * G, dtype=torch.float32, device=x.device)
        ws = ops.ws_for("groupnorm", x.device, Z=Z, B=B, HW=HW, C=C, G=G, ld=ld)
        ops.call("groupnorm_fwd", x=x2, y=y, gamma=gamma, beta=beta, mean=stats[0], rstd=stats[1], Z=Z, B=B, HW=HW, C=C, G=G, ld=ld,
                 x_dtype=_dt(x2), y_dtype=_dt(y), relu=int(relu), eps=GN_EPS, ws=ws)
        ctx.save_for_backward(x2, gamma, beta, stats)
        ctx.meta = (geo, x.shape, x.dtype)
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        x2, gamma, beta, stats = ctx.saved_tensors
        (Z, B, HW, C, G, relu), shape, xdt = ctx.meta
        ld = x2.shape[-1]
        dy2 = dy.contiguous().view(-1, ld)
        dx = torch.empty(x2.shape, dtype=xdt, device=x2.device)
        dg = torch.empty(Z * C, dtype=torch.float32, device=x2.device)
        db = torch.empty(Z * C, dtype=torch.float32, device=x2.device)
        ws = ops.ws_for("groupnorm", x2.device, Z=Z, B=B, HW=HW, C=C, G=G, ld=ld)
        ops.call("groupnorm_bwd", x=x2, gamma=gamma, beta=beta, mean=stats[0], rstd=stats[1], dy=dy2, dx=dx, dgamma=dg, dbeta=db,
                 Z=Z, B=B, HW=HW, C=C, G=G, ld=ld, x_dtype=_dt(x2), dy_dtype=_dt(dy2), dx_dtype=_dt(dx), relu=int(relu), eps=GN_EPS, ws=ws)
        return dx.view(shape), dg, db, None, None


def _dcn_geom(geo):
    B, H, W, C, Ho, Wo, stride = geo
    Cp = pitch(C)
    return dict(B=B, H=H, W=W, C=C, Cp=Cp, Ho=Ho, Wo=Wo, stride=stride, pad=1, dil=1, ldx=Cp, ldc=9 * Cp)


class SampledConvFn(Function):
    """3x3 convolution (pad 1) through sampled im2col + mtt_gemm: the modulated deformable conv when `om` (the offset conv's output
    [rows, pitch(27)]: channels 0..17 offsets, 18..26 mask logits) is given, else a plain (strided) conv.
    x [B*H*W, pitch(C)] -> [B*Ho*Wo, pitch(Co)].  geo = (B, H, W, C, Ho, Wo, stride)."""

    @staticmethod
    def forward(ctx, x, om, weight, bias, geo, prec, tag):
        g = _dcn_geom(geo)
        Co, Cp = weight.shape[0], g['Cp']
        rows = g['B'] * g['Ho'] * g['Wo']
        K = 9 * Cp
        split = prec.split and ops.split_gemm_ok(K)
        if split:
            col = ops.Split.empty((rows, K), x.device)
        else:
            col = torch.empty(rows, K, dtype=prec.adt, device=x.device)
        offs = {}
        if om is not None:
            offs = dict(offset=om, ld_off=om.shape[-1], mask=om[:, 18:], ld_mask=om.shape[-1], mask_sigmoid=1, off_dtype=_dt(om))
        ops.call("dcn_im2col", x=x, x_dtype=_dt(x), col=ops._hi(col), col_lo=col.lo if split else None, col_dtype=_dt(col), **g, **offs)
        wpack = ops.pack_conv3([weight], prec, tag, split=split)
        y = ops.linear(col, wpack, Co, prec, bias=ops.stack_vec([bias], (tag, 'b')) if bias is not None else None)[0]
        ctx.save_for_backward(x, om, ops._hi(col), weight)
        ctx.meta = (geo, prec, tag, bias is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, om, col, weight = ctx.saved_tensors
        geo, prec, tag, has_bias = ctx.meta
        prec = prec.bwd
        g = _dcn_geom(geo)
        Co, Ci, Cp = weight.shape[0], weight.shape[1], g['Cp']
        rows, K = col.shape
        dy = _to_bwd(dy.contiguous(), prec)
        col = _to_bwd(col, prec)
        wpack = ops.pack_conv3([weight], prec, tag)[0]                       # [Co, 9*Cp], k = tap*Cp + ci
        dcol = _dgrad(dy, wpack, rows, K, Co, prec, dy.dtype)
        dW = _wgrad(dy, col, Co, K, prec)
        dW = dW.view(Co, 9, Cp)[:, :, :Ci].permute(0, 2, 1).reshape(Co, Ci, 3, 3)
        db = ops.colsum(dy, Co) if has_bias else None
        dx = torch.empty(x.shape, dtype=x.dtype, device=x.device)
        offs, dom = {}, None
        if om is not None:
            dom = torch.zeros_like(om)
            offs = dict(offset=om, ld_off=om.shape[-1], mask=om[:, 18:], ld_mask=om.shape[-1], mask_sigmoid=1, off_dtype=_dt(om),
                        doffset=dom, dmask=dom[:, 18:])
        ws = ops.ws_for("dcn_col2im", x.device, **g)
        ops.call("dcn_col2im_bwd", x=x, x_dtype=_dt(x), dcol=dcol, dcol_dtype=_dt(dcol), dx=dx, dx_dtype=_dt(dx), ws=ws, **g, **offs)
        return dx, dom, dW, db, None, None, None


class NearestAddFn(Function):
    """a [B*Ho*Wo, ld] + nearest-upsampled src [B*Hi*Wi, ld] (fpn.py top-down step)."""

    @staticmethod
    def forward(ctx, a, src, geo):
        B, C, Ho, Wo, Hi, Wi = geo
        out = torch.empty_like(a)
        ops.call("nearest_add", a=a, src=src, out=out, B=B, C=a.shape[-1], Ho=Ho, Wo=Wo, Hi=Hi, Wi=Wi, ld_a=a.shape[-1],
                 ld_src=src.shape[-1], ld_out=out.shape[-1], dtype=_dt(a))
        ctx.meta = (geo, src.shape, src.dtype)
        return out

    @staticmethod
    def backward(ctx, dout):
        (B, C, Ho, Wo, Hi, Wi), sshape, sdt = ctx.meta
        dout = dout.contiguous()
        dsrc = torch.empty(sshape, dtype=dout.dtype, device=dout.device)
        ops.call("nearest_add_bwd", a=dout, out=dsrc, B=B, C=dout.shape[-1], Ho=Ho, Wo=Wo, Hi=Hi, Wi=Wi, ld_a=dout.shape[-1],
                 ld_src=dsrc.shape[-1], ld_out=dsrc.shape[-1], dtype=_dt(dout))
        return dout, dsrc.to(sdt), None


class BboxPostFn(Function):
    """NHWC prediction groups -> one fp32 NCHW map, with the FCOS3D bbox tail when `scales` (fp32 [4]) is given."""

    @staticmethod
    def forward(ctx, scales, geo, *xs):
        B, H, W, dims, bbox2d = geo
        nch = sum(dims)
        out = torch.empty(B, nch, H, W, dtype=torch.float32, device=xs[0].device)
        xs = [x.reshape(-1, x.shape[-1]) for x in xs]
        ops.call("fcos_bbox_post", x=list(xs), ldx=[x.shape[-1] for x in xs], dims=list(dims), ngroups=len(dims), out=out, scales=scales,
                 bbox2d=int(bbox2d), B=B, H=H, W=W)
        ctx.save_for_backward(scales, *xs)
        ctx.meta = (geo, [x.shape for x in xs])
        return out

    @staticmethod
    def backward(ctx, dout):
        scales, *xs = ctx.saved_tensors
        (B, H, W, dims, bbox2d), shapes = ctx.meta
        dxs = [torch.empty_like(x) for x in xs]
        kw = {}
        if scales is not None:
            ds = torch.empty(4, dtype=torch.float32, device=dout.device)
            kw = dict(scales=scales, dscales=ds, ws=ops.ws_for("fcos_bbox_post", dout.device, B=B, H=H, W=W))
        ops.call("fcos_bbox_post_bwd", x=list(xs), ldx=[x.shape[-1] for x in xs], dims=list(dims), ngroups=len(dims), bbox2d=int(bbox2d),
                 B=B, H=H, W=W, dout=dout.contiguous(), dx=list(dxs), **kw)
        return (kw.get('dscales'), None) + tuple(d.view(1, *d.shape) for d in dxs)


# =====================================================================================================================
# modules (state-dict layout of the reference on mmcv 1.6.2)
# =====================================================================================================================
class Scale(nn.Module):
    """det_head.py:80-95 (a learnable scalar)."""

    def __init__(self, scale=1.0):
        super().__init__()
        self.scale = nn.Parameter(torch.tensor(scale, dtype=torch.float))

    def forward(self, x):
        return x * self.scale


class ModulatedDeformConv2dPack(nn.Module):
    """Parameters of mmcv's ModulatedDeformConv2dPack (3x3, stride 1, pad 1, deform_groups 1): weight, bias, conv_offset.  Its compute
    runs inside the head (SampledConvFn); the conv_offset init is zero as in mmcv."""

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, padding=1, dilation=1, groups=1, deform_groups=1, bias=True):
        super().__init__()
        if kernel_size not in (3, (3, 3)) or stride != 1 or padding != 1 or dilation != 1:
            raise NotImplementedError(f"DCNv2 with kernel_size={kernel_size}, stride={stride}, padding={padding}, dilation={dilation}")
        if groups != 1 or deform_groups != 1:
            raise NotImplementedError(f"DCNv2 with groups={groups}, deform_groups={deform_groups}")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, 3, 3))
        self.bias = nn.Parameter(torch.zeros(out_channels)) if bias else None
        self.conv_offset = nn.Conv2d(in_channels, 27, 3, padding=1, bias=True)
        stdv = 1.0 / float(np.sqrt(in_channels * 9))
        nn.init.uniform_(self.weight, -stdv, stdv)
        nn.init.zeros_(self.conv_offset.weight)
        nn.init.zeros_(self.conv_offset.bias)


class ConvModule(nn.Module):
    """mmcv.cnn.ConvModule as the head and the FPN use it: conv (-> GroupNorm) (-> ReLU); names `conv`, `gn`."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, conv_cfg=None, norm_cfg=None, act_cfg='relu',
                 bias='auto', inplace=True):
        super().__init__()
        dcn = conv_cfg is not None and conv_cfg.get('type') == 'DCNv2'
        if conv_cfg is not None and not dcn:
            raise NotImplementedError(f"conv_cfg={conv_cfg}")
        if norm_cfg is not None and norm_cfg.get('type') != 'GN':
            raise NotImplementedError(f"norm_cfg={norm_cfg}")
        if act_cfg not in (None, 'relu') and dict(act_cfg).get('type') != 'ReLU':
            raise NotImplementedError(f"act_cfg={act_cfg}")
        if padding != (kernel_size - 1) // 2 or (stride != 1 and kernel_size != 3):
            raise NotImplementedError(f"ConvModule kernel_size={kernel_size}, stride={stride}, padding={padding}")
        with_bias = (norm_cfg is None) if bias == 'auto' else bool(bias)
        if dcn:
            self.conv = ModulatedDeformConv2dPack(in_channels, out_channels, kernel_size, stride=stride, padding=padding, bias=with_bias)
        else:
            self.conv = nn.Conv2d(in_channels, out_channels, kernel_size, stride=stride, padding=padding, bias=with_bias)
            nn.init.kaiming_normal_(self.conv.weight, mode='fan_out', nonlinearity='relu')
            if with_bias:
                nn.init.zeros_(self.conv.bias)
        self.dcn, self.stride, self.k = dcn, stride, kernel_size
        self.with_act = act_cfg is not None
        self.groups = 0
        if norm_cfg is not None:
            self.groups = int(norm_cfg.get('num_groups', 32))
            self.gn = nn.GroupNorm(self.groups, out_channels)
            if norm_cfg.get('requires_grad', True) is False:
                raise NotImplementedError("norm_cfg requires_grad=False")


class FPN(nn.Module):
    """fpn.py FPN for what the 3ddet config uses: start_level 0, add_extra_convs 'on_output', no norm on the FPN convs."""

    def __init__(self, in_channels, out_channels, num_outs, start_level=0, end_level=-1, add_extra_convs=False,
                 relu_before_extra_convs=False, no_norm_on_lateral=False, conv_cfg=None, norm_cfg=None, act_cfg=None,
                 upsample_cfg=dict(mode='nearest'), init_cfg=None, type=None):
        super().__init__()
        assert isinstance(in_channels, (list, tuple))
        if start_level != 0:
            raise NotImplementedError(f"FPN start_level={start_level}")
        if end_level != -1:
            raise NotImplementedError(f"FPN end_level={end_level}")
        if add_extra_convs not in ('on_output',) and not (add_extra_convs is False and num_outs == len(in_channels)):
            raise NotImplementedError(f"FPN add_extra_convs={add_extra_convs}")
        if norm_cfg is not None:
            raise NotImplementedError(f"FPN norm_cfg={norm_cfg}")
        if conv_cfg is not None:
            raise NotImplementedError(f"FPN conv_cfg={conv_cfg}")
        if act_cfg is not None:
            raise NotImplementedError(f"FPN act_cfg={act_cfg}")
        if dict(upsample_cfg) != dict(mode='nearest'):
            raise NotImplementedError(f"FPN upsample_cfg={upsample_cfg}")
        self.in_channels, self.out_channels, self.num_outs = list(in_channels), out_channels, num_outs
        self.num_ins = len(in_channels)
        assert num_outs >= self.num_ins
        self.relu_before_extra_convs = relu_before_extra_convs
        self.add_extra_convs = add_extra_convs
        self.lateral_convs = nn.ModuleList([ConvModule(c, out_channels, 1, act_cfg=None) for c in in_channels])
        self.fpn_convs = nn.ModuleList([ConvModule(out_channels, out_channels, 3, padding=1, act_cfg=None) for _ in in_channels])
        for _ in range(num_outs - self.num_ins):
            self.fpn_convs.append(ConvModule(out_channels, out_channels, 3, stride=2, padding=1, act_cfg=None))
        if relu_before_extra_convs and num_outs - self.num_ins > 1:
            # a ReLU between two extra convs (fpn.py: only from the second extra level on) has no kernel here
            raise NotImplementedError("FPN relu_before_extra_convs with more than one extra level")


class FCOS3DHead(nn.Module):
    """det_head.py:128-457 (constructor signature, init_weights and forward contract of the reference)."""

    def __init__(self, num_classes, in_channels, centerness_on_reg=True, norm_cfg=dict(type='GN', num_groups=32, requires_grad=True),
                 centerness_branch=(64, ), feat_channels=256, stacked_convs=4, dcn_on_last_conv=False, conv_bias='auto',
                 use_direction_classifier=True, group_reg_dims=(2, 1, 3, 1, 2), cls_branch=(128, 64),
                 reg_branch=((128, 64), (128, 64), (64, ), (64, ), ()), fpn_scale_no=None, bbox_code_size=None, pred_bbox2d=True,
                 pred_keypoints=False, dir_branch=(64, ), conv_cfg=None, init_cfg=None, neck_cfg=None):
        super().__init__()
        if pred_keypoints:
            raise NotImplementedError("FCOS3DHead pred_keypoints=True")
        if conv_cfg is not None:
            raise NotImplementedError(f"FCOS3DHead conv_cfg={conv_cfg}")
        if norm_cfg is None or norm_cfg.get('type') != 'GN':
            raise NotImplementedError(f"FCOS3DHead norm_cfg={norm_cfg}")
        if neck_cfg is None or dict(neck_cfg).get('type', 'FPN') != 'FPN':
            raise NotImplementedError(f"FCOS3DHead neck_cfg={neck_cfg}")
        if not use_direction_classifier:
            raise NotImplementedError("FCOS3DHead use_direction_classifier=False")
        assert len(reg_branch) == len(group_reg_dims)
        assert sum(group_reg_dims) >= (10 if pred_bbox2d else 6)
        self.neck = FPN(**dict(neck_cfg))
        self.centerness_on_reg = centerness_on_reg
        self.centerness_branch = centerness_branch
        self.pred_attrs = False
        self.bbox_code_size = bbox_code_size
        self.cls_out_channels = num_classes
        self.in_channels = in_channels
        self.feat_channels = feat_channels
        self.stacked_convs = stacked_convs
        self.dcn_on_last_conv = dcn_on_last_conv
        assert conv_bias == 'auto' or isinstance(conv_bias, bool)
        self.conv_bias = conv_bias
        self.use_direction_classifier = use_direction_classifier
        self.group_reg_dims = list(group_reg_dims)
        self.cls_branch = cls_branch
        self.reg_branch = reg_branch
        self.out_channels = [r[-1] if len(r) > 0 else -1 for r in reg_branch]
        self.dir_branch = dir_branch
        self.conv_cfg = conv_cfg
        self.norm_cfg = norm_cfg
        self.pred_bbox2d = pred_bbox2d
        self.pred_keypoints = pred_keypoints
        self.fpn_scale_no = fpn_scale_no
        self.prec = Prec(DEFAULT_PREC)
        self._init_layers()

    # ---- layers (det_head.py:196-323) ----
    def _tower(self):
        convs = nn.ModuleList()
        for i in range(self.stacked_convs):
            chn = self.in_channels if i == 0 else self.feat_channels
            cfg = dict(type='DCNv2') if self.dcn_on_last_conv and i == self.stacked_convs - 1 else None
            convs.append(ConvModule(chn, self.feat_channels, 3, stride=1, padding=1, conv_cfg=cfg, norm_cfg=self.norm_cfg,
                                    bias=self.conv_bias))
        return convs

    def _init_branch(self, conv_channels=(64, ), conv_strides=(1, )):
        if isinstance(conv_channels, int):
            conv_channels, conv_strides = [self.feat_channels, conv_channels], [conv_strides]
        else:
            conv_channels, conv_strides = [self.feat_channels] + list(conv_channels), list(conv_strides)
        return nn.ModuleList([ConvModule(conv_channels[i], conv_channels[i + 1], 3, stride=conv_strides[i], padding=1,
                                         norm_cfg=self.norm_cfg, bias=self.conv_bias) for i in range(len(conv_strides))])

    def _init_layers(self):
        self.cls_convs = self._tower()
        self.reg_convs = self._tower()
        self.conv_cls_prev = self._init_branch(self.cls_branch, (1, ) * len(self.cls_branch))
        self.conv_cls = nn.Conv2d(self.cls_branch[-1], self.cls_out_channels, 1)
        self.conv_reg_prevs = nn.ModuleList()
        self.conv_regs = nn.ModuleList()
        for reg_dim, rb, oc in zip(self.group_reg_dims, self.reg_branch, self.out_channels):
            if len(rb) > 0:
                self.conv_reg_prevs.append(self._init_branch(rb, (1, ) * len(rb)))
                self.conv_regs.append(nn.Conv2d(oc, reg_dim, 1))
            else:
                self.conv_reg_prevs.append(None)
                self.conv_regs.append(nn.Conv2d(self.feat_channels, reg_dim, 1))
        self.conv_dir_cls_prev = self._init_branch(self.dir_branch, (1, ) * len(self.dir_branch))
        self.conv_dir_cls = nn.Conv2d(self.dir_branch[-1], 2 * 3, 1)
        self.conv_centerness_prev = self._init_branch(self.centerness_branch, (1, ) * len(self.centerness_branch))
        self.conv_centerness = nn.Conv2d(self.centerness_branch[-1], 1, 1)
        self.scale_dim = 3 + (1 if self.pred_bbox2d else 0)
        self.scales = nn.ModuleList([nn.ModuleList([Scale(1.0) for _ in range(self.scale_dim)]) for _ in range(self.fpn_scale_no)])

    def init_weights(self):
        """det_head.py:325-360."""
        def normal_init(m, std=0.01, bias=0.0):
            nn.init.normal_(m.weight, 0, std)
            if m.bias is not None:
                nn.init.constant_(m.bias, bias)
        convs = list(self.cls_convs) + list(self.reg_convs) + list(self.conv_cls_prev) + list(self.conv_dir_cls_prev)
        convs += [m for rp in self.conv_reg_prevs if rp is not None for m in rp] + list(self.conv_centerness_prev)
        for m in convs:
            if isinstance(m.conv, nn.Conv2d):
                normal_init(m.conv)
        bias_cls = float(-np.log((1 - 0.01) / 0.01))
        normal_init(self.conv_cls, bias=bias_cls)
        for conv_reg in self.conv_regs:
            normal_init(conv_reg)
        normal_init(self.conv_dir_cls, bias=bias_cls)
        normal_init(self.conv_centerness)

    def set_prec(self, prec):
        self.prec = prec if isinstance(prec, Prec) else Prec(prec)

    # ---- compute ----
    def _conv(self, mods, x, hw, tag):
        """A ConvModule (or Z of them with the same shapes, stacked: x [Z, rows, Cp]) on the HIP kernels -> [Z, rows, pitch(Co)]."""
        B, H, W = hw
        prec = self.prec
        m0 = mods[0]
        Co, Ci = m0.conv.out_channels, m0.conv.in_channels
        if m0.dcn:
            ys = []
            for z, m in enumerate(mods):
                om = Conv3x3Fn.apply(x[z:z + 1], (B, H, W, 27, Ci), prec, (tag, z, 'off'), m.conv.conv_offset.weight,
                                     m.conv.conv_offset.bias)[0]
                ys.append(SampledConvFn.apply(x[z], om, m.conv.weight, m.conv.bias, (B, H, W, Ci, H, W, 1), prec, (tag, z)))
            y = torch.stack(ys) if len(ys) > 1 else ys[0][None]
        else:
            ws = [m.conv.weight for m in mods]
            bs = [m.conv.bias for m in mods]
            y = Conv3x3Fn.apply(x, (B, H, W, Co, Ci), prec, tag, *ws, *bs)
        if m0.groups:
            Z = len(mods)
            gamma = torch.cat([m.gn.weight for m in mods]) if Z > 1 else mods[0].gn.weight
            beta = torch.cat([m.gn.bias for m in mods]) if Z > 1 else mods[0].gn.bias
            y = GroupNormActFn.apply(y, gamma, beta, (Z, B, H * W, Co, m0.groups, True), prec.adt)
        return y

    def _pred(self, conv, x, tag):
        """1x1 prediction conv -> [1, rows, pitch(N)] fp32."""
        return BLinearFn.apply(x, conv.out_channels, 'plain', None, torch.float32, self.prec, tag, None, conv.weight, conv.bias)

    def _neck(self, levels):
        """FPN on NHWC levels [(x [B*H*W, pitch(C)], (B, H, W))] -> 5 NHWC maps."""
        neck, prec = self.neck, self.prec
        lat = []
        for i, (x, (B, H, W)) in enumerate(levels):
            m = neck.lateral_convs[i].conv
            lat.append(BLinearFn.apply(x[None], m.out_channels, 'plain', None, prec.adt, prec, ('fpn_lat', id(self), i), None,
                                       m.weight, m.bias)[0])
        for i in range(len(lat) - 1, 0, -1):
            (B, Ho, Wo), (_, Hi, Wi) = levels[i - 1][1], levels[i][1]
            lat[i - 1] = NearestAddFn.apply(lat[i - 1], lat[i], (B, neck.out_channels, Ho, Wo, Hi, Wi))
        outs = []
        C = neck.out_channels
        for i, (x, hw) in enumerate(levels):
            m = neck.fpn_convs[i].conv
            outs.append((Conv3x3Fn.apply(lat[i][None], (*hw, C, C), prec, ('fpn_out', id(self), i), m.weight, m.bias)[0], hw))
        for i in range(len(levels), neck.num_outs):
            x, (B, H, W) = outs[-1]
            if i > len(levels) and neck.relu_before_extra_convs:
                raise NotImplementedError("FPN relu_before_extra_convs with more than one extra level")
            Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
            m = neck.fpn_convs[i].conv
            y = SampledConvFn.apply(x, None, m.weight, m.bias, (B, H, W, C, Ho, Wo, 2), prec, ('fpn_extra', id(self), i))
            outs.append((y, (B, Ho, Wo)))
        return outs

    def _single(self, x, hw, scale):
        """forward_single (det_head.py:392-457) on one FPN level x [B*H*W, pitch(C)]."""
        B, H, W = hw
        t = id(self)
        feat = x[None].expand(2, *x.shape).contiguous()                       # cls and reg towers as one task-batched stack
        for i in range(self.stacked_convs):
            feat = self._conv([self.cls_convs[i], self.reg_convs[i]], feat, hw, ('tower', t, i))
        cls_feat, reg_feat = feat[0:1], feat[1:2]
        y = cls_feat
        for i, m in enumerate(self.conv_cls_prev):
            y = self._conv([m], y, hw, ('cls_prev', t, i))
        cls_score = BboxPostFn.apply(None, (B, H, W, (self.cls_out_channels, ), False), self._pred(self.conv_cls, y, ('cls', t)))
        regs = []
        for g, (prev, conv) in enumerate(zip(self.conv_reg_prevs, self.conv_regs)):
            y = reg_feat
            if prev is not None:
                for i, m in enumerate(prev):
                    y = self._conv([m], y, hw, ('reg_prev', t, g, i))
            regs.append(self._pred(conv, y, ('reg', t, g)))
        s = torch.stack([sc.scale for sc in scale[:3]] + [scale[-1].scale if self.pred_bbox2d else scale[0].scale * 0])
        bbox_pred = BboxPostFn.apply(s, (B, H, W, tuple(self.group_reg_dims), self.pred_bbox2d), *regs)
        y = reg_feat
        for i, m in enumerate(self.conv_dir_cls_prev):
            y = self._conv([m], y, hw, ('dir_prev', t, i))
        dir_cls = BboxPostFn.apply(None, (B, H, W, (6, ), False), self._pred(self.conv_dir_cls, y, ('dir', t)))
        y = reg_feat if self.centerness_on_reg else cls_feat
        for i, m in enumerate(self.conv_centerness_prev):
            y = self._conv([m], y, hw, ('ctr_prev', t, i))
        centerness = BboxPostFn.apply(None, (B, H, W, (1, ), False), self._pred(self.conv_centerness, y, ('ctr', t)))
        return cls_score, bbox_pred, dir_cls, centerness

    def forward_nhwc(self, levels):
        """levels: 4 NHWC maps [(x [B*H*W, pitch(C_i)] in the activation dtype, (B, H, W))] -> the four output lists."""
        feats = self._neck(levels)
        res = [self._single(x, hw, self.scales[lv]) for lv, (x, hw) in enumerate(feats)]
        return tuple(map(list, zip(*res)))

    def forward(self, feat):
        """feat: the 4 level maps, NCHW (the reference contract) -> (cls_scores, bbox_preds, dir_cls_preds, centernesses)."""
        if not isinstance(feat, (list, tuple)) or len(feat) != self.neck.num_ins:
            raise ValueError(f"FCOS3DHead takes the list of the backbone's {self.neck.num_ins} level maps")
        levels = []
        for x in feat:
            B, C, H, W = x.shape
            # NCHW -> NHWC rows with the channel pitch (a layout change; zero padding channels)
            rows = torch.zeros(B * H * W, pitch(C), dtype=self.prec.adt, device=x.device)
            rows[:, :C] = x.permute(0, 2, 3, 1).reshape(B * H * W, C)
            levels.append((rows, (B, H, W)))
        return self.forward_nhwc(levels)
