"""Plain-torch CPU restatements for the 3ddet head tests (not product code).

`dcn_v2` restates mmcv 1.6.2's modulated_deform_conv2d (deform_groups = groups = 1) in differentiable torch: tap k = i*3 + j samples
h = ho*s - p + i*d + offset[2k], w = wo*s - p + j*d + offset[2k+1]; a point with h <= -1, w <= -1, h >= H or w >= W samples 0, and inside
that box corners outside the map contribute 0 (bilinear); the column value is the sample times mask[k].
`head_forward` runs an FCOS3DHead's parameters through nn.functional ops (conv2d / group_norm / interpolate + dcn_v2), the structure of
the reference's FPN.forward and FCOS3DHead.forward_single (det_head.py:392-457)."""
import torch
import torch.nn.functional as F


def dcn_v2(x, offset, mask, weight, bias, stride=1, pad=1, dil=1):
    """x [B, C, H, W], offset [B, 18, Ho, Wo] or None, mask [B, 9, Ho, Wo] or None, weight [Co, C, 3, 3] -> [B, Co, Ho, Wo]."""
    B, C, H, W = x.shape
    Ho = (H + 2 * pad - dil * 2 - 1) // stride + 1
    Wo = (W + 2 * pad - dil * 2 - 1) // stride + 1
    dt = x.dtype
    ho = torch.arange(Ho, dtype=dt).view(1, Ho, 1)
    wo = torch.arange(Wo, dtype=dt).view(1, 1, Wo)
    cols = []
    xf = x.reshape(B, C, H * W)
    for k in range(9):
        i, j = divmod(k, 3)
        h = (ho * stride - pad + i * dil).expand(B, Ho, Wo)
        w = (wo * stride - pad + j * dil).expand(B, Ho, Wo)
        if offset is not None:
            h = h + offset[:, 2 * k]
            w = w + offset[:, 2 * k + 1]
        inside = (h > -1) & (w > -1) & (h < H) & (w < W)
        hl, wl = torch.floor(h), torch.floor(w)
        lh, lw = h - hl, w - wl
        val = torch.zeros(B, C, Ho, Wo, dtype=dt)
        for dy, dx, wt in ((0, 0, (1 - lh) * (1 - lw)), (0, 1, (1 - lh) * lw), (1, 0, lh * (1 - lw)), (1, 1, lh * lw)):
            yy, xx = hl.long() + dy, wl.long() + dx
            ok = inside & (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1)
            idx = (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).view(B, 1, Ho * Wo).expand(B, C, Ho * Wo)
            g = torch.gather(xf, 2, idx).view(B, C, Ho, Wo)
            val = val + g * (wt * ok.to(dt)).unsqueeze(1)
        if mask is not None:
            val = val * mask[:, k].unsqueeze(1)
        cols.append(val)
    col = torch.stack(cols, 2)                                          # [B, C, 9, Ho, Wo]
    y = torch.einsum('bckhw,ock->bohw', col, weight.reshape(weight.shape[0], C, 9))
    return y if bias is None else y + bias.view(1, -1, 1, 1)


def dcn_brute(x, offset, mask, weight, bias, stride=1, pad=1, dil=1):
    """dcn_v2 as an explicit per-pixel loop (fp64 cross-check of the restatement)."""
    B, C, H, W = x.shape
    Co = weight.shape[0]
    Ho = (H + 2 * pad - dil * 2 - 1) // stride + 1
    Wo = (W + 2 * pad - dil * 2 - 1) // stride + 1
    out = torch.zeros(B, Co, Ho, Wo, dtype=x.dtype)
    for b in range(B):
        for oy in range(Ho):
            for ox in range(Wo):
                acc = torch.zeros(Co, dtype=x.dtype) if bias is None else bias.clone().to(x.dtype)
                for k in range(9):
                    i, j = divmod(k, 3)
                    h = oy * stride - pad + i * dil + (float(offset[b, 2 * k, oy, ox]) if offset is not None else 0.0)
                    w = ox * stride - pad + j * dil + (float(offset[b, 2 * k + 1, oy, ox]) if offset is not None else 0.0)
                    m = float(mask[b, k, oy, ox]) if mask is not None else 1.0
                    v = torch.zeros(C, dtype=x.dtype)
                    if h > -1 and w > -1 and h < H and w < W:
                        import math
                        h0, w0 = math.floor(h), math.floor(w)
                        lh, lw = h - h0, w - w0
                        for yy, xx, wt in ((h0, w0, (1 - lh) * (1 - lw)), (h0, w0 + 1, (1 - lh) * lw), (h0 + 1, w0, lh * (1 - lw)),
                                           (h0 + 1, w0 + 1, lh * lw)):
                            if 0 <= yy <= H - 1 and 0 <= xx <= W - 1:
                                v = v + wt * x[b, :, yy, xx]
                    acc = acc + weight[:, :, i, j] @ (v * m)
                out[b, :, oy, ox] = acc
    return out


def dcn_pack(x, mod):
    """ModulatedDeformConv2dPack.forward: o1, o2, m = chunk(conv_offset(x), 3); offset = cat(o1, o2); mask = sigmoid(m)."""
    om = F.conv2d(x, mod.conv_offset.weight.to(x.dtype), mod.conv_offset.bias.to(x.dtype), padding=1)
    o1, o2, m = torch.chunk(om, 3, dim=1)
    return dcn_v2(x, torch.cat((o1, o2), 1), torch.sigmoid(m), mod.weight.to(x.dtype),
                  None if mod.bias is None else mod.bias.to(x.dtype))


def _cm(m, x):
    """ConvModule: conv -> gn -> relu"""
    c = m.conv
    if getattr(m, 'dcn', False):
        y = dcn_pack(x, c)
    else:
        y = F.conv2d(x, c.weight.to(x.dtype), None if c.bias is None else c.bias.to(x.dtype), stride=c.stride, padding=c.padding)
    if getattr(m, 'groups', 0):
        y = F.relu(F.group_norm(y, m.groups, m.gn.weight.to(x.dtype), m.gn.bias.to(x.dtype), eps=1e-5))
    return y


def _c1(conv, x):
    return F.conv2d(x, conv.weight.to(x.dtype), conv.bias.to(x.dtype))


def head_forward(head, feats):
    """FPN + FCOS3DHead forward on NCHW inputs in their dtype."""
    neck = head.neck
    lat = [_c1(neck.lateral_convs[i].conv, x) for i, x in enumerate(feats)]
    for i in range(len(lat) - 1, 0, -1):
        lat[i - 1] = lat[i - 1] + F.interpolate(lat[i], size=lat[i - 1].shape[2:], mode='nearest')
    outs = [_cm(neck.fpn_convs[i], lat[i]) for i in range(len(lat))]
    for i in range(len(lat), neck.num_outs):
        outs.append(_cm(neck.fpn_convs[i], outs[-1]))
    res = {k: [] for k in ('cls', 'bbox', 'dir', 'ctr')}
    for lv, x in enumerate(outs):
        cls_feat, reg_feat = x, x
        for m in head.cls_convs:
            cls_feat = _cm(m, cls_feat)
        for m in head.reg_convs:
            reg_feat = _cm(m, reg_feat)
        y = cls_feat
        for m in head.conv_cls_prev:
            y = _cm(m, y)
        res['cls'].append(_c1(head.conv_cls, y))
        preds = []
        for prev, conv in zip(head.conv_reg_prevs, head.conv_regs):
            y = reg_feat
            for m in (prev if prev is not None else []):
                y = _cm(m, y)
            preds.append(_c1(conv, y))
        bp = torch.cat(preds, 1)
        sc = head.scales[lv]
        parts = [bp[:, :2] * sc[0].scale, (bp[:, 2:3] * sc[1].scale).exp(), (bp[:, 3:6] * sc[2].scale).exp() + 1e-6]
        if head.pred_bbox2d:
            parts += [bp[:, 6:-4], F.relu(bp[:, -4:] * sc[-1].scale)]
        else:
            parts += [bp[:, 6:]]
        res['bbox'].append(torch.cat(parts, 1))
        y = reg_feat
        for m in head.conv_dir_cls_prev:
            y = _cm(m, y)
        res['dir'].append(_c1(head.conv_dir_cls, y))
        y = reg_feat if head.centerness_on_reg else cls_feat
        for m in head.conv_centerness_prev:
            y = _cm(m, y)
        res['ctr'].append(_c1(head.conv_centerness, y))
    return res['cls'], res['bbox'], res['dir'], res['ctr']


def mini_head_params(in_channels=(32, 48, 64, 64), feat=64):
    """a miniature det_head_params (cs_swinB structure, 64-wide; cls_branch ends at 32 channels = one channel per GN group)"""
    neck = dict(type='FPN', in_channels=list(in_channels), out_channels=feat, start_level=0, add_extra_convs='on_output', num_outs=5,
                relu_before_extra_convs=True)
    return dict(num_classes=6, in_channels=feat, centerness_on_reg=True, norm_cfg=dict(type='GN', num_groups=32, requires_grad=True),
                dcn_on_last_conv=True, conv_bias=True, use_direction_classifier=True, group_reg_dims=(2, 1, 3, 3, 4),
                reg_branch=((feat, ),) * 5, centerness_branch=(feat, ), cls_branch=(feat, 32), dir_branch=(feat, ), fpn_scale_no=5,
                feat_channels=feat, stacked_convs=3, bbox_code_size=9, pred_bbox2d=True, pred_keypoints=False, conv_cfg=None,
                init_cfg=None, neck_cfg=neck)


def randomize(head, seed=0, offset_px=3.0):
    """weights with non-trivial GN affine parameters, Scales and DCN offsets of about +-offset_px (samples leave the map)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in head.named_parameters():
            if name.endswith('conv_offset.weight'):
                p.copy_(torch.randn(p.shape, generator=g) * (offset_px / (p.shape[1] * 9) ** 0.5))
            elif name.endswith('conv_offset.bias'):
                p.copy_(torch.randn(p.shape, generator=g) * 1.0)
            elif name.endswith('gn.weight'):
                p.copy_(1.0 + 0.3 * torch.randn(p.shape, generator=g))
            elif name.endswith('gn.bias'):
                p.copy_(0.3 * torch.randn(p.shape, generator=g))
            elif name.endswith('.scale'):
                p.copy_(0.8 + 0.4 * torch.rand(p.shape, generator=g))
            elif p.dim() == 4:
                fan_in = p.shape[1] * p.shape[2] * p.shape[3]
                p.copy_(torch.randn(p.shape, generator=g) * (2.0 / fan_in) ** 0.5)
            else:
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
