"""Plain-torch restatement of the reference FCOS3D criterion (TaskPrompter/detection_toolbox/det_model.py DetModel.loss with pred_bbox2d,
:253-481 and _get_target_single :858-955) for the tests and the timing tool (not product code).

`assign` works in fp32 in the reference's operation order (per image a [num_points, num_gts] intermediate), so its labels equal the
reference's bit for bit; `loss` evaluates the eight terms in `dtype` (fp64 by default; fp32 on the GPU restates the reference's own
path for timing) and is differentiable in the predictions.  tests/test_fcos3d_host.py pins it to tests/golden/fcos3d.*."""
import math

import torch
import torch.nn.functional as F

INF = 1e8
KEYS = ('loss_cls', 'loss_offset', 'loss_depth', 'loss_size', 'loss_rotsin', 'loss_dir', 'loss_centerness', 'loss_bbox2d')


def points(sizes, strides, device):
    out = []
    for (h, w), s in zip(sizes, strides):
        y, x = torch.meshgrid(torch.arange(h, dtype=torch.float32, device=device), torch.arange(w, dtype=torch.float32, device=device),
                              indexing='ij')
        out.append(torch.stack((x.reshape(-1) * s, y.reshape(-1) * s), dim=-1) + s // 2)
    return out


def assign_single(e, pts, lvl_of, strides, rr, radius, alpha, num_classes, dists_out=None):
    """one image -> labels [P] int64, targets [P, 13] (offsets and ltrb / stride), centerness [P]; dists_out (a list) receives the masked
    point-to-gt distance matrix [P, n] the assignment takes its minimum over"""
    P = pts.shape[0]
    dev = pts.device
    n = e['label'].shape[0]
    if n == 0:
        return (torch.full((P,), num_classes, dtype=torch.int64, device=dev), torch.zeros(P, 13, device=dev), torch.zeros(P, device=dev))
    box = e['bbox_modal'].float().to(dev)
    c2 = e['center_I'][:, :2].float().to(dev)
    dep = e['center_I'][:, 2].float().to(dev)
    s3 = torch.cat([e['size_S'], e['rotation_S']], 1).float().to(dev)
    xs, ys = pts[:, 0:1], pts[:, 1:2]                                          # [P, 1] against [1, n]
    dx, dy = xs - c2[None, :, 0], ys - c2[None, :, 1]
    left, right = xs - box[None, :, 0], box[None, :, 2] - xs
    top, bottom = ys - box[None, :, 1], box[None, :, 3] - ys
    st = torch.tensor([strides[l] * radius for l in range(len(strides))], dtype=torch.float32, device=dev)[lvl_of][:, None]
    cb = torch.stack((xs - (c2[None, :, 0] - st), ys - (c2[None, :, 1] - st), (c2[None, :, 0] + st) - xs, (c2[None, :, 1] + st) - ys), -1)
    inside = cb.min(-1)[0] > 0
    mx = torch.stack((left, top, right, bottom), -1).max(-1)[0]
    lo = torch.tensor([r[0] for r in rr], dtype=torch.float32, device=dev)[lvl_of][:, None]
    hi = torch.tensor([r[1] for r in rr], dtype=torch.float32, device=dev)[lvl_of][:, None]
    in_range = (mx >= lo) & (mx <= hi)
    dists = torch.sqrt(dx * dx + dy * dy)
    dists[~inside] = INF
    dists[~in_range] = INF
    if dists_out is not None:
        dists_out.append(dists.clone())
    md, mi = dists.min(dim=1)
    lab = e['label'].to(dev).long()[mi]
    lab[md == INF] = num_classes
    ar = torch.arange(P, device=dev)
    sdx, sdy = dx[ar, mi], dy[ar, mi]
    sf = torch.tensor([float(torch.tensor(s, dtype=torch.float32)) for s in strides], dtype=torch.float32, device=dev)[lvl_of]
    tgt = torch.cat([torch.stack((sdx / sf, sdy / sf, dep[mi]), 1), s3[mi],
                     torch.stack((left[ar, mi] / sf, top[ar, mi] / sf, right[ar, mi] / sf, bottom[ar, mi] / sf), 1)], 1)
    rel = torch.sqrt(sdx * sdx + sdy * sdy) / (1.414 * st[:, 0])
    return lab, tgt, torch.exp(-alpha * rel)


def assign(params, labels, sizes, device='cpu', dists_out=None):
    """-> keep (labelled batch indices), labels [n, P], targets [n, P, 13], centerness [n, P] (points in level order)"""
    strides = params['strides']
    pts = torch.cat(points(sizes, strides, device))
    lvl_of = torch.cat([torch.full((h * w,), l, dtype=torch.long, device=device) for l, (h, w) in enumerate(sizes)])
    dl, num = labels['det_labels'], labels['det_label_number']
    keep = [i for i in range(len(dl)) if int(num[i]) != 0]
    res = [assign_single(dl[i], pts, lvl_of, strides, params['regress_ranges'], params.get('center_sample_radius', 1.5),
                         params.get('centerness_alpha', 2.5), params['num_classes'], dists_out) for i in keep]
    if not res:
        return keep, None, None, None
    return keep, torch.stack([r[0] for r in res]), torch.stack([r[1] for r in res]), torch.stack([r[2] for r in res])


def _flat(maps, keep, C):
    """per-level NCHW maps of the kept images -> [n, P, C]"""
    return torch.cat([m[keep].flatten(2).transpose(1, 2) for m in maps], 1).reshape(len(keep), -1, C)


def loss(params, preds, labels, dtype=torch.float64):
    """-> (loss dict in KEYS order, loss_sum); differentiable in preds.  No image labelled: ({}, 0 * sum of the preds)."""
    cls, bbox, dirc, ctr = preds
    sizes = [tuple(m.shape[-2:]) for m in cls]
    dev = cls[0].device
    keep, lab, tgt, cen = assign(params, labels, sizes, dev)
    zero = sum(m.sum() for lst in preds for m in lst) * 0
    if not keep:
        return {}, zero.to(dtype)
    C = params['num_classes']
    x = _flat(cls, keep, C).to(dtype)
    bp = _flat(bbox, keep, 13).to(dtype)
    dp = _flat(dirc, keep, 6).to(dtype)
    cp = _flat(ctr, keep, 1).to(dtype)[..., 0]
    lw = lambda k: float(params[k].get('loss_weight', 1.0))
    fc = params['loss_cls']
    t = F.one_hot(lab, C + 1)[..., :C].to(dtype)
    s = x.sigmoid()
    pt = (1 - s) * t + s * (1 - t)
    fw = (fc['alpha'] * t + (1 - fc['alpha']) * (1 - t)) * pt.pow(fc['gamma'])
    focal = F.binary_cross_entropy_with_logits(x, t, reduction='none') * fw
    pos = (lab >= 0) & (lab < C)
    num_pos = pos.sum()
    out = {'loss_cls': lw('loss_cls') * focal.sum() / (num_pos + len(keep)).to(dtype)}
    npd = num_pos.clamp(min=1).to(dtype)                        # num_pos == 0: every positive sum is 0, as the reference's empty sums
    p, tg = bp[pos], tgt[pos].to(dtype)
    cw = torch.tensor(params.get('code_weight') or [1.0] * 13, dtype=dtype, device=dev)
    tr = tg[:, 6:9]
    pe = torch.cat([p[:, :6], torch.sin(p[:, 6:9]) * torch.cos(tr), p[:, 9:]], 1)
    te = torch.cat([tg[:, :6], torch.cos(p[:, 6:9]) * torch.sin(tr), tg[:, 9:]], 1)
    diff = (pe - te).abs()

    def sl1(sl, beta):
        d = diff[:, sl]
        return (torch.where(d < beta, 0.5 * d * d / beta, d - 0.5 * beta) * cw[sl]).sum() / npd

    b, b2 = params['loss_bbox']['beta'], params['loss_bbox2d']['beta']
    out['loss_offset'] = lw('loss_bbox') * sl1(slice(0, 2), b)
    out['loss_depth'] = lw('loss_bbox') * sl1(slice(2, 3), b)
    out['loss_size'] = lw('loss_bbox') * sl1(slice(3, 6), b)
    out['loss_rotsin'] = lw('loss_bbox') * sl1(slice(6, 9), b)
    rot = tgt[pos][:, 6:9] - params.get('dir_offset', 0)                                  # fp32, as get_direction_target
    period = 2 * math.pi
    lp = rot - torch.floor(rot / period + 0) * period
    bins = torch.floor(lp / (2 * math.pi / 2)).long().clamp(0, 1)
    d = dp[pos]
    out['loss_dir'] = sum(lw('loss_dir') * F.cross_entropy(d[:, 2 * r:2 * r + 2], bins[:, r], reduction='sum') / npd for r in range(3))
    out['loss_centerness'] = lw('loss_centerness') * F.binary_cross_entropy_with_logits(cp[pos], cen[pos].to(dtype), reduction='sum') / npd
    out['loss_bbox2d'] = lw('loss_bbox2d') * sl1(slice(9, 13), b2)
    out = {k: out[k] for k in KEYS}
    return out, sum(out.values()) + zero.to(dtype)
