"""TEST INFRASTRUCTURE ONLY — plain-torch restatement of the reference's FCOS3D box decoding for one image, as the Cityscapes-3D config
runs it (pred_bbox2d, norm_on_bbox, 9 + 4 regression channels, direction classifier), evaluable in fp32 and fp64 on any device:

  TaskPrompter/detection_toolbox/det_model.py   :231-250 denorm_on_bbox, :717-754 get_points, :555-681 _get_bboxes_single,
                                                :957-1002 get_results_from_bbox
  TaskPrompter/detection_toolbox/det_tools.py   :13-28 limit_period, :51-81 xywhpra2xyxya / bbox_bev, :85-210 box3d_multiclass_nms,
                                                :480-530 distance2bbox, :618-648 points_img2cam

Pinned to the unmodified reference by tests/golden/decode.npz (tests/golden/make_decode_golden.py) in tests/test_det_decode_host.py.
The per-class NMS is a callable `nms(boxes [n, 5], scores [n], thr, rotated) -> kept indices in score order`, the place of the
reference's nms_gpu / nms_normal_gpu: `oracle_nms` below (the CPU restatement of oracle/iou3d_oracle.py) or the HIP iou3d module."""
import math

import numpy as np
import torch

from oracle import iou3d_oracle

CFG_KEYS = ("use_rotate_nms", "nms_pre", "nms_thr", "score_thr", "max_per_img")


def oracle_nms(boxes, scores, thr, rotated):
    """descending sort + the greedy pass of oracle/iou3d_oracle.py's `nms`, its IoU evaluated only for pairs whose circumscribed circles
    come within reach of each other (the others are disjoint: IoU exactly 0, never above a positive threshold)"""
    assert thr > 0
    order = scores.sort(0, descending=True)[1]
    bx = boxes[order].detach().cpu().float().numpy()
    fn = iou3d_oracle.iou_bev if rotated else iou3d_oracle.iou_normal
    b64 = bx.astype(np.float64)
    ctr = np.stack([(b64[:, 0] + b64[:, 2]) / 2, (b64[:, 1] + b64[:, 3]) / 2], 1)
    rad = np.hypot(b64[:, 2] - b64[:, 0], b64[:, 3] - b64[:, 1]) / 2
    near = np.hypot(ctr[:, None, 0] - ctr[None, :, 0], ctr[:, None, 1] - ctr[None, :, 1]) <= (rad[:, None] + rad[None, :]) * 1.001 + 1e-3
    removed = np.zeros(len(bx), dtype=bool)
    keep = []
    for i in range(len(bx)):
        if removed[i]:
            continue
        keep.append(i)
        for j in np.nonzero(near[i, i + 1:] & ~removed[i + 1:])[0] + i + 1:
            if fn(bx[i], bx[j]) > np.float32(thr):
                removed[j] = True
    return order[torch.tensor(keep, dtype=torch.long, device=order.device)]


def hip_nms(boxes, scores, thr, rotated):
    """the product's iou3d.nms_gpu / nms_normal_gpu (one host read per call, as the reference's)"""
    import mtt_amd
    fn = mtt_amd.iou3d.nms_gpu if rotated else mtt_amd.iou3d.nms_normal_gpu
    return fn(boxes.float(), scores.float(), thr)


def get_points(sizes, strides, dtype, device):
    """:717-754: (x * stride, y * stride) + stride // 2 per level, row-major"""
    out = []
    for (h, w), stride in zip(sizes, strides):
        y, x = torch.meshgrid(torch.arange(h, dtype=dtype, device=device), torch.arange(w, dtype=dtype, device=device), indexing='ij')
        out.append(torch.stack((x.reshape(-1) * stride, y.reshape(-1) * stride), dim=-1) + stride // 2)
    return out


def points_img2cam(points, cam2img):
    """det_tools.py:618-648; the inverse is taken in the points' dtype"""
    xys, depths = points[:, :2], points[:, 2].view(-1, 1)
    unnormed = torch.cat([xys * depths, depths], dim=1)
    pad = torch.eye(4, dtype=xys.dtype, device=xys.device)
    pad[:cam2img.shape[0], :cam2img.shape[1]] = cam2img.to(device=xys.device, dtype=xys.dtype)
    inv = torch.inverse(pad.cpu()).to(xys.device).transpose(0, 1)
    homo = torch.cat([unnormed, xys.new_ones((unnormed.shape[0], 1))], dim=1)
    return torch.mm(homo, inv)[:, :3]


def limit_period(val, offset, period):
    return val - torch.floor(val / period + offset) * period


def decode_single(cls_scores, bbox_preds, dir_cls_preds, centernesses, strides, K, img_size, cfg, nms, dtype=torch.float32,
                  dir_offset=0, denorm=True, trace=None):
    """One image: per-level [C, H, W], [13, H, W], [6, H, W], [1, H, W] maps of the head (normalised: denorm=True applies
    denorm_on_bbox) -> dict(boxes_3d [n, 9], scores_3d [n], labels_3d [n] int64, centers2d [n, 3], bbox2d [n, 5]).  `trace`, a dict,
    receives the intermediate quantities the fixture generator takes its decision margins from."""
    C = cls_scores[0].shape[0]
    dev = cls_scores[0].device
    sizes = [tuple(c.shape[-2:]) for c in cls_scores]
    mlvl_points = get_points(sizes, strides, dtype, dev)
    c2d, boxes, scs, dirs, ctrs, b2d, keys, dir_logits = [], [], [], [], [], [], [], []
    for lv, points in enumerate(mlvl_points):
        bbox = bbox_preds[lv].to(dtype).clone()
        if denorm:                                                             # :231-250
            bbox[:2] *= strides[lv]
            bbox[-4:] *= strides[lv]
        scores = cls_scores[lv].to(dtype).permute(1, 2, 0).reshape(-1, C).sigmoid()
        dlog = dir_cls_preds[lv].to(dtype).permute(1, 2, 0).reshape(-1, 3, 2)
        dir_cls = torch.max(dlog, dim=-1)[1]
        ctr = centernesses[lv].to(dtype).permute(1, 2, 0).reshape(-1).sigmoid()
        bbox = bbox.permute(1, 2, 0).reshape(-1, 13)
        b3, bd2 = bbox[:, :9].clone(), bbox[:, -4:]
        key = (scores * ctr[:, None]).max(dim=1)[0]
        keys.append(key)
        if cfg["nms_pre"] > 0 and scores.shape[0] > cfg["nms_pre"]:            # :615-626
            _, top = key.topk(cfg["nms_pre"])
            points, b3, scores, dlog, dir_cls, ctr, bd2 = points[top], b3[top], scores[top], dlog[top], dir_cls[top], ctr[top], bd2[top]
        b3[:, :2] = points - b3[:, :2]
        c2d.append(b3[:, :3].clone())
        b3[:, :3] = points_img2cam(b3[:, :3], K)
        boxes.append(b3)
        scs.append(scores)
        dirs.append(dir_cls)
        dir_logits.append(dlog)
        ctrs.append(ctr)
        x1, y1 = points[:, 0] - bd2[:, 0], points[:, 1] - bd2[:, 1]            # distance2bbox, det_tools.py:480-509
        x2, y2 = points[:, 0] + bd2[:, 2], points[:, 1] + bd2[:, 3]
        bb = torch.stack([x1, y1, x2, y2], -1)
        bb[:, 0::2] = bb[:, 0::2].clamp(min=0, max=float(img_size[1]))
        bb[:, 1::2] = bb[:, 1::2].clamp(min=0, max=float(img_size[0]))
        b2d.append(bb)
    c2d, boxes, dirs, b2d = torch.cat(c2d), torch.cat(boxes), torch.cat(dirs), torch.cat(b2d)
    raw_rot = boxes[:, 6:9].clone()
    for i, rot in enumerate(range(6, 9)):                                      # :651-657
        dir_rot = limit_period(boxes[:, rot] - dir_offset, 0, np.pi)
        boxes[:, rot] = dir_rot + dir_offset + np.pi * dirs[:, i].to(dtype)
    bev = boxes[:, [0, 2, 4, 3, 6, 7, 8]]                                      # bbox_bev, xywhpra2xyxya
    nb = torch.zeros(boxes.shape[0], 5, dtype=dtype, device=dev)
    nb[:, 0], nb[:, 1] = bev[:, 0] - bev[:, 2] / 2, bev[:, 1] - bev[:, 3] / 2
    nb[:, 2], nb[:, 3] = bev[:, 0] + bev[:, 2] / 2, bev[:, 1] + bev[:, 3] / 2
    nb[:, 4] = bev[:, 6]
    nms_scores = torch.cat(scs) * torch.cat(ctrs)[:, None]                     # :670 (the padded background column is never read)
    if trace is not None:
        trace.update(keys=keys, scores=nms_scores, nms_boxes=nb, raw_rot=raw_rot, dir_logits=torch.cat(dir_logits), boxes=boxes,
                     centers2d=c2d, bbox2d=b2d)
    ob, osc, ol, oc, o2 = [], [], [], [], []
    for c in range(C):                                                         # box3d_multiclass_nms, det_tools.py:130-163
        m = nms_scores[:, c] > cfg["score_thr"]
        if not m.any():
            continue
        s = nms_scores[m, c]
        sel = nms(nb[m], s, cfg["nms_thr"], bool(cfg["use_rotate_nms"]))
        ob.append(boxes[m][sel]); osc.append(s[sel]); oc.append(c2d[m][sel]); o2.append(b2d[m][sel])
        ol.append(torch.full((len(sel),), c, dtype=torch.long, device=dev))
    if ob:
        ob, osc, ol, oc, o2 = torch.cat(ob), torch.cat(osc), torch.cat(ol), torch.cat(oc), torch.cat(o2)
        if ob.shape[0] > cfg["max_per_img"]:                                   # :176-188
            inds = osc.sort(descending=True)[1][:cfg["max_per_img"]]
            ob, osc, ol, oc, o2 = ob[inds], osc[inds], ol[inds], oc[inds], o2[inds]
    else:
        ob, osc, ol = torch.zeros(0, 9, dtype=dtype, device=dev), torch.zeros(0, dtype=dtype, device=dev), torch.zeros(0, dtype=torch.long, device=dev)
        oc, o2 = torch.zeros(0, 3, dtype=dtype, device=dev), torch.zeros(0, 4, dtype=dtype, device=dev)
    return dict(boxes_3d=ob, scores_3d=osc, labels_3d=ol, centers2d=oc, bbox2d=torch.cat([o2, osc[:, None]], dim=1))


def decode_batch(preds, strides, label, cfg, nms, dtype=torch.float32, dir_offset=0, denorm=True):
    """get_results_from_bbox (:957-1002) on the restatement: one dict per image"""
    cls_scores, bbox_preds, dir_cls_preds, centernesses = preds
    meta = label['meta']
    out = []
    for b in range(len(meta['img_name'])):
        pick = lambda lst: [t[b].detach() for t in lst]
        out.append(decode_single(pick(cls_scores), pick(bbox_preds), pick(dir_cls_preds), pick(centernesses), strides,
                                 torch.as_tensor(meta['K_matrix'][b]), meta['img_size'][b], cfg, nms, dtype, dir_offset, denorm))
    return out


COLUMNS = ("boxes_3d", "scores_3d", "centers2d", "bbox2d")


def columns(res):
    """the value columns of one image's result, in a fixed order: name -> 1-D float64 numpy array"""
    out = {}
    for k in COLUMNS:
        v = res[k].detach().cpu().double().numpy() if isinstance(res[k], torch.Tensor) else np.asarray(res[k], dtype=np.float64)
        v = v.reshape(v.shape[0], -1)
        for j in range(v.shape[1]):
            out[f"{k}[{j}]"] = v[:, j]
    return out


def from_product(res):
    """one image's dict of DetModel.get_results_from_bbox -> the restatement's result layout"""
    ib = res['img_bbox']
    b2 = res['img_bbox2d']
    b2 = torch.zeros(0, 5, dtype=torch.float64) if isinstance(b2, list) else torch.from_numpy(np.asarray(b2))
    return dict(boxes_3d=ib['boxes_3d'], scores_3d=ib['scores_3d'], labels_3d=ib['labels_3d'], centers2d=ib['centers2d'], bbox2d=b2)


def pi_distance(raw_rot):
    """distance of rot / pi from the nearest integer (a decision margin of floor())"""
    q = raw_rot.double() / math.pi
    return (q - q.round()).abs()
