"""The FCOS3D criterion and box decoding of the 3ddet task: `DetModel` of TaskPrompter/detection_toolbox/det_model.py (constructor
:41-127, `loss` :253-481, `get_bboxes` :483-681, `get_points` / `get_targets` :717-955, `get_results_from_bbox` :957-1002), with
`pred_bbox2d=True` as the Cityscapes-3D config builds it.

`DetModel.loss(preds, labels) -> (loss_dict, loss_sum)` takes the head's per-level NCHW fp32 lists (FCOS3DHead.forward) and the
reference's collated labels.  The host packs the ragged gt lists into one device buffer (shapes and the per-image `det_label_number`
only, both host data in the reference's loader); from there the HIP kernels of csrc/det_loss3d.hip assign the gts to the FPN points,
evaluate the eight loss terms straight from the NCHW maps and write every map's gradient.  num_pos and the averaging factors stay on the
device: no host synchronisation between the packed labels and `loss_sum`.  Raises on CPU tensors and non-fp32 maps (no fallback).

Differences from the reference, all outside its arithmetic:
- the loss dict has the key order of the reference's `num_pos > 0` branch whether or not there are positives (num_pos lives on the device);
  with no positives every positive-only term is exactly 0, as the reference's sums over empty tensors are;
- the constructor copies the loss config dicts instead of deleting their 'type' keys, so one parameter dict can build several criteria;
- options the kernels do not implement raise NotImplementedError naming the option.

`DetModel.get_results_from_bbox(preds, label, rescale=False)` and `get_bboxes(...)` decode the same maps at inference: pre-selection,
back-projection through the camera matrix, the direction classes, per-class rotated (or axis-aligned) NMS and the per-image cap all run
in the HIP kernels of csrc/det_decode.hip with fixed-capacity buffers; the one host synchronisation is the final device-to-host copy of
the kept rows and their counts (the reference synchronises once per class and again inside every NMS call).  The order of exactly equal
scores is unspecified, as in the reference; `rescale=True` raises NotImplementedError (the reference raises there too with pred_bbox2d).
"""
import copy

import numpy as np
import torch
import torch.nn as nn

from . import det_decode, ops

INF = 1e8
LOSS_KEYS = ('loss_cls', 'loss_offset', 'loss_depth', 'loss_size', 'loss_rotsin', 'loss_dir', 'loss_centerness', 'loss_bbox2d')
MAX_LEVELS = 8
_REC = 16                                            # floats per packed gt record (include/mtt_hip.h, ABI 15)

# per loss position: the reference config's type, and the options each type accepts (det_losses.py constructors)
_LOSS_SPEC = {
    'loss_cls': ('FocalLoss', dict(use_sigmoid=True)),
    'loss_bbox': ('SmoothL1Loss', {}),
    'loss_centerness': ('CrossEntropyLoss', dict(use_sigmoid=True)),
    'loss_dir': ('CrossEntropyLoss', dict(use_sigmoid=False)),
    'loss_bbox2d': ('SmoothL1Loss', {}),
    'loss_consistency': ('GIoULoss', {}),
}
_LOSS_ARGS = {
    'FocalLoss': dict(use_sigmoid=True, gamma=2.0, alpha=0.25, reduction='mean', loss_weight=1.0),
    'SmoothL1Loss': dict(beta=1.0, reduction='mean', loss_weight=1.0),
    'CrossEntropyLoss': dict(use_sigmoid=False, use_mask=False, reduction='mean', class_weight=None, ignore_index=None, loss_weight=1.0),
    'GIoULoss': dict(eps=1e-6, reduction='mean', loss_weight=1.0),
}


def _loss_cfg(pos, cfg):
    """the reference's build_loss (:131-147) for one loss position -> the resolved options; refuses what the kernels do not implement"""
    cfg = dict(cfg)
    typ = cfg.pop('type', None)
    want, fixed = _LOSS_SPEC[pos]
    if typ != want:
        raise NotImplementedError(f"{pos}: type {typ!r} (only {want!r} is implemented at this position)")
    args = dict(_LOSS_ARGS[typ])
    for k, v in cfg.items():
        if k not in args:
            raise TypeError(f"{pos}: {typ} got an unexpected option {k!r}")
        args[k] = v
    for k, v in fixed.items():
        if args[k] != v:
            raise NotImplementedError(f"{pos}: {k}={args[k]!r} (only {v!r} is implemented)")
    if args['reduction'] != 'mean':
        raise NotImplementedError(f"{pos}: reduction={args['reduction']!r} (only 'mean' is implemented)")
    for k in ('class_weight', 'ignore_index'):
        if args.get(k) is not None:
            raise NotImplementedError(f"{pos}: {k}={args[k]!r} (only None is implemented)")
    if args.get('use_mask'):
        raise NotImplementedError(f"{pos}: use_mask=True")
    return args


class PackedDetLabels:
    """The labels of one batch on the device: `img` int32 [3 n_lab + B] (gt offset, gt count and batch index of every labelled image,
    then the labelled index of every batch image or -1) and `gts` fp32 [max(n_gts, 1), 16] records (include/mtt_hip.h, ABI 15)."""

    def __init__(self, img, gts, B, keep, counts):
        self.img, self.gts, self.B, self.keep, self.counts = img, gts, B, list(keep), list(counts)
        self.n_lab = len(self.keep)


def _records(bbox_modal, label, center_I, size_S, rotation_S):
    n = bbox_modal.shape[0]
    dev = bbox_modal.device
    f = lambda t, c: t.reshape(n, c).to(device=dev, dtype=torch.float32)
    return torch.cat([f(bbox_modal, 4), f(label, 1), f(center_I, 3), f(size_S, 3), f(rotation_S, 3),
                      torch.zeros(n, 2, dtype=torch.float32, device=dev)], 1)


def _pack(B, keep, recs, device):
    counts = [int(r.shape[0]) for r in recs]
    offs, o = [], 0
    for c in counts:
        offs.append(o)
        o += c
    compact = [-1] * B
    for k, b in enumerate(keep):
        compact[b] = k
    img = torch.tensor(offs + counts + list(keep) + compact, dtype=torch.int32).to(device, non_blocking=True)
    recs = [r.to(device, non_blocking=True) for r in recs]
    gts = torch.cat(recs) if o > 0 else torch.zeros(1, _REC, dtype=torch.float32, device=device)
    return PackedDetLabels(img, gts, B, keep, counts)


def pack_det_labels(labels, device):
    """The reference's collated labels (det_model.py:262-289: labels['det_labels'][i] with bbox_modal [n, 4], label [n], center_S,
    size_S, rotation_S, center_I [n, 3]; labels['det_label_number'] beside it) -> PackedDetLabels on `device`.  Images with
    det_label_number == 0 leave the batch.  Reads only shapes and the counts (host data in the reference's loader)."""
    dl, nums = labels['det_labels'], labels['det_label_number']
    B = len(dl)
    keep = [i for i in range(B) if int(nums[i]) != 0]
    recs = []
    for i in keep:
        e = dl[i]
        if e['center_S'].shape[0] != e['label'].shape[0]:
            raise ValueError(f"image {i}: center_S has {e['center_S'].shape[0]} rows for {e['label'].shape[0]} labels")
        recs.append(_records(e['bbox_modal'], e['label'], e['center_I'], e['size_S'], e['rotation_S']))
    return _pack(B, keep, recs, torch.device(device))


class _DetLossFn(torch.autograd.Function):
    """(crit, packed, geometry, *maps) -> out [9] = the eight components and loss_sum; backward writes the gradient of every map"""

    @staticmethod
    def forward(ctx, crit, packed, geo, *maps):
        L = len(maps) // 4
        dev = maps[0].device
        ctx.crit, ctx.packed, ctx.geo = crit, packed, geo
        if packed.n_lab == 0:                                 # every image dropped: a zero connected to the predictions (:290-292)
            ctx.empty = True
            ctx.shapes = [m.shape for m in maps]
            return torch.zeros(9, dtype=torch.float32, device=dev)
        ctx.empty = False
        B, P = packed.B, geo['P']
        label = torch.empty(packed.n_lab, P, dtype=torch.int32, device=dev)
        target = torch.empty(packed.n_lab, 13, P, dtype=torch.float32, device=dev)
        ctr = torch.empty(packed.n_lab, P, dtype=torch.float32, device=dev)
        out = torch.empty(9, dtype=torch.float32, device=dev)
        stats = torch.empty(2, dtype=torch.float32, device=dev)
        kw = crit._desc(geo, packed, label, target, ctr)
        kw.update(cls=list(maps[:L]), bbox=list(maps[L:2 * L]), dir=list(maps[2 * L:3 * L]), ctr=list(maps[3 * L:]), out=out, stats=stats)
        kw['ws'] = ops.ws_for("fcos3d", dev, P=P, n_lab=packed.n_lab)
        ops.call("fcos3d_loss_fwd", **kw)
        ctx.kw = {k: v for k, v in kw.items() if k not in ('cls', 'bbox', 'dir', 'ctr', 'ws', 'out')}
        ctx.save_for_backward(*maps)
        return out

    @staticmethod
    def backward(ctx, gout):
        if ctx.empty:
            return (None, None, None) + tuple(gout.new_zeros(s) for s in ctx.shapes)
        maps = ctx.saved_tensors
        L = len(maps) // 4
        grads = [torch.empty_like(m) for m in maps]
        kw = dict(ctx.kw)
        kw.update(cls=list(maps[:L]), bbox=list(maps[L:2 * L]), dir=list(maps[2 * L:3 * L]), ctr=list(maps[3 * L:]),
                  dcls=grads[:L], dbbox=grads[L:2 * L], ddir=grads[2 * L:3 * L], dctr=grads[3 * L:], gout=gout.float().contiguous())
        ops.call("fcos3d_loss_bwd", **kw)
        return (None, None, None) + tuple(grads)


class DetModel(nn.Module):
    """FCOS3D target assignment and loss (det_model.py:41-481), same constructor signature and defaults."""

    def __init__(self,
                 num_classes,
                 regress_ranges=((-1, 48), (48, 96), (96, 192), (192, 384), (384, INF)),
                 center_sampling=True,
                 center_sample_radius=1.5,
                 norm_on_bbox=True,
                 centerness_on_reg=True,
                 centerness_alpha=2.5,
                 loss_cls=dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0),
                 loss_bbox=dict(type='SmoothL1Loss', beta=1.0 / 9.0, loss_weight=1.0),
                 loss_centerness=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0),
                 loss_dir=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0),
                 loss_bbox2d=dict(type='SmoothL1Loss', beta=1.0 / 9.0, loss_weight=1.0),
                 loss_consistency=dict(type='GIoULoss', loss_weight=1.0),
                 stacked_convs=4,
                 strides=(4, 8, 16, 32, 64),
                 conv_bias='auto',
                 background_label=None,
                 use_direction_classifier=True,
                 diff_rad_by_sin=True,
                 dir_offset=0,
                 bbox_code_size=9,
                 pred_bbox2d=False,
                 pred_keypoints=False,
                 group_reg_dims=(2, 1, 3, 1, 2),
                 code_weight=None,
                 test_cfg=None,
                 ):
        super().__init__()
        self.regress_ranges = regress_ranges
        self.center_sampling = center_sampling
        self.center_sample_radius = center_sample_radius
        self.norm_on_bbox = norm_on_bbox
        self.centerness_on_reg = centerness_on_reg
        self.centerness_alpha = centerness_alpha
        self.num_classes = num_classes
        self.cls_out_channels = num_classes
        self.stacked_convs = stacked_convs
        self.strides = strides
        assert conv_bias == 'auto' or isinstance(conv_bias, bool)
        self.conv_bias = conv_bias
        self.use_direction_classifier = use_direction_classifier
        self.diff_rad_by_sin = diff_rad_by_sin
        self.dir_offset = dir_offset
        self.bbox_code_size = bbox_code_size
        self.group_reg_dims = list(group_reg_dims)
        self.code_weight = code_weight
        self.pred_bbox2d = pred_bbox2d
        self.pred_keypoints = pred_keypoints
        self.out_channels = []
        self.fp16_enabled = False
        self.background_label = num_classes if background_label is None else background_label
        assert self.background_label == 0 or self.background_label == num_classes
        self.test_cfg = test_cfg
        for name, ok in (('pred_keypoints=True', not pred_keypoints), ('center_sampling=False', center_sampling),
                         ('use_direction_classifier=False', use_direction_classifier), ('pred_bbox2d=False', pred_bbox2d),
                         ('diff_rad_by_sin=False', diff_rad_by_sin), ('norm_on_bbox=False', norm_on_bbox),
                         ('background_label=0', self.background_label == num_classes)):
            if not ok:
                raise NotImplementedError(f"DetModel: {name} is not implemented")
        if bbox_code_size != 9 or sum(self.group_reg_dims) != 13:
            raise NotImplementedError(f"DetModel: bbox_code_size={bbox_code_size}, group_reg_dims={tuple(group_reg_dims)} "
                                      "(only the 9 + 4 regression channels of the Cityscapes-3D config are implemented)")
        if len(strides) != len(regress_ranges) or not 0 < len(strides) <= MAX_LEVELS:
            raise NotImplementedError(f"DetModel: {len(strides)} strides for {len(regress_ranges)} regress ranges (1..{MAX_LEVELS} levels)")
        if code_weight and len(code_weight) != 13:
            raise ValueError(f"code_weight has {len(code_weight)} entries for 13 regression channels")
        self.cfg_cls = _loss_cfg('loss_cls', loss_cls)
        self.cfg_bbox = _loss_cfg('loss_bbox', loss_bbox)
        self.cfg_centerness = _loss_cfg('loss_centerness', loss_centerness)
        self.cfg_dir = _loss_cfg('loss_dir', loss_dir)
        self.cfg_bbox2d = _loss_cfg('loss_bbox2d', loss_bbox2d)
        self.cfg_consistency = _loss_cfg('loss_consistency', loss_consistency)     # built by the reference, never evaluated in loss
        for c in (self.cfg_bbox, self.cfg_bbox2d):
            if not c['beta'] > 0:
                raise ValueError("SmoothL1Loss needs beta > 0")

    # ---- kernel descriptor -------------------------------------------------------------------------------------------------------
    def _geometry(self, sizes):
        """featmap sizes -> the per-level fp32 constants of the kernels, computed as the reference computes them"""
        L = len(sizes)
        if L != len(self.strides):
            raise ValueError(f"{L} feature levels for {len(self.strides)} strides")
        f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))
        geo = dict(H=[int(h) for h, _ in sizes], W=[int(w) for _, w in sizes], nlev=L)
        geo['stride'] = [f32(s) for s in self.strides]                               # points: x * stride (fp32)
        geo['half'] = [f32(s // 2) for s in self.strides]                            #   + stride // 2 (a float floor-division)
        geo['radius'] = [f32(s * self.center_sample_radius) for s in self.strides]   # :907-911, the product in double, stored fp32
        geo['rr_lo'] = [f32(r[0]) for r in self.regress_ranges]
        geo['rr_hi'] = [f32(r[1]) for r in self.regress_ranges]
        geo['P'] = sum(h * w for h, w in zip(geo['H'], geo['W']))
        return geo

    def _desc(self, geo, packed, label, target, ctr):
        pad = lambda v, n, z: list(v) + [z] * (n - len(v))
        cw = self.code_weight if self.code_weight else [1.0] * 13
        return dict(H=pad(geo['H'], 8, 0), W=pad(geo['W'], 8, 0), stride=pad(geo['stride'], 8, 0.0), half=pad(geo['half'], 8, 0.0),
                    radius=pad(geo['radius'], 8, 0.0), rr_lo=pad(geo['rr_lo'], 8, 0.0), rr_hi=pad(geo['rr_hi'], 8, 0.0),
                    nlev=geo['nlev'], B=packed.B, n_lab=packed.n_lab, C=self.num_classes, P=geo['P'], img=packed.img, gts=packed.gts,
                    label=label, target=target, centerness=ctr, code_weight=[float(w) for w in cw],
                    loss_weight=[float(self.cfg_cls['loss_weight']), float(self.cfg_bbox['loss_weight']), float(self.cfg_dir['loss_weight']),
                                 float(self.cfg_centerness['loss_weight']), float(self.cfg_bbox2d['loss_weight'])],
                    gamma=float(self.cfg_cls['gamma']), alpha=float(self.cfg_cls['alpha']), beta=float(self.cfg_bbox['beta']),
                    beta2d=float(self.cfg_bbox2d['beta']), ctr_alpha=float(self.centerness_alpha), dir_offset=float(self.dir_offset))

    def pack_labels(self, labels, device):
        """pack_det_labels: do it ahead of `loss` to keep the packing's host-to-device copy out of the step"""
        return pack_det_labels(labels, device)

    # ---- the criterion -----------------------------------------------------------------------------------------------------------
    def loss(self, preds, labels):
        """preds = (cls_scores, bbox_preds, dir_cls_preds, centernesses), per-level NCHW fp32 lists; labels: the collated dict or a
        PackedDetLabels -> (loss_dict, loss_sum).  No image labelled: ({}, a zero scalar connected to the predictions)."""
        cls_scores, bbox_preds, dir_cls_preds, centernesses = preds
        L = len(cls_scores)
        if not (len(bbox_preds) == len(dir_cls_preds) == len(centernesses) == L):
            raise ValueError("the four prediction lists differ in length")
        maps = list(cls_scores) + list(bbox_preds) + list(dir_cls_preds) + list(centernesses)
        dev = maps[0].device
        for m in maps:
            if not m.is_cuda:
                raise RuntimeError("DetModel.loss runs on the HIP kernels: predictions must be on the GPU (no CPU path)")
            if m.dtype != torch.float32:
                raise RuntimeError(f"DetModel.loss takes fp32 predictions, got {m.dtype}")
            if m.dim() != 4:
                raise ValueError("DetModel.loss takes NCHW prediction maps")
        B = cls_scores[0].shape[0]
        sizes = [tuple(c.shape[-2:]) for c in cls_scores]
        for lv in range(L):
            H, W = sizes[lv]
            for m, ch, what in ((cls_scores[lv], self.num_classes, 'cls_scores'), (bbox_preds[lv], 13, 'bbox_preds'),
                                (dir_cls_preds[lv], 6, 'dir_cls_preds'), (centernesses[lv], 1, 'centernesses')):
                if tuple(m.shape) != (B, ch, H, W):
                    raise ValueError(f"{what}[{lv}] has shape {tuple(m.shape)}, expected {(B, ch, H, W)}")
        packed = labels if isinstance(labels, PackedDetLabels) else pack_det_labels(labels, dev)
        if packed.B != B:
            raise ValueError(f"labels for {packed.B} images, predictions for {B}")
        geo = self._geometry(sizes)
        out = _DetLossFn.apply(self, packed, geo, *[m.contiguous() for m in maps])
        if packed.n_lab == 0:
            return {}, out[8]
        return {k: out[i] for i, k in enumerate(LOSS_KEYS)}, out[8]

    # ---- inference: box decoding -------------------------------------------------------------------------------------------------
    def _test_cfg(self, cfg):
        """the reference's test_cfg (a dict or an attribute object) -> the five options the decode path reads"""
        cfg = self.test_cfg if cfg is None else cfg
        if cfg is None:
            raise ValueError("DetModel was built without a test_cfg (see cs_test_cfg())")
        get = (lambda k: cfg[k]) if isinstance(cfg, dict) else (lambda k: getattr(cfg, k))
        out = dict(use_rotate_nms=bool(get('use_rotate_nms')), nms_pre=int(get('nms_pre')), nms_thr=float(get('nms_thr')),
                   score_thr=float(get('score_thr')), max_per_img=int(get('max_per_img')))
        if out['max_per_img'] <= 0:
            raise NotImplementedError(f"test_cfg: max_per_img={out['max_per_img']} (the output capacity; only > 0 is implemented)")
        return out

    def _decode(self, cls_scores, bbox_preds, dir_cls_preds, centernesses, img_metas, cfg, rescale, denorm):
        if rescale:
            raise NotImplementedError("DetModel: rescale=True is not implemented (the reference raises there as well when pred_bbox2d is set)")
        cfg = self._test_cfg(cfg)
        L = len(cls_scores)
        if not (len(bbox_preds) == len(dir_cls_preds) == len(centernesses) == L):
            raise ValueError("the four prediction lists differ in length")
        maps = (list(cls_scores), list(bbox_preds), list(dir_cls_preds), list(centernesses))
        for m in (m for lst in maps for m in lst):
            if not m.is_cuda:
                raise RuntimeError("DetModel box decoding runs on the HIP kernels: predictions must be on the GPU (no CPU path)")
            if m.dtype != torch.float32:
                raise RuntimeError(f"DetModel box decoding takes fp32 predictions, got {m.dtype}")
            if m.dim() != 4:
                raise ValueError("DetModel box decoding takes NCHW prediction maps")
        dev = cls_scores[0].device
        B, C = len(img_metas), self.num_classes
        sizes = [tuple(c.shape[-2:]) for c in cls_scores]
        for lv in range(L):
            H, W = sizes[lv]
            for m, ch, what in ((cls_scores[lv], C, 'cls_scores'), (bbox_preds[lv], 13, 'bbox_preds'),
                                (dir_cls_preds[lv], 6, 'dir_cls_preds'), (centernesses[lv], 1, 'centernesses')):
                if tuple(m.shape) != (B, ch, H, W):
                    raise ValueError(f"{what}[{lv}] has shape {tuple(m.shape)}, expected {(B, ch, H, W)}")
        geo = det_decode.geometry(sizes, self.strides, cfg['nms_pre'], denorm)
        bufs = det_decode.buffers(B, C, geo, cfg['max_per_img'], dev)
        # per image: the inverse of the 4 x 4 padded camera matrix, fp32 on the host as points_img2cam (det_tools.py:639-641) takes it
        # from the loader's matrix, and img_size = (H, W)
        host = torch.zeros(B, 18, dtype=torch.float32)
        for b, meta in enumerate(img_metas):
            K = torch.as_tensor(meta['K_matrix']).detach().to(device='cpu', dtype=torch.float32)
            if K.dim() != 2 or K.shape[0] > 4 or K.shape[1] > 4:
                raise ValueError(f"K_matrix of image {b} has shape {tuple(K.shape)}")
            padded = torch.eye(4, dtype=torch.float32)
            padded[:K.shape[0], :K.shape[1]] = K
            host[b, :16] = torch.inverse(padded).reshape(16)
            host[b, 16], host[b, 17] = float(meta['img_size'][0]), float(meta['img_size'][1])
        host = host.to(dev, non_blocking=True)
        det_decode.run(tuple([m.detach().contiguous() for m in lst] for lst in maps), geo, bufs, B, C, host[:, :16].contiguous(),
                       host[:, 16:].contiguous(), dir_offset=self.dir_offset, score_thr=cfg['score_thr'], nms_thr=cfg['nms_thr'],
                       rotated=cfg['use_rotate_nms'], max_per_img=cfg['max_per_img'])
        packed = bufs['packed'].cpu()                                                    # the one host synchronisation
        M, cols = cfg['max_per_img'], det_decode.OUT_COLS
        rows = packed[:B * M * cols].view(B, M, cols)
        count = packed[B * M * cols:].view(torch.int32)
        out = []
        for b in range(B):
            r = rows[b, :int(count[b])]
            scores = r[:, 9].clone()
            out.append((r[:, :9].clone(), scores, r[:, 17].contiguous().view(torch.int32).long(), r[:, 10:13].clone(),
                        torch.cat([r[:, 13:17], scores[:, None]], dim=1)))
        return out

    def get_bboxes(self, cls_scores, bbox_preds, dir_cls_preds, centernesses, img_metas, cfg=None, rescale=None):
        """(:483-553) per-level NCHW fp32 maps with ALREADY DENORMALISED bbox_preds, one meta dict per image (K_matrix, img_size) ->
        per image (bboxes [n, 9], scores [n], labels [n] int64, centers2d [n, 3], bboxes2d [n, 5] = box + score), CPU tensors."""
        return self._decode(cls_scores, bbox_preds, dir_cls_preds, centernesses, img_metas, cfg, rescale, denorm=False)

    def get_results_from_bbox(self, preds, label, rescale=False):
        """(:957-1002) preds = the head's (cls_scores, bbox_preds, dir_cls_preds, centernesses); label['meta'] = the collated meta dict
        (img_name, K_matrix, img_size per image) -> per image dict(img_bbox=dict(boxes_3d, scores_3d, labels_3d, centers2d),
        img_bbox2d = numpy [n, 5], or the reference's list of num_classes empty (0, 5) float64 arrays when n == 0).
        `denorm_on_bbox` (:231-250) is not built as a separate method: the decode kernel multiplies the offsets and the 2-D distances
        by the level's stride as it reads them, instead of materialising denormalised copies of every bbox map."""
        bs = len(label['meta']['img_name'])
        img_metas = [{k: v[s] for k, v in label['meta'].items()} for s in range(bs)]
        cls_scores, bbox_preds, dir_cls_preds, centernesses = preds
        outs = self._decode(cls_scores, bbox_preds, dir_cls_preds, centernesses, img_metas, self.test_cfg, rescale, denorm=self.norm_on_bbox)
        results = []
        for bboxes, scores, labels, centers2d, bboxes2d in outs:
            b2 = [np.zeros((0, 5), dtype=np.float64) for _ in range(self.num_classes)] if bboxes2d.shape[0] == 0 else bboxes2d.numpy()
            results.append(dict(img_bbox=dict(boxes_3d=bboxes, scores_3d=scores, labels_3d=labels, centers2d=centers2d), img_bbox2d=b2))
        return results

    # ---- inspection --------------------------------------------------------------------------------------------------------------
    def get_points(self, featmap_sizes, dtype, device, flatten=False):
        """points of every level (:717-754): [H*W, 2] = (x * stride, y * stride) + stride // 2"""
        out = []
        for (h, w), stride in zip(featmap_sizes, self.strides):
            y, x = torch.meshgrid(torch.arange(h, dtype=dtype, device=device), torch.arange(w, dtype=dtype, device=device), indexing='ij')
            out.append(torch.stack((x.reshape(-1) * stride, y.reshape(-1) * stride), dim=-1) + stride // 2)
        return out

    def get_targets(self, points, gt_bboxes_list, gt_labels_list, gt_bboxes_3d_list, gt_labels_3d_list, centers2d_list, depths_list):
        """(:756-856) -> (labels_3d, bbox_targets_3d, centerness_targets), each a list over levels of the images concatenated: [n*P_l],
        [n*P_l, 13], [n*P_l].  For inspection and tests (reads the level widths off `points`: a host synchronisation)."""
        if len(points) != len(self.regress_ranges):
            raise ValueError("one point set per regress range")
        dev = points[0].device
        sizes = []
        for pts in points:
            w = int((pts[:, 1] == pts[0, 1]).sum())
            sizes.append((pts.shape[0] // w, w))
        n = len(gt_bboxes_list)
        recs = []
        for i in range(n):
            g3 = gt_bboxes_3d_list[i]
            k = g3.shape[0]
            ci = torch.cat([centers2d_list[i].reshape(k, 2).float(), depths_list[i].reshape(k, 1).float()], 1)
            recs.append(_records(gt_bboxes_list[i], gt_labels_3d_list[i], ci.to(g3.device), g3[:, 3:6], g3[:, 6:9]))
        packed = _pack(n, list(range(n)), recs, dev)
        geo = self._geometry(sizes)
        P = geo['P']
        label = torch.empty(n, P, dtype=torch.int32, device=dev)
        target = torch.empty(n, 13, P, dtype=torch.float32, device=dev)
        ctr = torch.empty(n, P, dtype=torch.float32, device=dev)
        ops.call("fcos3d_targets", **self._desc(geo, packed, label, target, ctr))
        lab, tgt, cen, o = [], [], [], 0
        for h, w in sizes:
            s = slice(o, o + h * w)
            lab.append(label[:, s].reshape(-1).long())
            tgt.append(target[:, :, s].permute(0, 2, 1).reshape(-1, 13))
            cen.append(ctr[:, s].reshape(-1))
            o += h * w
        return lab, tgt, cen


# ---- configuration ---------------------------------------------------------------------------------------------------------------
def cs_test_cfg():
    """test_cfg of TaskPrompter/configs/cityscapes3d/det_head_params.py:4-12 (nms_across_levels and min_bbox_size are carried as the
    reference carries them: its decode path never reads them)"""
    return dict(use_rotate_nms=True, nms_across_levels=False, nms_pre=1000, nms_thr=0.3, score_thr=0.05, min_bbox_size=0, max_per_img=200)


def cs_det_model_params():
    """det_model_params of TaskPrompter/configs/cityscapes3d/det_head_params.py (the Cityscapes-3D config), strides not yet scaled"""
    return dict(
        num_classes=6, regress_ranges=((-1, 96), (96, 192), (192, 384), (384, 768), (768, INF)), center_sampling=True,
        center_sample_radius=1.5, norm_on_bbox=True, centerness_alpha=2.5,
        loss_cls=dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=5.0),
        loss_dir=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0),
        loss_bbox=dict(type='SmoothL1Loss', beta=1.0 / 9.0, loss_weight=1.0),
        loss_centerness=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0),
        loss_bbox2d=dict(type='SmoothL1Loss', beta=1.0 / 9.0, loss_weight=1.0),
        loss_consistency=dict(type='GIoULoss', loss_weight=1.0), stacked_convs=3, strides=[8, 16, 32, 32, 64],
        use_direction_classifier=True, background_label=None, diff_rad_by_sin=True, dir_offset=0, bbox_code_size=9, pred_bbox2d=True,
        pred_keypoints=False, group_reg_dims=(2, 1, 3, 3, 4),
        code_weight=[1.0, 1.0, 0.2, 1.0, 1.0, 1.0, 5.0, 5.0, 5.0, 1.0, 1.0, 1.0, 1.0], test_cfg=cs_test_cfg())


def configure_3ddet(p, det_model_params=None):
    """TaskPrompter/utils/config.py:149-163: strides * (IMAGE_ORI_SIZE[0] // TRAIN.SCALE[0]) / img_ds_ratio, then p.det_model_params and
    p.detmodel = DetModel(**det_model_params).  `p` is attribute- or item-addressable; returns it."""
    def get(obj, k):
        return obj[k] if isinstance(obj, dict) else getattr(obj, k)
    params = copy.deepcopy(det_model_params if det_model_params is not None else cs_det_model_params())
    ds_ratio = get(p, 'IMAGE_ORI_SIZE')[0] // get(get(p, 'TRAIN'), 'SCALE')[0]
    strides = [s * ds_ratio for s in params['strides']]
    params['strides'] = [s / get(p, 'img_ds_ratio') for s in strides]
    model = DetModel(**params)
    if isinstance(p, dict):
        p['det_model_params'], p['detmodel'] = params, model
    else:
        p.det_model_params, p.detmodel = params, model
    return p


def synthetic_det_labels(B, img_size, n_gts, num_classes=6, unlabelled=(), device='cpu', seed=0):
    """The collated label structure of the Cityscapes-3D loader (det_model.py:262-289) with random boxes inside img_size = (H, W):
    n_gts boxes per image (an int or one count per image; 0 gives an image with no gts that still counts as labelled), the images in
    `unlabelled` with det_label_number 0."""
    g = torch.Generator().manual_seed(seed)
    H, W = img_size
    counts = [n_gts] * B if isinstance(n_gts, int) else list(n_gts)
    dl = []
    for i in range(B):
        n = counts[i]
        wh = torch.rand(n, 2, generator=g) * torch.tensor([W * 0.4, H * 0.4]) + torch.tensor([W * 0.01, H * 0.01])
        c = torch.rand(n, 2, generator=g) * torch.tensor([W, H])
        x1y1 = c - wh * (0.3 + 0.4 * torch.rand(n, 2, generator=g))
        box = torch.cat([x1y1, x1y1 + wh], 1)
        dl.append(dict(bbox_modal=box, label=torch.randint(0, num_classes, (n,), generator=g),
                       center_S=torch.randn(n, 3, generator=g) * 10.0, size_S=torch.rand(n, 3, generator=g) * 4.0 + 0.5,
                       rotation_S=(torch.rand(n, 3, generator=g) * 2 - 1) * 3.14159,
                       center_I=torch.cat([c, torch.rand(n, 1, generator=g) * 60.0 + 2.0], 1)))
        dl[-1] = {k: v.to(device) for k, v in dl[-1].items()}
    nums = torch.tensor([0 if i in unlabelled else max(counts[i], 1) for i in range(B)])
    meta = dict(img_name=[f"synthetic_{i}" for i in range(B)])
    return dict(det_labels=dl, det_label_number=nums, meta=meta)
