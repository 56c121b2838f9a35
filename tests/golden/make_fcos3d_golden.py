"""Golden fixture of the FCOS3D criterion (DetModel.loss), generated from the UNMODIFIED reference files
TaskPrompter/detection_toolbox/det_model.py and det_losses.py on the CPU:

    python tests/golden/make_fcos3d_golden.py    ->  tests/golden/fcos3d.json, tests/golden/fcos3d.npz

det_model.py imports mmdet3d, and its det_tools imports cv2, pyquaternion, mmdet3d, cityscapesscripts, data.cityscapes3d and the iou3d
extension; det_losses.py imports mmcv and its compiled ops, det_head_params.py easydict.  None is installed: import-only stand-ins are
put in sys.modules, mmcv being tests/det_refshim's (no arithmetic; `limit_period` is det_tools' own plain-torch function, the focal loss takes the reference's host path
py_sigmoid_focal_loss).  The cs parameters are the reference's det_head_params.det_model_params with the strides scaled as config.py:157-160
does for img_ds_ratio 0.75.  Cases:
  a  B = 3 with the middle image unlabelled; ties (two gts with one centre, a mirrored pair), a point exactly on a centre-sampling
     boundary and one exactly on a regress-range boundary, a gt centred off the image that no point takes;
  b  two labelled images whose gts no point takes (num_pos == 0);
  c  no labelled image;
  d  the mini_det head (make_det_golden.py) feeding DetModel.loss, per-parameter head gradients in the mini_det manner.
Stored per case: inputs, per-point labels (reference layout: levels, then images), targets and centerness on the positives, the loss
dict, loss_sum, d loss_sum / d every pred map and (a) d loss_rotsin / d every pred map."""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
REF = os.environ.get("MTT_REFERENCE_ROOT", "/root/reference")
IMG_DS_RATIO = 0.75
LEVELS_A = ((10, 20), (5, 10), (3, 5), (3, 5), (2, 3))
LEVELS_B = ((6, 12), (3, 6), (2, 3), (2, 3), (1, 2))
NCH = (6, 13, 6, 1)                                            # cls, bbox, dir, centerness channels
KEYS = ('loss_cls', 'loss_offset', 'loss_depth', 'loss_size', 'loss_rotsin', 'loss_dir', 'loss_centerness', 'loss_bbox2d')


def _stub(name, **attrs):
    mod = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(mod, k, v)
    sys.modules[name] = mod
    return mod


class _EasyDict(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k) from None

    def __setattr__(self, k, v):
        self[k] = v


def install_stubs():
    ident = lambda *a, **kw: (lambda fn: fn)
    shim = os.path.join(TESTS, "det_refshim")           # the mmcv stand-in of make_det_golden.py (case d builds the head through it)
    if shim not in sys.path:
        sys.path.insert(0, shim)
    import mmcv
    if not hasattr(mmcv, "jit"):
        mmcv.jit = ident                                # the decorator of giou_loss (det_losses.py:671), an identity outside parrots
    _stub("mmcv._ext", **{f: None for f in ("sigmoid_focal_loss_forward", "sigmoid_focal_loss_backward", "softmax_focal_loss_forward",
                                             "softmax_focal_loss_backward")})
    _stub("mmdet")
    _stub("mmdet.core", bbox_overlaps=None)
    _stub("mmdet3d")
    _stub("mmdet3d.core")
    _stub("mmdet3d.core.utils", array_converter=ident)
    _stub("mmdet3d.core.bbox", CameraInstance3DBoxes=object)
    _stub("cv2", FONT_HERSHEY_SIMPLEX=0, LINE_AA=16)            # constants read at import time (det_tools.py:356)
    _stub("pyquaternion", Quaternion=object)
    _stub("cityscapesscripts")
    _stub("cityscapesscripts.helpers")
    _stub("cityscapesscripts.helpers.annotation", CsBbox3d=object)
    _stub("data")
    _stub("data.cityscapes3d", evalLabels=None)
    _stub("detection_toolbox.iou3d.iou3d_cuda")
    _stub("easydict", EasyDict=_EasyDict)
    p = os.path.join(REF, "TaskPrompter")
    if p not in sys.path:
        sys.path.insert(0, p)


def reference():
    install_stubs()
    from detection_toolbox import det_model
    from configs.cityscapes3d import det_head_params as dhp
    return det_model, dhp


def cs_params(dhp):
    """det_model_params with config.py:157-160's strides (IMAGE_ORI_SIZE[0] // TRAIN.SCALE[0] = 1, img_ds_ratio 0.75)"""
    import copy
    p = copy.deepcopy(dict(dhp.det_model_params))
    p['strides'] = [s * 1 / IMG_DS_RATIO for s in p['strides']]
    return p


def plain(p):
    return json.loads(json.dumps({k: (v if not isinstance(v, tuple) else list(v)) for k, v in p.items() if k != 'test_cfg'}))


def _f32(v):
    return float(np.float32(v))


def _gt(box, label, ci, g):
    n = len(label)
    return dict(bbox_modal=torch.tensor(box, dtype=torch.float32), label=torch.tensor(label, dtype=torch.int64),
                center_S=torch.randn(n, 3, generator=g) * 10, size_S=torch.rand(n, 3, generator=g) * 4 + 0.5,
                rotation_S=(torch.rand(n, 3, generator=g) * 2 - 1) * 3.1, center_I=torch.tensor(ci, dtype=torch.float32))


def _random_gts(n, H, W, g, off_image=False, num_classes=6):
    wh = torch.rand(n, 2, generator=g) * torch.tensor([W * 0.5, H * 0.5]) + 6.0
    c = torch.rand(n, 2, generator=g) * torch.tensor([W, H])
    if off_image:
        c = c - torch.tensor([W * 4.0, 0.0])
    x1y1 = c - wh * (0.3 + 0.4 * torch.rand(n, 2, generator=g))
    box = torch.cat([x1y1, x1y1 + wh], 1)
    ci = torch.cat([c, torch.rand(n, 1, generator=g) * 50 + 2], 1)
    return _gt(box.tolist(), torch.randint(0, num_classes, (n,), generator=g).tolist(), ci.tolist(), g)


def case_a_labels(strides, g, radius=1.5, range_end=96.0, num_classes=6):
    """the hand-made gts of case a; radius = center_sample_radius, range_end = the upper end of level 0's regress range, the labels
    folded into num_classes"""
    s0 = np.float32(strides[0])
    half = np.float32(strides[0] // 2)
    xs = lambda i: np.float32(np.float32(i) * s0) + half                # level-0 point coordinates, as get_points computes them
    rad = np.float32(strides[0] * radius)
    box, lab, ci = [], [], []
    # two gts with one centre: every point ties, the first wins (the second is taken by no point)
    box += [[30.0, 20.0, 100.0, 80.0], [34.0, 22.0, 96.0, 78.0]]; lab += [2, 4]; ci += [[64.0, 48.0, 20.0], [64.0, 48.0, 30.0]]
    # a mirrored pair around the point (12, 6): equal distances there
    for i in range(12, 20):
        a, b = np.float32(xs(i) - np.float32(7.0)), np.float32(xs(i) + np.float32(7.0))
        if np.float32(xs(i) - a) == -np.float32(xs(i) - b):
            break
    y6 = xs(6)
    box += [[float(a) - 20, float(y6) - 15, float(a) + 20, float(y6) + 15], [float(b) - 20, float(y6) - 15, float(b) + 20, float(y6) + 15]]
    lab += [1, 3]; ci += [[float(a), float(y6), 11.0], [float(b), float(y6), 12.0]]
    # the point (4, 1) exactly on the left edge of a centre-sampling box: cx - radius == xs
    # (the first point of 4, 5, 3, 6, ... and the first centre, upwards then downwards from xs + radius, for which the fp32 difference is
    # exact: not every radius has one at point 4; the cs set does, at or above xs + radius)
    for bx in (4, 5, 3, 6, 2, 7):
        for step in (np.float32(np.inf), np.float32(-np.inf)):
            cx = np.float32(xs(bx) + rad)
            for _ in range(16):
                if np.float32(cx - rad) == xs(bx):
                    break
                cx = np.nextafter(cx, step, dtype=np.float32)
            if np.float32(cx - rad) == xs(bx):
                break
        if np.float32(cx - rad) == xs(bx):
            break
    assert np.float32(cx - rad) == xs(bx)
    y1 = xs(1)
    box += [[float(cx) - 25, float(y1) - 12, float(cx) + 25, float(y1) + 12]]; lab += [0]; ci += [[float(cx), float(y1) + 3.0, 7.0]]
    # the point (8, 8) exactly on the upper end of level 0's regress range: max(l, t, r, b) == range_end (96 in the cs set)
    x8 = xs(8)
    x1 = np.float32(x8 - np.float32(range_end))
    assert np.float32(x8 - x1) == np.float32(range_end)
    box += [[float(x1), float(xs(8)) - 30, float(x8) + 40, float(xs(8)) + 30]]; lab += [5]; ci += [[float(x8) + 2.0, float(xs(8)) - 2.0, 9.0]]
    # centred off the image: no point takes it
    box += [[-400.0, 10.0, -200.0, 60.0]]; lab += [1]; ci += [[-300.0, 35.0, 30.0]]
    return _gt(box, [l % num_classes for l in lab], ci, g), dict(mirror_x=i, boundary_cx=float(cx), range_x1=float(x1),
                                                                  **({} if bx == 4 else dict(boundary_x=bx)))


def make_labels(case, strides, g, params=None):
    """params: the parameter set the hand-made boundaries and the label range of cases a / b come from (None: the cs values)"""
    H, W = 110.0, 215.0
    info = {}
    geo = {} if params is None else dict(radius=params['center_sample_radius'], range_end=float(params['regress_ranges'][0][1]),
                                         num_classes=params['num_classes'])
    nc = geo.get('num_classes', 6)
    if case == 'a':
        e0, info = case_a_labels(strides, g, **geo)
        dl = [e0, _random_gts(3, H, W, g, num_classes=nc), _random_gts(5, H, W, g, num_classes=nc)]
        num = [len(dl[0]['label']), 0, 5]
    elif case == 'b':
        dl = [_random_gts(3, 64, 128, g, off_image=True, num_classes=nc), _random_gts(2, 64, 128, g, off_image=True, num_classes=nc)]
        num = [3, 2]
    elif case == 'c':
        dl = [_random_gts(2, 64, 128, g), _random_gts(1, 64, 128, g)]
        num = [0, 0]
    else:
        dl = [_random_gts(6, 128, 213, g), _random_gts(4, 128, 213, g)]
        num = [6, 4]
    B = len(dl)
    labels = dict(det_labels=dl, det_label_number=torch.tensor(num), meta=dict(img_name=[f"img{i}" for i in range(B)]))
    return labels, info


def random_preds(B, levels, g, nch=NCH):
    return [[torch.randn(B, c, h, w, generator=g) * (2.0 if k == 0 else 1.0) for (h, w) in levels] for k, c in enumerate(nch)]


def reference_targets(crit, labels, featmap_sizes):
    """the lists DetModel.loss builds (:262-289) -> get_points / get_targets of the reference"""
    dl, num = labels['det_labels'], labels['det_label_number']
    keep = [i for i in range(len(dl)) if num[i] != 0]
    if not keep:
        return None
    gb = [dl[i]['bbox_modal'] for i in keep]
    gl = [dl[i]['label'] for i in keep]
    g3 = [torch.cat([dl[i]['center_S'], dl[i]['size_S'], dl[i]['rotation_S']], 1) for i in keep]
    c2 = [dl[i]['center_I'][:, :2] for i in keep]
    dp = [dl[i]['center_I'][:, 2] for i in keep]
    pts = crit.get_points(featmap_sizes, torch.float32, 'cpu')
    lab, tgt, ctr = crit.get_targets(pts, gb, gl, g3, gl, c2, dp)
    return torch.cat(lab), torch.cat(tgt), torch.cat(ctr)


def run_case(det_model, params, labels, preds, single=None):
    """DetModel.loss on (copies of) the preds -> (loss dict, loss_sum, d loss_sum / d maps, d single / d maps)"""
    leaves = [[p.clone().requires_grad_(True) for p in lst] for lst in preds]
    crit = det_model.DetModel(**json.loads(json.dumps(params)))
    ld, ls = crit.loss(tuple(list(lst) for lst in leaves), labels)
    flat = [p for lst in leaves for p in lst]
    gsum = torch.autograd.grad(ls, flat, retain_graph=single is not None, allow_unused=True)
    gsum = [torch.zeros_like(p) if g is None else g for p, g in zip(flat, gsum)]
    gone = None
    if single is not None:
        gone = torch.autograd.grad(ld[single], flat, allow_unused=True)
        gone = [torch.zeros_like(p) if g is None else g for p, g in zip(flat, gone)]
    return crit, ld, ls, gsum, gone


def store_labels(out, name, labels):
    out[f"{name}/num"] = labels['det_label_number'].numpy()
    for i, e in enumerate(labels['det_labels']):
        for k, v in e.items():
            out[f"{name}/gt{i}/{k}"] = v.numpy()


def load_labels(arrs, name, B):
    """the collated label dict of a stored case (tests read it back with this)"""
    dl = []
    for i in range(B):
        dl.append({k: torch.from_numpy(np.asarray(arrs[f"{name}/gt{i}/{k}"])) for k in
                   ('bbox_modal', 'label', 'center_S', 'size_S', 'rotation_S', 'center_I')})
    return dict(det_labels=dl, det_label_number=torch.from_numpy(np.asarray(arrs[f"{name}/num"])),
                meta=dict(img_name=[f"img{i}" for i in range(B)]))


def generate():
    torch.set_num_threads(1)
    det_model, dhp = reference()
    params = plain(cs_params(dhp))
    meta = dict(params=params, img_ds_ratio=IMG_DS_RATIO, keys=list(KEYS), cases={})
    out = {}
    for name, levels in (('a', LEVELS_A), ('b', LEVELS_B), ('c', LEVELS_B)):
        g = torch.Generator().manual_seed(ord(name))
        labels, info = make_labels(name, params['strides'], g)
        B = len(labels['det_labels'])
        preds = random_preds(B, levels, g)
        crit, ld, ls, gsum, gone = run_case(det_model, params, labels, preds, single='loss_rotsin' if name == 'a' else None)
        tg = reference_targets(crit, labels, levels)
        store_labels(out, name, labels)
        for j, p in enumerate(p for lst in preds for p in lst):
            out[f"{name}/pred{j}"] = p.numpy()
            out[f"{name}/grad{j}"] = gsum[j].numpy()
            if gone is not None:
                out[f"{name}/grad_rotsin{j}"] = gone[j].numpy()
        m = dict(B=B, levels=[list(l) for l in levels], loss={k: float(v) for k, v in ld.items()}, loss_keys=list(ld.keys()),
                 loss_sum=float(ls), info=info)
        if tg is not None:
            lab, tgt, ctr = tg
            pos = (lab >= 0) & (lab < 6)
            out[f"{name}/labels"] = lab.numpy().astype(np.int8)
            out[f"{name}/pos_targets"] = tgt[pos].numpy()
            out[f"{name}/pos_ctr"] = ctr[pos].numpy()
            m['num_pos'] = int(pos.sum())
        meta['cases'][name] = m
    # d: the mini_det head of make_det_golden.py feeding the reference criterion
    sys.path.insert(0, HERE)
    import make_det_golden as mdg
    head = mdg.reference_head()
    head.eval()
    feats = mdg.inputs()
    g = torch.Generator().manual_seed(ord('d'))
    labels, _ = make_labels('d', params['strides'], g)
    outs = head(feats)
    for lst in outs:
        for t in lst:
            t.retain_grad()
    crit = det_model.DetModel(**json.loads(json.dumps(params)))
    ld, ls = crit.loss(tuple(list(lst) for lst in outs), labels)
    ls.backward()
    flat = [t for lst in outs for t in lst]
    store_labels(out, 'd', labels)
    for j, t in enumerate(flat):
        out[f"d/grad{j}"] = t.grad.numpy()
    levels = [list(t.shape[-2:]) for t in outs[0]]
    tg = reference_targets(crit, labels, levels)
    lab = tg[0]
    out["d/labels"] = lab.numpy().astype(np.int8)
    meta['cases']['d'] = dict(B=2, levels=levels, loss={k: float(v) for k, v in ld.items()}, loss_keys=list(ld.keys()), loss_sum=float(ls),
                              num_pos=int(((lab >= 0) & (lab < 6)).sum()),
                              grad_stats=mdg.grad_stats((k, p.grad) for k, p in head.named_parameters()))
    return meta, out


# The alt parameter set: nothing coincides (the cs set has gamma 2, beta == beta2d, loss weights (5, 1, 1, 1, 1), dir_offset 0), so an
# index, a beta or a sign mixed up in the kernels or in DetModel._desc changes an asserted number.  gamma >= 1: below 1 the reference's
# own gradient is NaN at saturated logits.  Both betas are large enough that N(0, 1) predictions fill the quadratic smooth-L1 branch.
ALT = dict(num_classes=3, center_sample_radius=2.0, centerness_alpha=1.7, dir_offset=0.7854,
           loss_cls=dict(type='FocalLoss', use_sigmoid=True, gamma=1.5, alpha=0.4, loss_weight=3.0),
           loss_bbox=dict(type='SmoothL1Loss', beta=0.5, loss_weight=1.3),
           loss_dir=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=0.7),
           loss_centerness=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.9),
           loss_bbox2d=dict(type='SmoothL1Loss', beta=2.0, loss_weight=0.45),
           code_weight=[1.0, 0.9, 0.2, 1.1, 1.2, 0.8, 5.0, 4.0, 3.0, 0.7, 0.6, 1.4, 1.5])
ALT_GOUT = (0.7, -1.3, 2.1, 0.4, -0.9, 1.6, -2.4, 3.2, 0.55)         # upstream gradient of (the eight components, loss_sum)


def alt_params(dhp):
    p = plain(cs_params(dhp))
    p.update(json.loads(json.dumps(ALT)))
    return p


def generate_alt():
    """fcos3d_alt.*: cases a (the geometry of fcos3d.* a: ties, boundary points, the middle image unlabelled) and b (num_pos == 0) under
    the alt parameter set; one gradient set per case, d (sum_i w_i * component_i + w_8 * loss_sum) / d every pred map, w = ALT_GOUT"""
    torch.set_num_threads(1)
    det_model, dhp = reference()
    params = alt_params(dhp)
    C = params['num_classes']
    meta = dict(params=params, img_ds_ratio=IMG_DS_RATIO, keys=list(KEYS), gout=list(ALT_GOUT), cases={})
    out = {}
    for name, levels in (('a', LEVELS_A), ('b', LEVELS_B)):
        g = torch.Generator().manual_seed(1000 + ord(name))
        labels, info = make_labels(name, params['strides'], g, params)
        B = len(labels['det_labels'])
        preds = random_preds(B, levels, g, (C, 13, 6, 1))
        leaves = [[p.clone().requires_grad_(True) for p in lst] for lst in preds]
        crit = det_model.DetModel(**json.loads(json.dumps(params)))
        ld, ls = crit.loss(tuple(list(lst) for lst in leaves), labels)
        assert sorted(ld) == sorted(KEYS)                               # (the num_pos == 0 branch orders them differently)
        total = sum(w * ld[k] for w, k in zip(ALT_GOUT, KEYS)) + ALT_GOUT[8] * ls
        flat = [p for lst in leaves for p in lst]
        grads = torch.autograd.grad(total, flat, allow_unused=True)
        lab, tgt, ctr = reference_targets(crit, labels, levels)
        pos = (lab >= 0) & (lab < C)
        store_labels(out, name, labels)
        for j, (p, gr) in enumerate(zip(flat, grads)):
            out[f"{name}/pred{j}"] = p.detach().numpy()
            out[f"{name}/grad{j}"] = (torch.zeros_like(p) if gr is None else gr).numpy()
        out[f"{name}/labels"] = lab.numpy().astype(np.int8)
        out[f"{name}/pos_targets"] = tgt[pos].numpy()
        out[f"{name}/pos_ctr"] = ctr[pos].numpy()
        meta['cases'][name] = dict(B=B, levels=[list(l) for l in levels], loss={k: float(v) for k, v in ld.items()}, loss_keys=list(ld.keys()),
                                   loss_sum=float(ls), info=info, num_pos=int(pos.sum()))
    return meta, out


def main(out_dir=HERE, which=("cs", "alt")):
    for tag, gen, stem in (("cs", generate, "fcos3d"), ("alt", generate_alt, "fcos3d_alt")):
        if tag not in which:
            continue
        meta, arrays = gen()
        with open(os.path.join(out_dir, stem + ".json"), "w") as f:
            json.dump(meta, f, indent=0, sort_keys=True)
        np.savez_compressed(os.path.join(out_dir, stem + ".npz"), **arrays)


if __name__ == "__main__":
    # an output directory other than tests/golden: a regeneration check; a third argument (cs / alt) writes that fixture alone
    main(sys.argv[1] if len(sys.argv) > 1 else HERE, tuple(sys.argv[2:3]) or ("cs", "alt"))
