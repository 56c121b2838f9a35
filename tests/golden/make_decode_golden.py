"""Golden fixture of the FCOS3D box decoding (DetModel.get_results_from_bbox), generated on the CPU from the UNMODIFIED reference files
TaskPrompter/detection_toolbox/det_model.py and det_tools.py:

    python tests/golden/make_decode_golden.py    ->  tests/golden/decode.json, tests/golden/decode.npz

The import stand-ins are make_fcos3d_golden.py's.  ONE substitution: the names `nms_gpu` / `nms_normal_gpu` that det_tools imported from
its CUDA extension (det_tools.py:84; the extension cannot load here) are replaced by a descending sort plus `ref_nms` of
oracle/_ref/libiou3d_ref.so, the reference's own iou3d device functions compiled for the host (oracle/build_ref_iou3d.sh).  Everything
else (denorm_on_bbox, get_bboxes, _get_bboxes_single, box3d_multiclass_nms, bbox2result, bbox3d2result) runs as the reference wrote it.

Cases (strides [8, 16, 32, 32, 64] / 0.75, a non-centred K, score_thr 0.05, nms_thr 0.3):
  s  levels (10,20) (5,10) (3,5) (3,5) (2,3), B = 2, nms_pre 24 (two levels select, three pass whole), max_per_img 20 (the cut is taken);
  t  the same levels, nms_pre 1000, max_per_img 200: nothing selects, nothing is cut; class 3 below the threshold everywhere; image 1 has
     no score above it (the empty result, with the list of float64 arrays as img_bbox2d);
  w  levels (24,48) (12,24) (6,12) (6,12) (3,6), B = 1, nms_pre 1000 (level 0 selects), class logits 2 randn - 5: more than 64 candidates
     per class, so a segment spans several 64-box blocks and mask words;
  n  case s with use_rotate_nms=False.
Each case steps its seed until the inputs keep every selection decision away from its boundary by the margins of MARGINS (so that a
device's last-place differences in exp / division cannot flip one); the seed used and the measured margins are recorded in decode.json."""
import ctypes
import copy
import json
import os
import subprocess
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for p in (ROOT, TESTS, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import make_fcos3d_golden as mfg                 # noqa: E402
import det_decode_ref as ddr                     # noqa: E402

LEVELS_S = ((10, 20), (5, 10), (3, 5), (3, 5), (2, 3))
LEVELS_W = ((24, 48), (12, 24), (6, 12), (6, 12), (3, 6))
BASE_CFG = dict(use_rotate_nms=True, nms_across_levels=False, nms_pre=1000, nms_thr=0.3, score_thr=0.05, min_bbox_size=0, max_per_img=200)
CASES = dict(
    s=dict(levels=LEVELS_S, B=2, cfg=dict(nms_pre=24, max_per_img=20), img=(105, 210), K=(140.0, 150.0, 96.5, 47.25)),
    t=dict(levels=LEVELS_S, B=2, cfg=dict(), img=(105, 210), K=(140.0, 150.0, 96.5, 47.25)),
    w=dict(levels=LEVELS_W, B=1, cfg=dict(), img=(250, 500), K=(330.0, 340.0, 231.5, 118.25)),
    n=dict(levels=LEVELS_S, B=2, cfg=dict(nms_pre=24, max_per_img=20, use_rotate_nms=False), img=(105, 210), K=(140.0, 150.0, 96.5, 47.25)),
)
# quantity -> required margin
MARGINS = dict(preselect_rel=1e-4, threshold_abs=2e-6, score_rel=1e-5, iou_abs=1e-4, period_abs=1e-5, dir_abs=1e-4)
OUT_KEYS = ("boxes_3d", "scores_3d", "labels_3d", "centers2d")


def ref_lib():
    so = subprocess.check_output(["bash", os.path.join(ROOT, "oracle", "build_ref_iou3d.sh")]).decode().strip().splitlines()[-1]
    lib = ctypes.CDLL(so)
    lib.ref_nms.restype = ctypes.c_int
    return lib


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def substitute_nms(det_tools, lib):
    """the one substitution: det_tools.nms_gpu / nms_normal_gpu -> sort + ref_nms (signatures of iou3d_utils.py:26, :54)"""
    def make(rotated):
        def fn(boxes, scores, thresh, pre_maxsize=None, post_max_size=None):
            order = scores.sort(0, descending=True)[1]
            if pre_maxsize is not None:
                order = order[:pre_maxsize]
            bx = np.ascontiguousarray(boxes[order].detach().cpu().numpy().astype(np.float32))
            keep = np.zeros(len(bx), np.int64)
            k = lib.ref_nms(len(bx), _ptr(bx), ctypes.c_float(thresh), rotated, _ptr(keep))
            keep = order[torch.from_numpy(keep[:k])].contiguous()
            return keep if post_max_size is None else keep[:post_max_size]
        return fn
    det_tools.nms_gpu, det_tools.nms_normal_gpu = make(1), make(0)


def make_inputs(name, seed):
    """the head's normalised maps (cls, bbox, dir, centerness lists of [B, c, H, W]) and the label with the reference's meta layout"""
    c = CASES[name]
    g = torch.Generator().manual_seed(seed)
    B = c['B']
    cls, bbox, dirs, ctr = [], [], [], []
    for (h, w) in c['levels']:
        z = torch.randn(B, 6, h, w, generator=g) * 2.0
        if name == 'w':
            z = z - 5.0
        if name == 't':
            z = z - 6.0
            z[:, 3] -= 20.0                                                     # class 3 never passes the threshold
            z[1] = torch.randn(6, h, w, generator=g) - 12.0                     # image 1: nothing passes
        cls.append(z)
        bb = torch.empty(B, 13, h, w)
        bb[:, 0:2] = torch.randn(B, 2, h, w, generator=g)                       # offsets, in strides
        bb[:, 2:3] = torch.rand(B, 1, h, w, generator=g) * 40.0 + 4.0           # depth
        bb[:, 3:6] = torch.rand(B, 3, h, w, generator=g) * 3.0 + 1.0            # size
        bb[:, 6:9] = torch.randn(B, 3, h, w, generator=g) * 2.5                 # angles, well beyond one period
        bb[:, 9:13] = torch.randn(B, 4, h, w, generator=g) * 2.0 + 1.0          # 2-D distances, in strides: some boxes leave the image
        bbox.append(bb)
        dirs.append(torch.randn(B, 6, h, w, generator=g))
        ctr.append(torch.randn(B, 1, h, w, generator=g) + 1.0)
    fx, fy, u0, v0 = c['K']
    Ks = torch.tensor([[[fx + i, 0.0, u0 + 2.0 * i], [0.0, fy + i, v0 - i], [0.0, 0.0, 1.0]] for i in range(B)], dtype=torch.float32)
    label = dict(meta=dict(img_name=[f"img{i}" for i in range(B)], K_matrix=Ks, img_size=[tuple(c['img'])] * B,
                           scale_factor=[np.array([1.0, 1.0])] * B))
    return (cls, bbox, dirs, ctr), label


def case_cfg(name):
    cfg = dict(BASE_CFG)
    cfg.update(CASES[name]['cfg'])
    return cfg


def measure(name, preds, label, strides, lib):
    """the decision margins of one case's inputs, from the fp32 restatement's intermediate quantities (the smallest over the images)"""
    cfg = case_cfg(name)
    m = dict(preselect_rel=np.inf, threshold_abs=np.inf, score_rel=np.inf, iou_abs=np.inf, period_abs=np.inf, dir_abs=np.inf)
    counts = []
    for b in range(CASES[name]['B']):
        tr = {}
        pick = lambda lst: [t[b] for t in lst]
        ddr.decode_single(pick(preds[0]), pick(preds[1]), pick(preds[2]), pick(preds[3]), strides, label['meta']['K_matrix'][b],
                          label['meta']['img_size'][b], cfg, lambda bx, s, t, r: s.sort(descending=True)[1][:0], trace=tr)    # no NMS needed
        for key in tr['keys']:
            if cfg['nms_pre'] > 0 and key.numel() > cfg['nms_pre']:
                srt = key.double().sort(descending=True)[0]
                k = cfg['nms_pre']
                m['preselect_rel'] = min(m['preselect_rel'], float((srt[k - 1] - srt[k]) / srt[k - 1]))
        sc = tr['scores'].double()
        m['threshold_abs'] = min(m['threshold_abs'], float((sc - float(np.float32(cfg['score_thr']))).abs().min()))
        m['period_abs'] = min(m['period_abs'], float(ddr.pi_distance(tr['raw_rot']).min()))
        dl = tr['dir_logits'].double()
        m['dir_abs'] = min(m['dir_abs'], float((dl[..., 0] - dl[..., 1]).abs().min()))
        per_class = []
        for c in range(sc.shape[1]):
            on = tr['scores'][:, c] > cfg['score_thr']
            n = int(on.sum())
            per_class.append(n)
            if n > 1:
                srt = sc[on, c].sort(descending=True)[0]
                m['score_rel'] = min(m['score_rel'], float(((srt[:-1] - srt[1:]) / srt[:-1]).min()))
                bx = np.ascontiguousarray(tr['nms_boxes'][on].numpy().astype(np.float32))
                iou = np.zeros((n, n), np.float32)
                if cfg['use_rotate_nms']:
                    lib.ref_boxes_iou_bev(n, _ptr(bx), n, _ptr(bx), _ptr(iou))
                else:
                    from oracle import iou3d_oracle
                    iou = np.array([[iou3d_oracle.iou_normal(p, q) for q in bx] for p in bx], np.float32)
                off = np.abs(iou.astype(np.float64) - float(np.float32(cfg['nms_thr'])))[~np.eye(n, dtype=bool)]
                m['iou_abs'] = min(m['iou_abs'], float(off.min()))
        counts.append(per_class)
    return m, counts


def meets(m):
    return all(m[k] >= MARGINS[k] for k in MARGINS)


def run_reference(det_model, params, name, preds, label):
    crit = det_model.DetModel(**copy.deepcopy(params), test_cfg=mfg._EasyDict(case_cfg(name)))
    with torch.no_grad():
        return crit.get_results_from_bbox(tuple([t.clone() for t in lst] for lst in preds), label, rescale=False)


def store_inputs(out, name, preds, label):
    for j, t in enumerate(t for lst in preds for t in lst):
        out[f"{name}/pred{j}"] = t.numpy()
    out[f"{name}/K"] = label['meta']['K_matrix'].numpy()


def load_inputs(arrs, meta, name):
    """(preds, label) of a stored case (tests read the fixture back with this)"""
    c = meta['cases'][name]
    L = len(c['levels'])
    flat = [torch.from_numpy(np.asarray(arrs[f"{c['inputs']}/pred{j}"])) for j in range(4 * L)]
    preds = tuple(flat[k * L:(k + 1) * L] for k in range(4))
    label = dict(meta=dict(img_name=[f"img{i}" for i in range(c['B'])], K_matrix=torch.from_numpy(np.asarray(arrs[f"{c['inputs']}/K"])),
                           img_size=[tuple(c['img_size'])] * c['B'], scale_factor=[np.array([1.0, 1.0])] * c['B']))
    return preds, label


def load_expected(arrs, meta, name):
    """the reference's result of a stored case, one dict per image in the restatement's layout (float32 values, int64 labels)"""
    out = []
    for b in range(meta['cases'][name]['B']):
        r = {k: torch.from_numpy(np.asarray(arrs[f"{name}/out{b}/{k}"])) for k in OUT_KEYS + ("bbox2d",)}
        out.append(r)
    return out


def generate():
    torch.set_num_threads(1)
    det_model, dhp = mfg.reference()
    from detection_toolbox import det_tools
    lib = ref_lib()
    substitute_nms(det_tools, lib)
    params = {k: v for k, v in mfg.cs_params(dhp).items() if k != 'test_cfg'}
    ref_cfg = {k: (v if not isinstance(v, float) else float(v)) for k, v in dict(dhp.test_cfg).items()}
    meta = dict(params=mfg.plain(mfg.cs_params(dhp)), test_cfg=ref_cfg, margins_required=MARGINS, cases={})
    out = {}
    seeds = {}
    for name in ('s', 't', 'w', 'n'):
        c = CASES[name]
        if name == 'n':                                     # the inputs of s
            seed = seeds['s']
            preds, label = make_inputs('s', seed)
            m, counts = measure(name, preds, label, params['strides'], lib)
            assert meets(m), (name, m)
        else:
            seed, skipped = 0, []
            while True:
                preds, label = make_inputs(name, seed)
                m, counts = measure(name, preds, label, params['strides'], lib)
                if meets(m):
                    break
                skipped.append(seed)
                seed += 1
                assert seed < 64, (name, m)
            seeds[name] = seed
            store_inputs(out, name, preds, label)
        res = run_reference(det_model, params, name, preds, label)
        ns = []
        for b, r in enumerate(res):
            for k in OUT_KEYS:
                out[f"{name}/out{b}/{k}"] = r['img_bbox'][k].numpy()
            b2 = r['img_bbox2d']
            empty = isinstance(b2, list)
            if empty:
                assert len(b2) == 6 and all(a.shape == (0, 5) and a.dtype == np.float64 for a in b2)
            out[f"{name}/out{b}/bbox2d"] = np.zeros((0, 5), np.float32) if empty else np.asarray(b2)
            ns.append(int(r['img_bbox']['scores_3d'].shape[0]))
        cfg = case_cfg(name)
        if name in ('s', 'n'):
            assert all(n == cfg['max_per_img'] for n in ns), ns         # the final cut is taken
        if name == 't':
            assert 0 < ns[0] < cfg['max_per_img'] and ns[1] == 0, ns
            assert all(cnt[3] == 0 for cnt in counts)
        if name == 'w':
            assert min(counts[0]) > 64 and max(counts[0]) > 128, counts
        meta['cases'][name] = dict(B=c['B'], levels=[list(l) for l in c['levels']], cfg=cfg, img_size=list(c['img']), seed=seed,
                                   seeds_skipped=[] if name == 'n' else skipped, inputs='s' if name == 'n' else name,
                                   margins=m, above_threshold=counts, n_out=ns)
        print(name, "seed", seed, "margins", {k: f"{v:.2e}" for k, v in m.items()}, "per-class", counts, "out", ns, file=sys.stderr)
    return meta, out


def main(out_dir=HERE):
    meta, arrays = generate()
    with open(os.path.join(out_dir, "decode.json"), "w") as f:
        json.dump(meta, f, indent=0, sort_keys=True)
    np.savez_compressed(os.path.join(out_dir, "decode.npz"), **arrays)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)       # an output directory other than tests/golden: a regeneration check
