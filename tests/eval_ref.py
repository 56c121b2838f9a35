"""fp64 numpy restatement of the reference's get_output and task meters, for the evaluation tests.

Every function names the reference lines it restates (paths under TaskPrompter/).  Inputs are the fp32 logits and labels; all
arithmetic is fp64, so the float sums are the yardstick both for the reference's own fp32 results (tests/test_eval_host.py pins this
file to the committed fixture) and for the HIP kernels (tests/test_gpu_eval.py).  Decisions (arg-max, masks, thresholds) are taken on
the fp32 values where they are exact in fp32, and the saliency inputs keep every score 1e-4 away from a threshold.
"""
import numpy as np

CS_VALID_CLASSES = [7, 8, 11, 12, 13, 17, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 31, 32, 33]
F32_TINY_DEPTH = float(np.float32(1e-9))      # eval_depth.py:41-42 writes the python float 1e-9 into an fp32 tensor


def _d(a):
    return np.asarray(a, dtype=np.float64)


# ---- utils/utils.py:27-63 -------------------------------------------------------------------------------------------------------------
def map_ref(task, x, semseg_save_train_class=True):
    """x [B, C, H, W] fp32 -> the map of get_output, fp64 (int64 for the arg-max tasks)"""
    x = _d(x)
    if task in ('semseg', 'human_parts'):
        out = np.argmax(x, axis=1).astype(np.int64)              # :35 torch.max: the first index wins ties, as numpy's argmax
        if task == 'semseg' and not semseg_save_train_class:     # :18-24
            src = out.copy()
            for c in range(19):
                out[src == c] = CS_VALID_CLASSES[c]
        return out
    if task == 'normals':                                        # :30-31
        v = np.transpose(x, (0, 2, 3, 1))
        n = np.maximum(np.sqrt((v * v).sum(-1, keepdims=True)), 1e-12)
        return (v / n + 1.0) * 255 / 2.0
    if task == 'edge':                                           # :46-47
        return 255.0 / (1.0 + np.exp(-x[:, 0]))
    if task == 'sal':                                            # :50-51
        m = x.max(axis=1, keepdims=True)
        e = np.exp(x - m)
        return e[:, 1] / e.sum(axis=1) * 255
    if task == 'depth':                                          # :54-55
        return np.transpose(np.maximum(x, 0.0), (0, 2, 3, 1))
    raise ValueError(task)


# ---- evaluation/eval_semseg.py:70-81, eval_human_parts.py:32-42 --------------------------------------------------------------------------
def confusion_ref(pred_map, gt, n_classes, ignore):
    pred, gt = np.asarray(pred_map).reshape(-1), _d(gt).reshape(-1)
    valid = gt != ignore
    tp, fp, fn = [], [], []
    for i in range(n_classes):
        tmp_gt, tmp_pred = gt == i, pred == i
        tp.append(int((tmp_gt & tmp_pred & valid).sum()))
        fp.append(int((~tmp_gt & tmp_pred & valid).sum()))
        fn.append(int((tmp_gt & ~tmp_pred & valid).sum()))
    return dict(tp=tp, fp=fp, fn=fn)


# ---- evaluation/eval_sal.py:21-60 ------------------------------------------------------------------------------------------------------
def sal_score_ref(sal_map):
    """:30,43: the meter squashes map / 255, a probability, with a sigmoid"""
    return 1.0 / (1.0 + np.exp(-(_d(sal_map) / 255.0)))


def sal_ref(sal_map, gt, thresholds, ignore):
    s, gt = sal_score_ref(sal_map).reshape(-1), _d(gt).reshape(-1)
    valid = gt != ignore
    t = gt.astype(np.int64)
    tp, pp, ap = [], [], []
    for th in thresholds:                                        # the fp32 values of torch.arange(step, 1, step)
        f = (s >= float(th)) & valid
        tp.append(int(t[f].sum()))
        pp.append(int(f.sum()))
        ap.append(int(t[valid].sum()))
    return dict(true_positives=tp, predicted_positives=pp, actual_positives=ap)


def sal_margin(sal_map, thresholds):
    """smallest distance of any pixel's score from any threshold"""
    s = sal_score_ref(sal_map).reshape(-1, 1)
    return float(np.abs(s - _d(thresholds).reshape(1, -1)).min())


# ---- evaluation/eval_depth.py:30-54 (and :83-106 for the ignore-index mask) --------------------------------------------------------------
def depth_ref(depth_map, gt, max_depth=None, min_depth=None, ignore=None):
    pred, gt = _d(depth_map).reshape(-1), _d(gt).reshape(-1)
    mask = (gt != ignore) if ignore is not None else ((gt < max_depth) & (gt > min_depth))
    gt = np.where(gt <= 0, F32_TINY_DEPTH, gt)[mask]
    pred = np.where(pred <= 0, F32_TINY_DEPTH, pred)[mask]
    return dict(n_valid=int(mask.sum()),
                total_log_rmses=float(((np.log(gt) - np.log(pred)) ** 2).sum()),
                total_rmses=float(((gt - pred) ** 2).sum()),
                abs_rel=float((np.abs(gt - pred) / gt).sum()),
                sq_rel=float((((gt - pred) ** 2) / gt).sum()))


# ---- evaluation/eval_normals.py:19-45 --------------------------------------------------------------------------------------------------
def _normalize_tensor(v):
    n = np.sqrt((v * v).sum(1, keepdims=True))
    zero = n == 0
    out = v / np.where(zero, 1.0, n)
    return np.where(zero, 0.0, out)


def normals_ref(normals_map, gt, ignore):
    pred = np.transpose(_d(normals_map), (0, 3, 1, 2))
    pred = 2 * pred / 255 - 1
    gt = _d(gt)
    valid = (gt != ignore).all(axis=1)
    pred, gt = _normalize_tensor(pred), _normalize_tensor(gt)
    deg = np.rad2deg(2 * np.arctan2(np.sqrt(((pred - gt) ** 2).sum(1)), np.sqrt(((pred + gt) ** 2).sum(1))))
    return dict(sum_deg_diff=float(deg[valid].sum()), total=int(valid.sum()))


# ---- evaluation/eval_edge.py:20-31 with losses/loss_functions.py:56-88 -------------------------------------------------------------------
def edge_ref(edge_map, gt, pos_weight, ignore):
    z, y = _d(edge_map).reshape(-1) / 255.0, _d(gt).reshape(-1)
    valid = y != ignore
    z, y = z[valid], y[valid]
    w = float(np.float32(pos_weight))                            # :79 torch.as_tensor(pos_weight) is fp32
    factor = 1.0 / (1.0 - w)
    pw = w * factor
    term = (1 - y) * z + (1 + (pw - 1) * y) * (np.log1p(np.exp(-np.abs(z))) + np.maximum(-z, 0.0))
    return dict(loss=float(term.sum() / factor), n=int(valid.sum()))


def state_ref(case, x, gt):
    """the meter state one update adds, from logits x and labels gt, for a fixture case record (eval.json)"""
    task, a = case["task"], case["meter_args"]
    m = map_ref(task, x)
    if task in ('semseg', 'human_parts'):
        return confusion_ref(m, gt, case["n_classes"], a["ignore"])
    if task == 'sal':
        return sal_ref(m, gt, case["thresholds"], a["ignore"])
    if task == 'depth':
        return depth_ref(m, gt, a.get("max_depth"), a.get("min_depth"), a.get("ignore"))
    if task == 'normals':
        return normals_ref(m, gt, a["ignore"])
    if task == 'edge':
        return edge_ref(m, gt, a["pos_weight"], a["ignore"])
    raise ValueError(task)


def add_states(a, b):
    out = {}
    for k in a:
        out[k] = [u + v for u, v in zip(a[k], b[k])] if isinstance(a[k], list) else a[k] + b[k]
    return out


INT_KEYS = {"tp", "fp", "fn", "true_positives", "predicted_positives", "actual_positives", "n_valid", "total", "n"}


def compare_states(got, want, rtol):
    """(worst relative error of the float sums); asserts integer counters equal"""
    worst = 0.0
    for k, w in want.items():
        g = got[k]
        g = g.tolist() if hasattr(g, "tolist") else g
        if k in INT_KEYS:
            gi = [int(round(float(v))) for v in g] if isinstance(g, list) else int(round(float(g)))
            wi = [int(round(float(v))) for v in w] if isinstance(w, list) else int(round(float(w)))
            assert gi == wi, (k, gi, wi)
        else:
            err = abs(float(g) - float(w)) / max(abs(float(w)), 1e-300)
            worst = max(worst, err)
            assert err <= rtol, (k, float(g), float(w), err)
    return worst
