"""Shared by tests/test_eval_host.py and tests/test_gpu_eval.py: the evaluation fixture (tests/golden/eval.npz + eval.json, written by
tests/golden/make_eval_golden.py from the unmodified reference), loaded once, and the product meter of a fixture case."""
import functools

import numpy as np
import torch

import conftest
import eval_ref

IGNORE = 255
SAL_MARGIN = 1e-4          # every saliency score keeps this distance from every threshold (the fp32 chain errs by about 1e-7)
SECOND = slice(0, -1)      # the images of the second update: one fewer than the first, and other content



@functools.lru_cache(maxsize=None)
def fixture():
    meta, arrs = conftest.load_golden("eval")
    return meta, {k: arrs[k] for k in arrs.files}


def case_names():
    return list(fixture()[0]["cases"])


def inputs(name):
    """(logits fp32 [B, C, H, W], labels fp32) as numpy; the fixture stores the logits as the fp16 values they are"""
    _, arrs = fixture()
    return arrs[name + ".x"].astype(np.float32), arrs[name + ".gt"].astype(np.float32)


def make_meter(case):
    import mtt_amd
    ev = mtt_amd.evaluation
    if case["meter"] == "DepthMeter_legacy":                       # InvPT's DepthMeter(ignore_index)
        return ev.DepthMeter(ignore_index=case["kwargs"]["ignore_index"])
    return getattr(ev, case["meter"])(**case["kwargs"])


def fixture_state_tensors(case, which):
    """the reference's recorded state as the dict of CPU tensors the product's state() returns"""
    st = case[which]
    out = {}
    for k, v in st.items():
        if k in ("tp", "fp", "fn", "true_positives", "predicted_positives", "actual_positives"):
            out[k] = torch.tensor([int(round(u)) for u in v], dtype=torch.int64)
        elif k in ("n_valid", "total", "n"):
            out[k] = torch.tensor(int(round(v)), dtype=torch.int64)
        else:
            out[k] = torch.tensor(float(v), dtype=torch.float64)
    return out


# ---- inputs with the edge cases the meters can get wrong; shared by the fixture generator and the synthetic GPU cases ---------------------
def fp16(a):
    return np.asarray(a, dtype=np.float32).astype(np.float16).astype(np.float32)


def make_inputs(task, shape, n_classes, thresholds, rng):
    B, C, H, W = shape
    x = fp16(rng.normal(0.0, 2.0, size=shape))
    ign = rng.random((B, 1, H, W)) < 0.05
    if task in ("semseg", "human_parts"):
        tie = rng.random((B, H, W)) < 0.03                     # exact ties at the maximum: a second (later AND earlier) channel equals it
        mx = x.max(axis=1)
        for c in (rng.integers(0, C), C - 1, 0):
            sel = tie & (rng.random((B, H, W)) < 0.5)
            x[:, c][sel] = mx[sel]
        gt = rng.integers(0, n_classes, size=(B, 1, H, W)).astype(np.float32)
        gt[rng.random((B, 1, H, W)) < 0.01] = 254              # a label outside [0, n) that is not the ignore value
        gt[ign] = IGNORE
    elif task == "sal":
        tie = rng.random((B, H, W)) < 0.02                     # some exact ties (p = 0.5)
        x[:, 1][tie] = x[:, 0][tie]
        th = np.asarray(thresholds, dtype=np.float64).reshape(1, -1)
        for _ in range(100):                                   # resample every pixel whose fp64 score is within SAL_MARGIN of a threshold
            s = eval_ref.sal_score_ref(eval_ref.map_ref("sal", x))
            near = (np.abs(s.reshape(-1, 1) - th).min(axis=1) < SAL_MARGIN).reshape(B, H, W)
            if not near.any():
                break
            for c in range(2):
                x[:, c][near] = fp16(rng.normal(0.0, 2.0, size=int(near.sum())))
        else:
            raise RuntimeError("saliency resampling did not converge")
        gt = rng.integers(0, 2, size=(B, 1, H, W)).astype(np.float32)
        gt[ign] = IGNORE
    elif task == "normals":
        x = fp16(rng.normal(0.0, 1.0, size=shape))
        x[0, :, 2, 3] = 0.0                                    # one all-zero prediction
        g = rng.normal(0.0, 1.0, size=shape)
        gt = (g / np.sqrt((g * g).sum(1, keepdims=True))).astype(np.float32)
        gt[-1, :, 4, 5] = 0.0                                  # one all-zero label
        gt[np.broadcast_to(ign, shape)] = IGNORE
        one = rng.random((B, H, W)) < 0.01                     # a single channel at the ignore value invalidates the pixel too
        gt[:, 1][one] = IGNORE
    elif task == "depth":
        x = fp16(rng.normal(2.0, 2.0, size=shape))             # predictions on both sides of 0
        x[0, 0, 0, :4] = 0.0
        gt = (rng.random((B, 1, H, W)) * 9.9 + 0.1).astype(np.float32)      # on both sides of min_depth / max_depth
        gt[0, 0, 1, :3] = (0.0, -1.0, 0.5)                     # labels <= 0 (valid under the ignore-index mask) and one on a bound
        gt[ign] = IGNORE
    elif task == "edge":
        gt = (rng.random((B, 1, H, W)) < 0.3).astype(np.float32)
        gt[ign] = IGNORE
    if B == 3:
        gt[1] = IGNORE                                         # one all-ignored image (for depth: outside (min, max) as well), in both updates
    return x, gt


def case_record(task, shape, cls, kw, n_classes, thresholds):
    """what tests/eval_ref.state_ref and make_meter need to know about a case (the fixture's eval.json holds these per case)"""
    margs = dict(ignore=IGNORE, **{k: v for k, v in kw.items() if k in ("max_depth", "min_depth", "pos_weight")})
    if cls == "DepthMeter":
        del margs["ignore"]
    return dict(task=task, shape=list(shape), meter=cls, kwargs=kw, meter_args=margs, n_classes=n_classes, thresholds=thresholds)
