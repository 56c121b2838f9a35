"""Generate tests/golden/eval.npz + eval.json: the UNMODIFIED reference get_output and task meters run on the CPU.

Run from the repository root where the reference checkout is available (oracle/ref_import.REFERENCE_ROOT):
    python tests/golden/make_eval_golden.py
The reference's evaluation modules import cv2 and imageio at module level without using them in the code run here; empty stand-in
modules are placed in sys.modules for the import (here only).

Per case the fixture holds the inputs (logits as float16: every logit is an fp16 value, so the test's fp32 copy is exact), the
get_output maps, the meter state after a first update on the whole batch and a second one on images [:-1] (a different batch size and,
with the all-ignored image in the middle of the batches of three, different content),
the get_score results, and the inspect.signature strings of the reference's interface.
"""
import inspect
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import eval_ref  # noqa: E402
import eval_util  # noqa: E402
from oracle import ref_import  # noqa: E402

IGNORE = eval_util.IGNORE
CASES = [  # name, task, (B, C, H, W), meter class, constructor kwargs
    ("semseg_pascal", "semseg", (3, 21, 23, 37), "SemsegMeter", dict(database="PASCALContext", ignore_idx=IGNORE)),
    ("semseg_nyud", "semseg", (2, 40, 5, 7), "SemsegMeter", dict(database="NYUD", ignore_idx=IGNORE)),
    ("semseg_cs", "semseg", (2, 19, 64, 80), "SemsegMeter", dict(database="Cityscapes3D", ignore_idx=IGNORE)),
    # more logit channels than the meter has classes: predictions outside [0, n_classes) count nowhere
    ("semseg_extra", "semseg", (2, 24, 8, 12), "SemsegMeter", dict(database="PASCALContext", ignore_idx=IGNORE)),
    ("human_parts", "human_parts", (3, 7, 23, 37), "HumanPartsMeter", dict(database="PASCALContext", ignore_idx=IGNORE)),
    ("sal", "sal", (3, 2, 23, 37), "SaliencyMeter", dict(ignore_index=IGNORE, threshold_step=0.05, beta_squared=0.3)),
    ("sal_big", "sal", (2, 2, 64, 80), "SaliencyMeter", dict(ignore_index=IGNORE, threshold_step=0.05, beta_squared=0.3)),
    ("normals", "normals", (3, 3, 23, 37), "NormalsMeter", dict(ignore_index=IGNORE)),
    ("depth_range", "depth", (3, 1, 23, 37), "DepthMeter", dict(max_depth=8.0, min_depth=0.5)),
    ("depth_ignore", "depth", (3, 1, 23, 37), "DepthMeter_legacy", dict(ignore_index=IGNORE)),
    ("edge", "edge", (3, 1, 23, 37), "EdgeMeter", dict(pos_weight=0.95, ignore_index=IGNORE)),
]
SAL_MARGIN = eval_util.SAL_MARGIN


def load_reference():
    for name in ("cv2", "imageio"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.path.insert(0, os.path.join(ref_import.REFERENCE_ROOT, "TaskPrompter"))
    import evaluation.eval_depth as ed
    import evaluation.eval_edge as ee
    import evaluation.eval_human_parts as eh
    import evaluation.eval_normals as en
    import evaluation.eval_sal as es
    import evaluation.eval_semseg as ess
    import evaluation.evaluate_utils as eu
    import utils.utils as uu
    return dict(get_output=uu.get_output, SemsegMeter=ess.SemsegMeter, HumanPartsMeter=eh.HumanPartsMeter, SaliencyMeter=es.SaliencyMeter,
                NormalsMeter=en.NormalsMeter, DepthMeter=ed.DepthMeter, DepthMeter_legacy=ed.DepthMeter_legacy, EdgeMeter=ee.EdgeMeter,
                PerformanceMeter=eu.PerformanceMeter)


def state_of(meter, task):
    if task in ("semseg", "human_parts"):
        return dict(tp=[int(v) for v in meter.tp], fp=[int(v) for v in meter.fp], fn=[int(v) for v in meter.fn])
    if task == "sal":
        return {k: [float(v) for v in getattr(meter, k)] for k in ("true_positives", "predicted_positives", "actual_positives")}
    if task == "depth":
        return {k: float(getattr(meter, k)) for k in ("n_valid", "total_rmses", "total_log_rmses", "abs_rel", "sq_rel")}
    if task == "normals":
        return dict(sum_deg_diff=float(meter.sum_deg_diff), total=int(meter.total))
    return dict(loss=float(meter.loss), n=int(meter.n))


def main():
    ref = load_reference()
    rng = np.random.default_rng(20240917)
    arrays, meta = {}, dict(cases={}, signatures={})
    for name, task, shape, cls, kw in CASES:
        meter = ref[cls](**kw)
        n_classes = getattr(meter, "n_classes", None) or (getattr(meter, "n_parts", 0) + 1)
        thresholds = [float(v) for v in meter.thresholds] if task == "sal" else None
        x, gt = eval_util.make_inputs(task, shape, n_classes, thresholds, rng)
        states, maps = [], []
        for sl in (slice(0, None), eval_util.SECOND):
            xs, gs = torch.from_numpy(x[sl].copy()), torch.from_numpy(gt[sl].copy())      # depth mutates both in place
            m = ref["get_output"](xs, task)
            maps.append(m.contiguous().numpy().copy())
            meter.update(m, gs)
            states.append(state_of(meter, task))
        score = {k: float(v) for k, v in meter.get_score(verbose=False).items()}
        arrays[name + ".x"] = x.astype(np.float16)
        arrays[name + ".gt"] = gt
        arrays[name + ".map"] = maps[0].astype(np.uint8) if maps[0].dtype == np.int64 else maps[0]
        if name == "semseg_cs":
            arrays[name + ".map_labelid"] = ref["get_output"](torch.from_numpy(x.copy()), task, semseg_save_train_class=False).numpy().astype(np.uint8)
        case = eval_util.case_record(task, shape, cls, kw, n_classes, thresholds)
        case.update(state1=states[0], state2=states[1], score=score)
        # the fp64 restatement must agree with what the reference computed: counts exactly, its fp32 sums within 1e-5
        want1 = eval_ref.state_ref(case, x, gt)
        want2 = eval_ref.add_states(want1, eval_ref.state_ref(case, x[eval_util.SECOND], gt[eval_util.SECOND]))
        w1 = eval_ref.compare_states(states[0], want1, 1e-5)
        w2 = eval_ref.compare_states(states[1], want2, 1e-5)
        if task == "sal":
            case["sal_margin"] = eval_ref.sal_margin(eval_ref.map_ref("sal", x), thresholds)
            assert case["sal_margin"] >= SAL_MARGIN
        print("%-14s reference fp32 vs fp64 restatement: %.2e / %.2e   score %s" % (name, w1, w2, score))
        meta["cases"][name] = case
    sig = lambda f: str(inspect.signature(f))           # noqa: E731
    meta["signatures"]["get_output"] = sig(ref["get_output"])
    for cls in ("SemsegMeter", "HumanPartsMeter", "SaliencyMeter", "NormalsMeter", "DepthMeter", "EdgeMeter", "PerformanceMeter"):
        for fn in ("__init__", "update", "get_score"):
            meta["signatures"]["%s.%s" % (cls, fn)] = sig(getattr(ref[cls], fn))
    np.savez_compressed(os.path.join(HERE, "eval.npz"), **arrays)
    with open(os.path.join(HERE, "eval.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("eval.npz: %d bytes" % os.path.getsize(os.path.join(HERE, "eval.npz")))


if __name__ == "__main__":
    main()
