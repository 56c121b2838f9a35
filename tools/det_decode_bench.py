"""FCOS3D box decoding (det_model.DetModel.get_results_from_bbox) at the Cityscapes-3D inference geometry (five levels 96x192 ... 12x24
of a 768 x 1536 input, cs_test_cfg(): nms_pre 1000, 200 per image) next to the torch-on-GPU restatement of the reference path
(tests/det_decode_ref.py in fp32, its per-class NMS through iou3d.nms_gpu with its host read per class).  Prints one JSON line per
(path, batch): milliseconds per call (results on the host, as the reference returns them), device kernels launched per call (torch
profiler) and host synchronisations per call (torch's sync debug mode).  Run from the repository root:
    python tools/det_decode_bench.py [B ...]"""
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import det_decode_ref as ddr  # noqa: E402
import mtt_amd  # noqa: E402

LEVELS = ((96, 192), (48, 96), (24, 48), (24, 48), (12, 24))
STRIDES = [8.0, 16.0, 32.0, 32.0, 64.0]


def case(B):
    g = torch.Generator().manual_seed(3)
    cls, bbox, dirs, ctr = [], [], [], []
    for h, w in LEVELS:
        cls.append((torch.randn(B, 6, h, w, generator=g) * 2 - 3).cuda())
        bb = torch.randn(B, 13, h, w, generator=g)
        bb[:, 2] = torch.rand(B, h, w, generator=g) * 60 + 3
        bb[:, 3:6] = torch.rand(B, 3, h, w, generator=g) * 3 + 1
        bbox.append(bb.cuda())
        dirs.append(torch.randn(B, 6, h, w, generator=g).cuda())
        ctr.append(torch.randn(B, 1, h, w, generator=g).cuda())
    K = torch.tensor([[1100.0, 0.0, 780.0], [0.0, 1100.0, 390.0], [0.0, 0.0, 1.0]])
    label = dict(meta=dict(img_name=[f"img{i}" for i in range(B)], K_matrix=torch.stack([K] * B), img_size=[(768, 1536)] * B,
                           scale_factor=[np.array([1.0, 1.0])] * B))
    return (cls, bbox, dirs, ctr), label


def kernels(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type.name == "CUDA")


def host_syncs(fn):
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    return sum(1 for w in rec if "synchroniz" in str(w.message))


def timed(fn, reps=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def main(batches):
    cfg = mtt_amd.det_model.cs_test_cfg()
    params = dict(mtt_amd.det_model.cs_det_model_params(), strides=STRIDES)
    crit = mtt_amd.det_model.DetModel(**params)
    for B in batches:
        preds, label = case(B)

        def hip():
            return crit.get_results_from_bbox(preds, label)

        def ref():
            return [{k: v.cpu() for k, v in r.items()} for r in ddr.decode_batch(preds, STRIDES, label, cfg, ddr.hip_nms, torch.float32)]

        n_hip = [int(r["img_bbox"]["scores_3d"].shape[0]) for r in hip()]
        n_ref = [int(r["scores_3d"].shape[0]) for r in ref()]
        for name, fn, n in (("hip", hip, n_hip), ("torch_restatement", ref, n_ref)):
            ms = timed(fn)
            print(json.dumps(dict(path=name, B=B, ms_per_call=round(ms, 4), kernels_per_call=kernels(fn), host_syncs_per_call=host_syncs(fn),
                                  kept=n)), flush=True)


if __name__ == "__main__":
    main([int(a) for a in sys.argv[1:]] or [1, 2])
