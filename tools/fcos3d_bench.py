"""The FCOS3D criterion (det_model.DetModel.loss, forward + backward) at the Cityscapes-3D geometry (five levels 96x192 ... 12x24, strides
[8, 16, 32, 32, 64] / 0.75, 40 gts per image) next to a torch-on-GPU restatement of the reference path (tests/fcos3d_ref.py in fp32:
per-image [points, gts] intermediates, boolean-mask gathers, host syncs).  Prints one JSON line per (path, batch): milliseconds per
forward + backward (labels packed beforehand for the HIP path, as a data loader would) and device kernels launched per call (torch
profiler).  Run from the repository root:  python tools/fcos3d_bench.py [B ...]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import fcos3d_ref  # noqa: E402
import mtt_amd  # noqa: E402

LEVELS = ((96, 192), (48, 96), (24, 48), (24, 48), (12, 24))


def case(B):
    dm = mtt_amd.det_model
    p = {"IMAGE_ORI_SIZE": (1024, 2048), "TRAIN": {"SCALE": (1024, 2048)}, "img_ds_ratio": 0.75}
    dm.configure_3ddet(p)
    labels = dm.synthetic_det_labels(B, (1024, 2048), 40, seed=B)
    g = torch.Generator().manual_seed(7)
    preds = [[torch.randn(B, ch, h, w, generator=g).cuda().requires_grad_(True) for h, w in LEVELS] for ch in (6, 13, 6, 1)]
    return p, labels, preds


def kernels(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type.name == "CUDA")


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
    for B in batches:
        p, labels, preds = case(B)
        crit = p["detmodel"]
        packed = crit.pack_labels(labels, "cuda")
        gl = {k: ([{kk: vv.cuda() for kk, vv in e.items()} for e in v] if k == "det_labels" else v) for k, v in labels.items()}

        def hip():
            crit.loss(preds, packed)[1].backward()

        def ref():
            fcos3d_ref.loss(p["det_model_params"], preds, gl, dtype=torch.float32)[1].backward()

        for name, fn in (("hip", hip), ("torch_restatement", ref)):
            ms = timed(fn)
            print(json.dumps(dict(path=name, B=B, ms_fwd_bwd=round(ms, 4), kernels_per_call=kernels(fn))), flush=True)


if __name__ == "__main__":
    main([int(a) for a in sys.argv[1:]] or [1, 8])
