"""Training-batch augmentation on the device, PASCAL-5 at 512 x 512, batch 126 (the batch of the headline step): ragged uint8 images and
fp32 label maps of up to 500 x 500, scales across [0.5, 2], every stage of the train pipeline on.

    python tools/augment_bench.py [--batch 126] [--size 512] [--iters 30] [--seed 0]

Prints one JSON line.  Times are medians of per-call device-event intervals after warm-up: the whole `aug(samples, params)` call (packing
the ragged batch with torch.cat, the table upload, the select, image and label launches), the packing alone (`aug.pack`), and `aug.run` on a batch that
is already packed (the table upload and the kernels).  GB/s is against the algorithmic bytes: the source pixels under each sample's crop window
(the window mapped back through the scale, capped by the source) for every key, plus every output byte written (40 per output pixel).
There is no pass / fail threshold."""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mtt_amd  # noqa: E402

TASKS = ["semseg", "human_parts", "sal", "edge", "normals"]
CHANNELS = mtt_amd.augment.CHANNELS


def make_samples(B, seed, lo=300, hi=500):
    g = np.random.RandomState(seed)
    samples = []
    for _ in range(B):
        H, W = int(g.randint(lo, hi + 1)), int(g.randint(lo, hi + 1))
        yy, xx = np.mgrid[0:H, 0:W]
        semseg = ((yy * 4 // H) * 5 + xx * 5 // W).astype(np.float32)                    # 20 blocks: crops see several classes
        normals = g.randn(H, W, 3).astype(np.float32)
        s = {"image": g.randint(0, 256, (H, W, 3)).astype(np.uint8), "semseg": semseg[..., None],
             "human_parts": g.randint(0, 7, (H, W, 1)).astype(np.float32), "sal": (g.rand(H, W, 1) < 0.4).astype(np.float32),
             "edge": (g.rand(H, W, 1) < 0.1).astype(np.float32), "normals": normals}
        samples.append({k: torch.from_numpy(v).to("cuda:0") for k, v in s.items()})
    return samples


def algorithmic_bytes(P, size):
    h, w = size
    src_px = 0.0
    for (H, W), (Sh, Sw) in zip(P.shapes.tolist(), P.scaled.tolist()):
        src_px += min(min(Sh, h) * H / Sh, H) * min(min(Sw, w) * W / Sw, W)
    per_src_px = 3 + sum(4 * CHANNELS.get(t, 1) for t in TASKS)                          # uint8 image + fp32 labels
    per_out_px = 4 * (3 + sum(CHANNELS.get(t, 1) for t in TASKS))
    return src_px * per_src_px, len(P) * h * w * per_out_px


def event_median(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=126)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "augment_bench.py measures on the GPU only"
    size = (a.size, a.size)
    samples = make_samples(a.batch, a.seed)
    aug = mtt_amd.DeviceAugment(TASKS, size)
    t0 = time.perf_counter()
    P = aug.draw([s["image"].shape[:2] for s in samples], random.Random(a.seed))
    draw_us = (time.perf_counter() - t0) * 1e6
    read_b, write_b = algorithmic_bytes(P, size)

    def whole():
        aug(samples, P)

    def pack():
        aug.pack(samples)

    flat, shapes = aug.pack(samples)

    def run():
        aug.run(flat, shapes, P)

    res = dict(batch=a.batch, size=list(size), tasks=TASKS, source_sizes=[int(P.shapes.min()), int(P.shapes.max())],
               scales=[round(float(P.scale.min()), 3), round(float(P.scale.max()), 3)], draw_host_us=round(draw_us, 1),
               algorithmic_MB=dict(read=round(read_b / 1e6, 1), written=round(write_b / 1e6, 1)))
    for name, fn in (("call", whole), ("pack_only", pack), ("run_packed", run)):
        med, lo, hi = event_median(fn, a.iters)
        res[name] = dict(us_per_batch=round(med, 1), min_us=round(lo, 1), max_us=round(hi, 1))
        if name != "pack_only":
            res[name]["GBps_vs_algorithmic_bytes"] = round((read_b + write_b) / med / 1e3, 1)
    # host time of one call (launch-bound or not): wall clock around call + synchronise
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.iters):
        whole()
    torch.cuda.synchronize()
    res["call_wall_us"] = round((time.perf_counter() - t0) / a.iters * 1e6, 1)
    res["images_per_s_wall"] = round(a.batch / (res["call_wall_us"] * 1e-6), 0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
