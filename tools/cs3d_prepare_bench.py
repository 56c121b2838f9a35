"""Cityscapes-3D batch preparation on the device, 1024 x 2048 frames: the shipped configuration (image kept, label maps to 512 x 1024)
and a resized one (image to 768 x 1536 as well), for batches of 4 and of 16.

    python tools/cs3d_prepare_bench.py [--iters 50] [--host-frames 2] [--log profiles/cs3d_prepare_bench.log]

Prints one JSON line per (configuration, batch) and appends it to the log.  Device times are medians of per-launch event intervals after
warm-up: `prep.run` on a stacked batch (both launches and the flag clear) and the image launch alone; the label launch is their difference.  Bytes are what the kernels have
to move at cache-line granularity: every source byte of the image; of the label and disparity maps the rows the nearest table selects
(a stride of two along x still touches every line of such a row); every output byte (12 per image pixel; 8 + 4 per label pixel).  The
fraction is against the 8.0 TB/s HBM3E specification.
The host side is timed on `--host-frames` frames and scaled to the batch: the numpy restatement tests/cs3d_ref.py, and the reference's
own arithmetic with Pillow doing the resizes (PIL.Image.resize + numpy, what cityscapes3d.py runs per sample), each on one thread and on
16 threads that take a frame each (numpy and Pillow release the interpreter lock in their loops).  PNG decoding is not part of either
side.  There is no pass / fail threshold."""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mtt_amd  # noqa: E402
import cs3d_ref  # noqa: E402

HBM_SPEC = 8.0e12
FRAME = (1024, 2048)
CONFIGS = {"shipped": ((1024, 2048), (512, 1024)), "image_resized": ((768, 1536), (512, 1024))}


def make_frames(n, seed=0):
    g = np.random.RandomState(seed)
    ids = np.array(cs3d_ref.VOID + cs3d_ref.VALID, dtype=np.uint8)
    H, W = FRAME
    return (g.randint(0, 256, (n, H, W, 3)).astype(np.uint8), ids[g.randint(0, len(ids), (n, H, W))], g.randint(0, 1 << 16, (n, H, W)).astype(np.uint16))


def bytes_moved(prep, B):
    H, W = FRAME
    h, w = prep.img_size
    lh, lw = prep.label_size(FRAME)
    image = B * (H * W * 3 + h * w * 12)
    rows = len(set(prep.label_tables(FRAME)[0].tolist())) if prep.label_tables(FRAME) is not None else H
    labels = B * (rows * W * 3 + lh * lw * 12)
    return image, labels


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


def pillow_frame(image, labels, disp, prep):
    """cityscapes3d.py:137-241 for one decoded frame, its own numpy statements over Pillow's resize"""
    from PIL import Image

    def imresize(a, size, resample):
        return np.array(Image.fromarray(a).resize((size[1], size[0]), resample))

    img = np.ascontiguousarray(image[..., ::-1]) if prep.bgr else image
    depth = disp.astype(np.float32)
    depth[depth > 0] = (depth[depth > 0] - 1) / 256
    depth[depth == 0] = -1
    depth[labels == 10] = 0
    lbl = cs3d_ref.encode_lut()[labels].astype(np.uint8)
    if prep.img_size != FRAME:
        img = imresize(img, prep.img_size, Image.BILINEAR)
    np.unique(lbl)
    lbl = lbl.astype(float)
    if prep.dd_label_map_size != prep.ori_img_size:
        lbl = imresize(lbl, prep.dd_label_map_size, Image.NEAREST)
        depth = imresize(depth, prep.dd_label_map_size, Image.NEAREST)
    lbl = lbl.astype(int)
    np.unique(lbl[lbl != 255])
    t = img.transpose(2, 0, 1).astype(np.float32) / np.float32(255)
    return (t - np.asarray(prep.mean, np.float32)[:, None, None]) / np.asarray(prep.std, np.float32)[:, None, None], lbl, depth[None]


def host_seconds_per_frame(fn, frames, threads):
    n = len(frames[0])
    jobs = [tuple(a[i] for a in frames) for i in range(n)] * (threads if threads > 1 else 1)
    with ThreadPoolExecutor(max_workers=threads) as ex:
        list(ex.map(lambda j: fn(*j), jobs[:threads]))                                   # warm-up
        t0 = time.perf_counter()
        list(ex.map(lambda j: fn(*j), jobs))
        return (time.perf_counter() - t0) / len(jobs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--host-frames", type=int, default=2)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "cs3d_prepare_bench.log"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "cs3d_prepare_bench.py measures on the GPU only"
    try:
        import PIL  # noqa: F401
        have_pil = True
    except ImportError:
        have_pil = False
    images, labels, disps = make_frames(16)
    lines = []
    for name, (img_size, label_size) in CONFIGS.items():
        prep = mtt_amd.Cityscapes3DPrepare(["semseg", "depth"], img_size, label_size)
        host = {}
        sub = tuple(x[:a.host_frames] for x in (images, labels, disps))
        for threads in (1, 16):
            host[f"restatement_ms_per_frame_{threads}_threads"] = round(1e3 * host_seconds_per_frame(
                lambda im, lab, d: cs3d_ref.prepare_frame(im, lab, d, prep.img_size, prep.dd_label_map_size, prep.mean, prep.std, bgr=prep.bgr), sub, threads), 2)
            if have_pil:
                host[f"pillow_ms_per_frame_{threads}_threads"] = round(1e3 * host_seconds_per_frame(lambda im, lab, d: pillow_frame(im, lab, d, prep), sub, threads), 2)
        for B in (4, 16):
            packed = {"image": torch.from_numpy(images[:B]).to("cuda:0"), "semseg": torch.from_numpy(labels[:B]).to("cuda:0"),
                      "depth": torch.from_numpy(disps[:B]).to("cuda:0")}
            out = prep.run(packed)
            prep.check(out)
            image_b, label_b = bytes_moved(prep, B)
            only_image = mtt_amd.Cityscapes3DPrepare([], img_size, label_size)
            res = dict(config=name, batch=B, img_size=list(img_size), label_size=list(label_size), MB_moved=dict(image=round(image_b / 1e6, 1), labels=round(label_b / 1e6, 1)))
            for what, fn, nbytes in (("run", lambda: prep.run(packed, out=out), image_b + label_b),
                                     ("image_only", lambda: only_image.run(packed, out=out), image_b)):
                med, lo, hi = event_median(fn, a.iters)
                res[what] = dict(us_per_batch=round(med, 1), min_us=round(lo, 1), max_us=round(hi, 1), GBps=round(nbytes / med / 1e3, 1),
                                 fraction_of_HBM_spec=round(nbytes / (med * 1e-6) / HBM_SPEC, 3))
            res["labels_us_by_difference"] = round(res["run"]["us_per_batch"] - res["image_only"]["us_per_batch"], 1)
            res["images_per_s_device"] = round(B / (res["run"]["us_per_batch"] * 1e-6), 0)
            res["host"] = dict(host, **{k.replace("ms_per_frame", "ms_per_batch"): round(v * B, 1) for k, v in host.items()})
            lines.append(json.dumps(res))
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.log), exist_ok=True)
    with open(a.log, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
