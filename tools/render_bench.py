"""Rendering predictions on the device at the sizes a user runs, every task on each:

    cityscapes_identity   19 x 1024 x 2048 at its own size, B = 4
    cityscapes_resized    19 x 768 x 1536 -> (1024, 2048), B = 4
    pascal_resized        21 x 512 x 512 -> (375, 500), B = 16
    nyud_identity         40 x 448 x 576 at its own size, B = 8

    python tools/render_bench.py [--iters 10] [--rounds 3] [--log profiles/render_bench.log]

Prints one JSON line per (shape, task) and appends it to the log.  Three legs alternate in the same run, `--rounds` times `--iters`
calls each, and the figure of a leg is the median of its per-call event intervals over all rounds:
  fused   PredictionRenderer.render into a preallocated output (for depth both launches: the minimum / maximum pass and the map)
  torch   the reference's op sequence (visualization_utils.py:126-191 with utils.py:27-63) as torch ops on the same device:
          F.interpolate(bilinear), permute, max / sigmoid / softmax / normalize / clamp, the colour-table lookup, .to(uint8) and the
          channel swap; the int64 / fp32 map it produces is what the reference then copies to the host
  copy    dst.copy_(src) of fp32 tensors sized so that the copy moves as many bytes as the fused leg has to: the logits read once (twice
          the single depth channel) plus the bytes written, half of them read and half written
`x_torch` is torch / fused, `of_copy_rate` is copy / fused (1.0 = the fused kernel moves its bytes as fast as a plain copy does).  There
is no pass / fail threshold."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mtt_amd  # noqa: E402

SHAPES = {
    "cityscapes_identity": dict(db="Cityscapes3D", B=4, C=19, src=(1024, 2048), size=(1024, 2048)),
    "cityscapes_resized": dict(db="Cityscapes3D", B=4, C=19, src=(768, 1536), size=(1024, 2048)),
    "pascal_resized": dict(db="PASCALContext", B=16, C=21, src=(512, 512), size=(375, 500)),
    "nyud_identity": dict(db="NYUD", B=8, C=40, src=(448, 576), size=(448, 576)),
}
CHANNELS = dict(human_parts=7, sal=2, edge=1, normals=3, depth=1)
TASKS = ["semseg", "human_parts", "sal", "edge", "normals", "depth"]


def torch_sequence(x, task, size, table):
    """what vis_pred_for_one_task computes before the file writer, kept on the device"""
    out = F.interpolate(x, size, mode="bilinear")
    if task == "normals":
        out = (F.normalize(out.permute(0, 2, 3, 1), p=2, dim=3) + 1.0) * 255 / 2.0
        return out.to(torch.uint8)[..., [2, 1, 0]]
    if task in ("semseg", "human_parts"):
        _, idx = torch.max(out.permute(0, 2, 3, 1), dim=3)
        return table[idx].to(torch.uint8)[..., [2, 1, 0]]
    if task == "edge":
        return torch.squeeze(255 * 1 / (1 + torch.exp(-out.permute(0, 2, 3, 1))), dim=3).to(torch.uint8)
    if task == "sal":
        return (F.softmax(out.permute(0, 2, 3, 1), dim=3)[:, :, :, 1] * 255).to(torch.uint8)
    out = out.clamp_(min=0.).permute(0, 2, 3, 1).squeeze(3)
    lo, hi = out.amin(dim=(1, 2), keepdim=True), out.amax(dim=(1, 2), keepdim=True)
    return table[((out - lo) / (hi - lo) * 255).to(torch.uint8).long()]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "render_bench.log"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "render_bench.py measures on the GPU only"
    dev = "cuda:0"
    lines = []
    for name, s in SHAPES.items():
        r = mtt_amd.PredictionRenderer(s["db"])
        B, (h, w), (H, W) = s["B"], s["src"], s["size"]
        for task in TASKS:
            C = s["C"] if task == "semseg" else CHANNELS[task]
            x = torch.randn(B, C, h, w, device=dev) * 3
            if task == "depth":
                x = x.abs_()
            channels = 1 if task in ("sal", "edge") else 3
            out = torch.empty(B * H * W * channels, dtype=torch.uint8, device=dev)
            table = r._table(task if task != "semseg" else "semseg", dev) if task in ("semseg", "human_parts", "depth") else None
            read = B * C * h * w * 4 + (B * h * w * 4 if task == "depth" else 0)
            written = B * H * W * channels
            n = (read + written) // 8
            src, dst = torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
            legs = {"fused": lambda: r.render(x, task, (H, W), out=out), "torch": lambda: torch_sequence(x, task, (H, W), table),
                    "copy": lambda: dst.copy_(src)}
            for fn in legs.values():                        # warm-up of every leg at this shape
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            times = {k: [] for k in legs}
            for _ in range(a.rounds):
                for k, fn in legs.items():
                    times[k] += [timed(fn) for _ in range(a.iters)]
            med = {k: statistics.median(v) for k, v in times.items()}
            res = dict(shape=name, task=task, batch=B, channels=C, src=[h, w], size=[H, W], MB_read=round(read / 1e6, 1), MB_written=round(written / 1e6, 1),
                       **{k + "_us": round(v, 1) for k, v in med.items()},
                       **{k + "_min_max_us": [round(min(v), 1), round(max(v), 1)] for k, v in times.items()},
                       fused_GBps=round((read + written) / med["fused"] / 1e3, 1), copy_GBps=round((read + written) / med["copy"] / 1e3, 1),
                       x_torch=round(med["torch"] / med["fused"], 2), of_copy_rate=round(med["copy"] / med["fused"], 3))
            lines.append(json.dumps(res))
            print(lines[-1], flush=True)
            del x, out, src, dst
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.log), exist_ok=True)
    with open(a.log, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
