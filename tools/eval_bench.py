"""Validation-batch evaluation, PASCAL-5 at 512 x 512, valBatch 6: the HIP meters (fused update_from_logits, and get_output + update)
against a torch-on-device restatement of the reference's get_output + meters (TaskPrompter/utils/utils.py:27-63, evaluation/eval_*.py),
which synchronises with the host after almost every reduction.  The restatement keeps the reference's reductions and host copies but
masks where the reference compacts (masked_select), so it does somewhat less device work and fewer synchronisations than the original.

    python tools/eval_bench.py [--batch 6] [--size 512] [--iters 20] [--lib build/variants/libmtt_<name>.so]

Prints one JSON line: microseconds per batch for each side, the achieved GB/s of the HIP paths against the minimum traffic (every logit
and label read once) and the host synchronisations per batch on each side, plus the fused path replayed from a captured graph (device time, whole batch
and per task as [us, GB/s]).
"""
import argparse
import json
import os
import sys
import time
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mtt_amd  # noqa: E402

TASKS = ["semseg", "human_parts", "sal", "edge", "normals"]
NUM = dict(semseg=21, human_parts=7, sal=2, edge=1, normals=3)


# ---- the reference's evaluation restated with torch ops on the device (same ops, same host synchronisations) ---------------------------
def torch_get_output(output, task):
    import torch.nn.functional as F
    output = output.permute(0, 2, 3, 1)
    if task == "normals":
        return (F.normalize(output, p=2, dim=3) + 1.0) * 255 / 2.0
    if task in ("semseg", "human_parts"):
        return torch.max(output, dim=3)[1]
    if task == "edge":
        return torch.squeeze(255 * 1 / (1 + torch.exp(-output)), dim=3)
    return F.softmax(output, dim=3)[:, :, :, 1] * 255


class TorchMeters(object):
    def __init__(self, n_sem=21, n_parts=7, ignore=255, edge_w=0.95):
        self.n = dict(semseg=n_sem, human_parts=n_parts)
        self.ignore, self.edge_w = ignore, edge_w
        self.c = {t: [[0] * n for _ in range(3)] for t, n in self.n.items()}
        self.th = torch.arange(0.05, 1, 0.05)
        self.sal = [torch.zeros(len(self.th)) for _ in range(3)]
        self.normals = [0.0, 0]
        self.edge = [0.0, 0]

    def update(self, pred, gt):
        for t, n in self.n.items():
            p, g = pred[t].squeeze(), gt[t].squeeze()
            valid = g != self.ignore
            for i in range(n):
                tg, tp = g == i, p == i
                self.c[t][0][i] += torch.sum(tg & tp & valid).item()
                self.c[t][1][i] += torch.sum(~tg & tp & valid).item()
                self.c[t][2][i] += torch.sum(tg & ~tp & valid).item()
        # saliency: per threshold three masked sums, each copied to the host (the reference also compacts both operands first)
        score, target = torch.sigmoid(pred["sal"].float() / 255.), gt["sal"].squeeze(1)
        valid = target != self.ignore
        positives = torch.where(valid, target, torch.zeros_like(target)).long()
        for i, th in enumerate(self.th):
            hit = ((score >= th) & valid).long()
            self.sal[0][i] += (hit * positives).sum().cpu()
            self.sal[1][i] += hit.sum().cpu()
            self.sal[2][i] += positives.sum().cpu()
        # normals: back from the 0..255 map, unit vectors (zero where the norm is zero), angle between them over the valid pixels
        valid = (gt["normals"] != self.ignore).all(dim=1)
        unit = []
        for v in (2 * pred["normals"].permute(0, 3, 1, 2) / 255 - 1, gt["normals"]):
            length = v.pow(2).sum(dim=1, keepdim=True).sqrt()
            unit.append(torch.where(length > 0, v / length.clamp_min(1e-30), torch.zeros_like(v)))
        far, near = (unit[0] - unit[1]).pow(2).sum(dim=1).sqrt(), (unit[0] + unit[1]).pow(2).sum(dim=1).sqrt()
        deg = torch.rad2deg(2 * torch.atan2(far, near))
        self.normals[0] += torch.where(valid, deg, torch.zeros_like(deg)).sum().item()
        self.normals[1] += int(valid.sum().item())
        g = gt["edge"].squeeze()
        valid = g != self.ignore
        z, y = pred["edge"][valid].float() / 255., g[valid]
        w = torch.as_tensor(self.edge_w, device=z.device)
        factor = 1. / (1 - w)
        loss = torch.nn.functional.binary_cross_entropy_with_logits(z, y, pos_weight=w * factor) / factor
        self.edge[0] += y.numel() * loss.item()
        self.edge[1] += y.numel()


def count_syncs(fn):
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    return sum(1 for w in rec if "synchroniz" in str(w.message))


def timed(fn, iters):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=6)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--lib", default=None, help="another build of the library, e.g. build/variants/libmtt_evalscalar.so (-DMTT_EVAL_VEC=0)")
    a = ap.parse_args()
    if a.lib:
        mtt_amd._lib.LIB_PATH = os.path.abspath(a.lib)
    B, H, W = a.batch, a.size, a.size
    AttrDict = mtt_amd.factory.AttrDict
    p = AttrDict(train_db_name="PASCALContext", ignore_index=255, edge_w=0.95, TASKS=AttrDict(NAMES=TASKS, NUM_OUTPUT=NUM))
    g = torch.Generator(device="cpu").manual_seed(0)
    out = {t: (torch.randn(B, NUM[t], H, W, generator=g) * 2).to("cuda:0") for t in TASKS}
    gt = mtt_amd.losses.synthetic_targets(p, B, H, W, "cuda:0", seed=1)
    pm = mtt_amd.PerformanceMeter(p, TASKS).to("cuda:0")
    ref = TorchMeters()

    def fused():
        pm.update_from_logits(out, gt)

    def mapped():
        pm.update({t: mtt_amd.get_output(out[t], t) for t in TASKS}, gt)

    def reference():
        ref.update({t: torch_get_output(out[t], t) for t in TASKS}, gt)

    res = dict(shape=[B, H, W], tasks=TASKS, library=os.path.relpath(mtt_amd._lib.LIB_PATH, ROOT))
    min_bytes = sum(out[t].numel() + gt[t].numel() for t in TASKS) * 4
    for name, fn in (("fused", fused), ("maps", mapped), ("torch_reference", reference)):
        us = timed(fn, a.iters if name != "torch_reference" else max(a.iters // 5, 2))
        res[name] = dict(us_per_batch=round(us, 1), host_syncs=count_syncs(fn))
        if name != "torch_reference":
            res[name]["GBps_vs_min_traffic"] = round(min_bytes / us / 1e3, 1)
    # the same launches replayed from a captured graph: the device time without the host's launch cost, all tasks and one task at a time
    def replayed(fn):
        fn()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            fn()
        return timed(graph.replay, a.iters)

    us = replayed(fused)
    res["fused_graph"] = dict(us_per_batch=round(us, 1), GBps_vs_min_traffic=round(min_bytes / us / 1e3, 1))
    res["fused_graph_per_task_us"] = {}
    for t in TASKS:
        us = replayed(lambda: pm.meters[t].update_from_logits(out[t], gt[t]))
        res["fused_graph_per_task_us"][t] = [round(us, 1), round((out[t].numel() + gt[t].numel()) * 4 / us / 1e3, 1)]     # us, GB/s
    res["min_traffic_MB"] = round(min_bytes / 1e6, 2)
    res["speedup_fused_vs_torch"] = round(res["torch_reference"]["us_per_batch"] / res["fused"]["us_per_batch"], 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
