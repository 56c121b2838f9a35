"""Micro-benchmark of the attention kernels through the C ABI (HIP-event timed).
Usage: python tools/attn_bench.py [B] [N] [nH] [T] [--lib build/variants/libmtt_<name>.so]
MTT_ATTN_PLAIN=1 forces the straightforward forward kernel (mtt_attn_desc.variant)."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import mtt_amd  # noqa: E402
from mtt_amd import ops  # noqa: E402

argv = [a for a in sys.argv[1:]]
if "--lib" in argv:
    i = argv.index("--lib")
    mtt_amd._lib.LIB_PATH = os.path.abspath(argv[i + 1])
    del argv[i:i + 2]
print(f"library: {mtt_amd._lib.LIB_PATH}", flush=True)
B, N, nH, T = [int(a) for a in argv[:4]] + [40, 1030, 16, 6][len(argv):]
C = nH * 64
prec = ops.Prec("bf16")
PLAIN = os.environ.get("MTT_ATTN_PLAIN") == "1"
if PLAIN:
    _call = ops.call
    ops.call = lambda name, **kw: _call(name, **(dict(kw, variant=1) if name == "attn_fwd" else kw))
dev = torch.device("cuda")
qkv = (torch.randn(B * N, 3 * C, device=dev) * 1.0).to(torch.bfloat16)
dao = torch.randn(B * N, C, device=dev).to(torch.bfloat16)
drawlog = torch.randn(B, nH, T, N, device=dev) * 0.01 if T else None


def timed(fn, iters=10):
    """microseconds per call: (median, min, max) over 5 timed groups of `iters` calls"""
    for _ in range(3):
        fn()
    ts = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / iters * 1e3)
    return statistics.median(ts), min(ts), max(ts)


ao, rawlog, lse = ops.attention(qkv, B, N, nH, T, prec, want_lse=True)
t_f = timed(lambda: ops.attention(qkv, B, N, nH, T, prec, want_lse=True))
dqkv = torch.empty_like(qkv)
dsum = torch.empty(B, nH, 2, (N + 3) // 4 * 4, device=dev)
t_b = timed(lambda: ops.call("attn_bwd", qkv=qkv, out=ao, rawlog=None, lse=lse, B=B, N=N, nH=nH, T=T, dtype=1, prec=0, scale=0.125,
                             xargs=[dao, drawlog, dqkv, dsum]))
gf = 4.0 * N * N * 64 * nH * B / 1e9
print(f"attention B={B} N={N} nH={nH} T={T} plain={int(PLAIN)}: fwd {t_f[0]:.0f} us [{t_f[1]:.0f}, {t_f[2]:.0f}] = {gf / t_f[0] * 1e3:.0f} TFLOP/s (2 GEMMs);"
      f"  bwd {t_b[0]:.0f} us [{t_b[1]:.0f}, {t_b[2]:.0f}] = {2.5 * gf / t_b[0] * 1e3:.0f} TFLOP/s (5 GEMMs algorithmic)", flush=True)
