"""Shared by tests/test_gpu_ops.py and tests/golden/make_attn_bitwise_golden.py: the 16 ragged shapes of the flash-attention bitwise check,
their inputs (drawn on the CPU from a seeded generator: the device RNG is no stable source for a golden), one forward / backward through
ops.call, and the sha256 digests that tests/golden/attn_bitwise.json records per shape."""
import functools
import hashlib
import json
import os

import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn_bitwise.json")
# (B, N, nH, T): one ragged tile, exact tiles, one row past a tile / a 128-row block, T = 0 and T = 16, the headline and the long sequence
SHAPES = [(2, 30, 2, 3), (1, 64, 1, 0), (3, 65, 2, 6), (2, 96, 1, 2), (2, 97, 1, 2), (2, 150, 2, 6), (1, 257, 2, 6), (2, 1030, 16, 6),
          (1, 8194, 4, 6), (1, 128, 3, 6), (1, 129, 3, 0), (3, 1030, 16, 6), (2, 1056, 16, 6), (2, 1057, 8, 0), (1, 192, 2, 16), (8, 257, 4, 6)]
FIELDS = ("out", "rawlog", "lse", "dqkv", "stat")


def shape_id(shape):
    return "B%d_N%d_H%d_T%d" % shape


def digest(t):
    """sha256 over the raw bytes of a tensor (None: no such output, e.g. rawlog with T = 0)"""
    if t is None:
        return None
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def make_inputs(shape, device):
    """qkv (x 1.5), dout (both bf16) and drawlog (x 0.01, fp32; None with T = 0)"""
    B, N, nH, T = shape
    g = torch.Generator().manual_seed(7919 * SHAPES.index(shape) + N)
    qkv = (torch.randn(B * N, 3 * nH * 64, generator=g) * 1.5).to(torch.bfloat16)
    dout = torch.randn(B * N, nH * 64, generator=g).to(torch.bfloat16)
    drawlog = torch.randn(B, nH, T, N, generator=g) * 0.01 if T else None
    return qkv.to(device), dout.to(device), None if drawlog is None else drawlog.to(device)


def inputs_digest(inputs):
    h = hashlib.sha256()
    for t in inputs:
        h.update((digest(t) or "-").encode())
    return h.hexdigest()


def forward(shape, inputs):
    """-> (out, rawlog or None, lse)"""
    from mtt_amd import ops
    B, N, nH, T = shape
    return ops.attention(inputs[0], B, N, nH, T, ops.Prec("bf16"), want_lse=True)


def backward(shape, inputs, fwd):
    """-> (dqkv, stat), both filled with NaN before the call: a value the kernels leave unwritten shows as non-finite"""
    from mtt_amd import ops
    B, N, nH, T = shape
    qkv, dout, drawlog = inputs
    out, _, lse = fwd
    dqkv = torch.full_like(qkv, float("nan"))
    stat = torch.full((B, nH, 2, (N + 3) // 4 * 4), float("nan"), device=qkv.device)
    ops.call("attn_bwd", qkv=qkv, out=out, rawlog=None, lse=lse, B=B, N=N, nH=nH, T=T, dtype=1, prec=0, scale=0.125,
             xargs=[dout, drawlog, dqkv, stat])
    return dqkv, stat


def digests(fwd, bwd):
    return dict(zip(FIELDS, (digest(t) for t in tuple(fwd) + tuple(bwd))))


@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN) as f:
        return json.load(f)
