"""-m gpu: the flash attention backward on the shapes at which its peeled tile loop, the stat values moved into the tile's LDS-DMA and the
D computed inside the dQ kernel can go wrong, against the fp64 emulator (every output judged, stat included, plus the untouched-memory
check of gpu_cases.run_case), and its run-to-run repeatability (a wait that is too weak shows as differences between launches)."""
import pytest
import torch

import gpu_cases
from oracle import abi_emul

# (B, N, nH, T): what the shape catches
SHAPES = [
    (1, 30, 2, 4),     # one tile, first and ragged at once
    (2, 64, 1, 3),     # one full tile, first = last
    (3, 65, 2, 6),     # ragged tile with one row, empty second half, Np padding of 3
    (2, 96, 1, 2),     # ragged tile ending at a half
    (2, 97, 1, 2),     # ragged tile ending just past a half
    (1, 128, 3, 6),    # two full tiles, a full query block
    (1, 129, 3, 0),    # odd tile count, a second block of one row with three inactive waves, no drawlog
    (1, 192, 2, 16),   # three full tiles, T at its maximum
    (1, 257, 2, 6),    # five tiles, both stages, ragged end
]


def _case(B, N, nH, T, seed):
    """inputs as gpu_cases.attn_cases() builds them: out / lse from the fp64 emulator of the forward"""
    g = torch.Generator().manual_seed(seed)
    C = nH * 64
    qkv = gpu_cases.rnd(g, B * N, 3 * C, dtype=torch.bfloat16)
    fw = dict(qkv=qkv, out=torch.zeros(B * N, C, dtype=torch.bfloat16), rawlog=None, lse=torch.zeros(B, nH, N), B=B, N=N, nH=nH, T=0,
              dtype=1, prec=0, scale=0.125)
    abi_emul.call("attn_fwd", **fw)
    return dict(qkv=qkv, out=fw["out"], rawlog=None, lse=fw["lse"], B=B, N=N, nH=nH, T=T, dtype=1, prec=0, scale=0.125,
                xargs=[gpu_cases.rnd(g, B * N, C, dtype=torch.bfloat16), gpu_cases.rnd(g, B, nH, T, N) * 0.05 if T else None,
                       torch.zeros(B * N, 3 * C, dtype=torch.bfloat16), torch.zeros(B, nH, 2, (N + 3) // 4 * 4)])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=["B%dN%dH%dT%d" % s for s in SHAPES])
def test_attn_bwd_tile_kinds_match_emulator(shape):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    B, N, nH, T = shape
    r = gpu_cases.run_case("attn_bwd", _case(B, N, nH, T, 100 + N), None, gpu_cases.TOL_ATTN_BWD)
    print(shape, r["errs"])
    assert r["ok"], r["errs"]


@pytest.mark.gpu
def test_attn_bwd_is_repeatable():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    B, N, nH, T = 8, 257, 4, 6
    lib = gpu_cases.pkg()._lib
    kw = _case(B, N, nH, T, 7)
    dev = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in kw.items() if k != "xargs"}
    dout, drawlog = kw["xargs"][0].cuda(), kw["xargs"][1].cuda()
    runs = []
    for _ in range(5):
        dqkv = torch.full((B * N, 3 * nH * 64), float("nan"), dtype=torch.bfloat16, device="cuda")
        stat = torch.full((B, nH, 2, (N + 3) // 4 * 4), float("nan"), device="cuda")
        lib.call("attn_bwd", **dev, xargs=[dout, drawlog, dqkv, stat])
        torch.cuda.synchronize()
        runs.append((dqkv, stat))
    assert bool(torch.isfinite(runs[0][0].float()).all()) and bool(torch.isfinite(runs[0][1]).all())
    for i, (dqkv, stat) in enumerate(runs[1:], 1):
        assert torch.equal(dqkv, runs[0][0]), f"dqkv of launch {i} differs from launch 0"
        assert torch.equal(stat, runs[0][1]), f"stat of launch {i} differs from launch 0"
