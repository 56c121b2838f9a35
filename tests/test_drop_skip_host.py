"""Host side of DropPath work skipping: the call sites hand the branch's table to the calls that may skip and to no others, and — through the
CPU emulator, which ignores the table and computes the unskipped values — a training step is the same with the switch on and off."""
import ctypes

import pytest
import torch

from oracle import abi_emul
from test_gpu_drop_skip import assert_steps_equal, drop_override, model_step

DEPTH, C, HIDDEN = 4, 128, 512         # the `tiny` backbone of mini_ctr: 4 blocks, 128 channels, MLP 4 x


def _recording(seen):
    def call(name, **kw):
        seen.append((name, kw))
        return abi_emul.call(name, **kw)
    return call


def test_descriptor_mirrors_carry_the_skip_fields_at_abi_17():
    import mtt_amd
    lib = mtt_amd._lib
    assert lib.ABI_VERSION == 17
    g = dict(lib.GemmDesc._fields_)
    assert [n for n, _ in lib.GemmDesc._fields_][-4:] == ["skip_scale", "skip_mb", "skip_prompt", "skip_row0"]
    assert g["skip_scale"] is ctypes.c_void_p and ctypes.sizeof(g["skip_mb"]) == 4 and ctypes.sizeof(g["skip_row0"]) == 8
    assert lib.AttnDesc._fields_[-1][0] == "skip_scale"
    lib.load()                           # the mtt_desc_size handshake: the C structs grew by the same fields


@pytest.mark.parametrize("prec", ["x3f", "bf16"])
def test_emulated_step_is_the_same_with_and_without_the_tables(prec, monkeypatch):
    import mtt_amd
    # the miniature's 128 channels / 60 token rows on the benchmark's backward path: transposed weight packs + token-major weight gradients
    monkeypatch.setattr(mtt_amd.autograd_path, "FAST_MIN_DIM", 64)
    monkeypatch.setattr(mtt_amd.autograd_path, "FAST_MIN_ROWS", 32)
    seen_on, seen_off = [], []
    on = model_step(prec, "cpu", _recording(seen_on), True)
    off = model_step(prec, "cpu", _recording(seen_off), False)
    assert_steps_equal(on, off)
    assert [n for n, _ in seen_on] == [n for n, _ in seen_off], "the switch must not change the launch sequence"
    assert not any("skip_scale" in kw for _, kw in seen_off)

    drop = drop_override()
    tables = [torch.stack([d[2], d[0]], 1) for d in drop] + [torch.stack([d[3], d[1]], 1) for d in drop]
    with_tab = [(n, kw) for n, kw in seen_on if kw.get("skip_scale") is not None]
    gemms = [kw for n, kw in with_tab if n == "gemm"]
    # forward: proj, fc1, fc2 of every block; backward: the input gradient of each of them (the weight gradients run whole)
    fwd = [kw for kw in gemms if kw.get("rowscale") is not None or kw.get("act") in (1, 5)]
    wgrad = [kw for kw in gemms if kw["a_op"] == 1]
    assert (len(fwd), len(wgrad), len(gemms)) == (3 * DEPTH, 0, 6 * DEPTH)
    for kw in gemms:
        assert kw["skip_mb"] == 30 and kw["skip_prompt"] == 6 and kw.get("skip_row0", 0) == 0
        assert 3 * C not in (kw["N"], kw["K"]), "the qkv GEMM and its input gradient stay unskipped"
        tab = kw["skip_scale"]
        assert any(torch.equal(tab, t) for t in tables)
        if kw.get("rowscale") is not None:
            assert kw["rowscale"] is tab
    fwd_ids = {id(kw) for kw in fwd}
    assert sorted((kw["N"], kw["K"]) for kw in gemms if id(kw) not in fwd_ids) == sorted([(C, C), (HIDDEN, C), (C, HIDDEN)] * DEPTH)
    assert sum(n == "attn_fwd" for n, _ in with_tab) == DEPTH
    assert sum(n == "attn_bwd" for n, _ in with_tab) == sum(n == "attn_bwd" for n, _ in seen_on) == DEPTH


def test_nothing_is_skipped_in_eval():
    seen = []
    model_step("x3f", "cpu", _recording(seen), True, training=False)
    assert seen and not any(kw.get("skip_scale") is not None for _, kw in seen)
