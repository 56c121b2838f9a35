"""-m gpu: the C-ABI entry points of libmtt_hip.so vs the CPU emulator (bit-for-bit identical inputs), every case of
gpu_cases.all_cases(); the entry points without a case are checked by the tests gpu_cases.COVERED_ELSEWHERE names."""
import pytest
import torch

import attn_bitwise_util as abu
import gpu_cases

CASES = gpu_cases.all_cases()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_entry_point_matches_emulator(case):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cname, entry, kw, tol = case
    r = gpu_cases.run_case(entry, kw, None, tol)
    assert r["ok"], f"{cname}: {r['errs']}"


@pytest.mark.gpu
@pytest.mark.parametrize("shape", abu.SHAPES, ids=[abu.shape_id(s) for s in abu.SHAPES])
def test_attention_variants_are_bitwise_identical_and_repeatable(shape):
    """The flash kernels (forward, dQ, dK/dV) on a ragged shape: finite outputs, bitwise equal from run to run (a staging race shows as
    run-to-run differences), and bitwise equal to what the register-staged generation of the kernels, an independently staged
    implementation with the same arithmetic order, wrote for the same inputs (tests/golden/attn_bitwise.json, recorded from it at the
    last commit that had it)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    want = abu.golden()["shapes"][abu.shape_id(shape)]
    inputs = abu.make_inputs(shape, "cuda")
    assert abu.inputs_digest(inputs) == want["inputs"], "the CPU generator no longer draws the inputs the golden was recorded on"
    fwd = abu.forward(shape, inputs)
    for _ in range(4):
        again = abu.forward(shape, inputs)
        assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(fwd, again)), "forward not repeatable"
    bwd = abu.backward(shape, inputs, fwd)
    for _ in range(2):                                      # 3 backward runs in all, each into NaN-filled dqkv and stat
        again = abu.backward(shape, inputs, fwd)
        assert all(torch.equal(a, b) for a, b in zip(bwd, again)), "backward not repeatable"
    for name, t in zip(abu.FIELDS, tuple(fwd) + tuple(bwd)):
        assert t is None or bool(torch.isfinite(t.float()).all()), f"{name} not finite"
    got = abu.digests(fwd, bwd)
    assert got == {k: want[k] for k in abu.FIELDS}, {k: (got[k], want[k]) for k in abu.FIELDS if got[k] != want[k]}


@pytest.mark.gpu
def test_segcopy_packs_refresh_and_gradient_scatter_on_device():
    """mtt_segcopy on the GPU: every persistent pack layout (casts, hi/lo planes, tap-major conv matrices, padded concatenations, LDS-tiled
    transposes), the one-launch refresh after a parameter update and the gradient scatter, bit-exact against plain torch re-layouts."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pack_check
    pack_check.check_packs("cuda")
    pack_check.check_pitch_key("cuda")
    pack_check.check_refresh("cuda")
    pack_check.check_unpack("cuda")
