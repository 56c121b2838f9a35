"""GPU: the batch augmentation kernels (csrc/augment.hip through mtt_amd.DeviceAugment) against the reference's own transforms
(tests/golden/augment.*) and against the one-pass restatement tests/augment_ref.py that the host suite pins to that fixture.

Every comparison is BITWISE: each step of the pipeline is an integer operation or a single-rounded fp32 operation in a stated order, so
there is no tolerance to choose."""
import itertools
import warnings

import numpy as np
import pytest
import torch

import augment_ref
import conftest
from tests.golden import make_augment_golden as mag

SIZE = (24, 32)


def _need_gpu():
    if not conftest.has_gpu():
        pytest.fail("marked gpu but no HIP device is visible")


def _fixture():
    meta, arrs = conftest.load_golden("augment")
    return meta, arrs, augment_ref.golden_sources(arrs)


def _upload(srcs, u8=False):
    out = []
    for s in srcs:
        d = {k: torch.from_numpy(np.ascontiguousarray(v)).to("cuda:0") for k, v in s.items()}
        d["image"] = d["image"] if u8 else d["image"].float()
        out.append(d)
    return out


def _run(aug, samples, P):
    import mtt_amd
    out = aug(samples, P)
    torch.cuda.synchronize()
    chosen = aug.last_table[:, mtt_amd._lib.AUG_CHOSEN].cpu().tolist()
    return {k: v.cpu().numpy() for k, v in out.items()}, chosen


def _assert_equal(got, want, keys, what):
    for k in keys:
        assert got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        bad = got[k].view(np.int32) != np.ascontiguousarray(want[k], dtype=np.float32).view(np.int32)
        if bad.any():
            at = tuple(int(v) for v in np.argwhere(bad)[0])
            pytest.fail(f"{what}: '{k}' differs in {int(bad.sum())} of {bad.size} values, first at {at}: {got[k][at]!r} vs {want[k][at]!r}")


# ---- 1. the reference's own outputs ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("u8", [False, True], ids=["fp32", "uint8"])
@pytest.mark.parametrize("case", [c["name"] for c in mag.cases()])
def test_matches_the_reference_fixture_bitwise(case, u8):
    """train cases (every switch, both contrast positions, both clips, the hue wrap, scales 0.5 / 1.0 / 1.37 / 2.0, a crop that is no
    multiple of 4 wide) and the valid pipeline: all six tasks and the image, and the crop candidate the reference's loop stopped at"""
    _need_gpu()
    import mtt_amd
    meta, arrs, srcs = _fixture()
    c = next(c for c in meta["cases"] if c["name"] == case)
    aug = mtt_amd.DeviceAugment(meta["tasks"], c["size"], train=c["mode"] == "train")
    P = augment_ref.params_from_rows(c["rows"], meta["shapes"], c["size"], c["mode"])
    got, chosen = _run(aug, _upload(srcs, u8), P)
    keys = ["image"] + meta["tasks"]
    _assert_equal(got, {k: arrs[f"{case}_{k}"] for k in keys}, keys, case)
    assert chosen == c["chosen"]


# ---- 2. parameters beyond the fixture ------------------------------------------------------------------------------------------------------
SWITCHES = {
    "none": dict(),
    "bright_up": dict(bright=32.0), "bright_down": dict(bright=-32.0),
    "contrast_low_first": dict(f_mode=True, contrast=0.5), "contrast_high_last": dict(contrast=1.5),
    "saturation": dict(sat=1.43), "hue_low": dict(hue=-18), "hue_high": dict(hue=17),
    "all_last": dict(bright=-17.5, contrast=1.37, sat=0.55, hue=-11), "all_first": dict(f_mode=True, bright=25.0, contrast=0.64, sat=1.5, hue=13),
}


@pytest.mark.gpu
@pytest.mark.parametrize("size", [SIZE, (24, 30)], ids=["w32_vector", "w30_scalar"])
@pytest.mark.parametrize("switches", list(SWITCHES))
def test_matches_the_restatement_bitwise(switches, size):
    """one batch of 24 samples: the three ragged sources x scales {0.5, 1.0, 1.37, 2.0} x flip off / on, under one setting of the
    photometric switches; uint8 and fp32 image sources must agree with the restatement and so with each other"""
    _need_gpu()
    import mtt_amd
    meta, arrs, srcs = _fixture()
    combos = list(itertools.product(range(3), (0.5, 1.0, 1.37, 2.0), (False, True)))
    rows = [mag.row(s, 50 + n, size=size, shape=meta["shapes"][j], flip=flip, **SWITCHES[switches]) for n, (j, s, flip) in enumerate(combos)]
    batch = [srcs[j] for j, _, _ in combos]
    shapes = [meta["shapes"][j] for j, _, _ in combos]
    aug = mtt_amd.DeviceAugment(meta["tasks"], size)
    P = augment_ref.params_from_rows(rows, shapes, size)
    want, want_chosen = augment_ref.augment_batch(batch, P, aug)
    keys = ["image"] + meta["tasks"]
    for u8 in (False, True):
        got, chosen = _run(aug, _upload(batch, u8), P)
        _assert_equal(got, want, keys, f"{switches} {'uint8' if u8 else 'fp32'}")
        assert chosen == want_chosen
    # what the sources were built to exercise did reach the outputs
    assert (want["normals"] == 255).all(axis=1).any() and (want["depth"] == -1).any()
    parts = want["human_parts"].reshape(len(combos), -1)
    lone = [(p == 255).all() for p in parts]
    assert lone == [j == 1 for j, _, _ in combos], "source 1 has no part label and is ignored as a whole; the others keep theirs"


# ---- 3. crop selection -----------------------------------------------------------------------------------------------------------------------
def _strip(windows):
    """a 24 x (32 * len(windows)) semseg map whose k-th 24 x 32 window holds the given {label: pixel count} (row-major fill)"""
    cols = []
    for counts in windows:
        flat = np.concatenate([np.full(n, lab, np.float32) for lab, n in counts.items()])
        assert flat.size == 24 * 32
        cols.append(flat.reshape(24, 32))
    return np.concatenate(cols, axis=1)[..., None]


FAIL80, PASS, SINGLE, EXACT75 = {1: 615, 2: 153}, {1: 384, 2: 384}, {3: 700, 255: 68}, {4: 576, 5: 192}
SELECT_CASES = {
    "four_fail_then_pass": ([FAIL80] * 4 + [PASS] + [FAIL80] * 6, 4),
    "all_ten_fail": ([FAIL80] * 10 + [PASS], 10),
    "single_class_fails": ([SINGLE, PASS] + [FAIL80] * 9, 1),
    "exactly_three_quarters_fails": ([EXACT75, {4: 575, 5: 193}] + [FAIL80] * 9, 1),
    # window 1: 520 / 668 fails, though 520 / 768 (ignore pixels counted in the sum) would pass
    "ignore_label_is_not_counted": ([{6: 576, 255: 192}, {6: 520, 7: 148, 255: 100}, {6: 400, 7: 168, 255: 200}] + [FAIL80] * 8, 2),
}


@pytest.mark.gpu
def test_crop_selection_picks_what_the_references_loop_would():
    """hand-made maps, candidate k = window k: a class at 80 % fails, a single class (next to ignore pixels) fails, a share of exactly
    0.75 fails (the comparison is strict) while 575 / 768 passes, 255 is left out of the shares; after ten failures the 11th is used"""
    _need_gpu()
    import mtt_amd
    L = mtt_amd._lib
    names = list(SELECT_CASES)
    samples, shapes, rows = [], [], []
    for n in names:
        seg = _strip(SELECT_CASES[n][0])
        H, W = seg.shape[:2]
        samples.append({"image": np.zeros((H, W, 3), np.uint8), "semseg": seg})
        shapes.append((H, W))
        rows.append(dict(mag.row(1.0, 0, shape=(H, W)), cands=[[0, 32 * k] for k in range(11)]))
    aug = mtt_amd.DeviceAugment(["semseg"], SIZE)
    P = augment_ref.params_from_rows(rows, shapes, SIZE)
    want, want_chosen = augment_ref.augment_batch(samples, P, aug)
    assert want_chosen == [SELECT_CASES[n][1] for n in names], "the restatement disagrees with the hand count"
    got, chosen = _run(aug, _upload(samples), P)
    assert dict(zip(names, chosen)) == dict(zip(names, want_chosen))
    _assert_equal(got, want, ["image", "semseg"], "selected crops")
    # cat_max_ratio >= 1: no candidate is tested, candidate 0 is used and CHOSEN stays 0
    free = mtt_amd.DeviceAugment(["semseg"], SIZE, cat_max_ratio=1.0)
    Pf = augment_ref.params_from_rows([dict(r, n_test=0) for r in rows], shapes, SIZE)
    got, chosen = _run(free, _upload(samples), Pf)
    assert chosen == [0] * len(names)
    _assert_equal(got, augment_ref.augment_batch(samples, Pf, free)[0], ["semseg"], "untested crop")
    assert L.AUG_CANDS == 11


# ---- 4. the host check -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_bad_table_row_is_refused_and_nothing_is_launched():
    _need_gpu()
    import mtt_amd
    L = mtt_amd._lib
    meta, arrs, srcs = _fixture()
    depth = [torch.from_numpy(s["depth"]).to("cuda:0") for s in srcs]
    flat = torch.cat([d.reshape(-1) for d in depth])
    P = mtt_amd.AugParams.identity(meta["shapes"])
    good = torch.from_numpy(P.table().copy())
    pixels = [h * w for h, w in meta["shapes"]]
    off_host = torch.tensor([0, pixels[0], pixels[0] + pixels[1]], dtype=torch.int64)
    out = torch.full((3, 1, 64, 56), -7.0, device="cuda:0")

    def call(table_host, off_h=off_host, numel=flat.numel()):
        return L.aug_call("aug_labels", src=flat, src_numel=numel, C=1, off=off_h.to("cuda:0"), off_host=off_h,
                          table=good.to("cuda:0"), table_host=table_host, out=out, B=3, h=64, w=56, kind=L.AUG_DEPTH, fill=0.0, depth_ignore=1)

    for col, val in ((L.AUG_H, 65), (L.AUG_W, 0), (L.AUG_SH, 1 << 20), (L.AUG_CAND_Y + 10, 1), (L.AUG_CAND_X + 2, -3), (L.AUG_CHOSEN, 11), (L.AUG_NTEST, 3)):
        bad = good.clone()
        bad[2, col] = val
        assert call(bad) == L.E_BADARG, col
    assert call(good, off_h=off_host + torch.tensor([0, 0, 1])) == L.E_BADARG, "the last sample would end one element past the buffer"
    assert call(good, off_h=off_host * torch.tensor([1, -1, 1])) == L.E_BADARG
    assert call(good, numel=flat.numel() - 1) == L.E_BADARG
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()), "a refused call wrote to its output"
    assert call(good) == 0
    torch.cuda.synchronize()
    valid = mtt_amd.DeviceAugment(["depth"], (64, 56), train=False)
    want = np.stack([augment_ref.augment_sample(s, P, i, ["depth"], (64, 56), False)[0]["depth"] for i, s in enumerate(srcs)])
    assert augment_ref.bits_equal(out.cpu().numpy(), want) and valid.size == (64, 56)


# ---- 5. reproducible, and no host synchronisation -----------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_call_is_reproducible_and_does_not_synchronise():
    """two calls with one parameter set are bitwise equal (no floating-point atomics; the crop choice is an integer minimum), and a call
    makes no host synchronisation and no device-to-host copy: the tables go up from pinned memory without blocking"""
    _need_gpu()
    import random
    import mtt_amd
    meta, arrs, srcs = _fixture()
    samples = _upload(srcs * 4, u8=True)
    aug = mtt_amd.DeviceAugment(meta["tasks"], SIZE)
    P = aug.draw([s["image"].shape[:2] for s in samples], random.Random(11))
    first = aug(samples, P)                                          # warm-up: library load, pinned allocations
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            second = aug(samples, P)
            third = aug(samples)                                     # its own draw, on the host
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert not [str(w.message) for w in rec if "synchroniz" in str(w.message)]
    torch.cuda.synchronize()
    for k in first:
        assert torch.equal(first[k].view(torch.int32), second[k].view(torch.int32)), k
        assert third[k].shape == first[k].shape and bool(torch.isfinite(third[k]).all())
    want, _ = augment_ref.augment_batch(srcs * 4, P, aug)
    _assert_equal({k: v.cpu().numpy() for k, v in second.items()}, want, list(want), "seeded draw")
