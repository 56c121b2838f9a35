"""-m gpu: the FCOS3D criterion (det_model.DetModel, csrc/det_loss3d.hip) against the unmodified reference (tests/golden/fcos3d.*,
make_fcos3d_golden.py) and the plain-torch restatement tests/fcos3d_ref.py: labels bit for bit, the eight components, loss_sum, every map
gradient, the mini_det head chain, run-to-run bitwise reproducibility, no host synchronisation, FusedMultiTaskLoss with '3ddet', and
the cs geometry, more than 128 gts per image."""
import json
import os

import numpy as np
import pytest
import torch

import conftest
import det_ref
import fcos3d_ref
import train_check
from tests.golden import make_fcos3d_golden as mfg

DEV = "cuda:0"


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _fixture():
    with open(os.path.join(conftest.GOLDEN, "fcos3d.json")) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(conftest.GOLDEN, "fcos3d.npz"))


def _crit(meta):
    import mtt_amd
    return mtt_amd.det_model.DetModel(**json.loads(json.dumps(meta["params"])))


def _preds(arrs, name, L, requires_grad=True):
    flat = [torch.from_numpy(arrs[f"{name}/pred{j}"]).to(DEV).requires_grad_(requires_grad) for j in range(4 * L)]
    return flat, [flat[k * L:(k + 1) * L] for k in range(4)]


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-30)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["a", "b", "d"])
def test_targets_match_the_reference_fixture(name):
    _need_gpu()
    meta, arrs = _fixture()
    c = meta["cases"][name]
    crit = _crit(meta)
    labels = mfg.load_labels(arrs, name, c["B"])
    keep = [i for i in range(c["B"]) if int(labels["det_label_number"][i]) != 0]
    dl = [labels["det_labels"][i] for i in keep]
    pts = crit.get_points([tuple(l) for l in c["levels"]], torch.float32, DEV)
    lab, tgt, ctr = crit.get_targets(pts, [e["bbox_modal"] for e in dl], [e["label"] for e in dl],
                                     [torch.cat([e["center_S"], e["size_S"], e["rotation_S"]], 1) for e in dl], [e["label"] for e in dl],
                                     [e["center_I"][:, :2] for e in dl], [e["center_I"][:, 2] for e in dl])
    lab, tgt, ctr = torch.cat(lab).cpu(), torch.cat(tgt).cpu(), torch.cat(ctr).cpu()
    ref = torch.from_numpy(arrs[f"{name}/labels"].astype(np.int64))
    assert torch.equal(lab, ref), int((lab != ref).sum())
    pos = lab < 6
    assert int(pos.sum()) == c["num_pos"]
    if name != "d":
        rt, rc = torch.from_numpy(arrs[f"{name}/pos_targets"]), torch.from_numpy(arrs[f"{name}/pos_ctr"])
        worst = lambda a, r: float(((a - r).abs() / r.abs().clamp(min=1e-6)).max()) if r.numel() else 0.0
        assert worst(tgt[pos], rt) <= 1e-6 and worst(ctr[pos], rc) <= 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_losses_and_gradients_match_the_reference_fixture(name):
    _need_gpu()
    meta, arrs = _fixture()
    c = meta["cases"][name]
    L = len(c["levels"])
    crit = _crit(meta)
    labels = mfg.load_labels(arrs, name, c["B"])
    flat, preds = _preds(arrs, name, L)
    ld, ls = crit.loss(preds, labels)
    assert sorted(ld) == sorted(c["loss"])
    for k, v in ld.items():
        ref = c["loss"][k]
        assert (float(v) == 0.0) if ref == 0.0 else _rel(float(v), ref) < 1e-5, (k, float(v), ref)
    assert _rel(float(ls), c["loss_sum"]) < 1e-5 if c["loss_sum"] else float(ls) == 0.0
    grads = torch.autograd.grad(ls, flat, retain_graph=bool(ld))
    for j, g in enumerate(grads):
        ref = torch.from_numpy(arrs[f"{name}/grad{j}"])
        g = g.cpu()
        assert float((g - ref).abs().max()) <= 1e-5 * max(float(ref.abs().max()), 1e-30), j
        if name == "a":
            assert not g[1].any(), "the unlabelled image must get zero gradient"
        if name == "c" or (name == "b" and j >= L):
            assert not g.any(), j
    if name == "a":                                           # backprop of one component
        grads = torch.autograd.grad(ld["loss_rotsin"], flat)
        for j, g in enumerate(grads):
            ref = torch.from_numpy(arrs[f"a/grad_rotsin{j}"])
            assert float((g.cpu() - ref).abs().max()) <= 1e-5 * max(float(ref.abs().max()), 1e-30), j


FIXTURE_GRAD_TOL = {"x3": 2.5e-2, "x3f": 0.15}                # the bounds test_gpu_det_head.py uses for the mini_det head


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["x3", "x3f", "bf16"])
def test_mini_det_head_chain_matches_the_reference_fixture(prec):
    """the HIP FCOS3DHead (mini_det weights and inputs) -> DetModel.loss -> backward, against the reference head + reference criterion:
    the components, and per head parameter the norm and a fixed random projection of d loss_sum / d parameter"""
    _need_gpu()
    import mtt_amd
    from tests.golden import make_det_golden as mdg
    meta, arrs = _fixture()
    c = meta["cases"]["d"]
    _, harr = conftest.load_golden("mini_det")
    torch.manual_seed(0)
    head = mtt_amd.det_head.FCOS3DHead(**det_ref.mini_head_params())
    head.init_weights()
    det_ref.randomize(head, 0)
    head.set_prec(prec)
    head = head.to(DEV)
    feats = [torch.from_numpy(np.asarray(harr[f"in{i}"])).to(DEV) for i in range(4)]
    ld, ls = _crit(meta).loss(head(feats), mfg.load_labels(arrs, "d", c["B"]))
    worst = max(_rel(float(v), c["loss"][k]) for k, v in ld.items())
    ls.backward()
    stats = mdg.grad_stats((k, p.grad.detach().cpu()) for k, p in head.named_parameters())
    ref = {k: tuple(v) for k, v in c["grad_stats"].items()}
    top = max(ref[k][0] / p.numel() ** 0.5 for k, p in head.named_parameters())
    errs = {}
    for k, p in head.named_parameters():
        n_ref, pr_ref = ref[k]
        if n_ref / p.numel() ** 0.5 < train_check.PER_PARAM["bf16"]["floor"] * top:
            continue
        n, pr = stats[k]
        errs[k] = max(abs(n - n_ref), abs(pr - pr_ref)) / n_ref
    wk = max(errs, key=errs.get)
    print(f"mini_det head -> DetModel.loss {prec}: worst component rel err {worst:.3e}; {len(errs)} parameters, worst gradient error "
          f"{errs[wk]:.3e} ({wk})")
    if prec in FIXTURE_GRAD_TOL:
        assert worst < 1e-3, worst
        assert errs[wk] < FIXTURE_GRAD_TOL[prec], (wk, errs[wk])
    else:
        # bf16: measured and reported, bounded by direction (the cosine of the gradient projections over the checked parameters)
        v = np.array([stats[k][1] for k in errs])
        r = np.array([ref[k][1] for k in errs])
        cos = float(v @ r / (np.linalg.norm(v) * np.linalg.norm(r)))
        print(f"mini_det head -> DetModel.loss bf16: projection cosine {cos:.4f}")
        assert cos > 0.8, cos


CS_LEVELS = ((96, 192), (48, 96), (24, 48), (24, 48), (12, 24))


def _cs_case(B, seed=0, n_gts=40):
    import mtt_amd
    dm = mtt_amd.det_model
    p = {"IMAGE_ORI_SIZE": (1024, 2048), "TRAIN": {"SCALE": (1024, 2048)}, "img_ds_ratio": 0.75}
    dm.configure_3ddet(p)
    labels = dm.synthetic_det_labels(B, (1024, 2048), n_gts, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    preds = [[(torch.randn(B, ch, h, w, generator=g) * (2.0 if k == 0 else 1.0)).to(DEV) for h, w in CS_LEVELS]
             for k, ch in enumerate((6, 13, 6, 1))]
    return p, labels, preds


@pytest.mark.gpu
def test_cs_geometry_matches_the_restatement():
    """five levels 96x192 ... 12x24, strides [8, 16, 32, 32, 64] / 0.75, B = 2, 40 gts per image: labels identical to the fp32
    restatement, components within 1e-5 of its fp64 losses"""
    _need_gpu()
    p, labels, preds = _cs_case(2)
    crit = p["detmodel"]
    ld, ls = crit.loss(preds, labels)
    keep, lab, _, _ = fcos3d_ref.assign(p["det_model_params"], labels, CS_LEVELS)
    pts = crit.get_points(CS_LEVELS, torch.float32, DEV)
    dl = labels["det_labels"]
    glab, _, _ = crit.get_targets(pts, [e["bbox_modal"] for e in dl], [e["label"] for e in dl],
                                  [torch.cat([e["center_S"], e["size_S"], e["rotation_S"]], 1) for e in dl], [e["label"] for e in dl],
                                  [e["center_I"][:, :2] for e in dl], [e["center_I"][:, 2] for e in dl])
    offs = np.cumsum([0] + [h * w for h, w in CS_LEVELS])
    ref = torch.cat([lab[:, offs[l]:offs[l + 1]].reshape(-1) for l in range(5)])
    assert torch.equal(torch.cat(glab).cpu(), ref)
    num_pos = int((ref < 6).sum())
    assert num_pos > 100
    rd, rs = fcos3d_ref.loss(p["det_model_params"], [[m.cpu() for m in lst] for lst in preds], labels)
    for k in rd:
        assert _rel(float(ld[k]), float(rd[k])) < 1e-5, (k, float(ld[k]), float(rd[k]))
    assert _rel(float(ls), float(rs)) < 1e-5
    print(f"cs geometry B=2: num_pos {num_pos}, " + ", ".join(f"{k} {float(v):.4f}" for k, v in ld.items()))


MANY_LEVELS = ((12, 20), (6, 10), (3, 5))


@pytest.mark.gpu
def test_more_than_128_gts_per_image_match_the_restatement():
    """fcos3d_fwd_kernel stages the gts in LDS 128 at a time: 128 (one full batch), 129 (a one-gt second batch) and 300 gts (three batches,
    ragged last) on three small levels, B = 3.  Labels identical to the fp32 restatement, components and loss_sum within 1e-5 of its fp64
    losses (the cs-geometry bound), every map gradient within 1e-5 * max|ref| of its fp64 autograd (the fixture test's bound)."""
    _need_gpu()
    import mtt_amd
    dm = mtt_amd.det_model
    params = dm.cs_det_model_params()
    params.update(strides=[8, 16, 32], regress_ranges=((-1, 48), (48, 96), (96, dm.INF)))
    p = {"IMAGE_ORI_SIZE": (96, 160), "TRAIN": {"SCALE": (96, 160)}, "img_ds_ratio": 1.0}
    dm.configure_3ddet(p, params)
    crit, B = p["detmodel"], 3
    labels = dm.synthetic_det_labels(B, (96, 160), (128, 129, 300), seed=9)
    g = torch.Generator().manual_seed(10)
    preds = [[(torch.randn(B, ch, h, w, generator=g) * (2.0 if k == 0 else 1.0)) for h, w in MANY_LEVELS] for k, ch in enumerate((6, 13, 6, 1))]
    dists = []
    keep, lab, _, _ = fcos3d_ref.assign(p["det_model_params"], labels, MANY_LEVELS, dists_out=dists)
    assert keep == [0, 1, 2] and [d.shape[1] for d in dists] == [128, 129, 300]
    for d in dists:                                            # no point has two gts at its minimum distance: the argmin is unambiguous
        two = torch.topk(d, 2, dim=1, largest=False)[0]
        assert bool(((two[:, 0] < two[:, 1]) | (two[:, 0] == fcos3d_ref.INF)).all())
    pts = crit.get_points(MANY_LEVELS, torch.float32, DEV)
    dl = labels["det_labels"]
    glab, _, _ = crit.get_targets(pts, [e["bbox_modal"] for e in dl], [e["label"] for e in dl],
                                  [torch.cat([e["center_S"], e["size_S"], e["rotation_S"]], 1) for e in dl], [e["label"] for e in dl],
                                  [e["center_I"][:, :2] for e in dl], [e["center_I"][:, 2] for e in dl])
    offs = np.cumsum([0] + [h * w for h, w in MANY_LEVELS])
    ref = torch.cat([lab[:, offs[l]:offs[l + 1]].reshape(-1) for l in range(len(MANY_LEVELS))])
    assert torch.equal(torch.cat(glab).cpu(), ref), int((torch.cat(glab).cpu() != ref).sum())
    num_pos = int((ref < 6).sum())
    assert num_pos > 0
    leaves = [[m.to(DEV).requires_grad_(True) for m in lst] for lst in preds]
    ld, ls = crit.loss(leaves, labels)
    rleaves = [[m.double().requires_grad_(True) for m in lst] for lst in preds]
    rd, rs = fcos3d_ref.loss(p["det_model_params"], rleaves, labels)
    for k in rd:
        assert _rel(float(ld[k]), float(rd[k])) < 1e-5, (k, float(ld[k]), float(rd[k]))
    assert _rel(float(ls), float(rs)) < 1e-5
    grads = torch.autograd.grad(ls, [m for lst in leaves for m in lst])
    rgrads = torch.autograd.grad(rs, [m for lst in rleaves for m in lst])
    for j, (gg, rg) in enumerate(zip(grads, rgrads)):
        assert float((gg.cpu().double() - rg).abs().max()) <= 1e-5 * max(float(rg.abs().max()), 1e-30), j
    print(f"3 levels, gts (128, 129, 300): num_pos {num_pos}")


@pytest.mark.gpu
def test_two_runs_are_bitwise_equal():
    _need_gpu()
    p, labels, preds = _cs_case(2, seed=4)
    runs = []
    for _ in range(2):
        leaves = [[m.clone().requires_grad_(True) for m in lst] for lst in preds]
        ld, ls = p["detmodel"].loss(leaves, labels)
        ls.backward()
        runs.append([torch.stack(list(ld.values())), ls.detach()] + [m.grad.clone() for lst in leaves for m in lst])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_forward_and_backward_do_not_synchronise_with_the_host():
    _need_gpu()
    p, labels, preds = _cs_case(2, seed=5)
    crit = p["detmodel"]
    leaves = [[m.clone().requires_grad_(True) for m in lst] for lst in preds]
    packed = crit.pack_labels(labels, DEV)
    crit.loss(leaves, packed)[1].backward()              # warm-up: the kernel workspace is sized outside the checked region
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ld, ls = crit.loss(leaves, packed)
        ls.backward()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert torch.isfinite(ls).item()


@pytest.mark.gpu
def test_fused_multitask_loss_with_3ddet():
    """['semseg', 'depth', '3ddet'] with weights {100, 1, 1}: the reference scheme's keys (loss_schemes.py:27-39) and total = the
    weighted sum"""
    _need_gpu()
    import mtt_amd
    p, labels, preds = _cs_case(1, seed=6)
    P = mtt_amd.factory.AttrDict(ignore_index=255, detmodel=p["detmodel"], TASKS=dict(NAMES=['semseg', 'depth'], NUM_OUTPUT=dict(semseg=19, depth=1)))
    crit = mtt_amd.losses.FusedMultiTaskLoss(P, ['semseg', 'depth', '3ddet'], {'semseg': 100.0, 'depth': 1.0, '3ddet': 1.0})
    gt = mtt_amd.losses.synthetic_targets(P, 1, 32, 64, DEV)
    gt.update(labels)
    pred = {'semseg': torch.randn(1, 19, 32, 64, device=DEV), 'depth': torch.rand(1, 1, 32, 64, device=DEV) * 5, '3ddet': preds}
    out = crit(pred, gt)
    keys = ['semseg', 'depth', '3ddet', 'loss_cls', 'loss_offset', 'loss_depth', 'loss_size', 'loss_rotsin', 'loss_dir', 'loss_centerness',
            'loss_bbox2d', 'total']
    assert list(out) == keys
    want = 100.0 * float(out['semseg']) + float(out['depth']) + float(out['3ddet'])
    assert _rel(float(out['total']), want) < 1e-6
    ld, ls = p["detmodel"].loss(preds, labels)
    assert float(out['3ddet']) == float(ls)


# ---- every component on its own, under the cs and the alt parameter set and on a batch without gts ------------------------------------------
def _alt_fixture():
    with open(os.path.join(conftest.GOLDEN, "fcos3d_alt.json")) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(conftest.GOLDEN, "fcos3d_alt.npz"))


def _forward(crit, labels, maps, call):
    """fcos3d_loss_fwd as _DetLossFn.forward launches it, through `call` (the device's ops.call or the emulator) -> (out [9], stats [2])"""
    import mtt_amd
    dev = maps[0].device
    L = len(maps) // 4
    packed = crit.pack_labels(labels, dev)
    geo = crit._geometry([tuple(m.shape[-2:]) for m in maps[:L]])
    P, n = geo["P"], packed.n_lab
    label = torch.full((n, P), -7, dtype=torch.int32, device=dev)
    target, ctr = torch.full((n, 13, P), 7.0, device=dev), torch.full((n, P), 7.0, device=dev)
    out, stats = torch.full((9,), 7.0, device=dev), torch.full((2,), 7.0, device=dev)
    kw = crit._desc(geo, packed, label, target, ctr)
    kw.update(cls=list(maps[:L]), bbox=list(maps[L:2 * L]), dir=list(maps[2 * L:3 * L]), ctr=list(maps[3 * L:]), out=out, stats=stats)
    if dev.type == "cuda":
        kw["ws"] = mtt_amd.ops.ws_for("fcos3d", dev, P=P, n_lab=n)
    call("fcos3d_loss_fwd", **kw)
    return out.cpu(), stats.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["cs", "alt", "zero_gt"])
def test_each_component_matches_its_reference(which):
    """out[9] spans a factor of 60 between loss_cls and loss_offset, so compare's rms-relative element bound is loose for the small
    components: each of the nine values within 1e-5 relative (the existing component bound, about 150 x the fp32 reference's own 6e-8
    distance from fp64) of the reference fixture (cs: fcos3d.* a; alt: fcos3d_alt.* a), or of the fp64 emulator on a batch whose labelled
    images have no gts (the reference cannot run those); exact zeros exactly zero; stats exact."""
    _need_gpu()
    import mtt_amd
    from oracle import abi_emul
    if which == "zero_gt":
        meta, _ = _alt_fixture()
        crit = _crit(meta)
        levels = ((10, 20), (5, 10), (3, 5), (3, 5), (2, 3))
        labels = mtt_amd.det_model.synthetic_det_labels(3, (110, 215), [0, 4, 0], num_classes=3, unlabelled=(1,), seed=2)
        g = torch.Generator().manual_seed(21)
        maps = [torch.randn(3, ch, h, w, generator=g) * (2.0 if k == 0 else 1.0) for k, ch in enumerate((3, 13, 6, 1)) for h, w in levels]
        ref, rstats = _forward(crit, labels, maps, abi_emul.call)
        ref, num_pos, n_lab = ref.double().tolist(), 0, 2
        assert rstats.tolist() == [0.0, 2.0] and ref[0] > 0 and not any(ref[1:8])
    else:
        meta, arrs = _fixture() if which == "cs" else _alt_fixture()
        c = meta["cases"]["a"]
        crit = _crit(meta)
        labels = mfg.load_labels(arrs, "a", c["B"])
        maps = [torch.from_numpy(arrs[f"a/pred{j}"]) for j in range(4 * len(c["levels"]))]
        ref = [c["loss"][k] for k in fcos3d_ref.KEYS] + [c["loss_sum"]]
        num_pos, n_lab = c["num_pos"], 2
    out, stats = _forward(crit, labels, [m.to(DEV) for m in maps], mtt_amd.ops.call)
    for i, r in enumerate(ref):
        got = float(out[i])
        print(f"{which} out[{i}]: device {got!r} reference {r!r} rel {_rel(got, r) if r else 0.0:.2e}")
    for i, r in enumerate(ref):
        got = float(out[i])
        assert (got == 0.0) if r == 0.0 else _rel(got, r) <= 1e-5, (i, got, r)
    assert stats.tolist() == [float(num_pos), float(num_pos + n_lab)]


@pytest.mark.gpu
def test_alt_weighted_gradient_matches_the_reference_per_element():
    """d (sum_i w_i * component_i + w_8 * loss_sum) / d every map under the alt set, nine distinct w: every element within
    1e-4 * rms(reference map) + 4 fp32 ulps (gpu_cases.compare's rule at TOL_ROW) of the unmodified reference's gradient"""
    _need_gpu()
    import mtt_amd
    import gpu_cases
    meta, arrs = _alt_fixture()
    c = meta["cases"]["a"]
    L = len(c["levels"])
    crit = _crit(meta)
    flat, preds = _preds(arrs, "a", L)
    ld, ls = crit.loss(preds, mfg.load_labels(arrs, "a", c["B"]))
    w = meta["gout"]
    total = sum(w[i] * ld[k] for i, k in enumerate(fcos3d_ref.KEYS)) + w[8] * ls
    grads = torch.autograd.grad(total, flat)
    worst = 0.0
    for j, g in enumerate(grads):
        ref = torch.from_numpy(arrs[f"a/grad{j}"]).double().reshape(-1)
        r, _ = gpu_cases._elem_ratio(g.cpu().double().reshape(-1), ref, 10 * gpu_cases.TOL_ROW["f32"], False)
        worst = max(worst, float(r.max()))
        assert float(r.max()) <= 1.0, (j, float(r.max()))
        assert not g[1].any(), "the unlabelled image must get zero gradient"
    print(f"alt weighted gradient: worst element error / bound {worst:.3e}")


def _parity_forward_cases():
    import gpu_cases
    return [f"fcos3d_loss_fwd_{b[0]}" for b in gpu_cases.FCOS3D_BATCHES if not b[8]]


@pytest.mark.gpu
@pytest.mark.parametrize("name", _parity_forward_cases())
def test_parity_case_components_match_the_emulator_individually(name):
    """the forward parity cases of gpu_cases.fcos3d_cases() without saturated logits (gamma 1, 1 and 10 classes, one and eight levels,
    images without gts, 128 / 129 / 257 gts): compare's element bound on `out` is relative to the rms of all nine values, which loss_cls
    dominates, so here each component is held to 1e-5 relative of the fp64 emulator (the component bound of the tests above), exact zeros
    exactly zero, stats exact"""
    _need_gpu()
    import gpu_cases
    import mtt_amd
    from oracle import abi_emul
    kw = next(c[2] for c in gpu_cases.fcos3d_cases() if c[0] == name)
    ekw, _ = gpu_cases.clone_storages(kw)
    abi_emul.call("fcos3d_loss_fwd", **ekw)
    dev = lambda v: v.to(DEV).contiguous() if isinstance(v, torch.Tensor) else v
    gkw = {k: [dev(a) for a in v] if isinstance(v, (list, tuple)) else dev(v) for k, v in kw.items()}
    gkw["ws"] = mtt_amd.ops.ws_for("fcos3d", torch.device(DEV), P=kw["P"], n_lab=kw["n_lab"])
    mtt_amd.ops.call("fcos3d_loss_fwd", **gkw)
    out, ref = gkw["out"].cpu().double(), ekw["out"].double()
    for i in range(9):
        got, r = float(out[i]), float(ref[i])
        print(f"{name} out[{i}]: device {got!r} emulator {r!r} rel {_rel(got, r) if r else 0.0:.2e}")
    for i in range(9):
        got, r = float(out[i]), float(ref[i])
        assert (got == 0.0) if r == 0.0 else _rel(got, r) <= 1e-5, (i, got, r)
    assert torch.equal(gkw["stats"].cpu(), ekw["stats"])
