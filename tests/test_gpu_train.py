"""-m gpu: one training step (forward + hand-written backward through the C ABI) vs the oracle's autograd."""
import pytest
import torch

import train_check


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mini_ctr", "mini_win", "mini_deconv", "mini_skip"])
def test_gradients_x3(name):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    fwd, errs = train_check.grad_errors(name, "x3", "cuda")
    assert max(fwd.values()) < 1e-3
    worst, med = train_check.summarize(errs)
    assert worst[0] < 1e-2 and med < 1e-3, (worst, med)     # tolerance: 1e-3 typical, 1e-2 on the smallest gradients


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mini_ctr", "mini_win", "mini_deconv"])
def test_gradients_bf16_are_bf16_accurate(name):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    fwd, errs = train_check.grad_errors(name, "bf16", "cuda")
    assert max(fwd.values()) < 4e-2
    worst, med = train_check.summarize(errs, floor=1e-4)
    assert med < 6e-2, (worst, med)
    train_check.assert_per_param(errs, "bf16")              # EVERY parameter, not the median (bounds: train_check.PER_PARAM)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mini_ctr", "mini_win", "mini_deconv", "mini_p32", "mini_skip"])
def test_gradients_x3f_forward_exact_backward_bf16(name):
    """x3f: the forward is the x3 arithmetic (1e-3 per head; split planes through the LDS-DMA kernel for the encoder Linears), the
    backward is bf16 on the hi planes — gradients are bf16-accurate, computed from fp32-class activations."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    fwd, errs = train_check.grad_errors(name, "x3f", "cuda")
    assert max(fwd.values()) < 1e-3, fwd
    worst, med = train_check.summarize(errs, floor=1e-4)
    assert med < 3e-2, (worst, med)
    # the DEFAULT mode's backward bounded per parameter: cosine >= 0.999 with the oracle's autograd or relative error <= 0.15 for every
    # parameter above the norm floor, none beyond 0.2 (train_check.PER_PARAM) — this is what executes ConvHeadFn / FuseTailFn /
    # TaskHeadsFn with bf16 gradient maps, which the x3 case above does not
    train_check.assert_per_param(errs, "x3f")


@pytest.mark.gpu
def test_invpt_x3f_runs_and_matches_forward():
    """InvPT under x3f: ViT encoder on split planes, decoder Linears whose width is not a multiple of 64 fall back to the register-staged
    x3 kernels; bf16 backward everywhere."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    fwd, errs, dead = train_check.invpt_grad_errors("mini8", "x3f", "cuda")
    assert max(fwd.values()) < 1e-3, fwd
    worst, med = train_check.summarize(errs, floor=1e-4)
    assert med < 2e-1, (worst, med)
    train_check.assert_per_param(errs, "x3f")


def _two_steps_bitwise(cfg, prec, B, kind):
    """Two training iterations (forward, fused criterion, backward, clip + Adam) from the SAME state on the same batch: every gradient
    and every updated parameter must be bitwise equal — no fp32 atomics anywhere on the path (since ABI 6: every cross-workgroup reduction
    sums caller-owned partials in a fixed order)."""
    import conftest
    import mtt_amd
    from oracle import weights
    if kind == "IP":
        import train_check
        train_check.skip_unless_own_pitch(cfg)
    model = conftest.build_product_model(cfg, prec, "cuda")
    contract = [(k, list(v.shape)) for k, v in model.state_dict().items()]
    sd = {k: v.cuda() for k, v in weights.synth_state_dict(contract, 0).items()}
    p = model.backbone.p if kind == "TP" else model.p
    crit = mtt_amd.losses.FusedMultiTaskLoss(p, p.TASKS.NAMES).cuda()
    H, W = cfg["img_size"]
    x = weights.synth_images(B, cfg["img_size"], 2).cuda()
    gt = mtt_amd.losses.synthetic_targets(p, B, H, W, "cuda", seed=1)
    runs = []
    for _ in range(2):
        model.load_state_dict(sd, strict=True)
        model.train()
        opt = mtt_amd.optim.FusedClipAdam(model.parameters(), lr=1e-3, weight_decay=1e-6, max_norm=1.0)
        loss = crit(model(x), gt)["total"]
        opt.zero_grad(set_to_none=True)
        loss.backward()
        grads = {k: v.grad.detach().clone() for k, v in model.named_parameters() if v.grad is not None}
        norm = opt.step()
        torch.cuda.synchronize()
        runs.append((float(loss.detach()), grads, {k: v.detach().clone() for k, v in model.named_parameters()}, norm.clone()))
    (l0, g0, p0, n0), (l1, g1, p1, n1) = runs
    assert l0 == l1
    assert bool(torch.equal(n0, n1))
    bad = [k for k in g0 if not torch.equal(g0[k], g1[k])] + [k for k in p0 if not torch.equal(p0[k], p1[k])]
    assert not bad, (len(bad), bad[:6])


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["bf16", "x3", "x3f"])
def test_training_step_is_bitwise_reproducible_taskprompter(prec):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from oracle import configs
    _two_steps_bitwise(configs.taskprompter("mini_ctr"), prec, 2, "TP")
    if prec != "x3":
        _two_steps_bitwise(configs.taskprompter("ns6"), prec, 2, "TP")          # the benchmarked shape (split reductions, many workgroups)


@pytest.mark.gpu
def test_training_step_is_bitwise_reproducible_invpt():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from oracle import configs
    _two_steps_bitwise(configs.invpt("mini8"), "bf16", 2, "IP")


@pytest.mark.gpu
def test_gradients_with_droppath_masks():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    g = torch.Generator().manual_seed(3)
    drop = [(torch.bernoulli(torch.full((4, 2), 0.6), generator=g) / 0.6) for _ in range(4)]
    fwd, errs = train_check.grad_errors("mini_ctr", "x3", "cuda", drop=drop)
    worst, med = train_check.summarize(errs)
    assert max(fwd.values()) < 1e-3 and med < 1e-3, (worst, med)


@pytest.mark.gpu
# x3 median bound 5e-3 (not 1e-3): the InvPT decoder is ReLU + train-mode BatchNorm on maps of a few hundred pixels; a
# pre-activation within 1e-5 of zero flips its ReLU mask between fp32 summation orders and moves every upstream gradient
# by a discrete amount (measured 0.9e-3 .. 1.4e-3 run to run on MI355X; 8e-6 on the fp64 emulator, tests/test_host_cpu.py).
@pytest.mark.parametrize("prec,ftol,mtol", [("x3", 1e-3, 5e-3), ("bf16", 4e-2, 2e-1)])
def test_invpt_gradients(prec, ftol, mtol):
    """InvPT (ViT + InvPT decoder + MLP heads) training forward + backward through the C ABI vs the oracle's autograd."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    fwd, errs, dead = train_check.invpt_grad_errors("mini8", prec, "cuda")
    assert max(fwd.values()) < ftol, fwd
    worst, med = train_check.summarize(errs, floor=1e-6 if prec == "x3" else 1e-4)
    assert med < mtol and (prec != "x3" or worst[0] < 3e-2), (worst, med)
    if prec == "bf16":
        train_check.assert_per_param(errs, "bf16")
    assert len(dead) == 10


@pytest.mark.gpu
def test_fused_clip_adam_matches_torch_on_gpu():
    """mtt_grad_sqnorm + mtt_adam_step vs clip_grad_norm_ + torch.optim.Adam (4 steps; chunk-spanning, tiny and 4-byte-aligned tensors)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import mtt_amd
    torch.manual_seed(0)
    flat = torch.randn(200001, device="cuda")
    shapes = [(300000,), (1024, 1024), (7,), (350, 350, 3, 3)]
    ref = [torch.nn.Parameter(torch.randn(s, device="cuda")) for s in shapes]
    mine = [torch.nn.Parameter(q.detach().clone()) for q in ref]
    o_ref = torch.optim.Adam(ref, lr=2e-3, weight_decay=1e-6)
    o_mine = mtt_amd.optim.FusedClipAdam(mine, lr=2e-3, weight_decay=1e-6, max_norm=10.0)
    for it in range(4):
        for i, (q, r, s) in enumerate(zip(mine, ref, shapes)):
            g = torch.randn(s, device="cuda") * (1.0 if it % 2 == 0 else 1e-3)
            if i == 0:                                   # a gradient that is only 4-byte aligned (DDP bucket views can be)
                flat[1:1 + 200000].normal_()
                g = torch.cat([flat[1:200001], g[200000:]])
            q.grad, r.grad = g.clone(), g.clone()
        n_ref = torch.nn.utils.clip_grad_norm_(ref, 10.0)
        o_ref.step()
        n_mine = o_mine.step()
        assert abs(float(n_ref) - float(n_mine)) < 1e-4 * float(n_ref)
        for q, r in zip(mine, ref):
            assert float((q.detach() - r.detach()).abs().max()) < 5e-6, it


@pytest.mark.gpu
def test_graphed_train_step_matches_eager_steps():
    """graphs.GraphedTrainStep (the whole iteration recorded in one hipGraph, FusedClipAdam(capturable=True)) against the same iteration
    launched eagerly FROM THE SAME STATE: before every replay an eager twin receives the graphed model's parameters, BatchNorm buffers and
    Adam moments, then both take one step on a new batch.  lr = 0.05 makes the updates (~lr per element) 5 orders of magnitude larger than
    fp32 rounding of the parameters, so the comparison measures the step and not rounding noise (with the reference's lr of 2e-5 on a
    64 x 64 miniature most updates are a few ulps, and two EAGER runs already differ by 4 % of the update norm).  DropPath is off: a graph
    draws from its own Philox offsets."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import copy
    import mtt_amd
    dev = torch.device("cuda")
    H = W = 64
    torch.manual_seed(0)
    p = mtt_amd.factory.make_p(mtt_amd.factory.TASK_ORDER, (H, W), backbone="TaskPrompter_vitB", head="conv", embed_dim=48, final_embed_dim=56,
                               chan_nheads=1, use_ctr=True, prec="bf16", drop_path_rate=0.0)
    model_g = mtt_amd.factory.get_model(p).to(dev).train()
    model_e = copy.deepcopy(model_g)
    crit = mtt_amd.losses.FusedMultiTaskLoss(p, p.TASKS.NAMES).to(dev)
    xs = [torch.randn(2, 3, H, W, device=dev) for _ in range(4)]
    gts = [mtt_amd.losses.synthetic_targets(p, 2, H, W, dev, seed=i) for i in range(4)]
    kw = dict(lr=0.05, weight_decay=1e-6, max_norm=10.0)
    og = mtt_amd.optim.FusedClipAdam(model_g.parameters(), capturable=True, **kw)
    oe = mtt_amd.optim.FusedClipAdam(model_e.parameters(), **kw)

    def eager(model, opt, x, gt):
        loss = crit(model(x), gt)["total"]
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        return loss

    eager(model_e, oe, xs[0], gts[0])                                      # creates the twin's optimizer state
    step = mtt_amd.graphs.GraphedTrainStep(model_g, crit, og, xs[0], gts[0], warmup=2)
    names = [n for n, _ in model_g.named_parameters()]
    report = []
    for i in range(1, 4):
        with torch.no_grad():                                              # twin <- graphed model (same state before the step)
            for (_, a), (_, b) in zip(model_g.state_dict().items(), model_e.state_dict().items()):
                b.copy_(a)
            for q, r in zip(model_g.parameters(), model_e.parameters()):
                for k in ("exp_avg", "exp_avg_sq"):
                    oe.state[r][k].copy_(og.state[q][k])
                oe.state[r]["step"].fill_(float(og.state[q]["step"]))
        torch.autograd.graph.increment_version(list(model_e.parameters()))
        mtt_amd.ops.bump_param_epoch()                                     # the twin's weight packs are stale now
        before = [q.detach().clone() for q in model_g.parameters()]
        le = float(eager(model_e, oe, xs[i], gts[i]).detach())
        lg = float(step(xs[i], gts[i]).detach())
        num = den = 0.0
        worst = (0.0, "")
        for n, q, r, b0 in zip(names, model_g.parameters(), model_e.parameters(), before):
            dn, dd = float((q.detach() - r.detach()).double().pow(2).sum()), float((r.detach() - b0).double().pow(2).sum())
            num, den = num + dn, den + dd
            if dd > 0:
                worst = max(worst, ((dn / dd) ** 0.5, n))
        report.append((i, le, lg, (num / den) ** 0.5, worst))
    for r in report:
        print("graphed vs eager step %d: loss %.6f / %.6f, |d theta_graph - d theta_eager| / |d theta_eager| = %.3e, worst tensor %.3e (%s)" % (r[0], r[1], r[2], r[3], r[4][0], r[4][1]))
    for i, le, lg, rel, worst in report:
        assert abs(le - lg) <= 1e-4 * max(1.0, abs(le)), report
        assert rel <= 1e-3, report
    assert float(og.state[next(iter(model_g.parameters()))]["step"]) == 5.0
    model_g.eval(), model_e.eval()
    with torch.no_grad():
        yg, ye = model_g(xs[0]), model_e(xs[0])                            # eager forward after replays: the packs must be rebuilt
    for t in yg:
        assert float((yg[t].float() - ye[t].float()).abs().max()) <= 2e-2 * float(ye[t].float().abs().max()) + 1e-6, t


@pytest.mark.gpu
def test_fused_losses_on_gpu():
    """mtt_loss_label_stats / mtt_loss_fwd / mtt_loss_bwd vs the torch restatement of the reference criterion (CPU, fp32)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from test_host_cpu import check_fused_losses
    check_fused_losses("cuda", 2e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mini_swin", "mini_swin_pad"])
@pytest.mark.parametrize("prec,fwd_tol,med_tol,worst_tol", [("x3", 1e-3, 1e-3, 2e-2), ("bf16", 5e-2, 1e-1, 1.0)])
def test_swin_training_gradients(name, prec, fwd_tol, med_tol, worst_tol):
    """TaskPrompter-Swin training step on the HIP kernels vs the oracle's autograd (measured errors printed)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import train_check
    fwd, errs, dead = train_check.swin_grad_errors(name, prec, "cuda")
    worst, med = train_check.summarize(errs)
    print(f"PARITY swin-train {name} {prec} fwd {max(fwd.values()):.3e} grad median {med:.3e} worst {worst[0]:.3e} ({worst[1]})")
    assert max(fwd.values()) < fwd_tol, fwd
    assert med < med_tol and worst[0] < worst_tol, (med, worst)


@pytest.mark.gpu
@pytest.mark.parametrize("family,name,prec", [("taskprompter", "mini_ctr", "x3f"), ("taskprompter", "mini_deconv", "bf16"), ("invpt", "mini8", "x3f"),
                                              ("swin", "mini_swin", "x3f"), ("swin", "mini_swin_pad", "bf16")])
def test_device_memory_is_steady_over_training_steps(family, name, prec):
    """The bytes allocated on the device after a training iteration (forward, backward, fused clip + Adam, pack refresh) are the same from the
    second iteration on: no autograd node keeps tensors alive across steps (the emulator twin counts host tensors: tests/test_host_cpu.py)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import gc
    import conftest
    import mtt_amd
    from oracle import configs, weights
    cfg = getattr(configs, family)(name)
    if family == "invpt":
        train_check.skip_unless_own_pitch(cfg)
    model = conftest.build_product_model(cfg, prec, "cuda")
    model.train()
    opt = mtt_amd.optim.FusedClipAdam(model.parameters(), lr=1e-4, weight_decay=1e-6, max_norm=10.0)
    x = weights.synth_images(2, cfg["img_size"], 1).cuda()
    held = []
    for _ in range(5):
        out = model(x)
        loss = sum(v.float().sum() for v in out.values() if torch.is_tensor(v)) + sum(v.float().sum() for v in (out.get("inter_preds") or {}).values())
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        del out, loss
        gc.collect()
        torch.cuda.synchronize()
        held.append(torch.cuda.memory_allocated())
    # (the caching allocator rounds block sizes and the weight packs are rebuilt every step: a fraction of a percent of jitter, no trend;
    # the leak this guards against grew the footprint by a block's qkv + out — tens of percent — per step)
    assert max(held[1:]) - min(held[1:]) <= 0.01 * held[1], held


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mini_swin_sp", "mini_swin", "mini_swin_pad"])
def test_swin_x3f_split_planes_and_matrix_core_window_attention(name, monkeypatch):
    """Swin in the tolerance-compliant mode on the device: split-plane Linears / task features, x3 MFMA window attention forward, bf16 MFMA
    window attention backward — eval forward < 5e-5 per head vs the oracle, every parameter gradient within the x3f bound."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from test_host_cpu import check_swin_x3f_split_planes
    check_swin_x3f_split_planes(name, "cuda", monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("name,prec", [("mini_swin_sp", "x3f"), ("mini_swin_pad", "bf16")])
def test_swin_level_features_do_not_depend_on_keep(name, prec, monkeypatch):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from test_host_cpu import check_swin_level_features_do_not_depend_on_keep
    check_swin_level_features_do_not_depend_on_keep(name, prec, "cuda", monkeypatch)


@pytest.mark.gpu
def test_swin_eval_pass_registers_no_second_pack_set():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import mtt_amd
    from test_host_cpu import check_swin_eval_pass_registers_no_second_pack_set
    try:
        check_swin_eval_pass_registers_no_second_pack_set("cuda")
    finally:
        mtt_amd.ops.clear_pack_cache()


@pytest.mark.gpu
def test_swin_training_path_checks_its_input_size():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from test_host_cpu import check_swin_training_path_checks_its_input_size
    check_swin_training_path_checks_its_input_size("cuda")


@pytest.mark.gpu
def test_invpt_eval_pass_registers_no_second_pack_set():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import mtt_amd
    from test_host_cpu import check_invpt_eval_pass_registers_no_second_pack_set
    try:
        check_invpt_eval_pass_registers_no_second_pack_set("cuda")
    finally:
        mtt_amd.ops.clear_pack_cache()


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["x3", "x3f"])
def test_invpt_one_forward_both_ways(prec):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from test_host_cpu import check_invpt_one_forward_both_ways
    check_invpt_one_forward_both_ways(prec, "cuda")


@pytest.mark.gpu
@pytest.mark.timeout(1500)
def test_mixed_precision_training_trajectory_follows_the_fp32_reference_over_200_steps():
    """Does x3f TRAIN like the reference?  The reference trains in fp32 (no AMP); x3f = fp32-class forward + bf16
    backward has bf16-class per-step gradients (median 8e-3 against the oracle's autograd).  200 optimizer steps of the whole iteration
    (train-mode BatchNorm, the reference's criterion, clip_grad_norm_(10), Adam — TaskPrompter/utils/train_utils.py:32-51) from the same
    state on the same cycle of 4 batches: the CPU oracle (fp32 autograd + torch.optim.Adam), the fully fp32-class product mode (x3)
    and x3f.  Bounds: the loss curve of x3f stays within 1.5 % of the oracle's at every step, within 0.5 % on 10-step running means, and
    the loss actually falls; x3 — the mode whose gradients match to 6e-5 — bounds how much of the gap is chaotic divergence of ANY
    fp32 re-implementation rather than the bf16 backward.  Measured on MI355X (profiles/r05_parity_report_a_full_suite.jsonl): loss
    37.52 -> 33.49 (oracle) / 33.46 (x3f) / 33.50 (x3); worst pointwise gap 0.43 % (x3f) vs 0.40 % (x3), running-mean gap 0.14 % both —
    the mixed-precision step is no further from the reference's trajectory than the fully fp32-class one."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import parity_util as pu
    curves = train_check.trajectory_check("mini_ctr", ["x3f", "x3"], "cuda", steps=200, lr=2e-4)
    gaps = train_check.trajectory_gaps(curves, window=10)
    o = curves["oracle"]
    pu.report("training_trajectory", config="mini_ctr", steps=200, lr=2e-4, oracle_first=o[0], oracle_last10=sum(o[-10:]) / 10,
              x3f_last10=sum(curves["x3f"][-10:]) / 10, x3_last10=sum(curves["x3"][-10:]) / 10,
              gaps={m: dict(max_pointwise=g[0], max_running10=g[1], final_running10=g[2]) for m, g in gaps.items()},
              every20={m: [round(c[i], 4) for i in range(0, 200, 20)] for m, c in curves.items()})
    assert sum(o[-10:]) / 10 < 0.93 * o[0], (o[0], o[-10:])                # it trains
    assert gaps["x3f"][0] < 1.5e-2 and gaps["x3f"][1] < 5e-3, gaps
    assert gaps["x3"][0] < 1.5e-2 and gaps["x3"][1] < 5e-3, gaps
