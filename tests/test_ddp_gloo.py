"""CPU, world_size 2 and 4, gloo: the data-parallel path (DistributedDataParallel gradient all-reduce + cross-rank
BatchNorm statistics through SyncBatchNorm holders) on the ABI emulator.  The ranks, each with its share of the images — the shares
may be UNEQUAL, the batch statistics are merged with per-rank counts — must produce the gradients of a single process running the
whole batch, as the reference's DDP + SyncBatchNorm training does (TaskPrompter/main.py:92-94, InvPT/main.py:87-89).  Also checks
that the stage-batched SyncBN exchange issues ONE collective per BatchNorm stage and that the fused clip + Adam step keeps the
replicas identical."""
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = {
    # name: (kind, config, image shares per rank[, arithmetic mode, bound on the worst gradient error])
    "taskprompter_2ranks": ("TP", "mini_ctr", [[0], [1]]),
    "taskprompter_3ranks_unequal": ("TP", "mini_ctr", [[0, 1], [2], [3]]),
    "invpt_4ranks": ("IP", "mini8", [[0], [1], [2], [3]]),
    # the DEFAULT mode (x3f) on decoder widths % 32: its Functions hand split planes to each other (two outputs, the lo plane without a
    # gradient) — DDP with find_unused_parameters=False must still see every parameter's gradient; bf16-class gradients
    "taskprompter_x3f_planes_2ranks": ("TP", "mini_p32", [[0], [1, 2]], "x3f", 1.5e-1),
    # TaskPrompter-Swin in the default mode (round 6: split-plane Linears / task features, matrix-core window attention), unequal shares;
    # its prompt outputs of the last block have no gradient in the reference either: find_unused_parameters
    "swin_x3f_2ranks_unequal": ("SW", "mini_swin_sp", [[0, 1], [2]], "x3f", 1.5e-1),
}


def _cfg_of(kind, name):
    from oracle import configs
    return configs.taskprompter(name) if kind == "TP" else (configs.invpt(name) if kind == "IP" else configs.swin(name))


def _contract_of(model):
    from oracle import weights
    return [(k, list(v.shape)) for k, v in model.state_dict().items() if k.rsplit(".", 1)[-1] not in weights.DERIVED_BUFFERS]


def _mode(case):
    c = CASES[case]
    return (c[3], c[4]) if len(c) > 3 else ("x3", 1e-3)


def _loss(out, rows, n_total, world, seed=7):
    """mean over the GLOBAL batch of <out, r> with global-batch random weights, restricted to this rank's images and scaled by the
    world size (DDP averages the ranks' gradients)."""
    g = torch.Generator().manual_seed(seed)
    tot = 0.0
    flat = {k: v for k, v in out.items() if k != "inter_preds"}
    if "inter_preds" in out:
        flat.update({"inter/" + k: v for k, v in out["inter_preds"].items()})
    for k in sorted(flat):
        r = torch.randn((n_total,) + tuple(flat[k].shape[1:]), generator=g)[rows]
        tot = tot + (flat[k] * r).sum() / (n_total * flat[k][0].numel()) * world
    return tot


def _worker(rank, world, port, case, q):
    try:
        _worker_body(rank, world, port, case, q)
    except BaseException as e:  # noqa: BLE001
        import traceback
        q.put(("error", f"rank {rank}: {e!r}\n{traceback.format_exc()}"))
        raise


def _worker_body(rank, world, port, case, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import conftest
    import mtt_amd
    from oracle import abi_emul, configs, weights
    mtt_amd.ops.call = abi_emul.call
    kind, name, shares = CASES[case][:3]
    cfg = _cfg_of(kind, name)
    if kind == "SW":                   # the miniature takes the split-plane paths Swin-B takes
        mtt_amd.autograd_path.AUTO_SPLIT_MIN_ROWS = 64
    model = conftest.build_product_model(cfg, _mode(case)[0])
    model.load_state_dict(weights.synth_state_dict(_contract_of(model), 0), strict=kind != "SW")   # (Swin: geometry-derived buffers are not synthesised)
    model.train()
    for m in model.modules():          # DDP refuses nn.SyncBatchNorm on CPU modules: plain holders flagged for sync (same code path)
        if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
            if isinstance(m, torch.nn.SyncBatchNorm):
                m.__class__ = torch.nn.BatchNorm2d
            m._mtt_sync = True
    n_coll = {"gather": 0}
    ag = dist.all_gather
    ar = dist.all_reduce

    def counted_reduce(t, *a, **k):
        if t.dim() == 3 and t.shape[0] == world and t.shape[-1] % 2 == 1:   # the rank-slotted [W, Z, 2C+1] statistics table of bn.train_stats
            n_coll["gather"] += 1
        return ar(t, *a, **k)
    dist.all_reduce = counted_reduce
    ddp = torch.nn.parallel.DistributedDataParallel(model, find_unused_parameters=(kind in ("IP", "SW")))
    n_total = sum(len(s) for s in shares)
    rows = shares[rank]
    x = weights.synth_images(n_total, cfg["img_size"], 2)[rows]
    out = ddp(x)
    _loss(out, rows, n_total, world).backward()
    grads = {k: (v.grad.clone() if v.grad is not None else None) for k, v in model.named_parameters()}
    n_bn_stages = n_coll["gather"]
    # the fused clip + Adam step consumes DDP's (bucket-view) gradients: parameters must stay identical on every rank
    opt = mtt_amd.optim.FusedClipAdam([p_ for p_ in model.parameters() if p_.grad is not None], lr=1e-3, weight_decay=1e-6, max_norm=0.5)
    norm = opt.step()
    chk = torch.stack([p_.detach().double().sum() for p_ in model.parameters()]).sum() + norm.double().sum()
    seen = [torch.zeros_like(chk) for _ in range(world)]
    ag(seen, chk)
    assert all(bool(torch.equal(seen[0], s_)) for s_ in seen), seen
    if rank == 0:
        q.put(({k: (v.numpy() if v is not None else None) for k, v in grads.items()}, n_bn_stages))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(900)
@pytest.mark.parametrize("case", sorted(CASES))
def test_ddp_ranks_match_single_process(case):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    kind, name, shares = CASES[case][:3]
    world = len(shares)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() % 1000) + 7 * sorted(CASES).index(case)
    procs = [ctx.Process(target=_worker, args=(r, world, port, case, q)) for r in range(world)]
    for p_ in procs:
        p_.start()
    got, n_stage_collectives = q.get(timeout=600)
    assert got != "error", n_stage_collectives
    for p_ in procs:
        p_.join(timeout=300)
        assert p_.exitcode == 0
    # single-process oracle gradients on the whole batch, same loss
    import conftest
    from oracle import configs, weights
    cfg = _cfg_of(kind, name)
    sd = weights.synth_state_dict(_contract_of(conftest.build_product_model(cfg, "x3")), 0)
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items() if v.dtype.is_floating_point and "running_" not in k}
    n_total = sum(len(s) for s in shares)
    x = weights.synth_images(n_total, cfg["img_size"], 2)
    if kind == "TP":
        from oracle import taskprompter_oracle as orc
    elif kind == "SW":
        from oracle import swin_oracle as orc
    else:
        from oracle import invpt_oracle as orc
    out = orc.forward(dict(sd, **params), cfg, x, training=True)
    _loss(out, list(range(n_total)), n_total, 1).backward()
    worst, errs, big = 0.0, [], []
    gmax = max(float(p_.grad.norm()) for p_ in params.values() if p_.grad is not None)
    for k, ref in params.items():
        if ref.grad is None or float(ref.grad.norm()) < (1e-6 if _mode(case)[0] == "x3" else 1e-4):
            continue
        assert got[k] is not None, k
        e = float((torch.from_numpy(got[k]) - ref.grad).norm() / ref.grad.norm())
        worst = max(worst, e)
        errs.append(e)
        if float(ref.grad.norm()) > 1e-2 * gmax:
            big.append((e, k))
    errs.sort()
    if _mode(case)[0] == "x3":
        assert worst < _mode(case)[1], worst
    else:
        # bf16 backward: the median and the 90th percentile over all parameters (single near-zero gradients can be off by more), AND a
        # worst-case bound on every gradient of non-negligible norm (> 1 % of the largest): one wrong parameter gradient must not pass
        assert errs[len(errs) // 2] < 3e-2 and errs[int(len(errs) * 0.9)] < _mode(case)[1], (errs[len(errs) // 2], worst)
        assert big and max(big)[0] < 8e-2, sorted(big, reverse=True)[:5]
    # SyncBN statistics: one all_gather per BatchNorm STAGE (a stage = all tasks' BatchNorms at one point of the network), not one
    # per BatchNorm layer: TaskPrompter has 4 taps + 1 head stage; InvPT's decoder has 2 + 3*... stages (fewer than its 2*T*... layers)
    n_layers = sum(1 for k in sd if k.endswith("running_mean"))
    assert 0 < n_stage_collectives < n_layers, (n_stage_collectives, n_layers)


def _run_bench_emulated(*flags, timeout=600):
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, OMP_NUM_THREADS="2")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "bench_emulated.py"), "--device", "cpu", "--config", "mini",
                        "--steps", "2", "--warmup", "1", "--no-fwd"] + list(flags), capture_output=True, text=True, timeout=timeout, env=env,
                       cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]                 # ONE JSON line, from rank 0
    return json.loads(lines[0])


def test_bench_gpus_flag_launches_that_many_ranks():
    """`python bench.py --gpus N` (the driver's form, no torchrun around it) must start N ranks itself (TaskPrompter/main.py:32,92-94 under
    run_taskprompter_*.sh:1): here N = 2 over gloo on the CPU emulator, miniature config.  The line reports n_gpus = 2, a global batch of
    2 x the per-GPU batch (weak scaling) and whole-job throughput; --gpus 1 stays a single process without a process group."""
    two = _run_bench_emulated("--gpus", "2")
    assert two["n_gpus"] == 2 and two["config"]["gloo_ranks"] == 2 and two["config"]["parallelism"] == "dp2"
    assert two["config"]["global_batch"] == 2 * two["config"]["per_gpu_batch"] and two["scaling"] == "weak"
    assert abs(two["value"] - two["config"]["global_batch"] / (two["ms_per_step"] * 1e-3)) < 1e-2 * two["value"]
    assert two["git"]["head"] and two["git"]["tree_sha"]
    one = _run_bench_emulated("--gpus", "1")
    assert one["n_gpus"] == 1 and one["config"]["gloo_ranks"] is None and one["config"]["parallelism"] == "dp1"
    # the same seeded weights, rank 0's batch is the single process's batch; SyncBN + the gradient mean change the trajectory, not the scale
    assert abs(two["config"]["loss"] - one["config"]["loss"]) < 0.5 * abs(one["config"]["loss"])


def test_bench_plain_run_and_dumped_outputs(tmp_path):
    """A run without --full times exactly --steps steps and leaves every other record null; --dump-outputs writes the last timed step's
    sampled task outputs, loss and parameters as float32 / float64 .npy files that two runs with the same arguments reproduce bit for bit."""
    import numpy as np
    dumps = []
    for i in range(2):
        d = tmp_path / f"run{i}"
        r = _run_bench_emulated("--gpus", "1", "--dump-outputs", str(d))
        assert r["steps"] == 2 and r["warmup"] == 1 and r["ms_per_step"] > 0 and r["unit"] == "images/s"
        assert all(r[k] is None for k in ("host", "fwd_ms_per_img", "roofline", "parity", "fast_mode", "full_fp32_mode", "ref_batch",
                                          "torch_rocm_baseline", "cpu_baseline"))
        dumps.append({f.name: np.load(f) for f in sorted(d.iterdir())})
    names = set(dumps[0])
    assert {"loss.npy", "params.npy", "out_semseg.npy", "out_depth.npy"} <= names and names == set(dumps[1])
    assert sum(v.nbytes for v in dumps[0].values()) <= 64 << 20
    for n in names:
        assert dumps[0][n].dtype in (np.float32, np.float64) and np.isfinite(dumps[0][n]).all(), n
        assert np.array_equal(dumps[0][n], dumps[1][n]), n


def test_bench_gpus_8_every_rank_takes_the_instrumented_step():
    """The driver's 8-GPU form `bench.py --gpus 8` end to end on the host: 8 gloo ranks on the CPU emulator, the
    instrumented roofline step kept (`--cpu-roofline`: wall-clock stamps instead of HIP events) so that every rank runs what it runs on the
    node — ranks != 0 take the extra step too, because under DDP its gradient all-reduce is a collective (a rank that skipped it would
    hang the others).  ONE line, from rank 0: n_gpus 8, dp8, global batch = 8 x per-GPU batch, whole-job throughput, a roofline record."""
    r = _run_bench_emulated("--gpus", "8", "--cpu-roofline", "--full", timeout=1500)
    assert r["n_gpus"] == 8 and r["config"]["gloo_ranks"] == 8 and r["config"]["parallelism"] == "dp8"
    assert r["config"]["global_batch"] == 8 * r["config"]["per_gpu_batch"] and r["scaling"] == "weak"
    assert abs(r["value"] - r["config"]["global_batch"] / (r["ms_per_step"] * 1e-3)) < 1e-2 * r["value"]
    # the miniature has no GEMM that the library would give to the 256 x 256 LDS-DMA kernels, so the record may be empty — what is
    # tested is that the instrumented step ran on all ranks (the run completed) and the line is well-formed
    assert "roofline" in r and r["steps"] == 2 and r["warmup"] == 1
