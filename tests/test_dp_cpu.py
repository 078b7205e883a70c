"""N>1 data-parallel path on CPU: world_size-2 `gloo` processes.  Each rank runs the CPU ORACLE step on
its shard of a global batch (the HIP step cannot run without a GPU), then the product's DP module
(pea_diffusion_amd/dist.py: ONE all-reduce of the flat adapter gradient, averaged) must reproduce the
gradient of the oracle step on the whole global batch."""
import os
import socket
import sys

import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(2)
    import torch.distributed as dist
    from oracle.step_ref import AdapterRef, synthetic_batch, training_step_ref
    from oracle.unet_ref import UNet2DConditionRef, UNetConfig, cast_hook_ref
    from pea_diffusion_amd import dist as pdist
    assert pdist.init_from_env("gloo") == world
    cfg = UNetConfig(sample_size=8, block_out_channels=(32, 64), down_block_types=("DownBlock2D", "CrossAttnDownBlock2D"),
                     up_block_types=("CrossAttnUpBlock2D", "UpBlock2D"), transformer_layers_per_block=(1, 1),
                     num_attention_heads=(1, 1), cross_attention_dim=32, addition_time_embed_dim=8,
                     projection_class_embeddings_input_dim=16 + 48, layers_per_block=1, name="dp-toy")
    torch.manual_seed(0)
    us, ut = UNet2DConditionRef(cfg), UNet2DConditionRef(cfg)
    for p in list(us.parameters()) + list(ut.parameters()):
        p.requires_grad_(False)
    ad = AdapterRef(24, 16, 20, 32, False)
    flat0 = torch.cat([p.detach().reshape(-1) for p in ad.parameters()])
    if rank == 1:
        flat0 = flat0 + 1.0                       # diverged replica: broadcast must repair it
    pdist.broadcast_params_(flat0, src=0)
    o = 0
    with torch.no_grad():
        for p in ad.parameters():
            p.copy_(flat0[o:o + p.numel()].view_as(p))
            o += p.numel()
    gb = synthetic_batch(cfg, 4, L=5, enc_dim=24, seed=3)
    local = pdist.shard_batch(gb, rank, world)
    assert local["latents"].shape[0] == 2
    out = training_step_ref(ad, us, ut, local, cast_hook_ref)
    out["loss"].backward()
    flat_grad = torch.cat([p.grad.reshape(-1) for p in ad.parameters()])
    pdist.allreduce_mean_(flat_grad)
    loss_t = out["loss"].detach().clone()
    dist.all_reduce(loss_t)
    if rank == 0:
        for p in ad.parameters():
            p.grad = None
        ref = training_step_ref(ad, us, ut, gb, cast_hook_ref)
        ref["loss"].backward()
        g_ref = torch.cat([p.grad.reshape(-1) for p in ad.parameters()])
        q.put((float((flat_grad - g_ref).abs().max()), float(g_ref.abs().max()),
               float(loss_t / world), float(ref["loss"])))
    dist.barrier()
    dist.destroy_process_group()


def test_dp2_gloo_allreduce_matches_global_batch():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    err, scale, loss_dp, loss_ref = q.get(timeout=240)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert err <= 1e-5 * max(scale, 1e-6) + 1e-9, (err, scale)
    assert abs(loss_dp - loss_ref) <= 1e-5 * abs(loss_ref)


def test_shard_batch_and_lr_schedule():
    sys.path.insert(0, ROOT)
    from pea_diffusion_amd import dist as pdist
    from pea_diffusion_amd.train import polynomial_lr
    b = {"x": torch.arange(8).view(8, 1), "s": 3}
    assert pdist.shard_batch(b, 1, 4)["x"].flatten().tolist() == [2, 3] and pdist.shard_batch(b, 0, 2)["s"] == 3
    # transformers polynomial decay with warmup (utils/model_utils.py:136-138): lr 1e-5, 100 warmup, end 5e-8
    assert polynomial_lr(0, 1e-5, 100, 2232142, 5e-8) == 0.0
    assert abs(polynomial_lr(50, 1e-5, 100, 2232142, 5e-8) - 5e-6) < 1e-12
    assert abs(polynomial_lr(100, 1e-5, 100, 2232142, 5e-8) - 1e-5) < 1e-12
    assert polynomial_lr(3_000_000, 1e-5, 100, 2232142, 5e-8) == 5e-8
    mid = polynomial_lr(1116121, 1e-5, 100, 2232142, 5e-8)
    assert 4.9e-6 < mid < 5.1e-6


def test_lr_used_by_optimizer_step_k_matches_transformers_lambda():
    """The reference schedules with transformers' polynomial decay through a LambdaLR stepped after every optimizer
    step (utils/model_utils.py:98-140): optimizer step k (1-indexed) runs with lambda(k - 1), so the first update has
    lr = 0.  PEATrainer.optimizer_step() computes its lr from global_step BEFORE incrementing it."""
    sys.path.insert(0, ROOT)
    from transformers.optimization import get_polynomial_decay_schedule_with_warmup
    from pea_diffusion_amd.train import polynomial_lr
    base, warm, total, end = 1e-5, 100, 2000, 5e-8
    w = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.AdamW([w], lr=base)
    sch = get_polynomial_decay_schedule_with_warmup(opt, warm, total, lr_end=end, power=1.0)
    used = []
    for k in range(1, 2105):
        used.append(opt.param_groups[0]["lr"])       # what optimizer step k runs with
        w.grad = torch.ones(1)
        opt.step()
        sch.step()
    for k in (1, 2, 3, 50, warm, warm + 1, warm + 2, 1000, total, total + 1, total + 50):
        ours = polynomial_lr(k - 1, base, warm, total, end)       # optimizer_step(): lr from the pre-increment step
        assert abs(ours - used[k - 1]) <= 1e-12 + 1e-9 * used[k - 1], (k, ours, used[k - 1])
    assert used[0] == 0.0 and polynomial_lr(0, base, warm, total, end) == 0.0


def test_bench_launcher_spawns_two_ranks_over_gloo():
    """`python bench.py --gpus 2` (no torch.distributed.run, no WORLD_SIZE): the script itself starts two ranks before
    any GPU call, the ranks rendezvous, all-reduce through pea_diffusion_amd.dist and rank 0's single JSON line comes
    back through the parent.  --dry-run-collective keeps it on CPU tensors over gloo (no kernel runs; the same launcher
    and rank plumbing carry the RCCL run on the GPU box)."""
    import json
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--dry-run-collective",
                        "--full"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["ranks"] == 2 and out["n_gpus"] == 2 and out["per_gpu_batch"] == 8 and out["global_batch"] == 16
    assert out["allreduce_max_abs_err"] < 1e-5 and out["dry_run"] is True
    # pre-flight of the 8 x batch-8 run: the per-rank HBM plan (host-only planning pass of the C ABI) fits 288 GB with room,
    # and every rank was pinned to its own slice of the host's cores
    assert 100.0 < out["hbm_plan_gb_per_rank"] < 0.92 * out["hbm_capacity_gb"] and out["per_gpu_batch"] == 8
    assert out["cores_per_rank"] >= 1
    # the whole --full control flow ran on BOTH ranks: warm-up + K timed steps + the instrumented replay (each step holds a
    # collective, so a replay on rank 0 only would have left this subprocess hanging) + the closing barrier
    # (+ 3 local-only steps: the single-GPU-equivalent block between two barriers, as in the GPU run)
    assert out["steps_run_per_rank"] == 3 + 2 + 3 + 2 and out["replay"] == {"replayed_steps": 2}
    # the N-rank line's schema (bench.NRANK_KEYS; the GPU line asserts the same keys): control plane on gloo, and what a CPU
    # run can measure of the collective
    sys.path.insert(0, ROOT)
    import bench
    for k in bench.NRANK_KEYS:
        assert k in out, k
    assert out["control_plane"] == "gloo" and out["rccl_ranks"] == 0 and "gloo" in out["collective"]
    assert out["allreduce_ms"] > 0 and out["allreduce_bytes"] == 16 * 64 * 4
    assert out["single_gpu_equivalent"]["ms_per_step"] >= 0


def test_bench_plain_run_is_lean_and_dumps_outputs(tmp_path):
    """without --full a run is set-up, W warm-up steps, EXACTLY K timed steps and the line: no replay, no single-GPU-equivalent
    steps; --dump-outputs writes what the last timed step computed (here: the all-reduced buffer) on rank 0"""
    import json
    import subprocess

    import numpy as np
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    d = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
                        "--dry-run-collective", "--dump-outputs", str(d)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["steps_run_per_rank"] == 1 + 3 and out["replay"] is None and out["single_gpu_equivalent"] is None
    assert sorted(os.listdir(d)) == ["allreduced_grad.npy"]
    got = np.load(d / "allreduced_grad.npy")
    g = torch.Generator().manual_seed(1234)
    want = torch.randn(2 * 8, 16, generator=g).view(2, 8, 16).sum(1).mean(0).repeat(64).numpy()
    assert got.dtype == np.float32 and got.shape == (1024,) and np.allclose(got, want, atol=1e-5)


@pytest.mark.parametrize("opt", [["--breakdown"], ["--dump-prof", "x.csv"], ["--cpu-reference-faithful"]])
def test_bench_full_only_options_need_full(opt):
    """options that report on the --full run's replay or CPU baseline are a usage error without --full, not a silent no-op"""
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--dry-run-collective"] + opt,
                       capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 2 and "add --full" in r.stderr and not r.stdout.strip(), (r.returncode, r.stderr[-500:])


def test_bench_dump_outputs_float32_and_capped_by_a_fixed_sample(tmp_path):
    """dump_outputs(): float64 stays float64, other dtypes become float32; over the size limit every array above an equal
    share is cut to the same seeded, sorted sample of its elements in every run"""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    arrays = {"big": torch.arange(1000, dtype=torch.float32), "f64": np.ones(10), "half": torch.ones(5, dtype=torch.bfloat16)}
    shapes = bench.dump_outputs(str(tmp_path / "a"), arrays, limit=1200)
    bench.dump_outputs(str(tmp_path / "b"), arrays, limit=1200)
    assert shapes == {"big": [100], "f64": [10], "half": [5]}
    big = np.load(tmp_path / "a" / "big.npy")
    assert big.dtype == np.float32 and np.all(np.diff(big) > 0) and np.array_equal(big, np.load(tmp_path / "b" / "big.npy"))
    assert np.load(tmp_path / "a" / "f64.npy").dtype == np.float64 and np.load(tmp_path / "a" / "half.npy").dtype == np.float32
    assert sum(os.path.getsize(tmp_path / "a" / f) - 128 for f in os.listdir(tmp_path / "a")) <= 1200   # 128-byte .npy headers
    bench.dump_outputs(str(tmp_path / "c"), arrays)                 # under the default 64 MB limit nothing is sampled
    assert np.array_equal(np.load(tmp_path / "c" / "big.npy"), np.arange(1000, dtype=np.float32))


@pytest.mark.parametrize("kind,code", [("error", 4), ("timeout", 5)])
def test_bench_native_comm_failure_is_fatal_with_its_own_exit_code(kind, code):
    """--collective native: a communicator that cannot be built (or whose rendezvous times out) stops every rank with exit
    code 4 (5) -- never a silent fall-back to another collective -- and the launcher relays that code, names the failed
    ranks and prints no result line.  The failure is injected behind the gloo rendezvous of the dry run (the GPU run
    reaches the same comm_failure_exit() from NativeComm.from_env())."""
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--dry-run-collective",
                        "--inject-comm-failure", kind], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == code, (r.returncode, r.stderr[-1500:])
    assert not r.stdout.strip()
    assert "native RCCL communicator" in r.stderr and "--collective native makes this fatal" in r.stderr
    assert ("rendezvous timed out" in r.stderr) == (kind == "timeout")


def test_control_plane_rendezvous_is_bounded():
    """a rank whose peers never arrive leaves init_control_plane() with an exception after the timeout (gloo's store),
    it does not hang: WORLD_SIZE=2 with only rank 1 started (rank 0 would host the store)"""
    import subprocess
    code = ("import sys, time; sys.path.insert(0, %r)\n"
            "from pea_diffusion_amd import dist as pdist\n"
            "t0 = time.time()\n"
            "try:\n"
            "    pdist.init_control_plane(timeout_s=3.0)\n"
            "except Exception as e:\n"
            "    print('RAISED', type(e).__name__, round(time.time() - t0, 1)); sys.exit(7)\n"
            "sys.exit(0)\n" % ROOT)
    env = dict(os.environ, RANK="1", LOCAL_RANK="1", WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 7 and "RAISED" in r.stdout, (r.returncode, r.stdout, r.stderr[-800:])


def test_bench_under_torch_distributed_run_as_the_driver_launches_it():
    """the driver's N > 1 command line -- `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1
    --master-port P bench.py --gpus N ...` -- on CPU: the ranks join the gloo control plane through torchrun's agent store
    (TORCHELASTIC_USE_AGENT_STORE), run the protocol and rank 0's ONE line is the launcher's stdout"""
    import json
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                        "--dry-run-collective", "--full"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["control_plane"] == "gloo" and out["allreduce_max_abs_err"] < 1e-5
    assert out["steps_run_per_rank"] == 1 + 2 + 3 + 2


def test_bench_launcher_kills_hung_ranks_at_the_deadline(tmp_path):
    """a rank that never exits (stuck in a collective) must not block the parent forever: launch_ranks() stops its own
    children at the deadline, names the ranks that were still alive and returns non-zero.  Only the parent imports bench
    (and with it torch): rank 0 must be done well before the deadline however slowly torch loads on the host."""
    import subprocess
    script = tmp_path / "hang.py"
    script.write_text(
        "import os, sys, time\n"
        "if os.environ.get('RANK') is None:\n"
        f"    sys.path.insert(0, {ROOT!r})\n"
        "    import bench\n"
        "    bench.__file__ = __file__\n"
        "    sys.exit(bench.launch_ranks(2, [], 10.0))\n"
        "if os.environ['RANK'] == '1':\n"
        "    time.sleep(600)\n"
        "print('{}')\n")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 124, (r.returncode, r.stderr[-1000:])
    assert "ranks still running: [1]" in r.stderr and not r.stdout.strip()


def test_bench_refuses_a_world_size_that_contradicts_gpus():
    import subprocess
    env = dict(os.environ, WORLD_SIZE="3", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-run-collective"],
                       capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 2 and "WORLD_SIZE=3" in r.stderr and not r.stdout.strip()
