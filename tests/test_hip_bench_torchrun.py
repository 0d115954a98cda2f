"""GPU: the exact command the driver uses for the multi-GPU scaling bench -- ``python -m torch.distributed.run --nnodes=1
--nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N --steps K --warmup W`` -- end to end with two
ranks.  A dev box has ONE GPU, so both ranks share cuda:0 and exchange over gloo (MCVC_DIST_BACKEND=gloo; RCCL refuses
duplicate devices): what is exercised is bench.py's own choreography (env rendezvous, barriers, MAX-reduce of the timed
region, ONE JSON line from rank 0 only, clean process-group teardown), not the transport."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_under_torchrun_two_ranks():
    env = dict(os.environ, MCVC_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29541", os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "2"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]                  # rank 0 only
    res = json.loads(lines[0])
    assert res["n_gpus"] == 2 and res["steps"] == 4 and res["warmup"] == 2 and res["scaling"] == "weak"
    assert res["config"]["global_batch"] == 2 and res["config"]["parallelism"] == "dp2"
    assert res["losses_finite"] and res["value"] > 0
    assert abs(res["value"] - 2 * 1e3 / res["ms_per_step"]) < 1e-6 * res["value"]        # whole-job rate = ranks x per-rank rate
    assert "cpu_baseline" not in res and "configs" not in res   # N=1 only
    assert res["dist"]["backend"] == "gloo" and res["dist"]["world"] == 2 and res["dist"]["rccl_ranks_seen"] == 2
    assert "degraded" not in res                   # (ranks sharing a GPU switch the persistent trunk off on purpose: not a degradation)


def test_multi_gpu_bench_fails_when_the_ranks_are_silently_degraded():
    """a SCALE line must not be quietly degraded.  Here the persistent trunk kernels are forced off their residency
    bound on both ranks (bench.py --test-force-residency 9: the engine claims 9 passes in flight = 576 workgroups > 256 compute units, what five
    free-running grouped passes did on data-parallel ranks after the identity cut-off before r5) while the ranks do NOT share a GPU as
    far as the job can tell (--test-distinct-gpus skips the shared-device switch): bench.py must print its line, say why, and exit
    non-zero; --allow-degraded turns that into a zero exit."""
    env = dict(os.environ, MCVC_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    base = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
            "--master-port", "29543", os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--no-trace",
            "--test-force-residency", "9", "--test-distinct-gpus"]
    r = subprocess.run(base, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode != 0 and len(lines) == 1, r.stdout[-2000:] + r.stderr[-3000:]
    res = json.loads(lines[0])
    assert res["degraded"] and "per-layer" in res["degraded"][0] and res["schedule"]["trunk_persistent_possible"] and not res["schedule"]["trunk_persistent"]
    r = subprocess.run(base + ["--allow-degraded"], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]


def test_default_single_gpu_bench_carries_every_baseline_config():
    """The full single-GPU invocation (`python bench.py --gpus 1 --full ...`; the test's name is from when this was the default run) must
    measure BASELINE configs[2], the per-GPU shape of configs[3] and configs[4] besides the bs=1 headline, each as a nested record with its
    own roofline (CPU samples skipped here for time)."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "3", "--cpu-iters", "0", "--full"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    res = json.loads(lines[0])
    assert res["config"]["global_batch"] == 1 and res["n_gpus"] == 1 and res["steps"] == 5 and res["losses_finite"]
    assert res["roofline"]["frac"] > 0 and res["dist"] == {"backend": None, "world": 1, "rccl_ranks_seen": 1}
    ids = [c["config_id"] for c in res["configs"]]
    assert len(ids) == 3 and ids[0].startswith("configs[2]") and ids[1].startswith("configs[3]") and ids[2].startswith("configs[4]")
    assert [c["config"]["global_batch"] for c in res["configs"]] == [32, 8, 16]
    for c in res["configs"]:
        assert c["value"] > 0 and c["ms_per_step"] > 0 and 0 < c["roofline"]["frac"] < 1 and c["roofline"]["kernel"]
    assert res["configs"][2]["dtype"] == "bf16" and res["configs"][2]["outputs_finite"]
    # the two byte counts are named for what they are, and the reference-exact loss readback is priced in the same run
    assert res["hbm_bytes_per_step_launcher"] > 0 and "hbm_bytes_per_step_pmc" in res and "hbm_bytes_per_step" not in res
    sc = res["schedule"]
    assert sc["sync_losses_ms_per_step"] > 0 and -0.2 < sc["sync_losses_cost"] < 1.0 and "two step()s earlier" in sc["loss_readback"]
    # ... and so is the regime after the identity cut-off (train.py:314-315), labelled, beside the headline (which stays the dearer regime)
    post = res["after_identity_cutoff"]
    assert post["identity_loss_lambda"] == 0 and 0 < post["ms_per_step"] < 1.1 * res["ms_per_step"] and res["identity_loss_lambda"] == 5


def _oracle_replay(n_steps):
    """The CPU oracle on bench.py's replay: default init (seed 0), the run's first synthetic batches, the benchmark's schedule
    (lr 2e-4 / 1e-4, cycle 10, identity 5); returns (losses of the last step, {net: parameter change on the dump's positions})."""
    sys.path.insert(0, ROOT)
    import bench
    import mcvc_oracle as orc
    nets = bench.build_nets("cpu")
    onets = orc.default_init_nets(0)
    names = {n: [k for k, _ in nets[n].named_parameters()] for n in nets}
    flat = lambda p: {n: torch.cat([p[n][k].reshape(-1) for k in names[n]]) for n in names}   # noqa: E731
    ref0 = bench.param_sample(nets)
    idx = {n: np.sort(np.random.default_rng(0).choice(v.numel(), ref0[n].numel(), replace=False)) for n, v in flat(onets).items()}
    p0 = {n: v[torch.from_numpy(idx[n])].clone() for n, v in flat(onets).items()}
    for n in names:                    # the oracle's init and positions are the benchmark's
        assert torch.equal(p0[n], ref0[n]), n
    so = orc.StepOracle(onets, skip_wasted=True)
    for b in bench.synthetic_batches(n_steps, 1, 64, 0, "cpu"):
        g_loss, d_loss = so.step(*b)
    p1 = {n: v[torch.from_numpy(idx[n])] for n, v in flat(onets).items()}
    return {"g_loss": g_loss, "d_loss": d_loss}, {n: (p1[n] - p0[n]).double().numpy() for n in names}


def test_plain_single_gpu_bench_times_the_headline_only_and_dumps_its_outputs(tmp_path):
    """`python bench.py --gpus 1 --steps K --warmup W`: exactly K timed steps and the headline line, nothing measured beside it (no
    traced step, no CPU baseline, no nested configs).  --dump-outputs (bench.replay_outputs): the run's first steps replayed from the
    seeded start -- the same in every run up to rounding, parameters moved by several Adam steps, and in agreement with the CPU
    oracle's replay of the same steps."""
    sys.path.insert(0, ROOT)
    import bench
    nets = ("generator_A2B", "generator_B2A", "discriminator_A", "discriminator_B", "discriminator_A2", "discriminator_B2")
    names = ["loss_%s.npy" % k for k in ("adv_loss", "cycle_loss", "d_loss", "g_loss", "identity_loss")] + ["dparams_%s.npy" % n for n in nets]
    dumps = []
    for run in ("a", "b"):
        out = tmp_path / run
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "2", "--dump-outputs", str(out)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1
        res = json.loads(lines[0])
        assert res["steps"] == 20 and res["warmup"] == 2 and res["losses_finite"] and res["dtype"] == "f32" and res["higher_is_better"]
        assert abs(res["value"] - 1e3 / res["ms_per_step"]) < 1e-6 * res["value"]
        for key in ("roofline", "kernel_time_ms_per_step", "cpu_baseline", "configs", "after_identity_cutoff"):
            assert key not in res, key
        assert sorted(os.listdir(str(out))) == sorted(names)
        arrays = {f: np.load(str(out / f)) for f in names}
        assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in arrays.values())
        assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
        dumps.append(arrays)
    rel = lambda a, b: float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))   # noqa: E731
    spread = {f: rel(dumps[1][f], dumps[0][f].astype(np.float64)) for f in names}
    ref_losses, ref_dp = _oracle_replay(bench.REPLAY_STEPS)
    loss_vs_oracle = {k: rel(dumps[0]["loss_%s.npy" % k], v) for k, v in ref_losses.items()}
    # the parameter change by DIRECTION: Adam's early updates are ~lr * sign(g), so rounding-level gradient differences near zero flip
    # whole +-lr steps of single elements (measured rel-L2 against the oracle 0.08-0.17 after 5 steps, cosine ~0.99); a wrong batch,
    # a missing phase or a wrong gradient turns the direction
    cos = {n: float(np.dot(dumps[0]["dparams_%s.npy" % n].astype(np.float64), v)
                    / (np.linalg.norm(dumps[0]["dparams_%s.npy" % n].astype(np.float64)) * np.linalg.norm(v))) for n, v in ref_dp.items()}
    print("run-to-run rel-L2:", {k: "%.1e" % v for k, v in spread.items()})
    print("losses vs oracle rel:", {k: "%.1e" % v for k, v in loss_vs_oracle.items()}, "parameter change cosine vs oracle:",
          {k: "%.4f" % v for k, v in cos.items()})
    for n in nets:
        # moved: the parameters the oracle moves (not the discriminators' downSample4: no gradient reaches it), by several lr steps
        lr = 2e-4 if n.startswith("generator") else 1e-4
        dp = dumps[0]["dparams_%s.npy" % n].astype(np.float64)
        moved, moved_ref = float(np.mean(dp != 0)), float(np.mean(ref_dp[n] != 0))
        rms = float(np.sqrt(np.mean(dp ** 2)))
        print("%s: %.4f of the sampled parameters moved (oracle %.4f), rms change %.2e" % (n, moved, moved_ref, rms))
        assert moved_ref > 0.3 and abs(moved - moved_ref) < 1e-2 and lr < rms < bench.REPLAY_STEPS * lr, (n, moved, moved_ref, rms)
    assert max(spread.values()) < 2e-3, spread            # measured <= 6.3e-4; the timed run's own final state: ~0.4 of the change
    assert max(loss_vs_oracle.values()) < 1e-2, loss_vs_oracle
    assert min(cos.values()) > 0.95, cos


def test_nccl_backend_refuses_fewer_gpus_than_ranks():
    import torch
    code = ("import os, sys; sys.path.insert(0, %r); "
            "os.environ.update(RANK='0', WORLD_SIZE='%d', LOCAL_RANK='0', LOCAL_WORLD_SIZE='%d', MASTER_ADDR='127.0.0.1', MASTER_PORT='29547'); "
            "from mask_cyclegan_vc.parallel import init_from_env; init_from_env(backend='nccl')")
    n = torch.cuda.device_count() + 1
    r = subprocess.run([sys.executable, "-c", code % (os.path.join(ROOT, "maskcyclegan-vc_amd"), n, n)], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "one GPU per local rank" in r.stderr
