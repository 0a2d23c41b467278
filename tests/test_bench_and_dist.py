"""The pod-arrival benchmark and its distributed path on CPU (gloo, simulated executor).

The driver runs `bench.py` under torch.distributed.run with one rank per GPU; here the
same code path runs with world_size 2 on gloo so placement broadcast, telemetry
all-gather and the max-over-ranks timing are exercised without a GPU.
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_sim_single_process():
    from k8s_gpu_scheduler_amd.parallel.podbench import main
    r = main(["--sim", "--gpus", "4", "--steps", "3", "--warmup", "1"])
    assert r["n_gpus"] == 4 and r["config"]["global_batch"] == 16 and r["unscheduled"] == 0
    assert r["value"] > 0 and r["simulated"] is True
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
              "scaling", "vs_baseline", "dtype", "data", "config"):
        assert k in r
    # speed-of-light bookkeeping: the floor at the hardware peaks is below the floor at the
    # measured-best rates, and both are positive for a run that did work
    floor = r["roofline_floor_ms_per_step"]
    assert 0 < floor["peak"] <= floor["achievable"]
    assert r["sol_pct"]["peak"] <= r["sol_pct"]["achievable"] and r["achieved_hbm_tbps_per_gpu"] > 0


def test_bench_pinned_effort_level_is_recorded_and_held():
    """--plan-effort pins the planner's level (the simulated bench never adapts): the JSON's
    config records the level and that adaptation was off, and every epoch ran at that level."""
    from k8s_gpu_scheduler_amd.parallel.podbench import main
    r = main(["--sim", "--gpus", "2", "--steps", "3", "--warmup", "1", "--plan-effort", "2"])
    assert r["config"]["plan_effort"] == 2 and r["config"]["cp_adaptive"] == 0
    assert "cp_effort_down" not in r["config"]
    assert set(r["planner"]["effort_epochs"]) == {"2"} and r["planner"]["slot_policy"] == "lpt"


def test_bench_random_policy_runs():
    from k8s_gpu_scheduler_amd.parallel.podbench import main
    r = main(["--sim", "--gpus", "2", "--steps", "2", "--warmup", "1", "--policy", "random"])
    assert r["config"]["policy"] == "random" and r["unscheduled"] == 0


@pytest.mark.slow
def test_bench_two_ranks_gloo(tmp_path):
    out = tmp_path / "r.json"
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", "29611", os.path.join(ROOT, "bench.py"),
           "--sim", "--gpus", "2", "--steps", "3", "--warmup", "1", "--out", str(out)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1                        # rank 0 prints exactly one JSON line
    r = json.loads(lines[0])
    assert r["n_gpus"] == 2 and r["config"]["parallelism"] == "dp2" and r["config"]["global_batch"] == 8
    assert json.loads(out.read_text())["value"] == r["value"]


def test_resize_loop_clears_backlog_sim():
    """Config 5 (simulated executor): with the admission loop the over-requested pods are
    shrunk to what their SLO needs, so the backlog that builds without it disappears."""
    from k8s_gpu_scheduler_amd.parallel import resize_loop
    on = resize_loop.run(n_gpus=2, epochs=15, rate=3.0, sim=True, resize=True)
    off = resize_loop.run(n_gpus=2, epochs=15, rate=3.0, sim=True, resize=False)
    assert on["created"] == off["created"]
    assert on["completed"] > off["completed"] and on["final_backlog"] < off["final_backlog"]
    assert on["mean_cu_request_placed"] < 128 and on["admission"]["resized"] > 0
    # the history the admission resized from was written by the node agent's per-process path
    assert on["history"]["samples"] == on["completed"]


def test_dead_control_plane_raises_instead_of_hanging():
    """A crashed control-plane process must fail the bench (torchrun then stops every
    rank), never leave rank 0 blocked at the next schedule forever."""
    from k8s_gpu_scheduler_amd.parallel.controlplane_proc import ControlPlaneProc
    cp = ControlPlaneProc(n_gpus=1, pods_per_gpu=2, iters=2, seed=0)
    try:
        assert cp.schedule_epoch().shape == (2, 8)
        cp.request_schedule()
        cp._p.kill()
        cp._p.join()
        with pytest.raises((RuntimeError, OSError)):
            # the child may have answered the request before the kill landed: that
            # buffered reply is returned once, the next read must then raise
            cp.get_schedule()
            cp.get_schedule()
        with pytest.raises((RuntimeError, OSError)):
            cp.schedule_epoch()
    finally:
        cp._outstanding = 0
        cp.close()


def _bench(args, timeout=300):
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                          timeout=timeout, env=env, cwd=ROOT)


def test_bench_sim_gpus4_without_torchrun_reports_4():
    """`python bench.py --sim --gpus 4` (no torchrun): N simulated GPUs, one JSON line."""
    p = _bench(["--sim", "--gpus", "4", "--steps", "2", "--warmup", "1"])
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    r = json.loads(lines[0])
    assert r["n_gpus"] == 4 and r["config"]["parallelism"] == "dp4"


@pytest.mark.slow
def test_bench_self_launches_one_process_per_rank():
    """`--launch spawn` without torchrun: the parent starts N rank processes itself (here
    gloo ranks of the simulated executor) -- the path `bench.py --gpus N` takes on a GPU
    host, where the parent never touches the GPU."""
    p = _bench(["--sim", "--launch", "spawn", "--gpus", "2", "--steps", "2", "--warmup", "1"])
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1                        # only rank 0 prints
    r = json.loads(lines[0])
    assert r["n_gpus"] == 2 and r["config"]["parallelism"] == "dp2" and r["config"]["global_batch"] == 8


def test_bench_more_gpus_than_visible_fails_fast():
    """No silent clamp: asking for 2 GPUs on a host with fewer fails with rc != 0."""
    import time
    t = time.time()
    p = _bench(["--gpus", "2", "--steps", "1", "--warmup", "0"], timeout=120)
    assert p.returncode != 0
    assert "GPU" in p.stderr and not [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert time.time() - t < 60


def test_launcher_propagates_rank_failure():
    from k8s_gpu_scheduler_amd.parallel.launch import spawn
    code = "import os,sys,time; r=int(os.environ['RANK']); time.sleep(0.2*r); sys.exit(3 if r==1 else 0)"
    assert spawn([sys.executable, "-c", code], 2, require_gpus=False) == 3
    code = ("import os; assert os.environ['WORLD_SIZE']=='3' and os.environ['MASTER_ADDR']=='127.0.0.1'; "
            "assert os.environ['RANK']==os.environ['LOCAL_RANK']")
    assert spawn([sys.executable, "-c", code], 3, require_gpus=False) == 0


def test_bench_dist_single_takes_the_collective_path():
    """--dist-single: a 1-rank process group runs the multi-rank collective code (broadcast,
    all-gather, all-reduce, barriers) -- on a 1-GPU box that is the RCCL path of the scaling run."""
    from k8s_gpu_scheduler_amd.parallel.podbench import main
    import torch.distributed as dist
    r = main(["--sim", "--dist-single", "1", "--steps", "3", "--warmup", "1", "--control-plane", "inline"])
    assert r["n_gpus"] == 1 and r["value"] > 0 and r["unscheduled"] == 0
    assert not dist.is_initialized() and "WORLD_SIZE" not in os.environ
    with pytest.raises(SystemExit):
        main(["--sim", "--dist-single", "1", "--gpus", "2", "--steps", "1", "--warmup", "0"])


def test_bench_dump_outputs_sim_is_reproducible_and_steps_are_counted(tmp_path):
    """--dump-outputs on the simulated executor (no kernels: placements.npy only): two runs with
    the same arguments write the same float32 rows, --steps sets the timed epochs, and --full
    (nothing beyond the plain run yet) reports the same result line."""
    import numpy as np

    from k8s_gpu_scheduler_amd.models import workloads as W
    from k8s_gpu_scheduler_amd.parallel.podbench import main
    got = []
    for d, extra in (("a", []), ("b", ["--full"])):
        r = main(["--sim", "--gpus", "2", "--steps", "4", "--warmup", "1", "--dump-outputs", str(tmp_path / d), *extra])
        assert r["steps"] == 4 and r["ms_per_step"] > 0 and r["value"] > 0
        # 4 timed epochs of 8 pods: value (pods/s) x ms_per_step x steps counts them
        assert r["value"] * r["ms_per_step"] * 4 / 1e3 == pytest.approx(32, rel=1e-3)
        assert sorted(os.listdir(tmp_path / d)) == ["placements.npy"]
        got.append((r, np.load(tmp_path / d / "placements.npy")))
    (ra, pa), (rb, pb) = got
    assert set(ra) == set(rb)
    assert pa.dtype == np.float32 and pa.shape == (8, 5) and np.array_equal(pa, pb)
    # units, workload id, iterations, SLO, masked of quarter-GPU Burstable pods, sorted by workload
    assert (pa[:, 0] == 2).all() and (pa[:, 2] == 20).all() and (pa[:, 4] == 0).all() and (pa[:, 3] > 0).all()
    assert ((0 <= pa[:, 1]) & (pa[:, 1] < len(W.NAMES))).all() and (np.diff(pa[:, 1]) >= 0).all()


def test_bench_operands_do_not_depend_on_the_process():
    """The executor seeds a workload's operands from its name: another process, whose str hashes
    differ, must draw the same ones (two bench runs are compared output for output)."""
    import torch

    from k8s_gpu_scheduler_amd.models import workloads as W
    from k8s_gpu_scheduler_amd.parallel.executor import _Buffers
    from k8s_gpu_scheduler_amd.parallel.podbench import DUMP_MAX_ELEMS, dump_sample
    code = ("import sys, torch; sys.path.insert(0, sys.argv[1]);"
            "from k8s_gpu_scheduler_amd.models import workloads as W;"
            "from k8s_gpu_scheduler_amd.parallel.executor import _Buffers;"
            "a, bt = _Buffers(W.CATALOG['onnx_mobilenet_1024'], torch.device('cpu')).ops[2][1][:2];"
            "print(a.double().sum().item(), bt.double().sum().item(), a[3, 5].item(), bt[7, 11].item())")
    seed = "1" if os.environ.get("PYTHONHASHSEED") != "1" else "2"
    p = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, PYTHONHASHSEED=seed, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES=""))
    assert p.returncode == 0, p.stderr[-2000:]
    a, bt = _Buffers(W.CATALOG["onnx_mobilenet_1024"], torch.device("cpu")).ops[2][1][:2]
    assert [float(x) for x in p.stdout.split()] == [a.double().sum().item(), bt.double().sum().item(),
                                                    a[3, 5].item(), bt[7, 11].item()]
    # the dump's sample of a large output: fixed per (pod, kernel), ascending, in range; small outputs whole
    assert dump_sample(DUMP_MAX_ELEMS, 0, 0) is None
    i0, i1 = dump_sample(10 * DUMP_MAX_ELEMS + 3, 1, 2), dump_sample(10 * DUMP_MAX_ELEMS + 3, 1, 2)
    assert torch.equal(i0, i1) and i0.shape == (DUMP_MAX_ELEMS,) and (i0[1:] >= i0[:-1]).all()
    assert 0 <= int(i0[0]) and int(i0[-1]) < 10 * DUMP_MAX_ELEMS + 3
    assert not torch.equal(i0, dump_sample(10 * DUMP_MAX_ELEMS + 3, 2, 2))


@pytest.mark.gpu
def test_dump_outputs_match_fp32_reference_on_gpu(tmp_path):
    """What --dump-outputs writes for a step the executor ran: every kernel output of the step's
    pods (bf16 GEMMs with and without a stream pass between them, the HBM stream kernel), equal
    to a PyTorch fp32 evaluation of the same op on the workload's seeded operands."""
    import numpy as np
    import torch

    from k8s_gpu_scheduler_amd.models import workloads as W
    from k8s_gpu_scheduler_amd.parallel.executor import DeviceExecutor, _Buffers
    from k8s_gpu_scheduler_amd.parallel.podbench import DUMP_MAX_ELEMS, _runs_for, dump_outputs, dump_sample
    names = ["tensorflow_ssd_mobilenet_1024", "onnx_mobilenet_1024", "onnx_resnet50_1024", "onnx_mobilenet_1024"]
    # rows as the scheduler returns them: gpu, first unit, units, workload id, iterations, SLO, masked, policy
    arr = np.array([[0, 2 * i, 2, W.INDEX[n], 1, 1000 * (4 - i), 0, 0] for i, n in enumerate(names)], dtype=np.int32)
    runs = _runs_for(arr, 0)
    ex = DeviceExecutor(0)
    try:
        ex.launch_epoch(runs)
        torch.cuda.synchronize()
        files = dump_outputs(str(tmp_path), arr, runs, ex)
    finally:
        ex.close()
    pl = np.load(tmp_path / "placements.npy")
    # rows by workload id (the onnx names sort before the tensorflow one), then SLO
    assert pl.dtype == np.float32 and np.array_equal(pl, arr[[3, 1, 2, 0]][:, 2:7].astype(np.float32))
    assert sorted(os.path.basename(f) for f in files) == sorted(
        ["placements.npy"] + [f"pod{k}_op{j}.npy" for k in range(4) for j in range(3)])
    assert sum(os.path.getsize(f) for f in files) <= 64 << 20
    refs = {}
    for k in range(4):
        w = W.CATALOG[W.NAMES[int(pl[k, 1])]]
        if w.name not in refs:
            refs[w.name] = _Buffers(w, torch.device("cuda", 0))
        for j, (o, t) in enumerate(refs[w.name].ops):
            got = np.load(tmp_path / f"pod{k}_op{j}.npy")
            assert got.dtype == np.float32
            if o.is_gemm:
                a, bt, bias, _ = t
                ref = torch.relu(a.float() @ bt.float().T + bias) if o.relu else a.float() @ bt.float().T + bias
            else:
                ref = t[1] + 1.0001 * t[2]
            ref = ref.reshape(-1)
            idx = dump_sample(ref.numel(), k, j)
            assert got.shape == (min(ref.numel(), DUMP_MAX_ELEMS),)
            ref = (ref if idx is None else ref[idx.to(ref.device)]).cpu().numpy()
            # GEMM: the bf16 rounding of an fp32 accumulation -- half a bf16 ulp is at most 2^-8
            # relative -- plus 1e-3 absolute for what the accumulation order changes in the fp32 sum
            # before it is rounded (|a| <= 1, |b| <= 0.05, K <= 2560: below 1e-4); the stream kernel is
            # one fp32 multiply-add, exact up to its fusing
            tol = 2.0 ** -8 * np.abs(ref) + 1e-3 if o.is_gemm else 2.0 ** -22 * np.abs(ref)
            err = np.abs(got - ref)
            print(f"pod{k} {w.name} op{j} {o.kind}: max err {err.max():.3g}, max |ref| {np.abs(ref).max():.3g}")
            assert (err <= tol).all(), (w.name, j, float(err.max()))


@pytest.mark.gpu
def test_bench_rccl_collective_path_on_gpu(tmp_path):
    """The scaling run's collective code over RCCL on one MI355X: bench.py --dist-single runs a
    1-rank nccl group (placement broadcast on the side stream, telemetry all-gather, result
    all-reduce / all-gather, barriers, destroy) through the real HIP executor -- and, with
    --dump-outputs, leaves the last step's placements and its 4 pods' 3 kernel outputs each."""
    import numpy as np
    out, dump = tmp_path / "b.json", tmp_path / "dump"
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dist-single", "1", "--steps", "5",
                        "--warmup", "2", "--out", str(out), "--dump-outputs", str(dump)],
                       env=env, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    r = json.loads(out.read_text())
    assert r["n_gpus"] == 1 and r["simulated"] is False and r["value"] > 0 and r["unscheduled"] == 0
    assert r["steps"] == 5 and r["ms_per_step"] > 0
    files = sorted(os.listdir(dump))
    assert files == sorted(["placements.npy"] + [f"pod{k}_op{j}.npy" for k in range(4) for j in range(3)])
    assert sum(os.path.getsize(dump / f) for f in files) <= 64 << 20
    for f in files:
        v = np.load(dump / f)
        assert v.dtype == np.float32 and np.isfinite(v).all() and np.abs(v).max() > 0, f
