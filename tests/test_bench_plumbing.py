"""bench.py's N > 1 plumbing on CPU: launched exactly as the driver launches it (torch.distributed.run, one rank per GPU)
with a stub engine in place of the HIP library.  Checked: rank 0's RCCL id reaches every rank, the barriers bracket the
timed region, the elapsed time is the MAX over ranks, ONE JSON line comes out, on rank 0's stdout only, `value` is the
whole-job aggregate, the rank processes exit 0 on their own (no os._exit) and never import torch (the launcher is the
only torch process: the ranks meet through debvader_amd.parallel.HostGroup).  A second launch without torch.distributed.run
(two plain processes with RANK / WORLD_SIZE / MASTER_* set, MASTER_PORT free) covers HostGroup's direct-port mode."""
import glob
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("world", [2, 8])
def test_multi_rank_bench_launch_with_a_stub_engine(tmp_path, world):
    """world 2, and world 8 - the node the driver's scaling run uses: rendezvous of eight ranks beside
    torchrun's store, eight communicator reports gathered into `multi_rank`, `verified` true, MAX over eight ranks."""
    log = str(tmp_path / "stub")
    env = dict(os.environ, DV_BENCH_STUB_ENGINE="tests.stub_engine", DV_STUB_LOG=log, PYTHONPATH=ROOT, OMP_NUM_THREADS="1")
    steps, warmup = 4, 2
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", str(world), "--steps", str(steps),
           "--warmup", str(warmup)]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1, r.stdout                         # one JSON line, from rank 0 only
    d = json.loads(lines[0])
    assert d["n_gpus"] == world and d["steps"] == steps and d["warmup"] == warmup and d["scaling"] == "weak"
    assert d["config"]["global_batch"] == 256 * world and d["config"]["parallelism"] == f"dp{world}"
    # the slowest rank (rank world-1: 5 + 20 ms per rank index and step) sets the time: MAX over ranks, not rank 0's own 5 ms
    assert d["ms_per_step"] >= 4.0 + 20.0 * (world - 1), d["ms_per_step"]
    assert abs(d["value"] - 256 * world * steps / (d["ms_per_step"] * 1e-3 * steps)) <= 1e-6 * d["value"]
    # the N > 1 line is self-verifying: what RCCL reports for the communicator on EVERY rank, which
    # device each rank drives, the communication of a step and its exposed part, and a whole-step fraction
    mr = d["multi_rank"]
    assert mr["world"] == world and mr["rccl_ranks"] == [world] * world and mr["rccl_rank_ids"] == list(range(world))
    assert [v["rank"] for v in mr["devices"]] == list(range(world)) and mr["distinct_devices"] == world
    assert len({v["pci_bus_id"] for v in mr["devices"]}) == world and mr["verified"] is True and mr["rehearsal"] is False
    assert mr["collectives_per_step"] == 5 and abs(mr["comm_ms_per_step"] - 0.4) < 1e-9
    assert abs(mr["exposed_comm_ms_per_step"] - 0.05 * world) < 1e-9          # MAX over ranks (rank r: 0.05 * (r + 1))
    assert d["roofline"]["whole_step_frac"] > 0 and d["roofline"]["bound"] == "mfma" and "rehearsal" not in d
    logs = {}
    for f in glob.glob(log + ".*"):
        logs[int(f.rsplit(".", 1)[1])] = [json.loads(ln) for ln in open(f)]
    assert sorted(logs) == list(range(world))
    uids = {rk: next(e["uid"] for e in ev if e["event"] == "ctx") for rk, ev in logs.items()}
    assert len(set(uids.values())) == 1 and len(uids[0]) == 256         # rank 0's 128 bytes on every rank
    for rk, ev in logs.items():
        ts = [e for e in ev if e["event"] == "train_steps"]
        assert [t["steps"] for t in ts] == [warmup, steps, steps]       # warm-up, the timed region, the comm-timing pass
        assert all(t["global_batch"] == 256 * world and t["B"] == 256 for t in ts)
        assert sum(e["event"] == "sync" for e in ev) >= 3      # before the timed region, inside it and at its end
        assert not any(e.get("torch_loaded") for e in ev), "torch was imported into a rank process"
        assert ev[-1]["event"] == "close"                      # the context was closed, the process left normally


def test_two_plain_processes_meet_on_master_port(tmp_path):
    """The same bench without a launcher: RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT by hand, the port free, so rank 0
    listens on it directly."""
    log = str(tmp_path / "stub")
    port, world, steps = _free_port(), 2, 3
    procs = []
    for rank in range(world):
        env = dict(os.environ, DV_BENCH_STUB_ENGINE="tests.stub_engine", DV_STUB_LOG=log, PYTHONPATH=ROOT, RANK=str(rank),
                   LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.pop("TORCHELASTIC_USE_AGENT_STORE", None)
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(world), "--steps", str(steps),
                                       "--warmup", "1"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env,
                                      cwd=ROOT))
    outs = [p.communicate(timeout=300) for p in procs]
    assert [p.returncode for p in procs] == [0, 0], [o[1][-1500:] for o in outs]
    lines0 = [ln for ln in outs[0][0].splitlines() if ln.strip().startswith("{")]
    assert len(lines0) == 1 and not [ln for ln in outs[1][0].splitlines() if ln.strip().startswith("{")]
    d = json.loads(lines0[0])
    assert d["n_gpus"] == world and d["ms_per_step"] >= 24.0


def test_bench_config_flag_selects_the_baseline_configuration(tmp_path):
    """--config 3 (128 px, 64 per GPU) and --config 2 (bf16) under the driver's launch line: the line names the
    configuration, the per-GPU batch and the stamp geometry it ran."""
    for conf, want_batch, want in ((3, 64, "128x128x6"), (2, 256, "59x59x6")):
        log = str(tmp_path / f"stub{conf}")
        env = dict(os.environ, DV_BENCH_STUB_ENGINE="tests.stub_engine", DV_STUB_LOG=log, PYTHONPATH=ROOT, OMP_NUM_THREADS="1")
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
               "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
               "--config", str(conf)]
        r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        d = json.loads([ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")][0])
        assert f"configs[{conf}]" in d["config"]["workload"] and d["config"]["per_gpu_batch"] == want_batch
        assert d["config"]["global_batch"] == 2 * want_batch and want in d["metric"]
        assert d["dtype"] == ("bf16" if conf == 2 else "f32") and d["multi_rank"]["verified"]


def test_plain_one_gpu_run_times_its_steps_and_dumps_the_last_one(tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR`, the stub engine in place of the HIP library: the engine
    runs the W warm-up steps and the K timed steps and nothing else, the line carries ms_per_step, and DIR holds the loss
    scalars and every weight after the last timed step as float32 .npy files - the same files on a second run."""
    dumps = []
    for run in range(2):
        log, out = str(tmp_path / f"stub{run}"), str(tmp_path / f"out{run}")
        env = dict(os.environ, DV_BENCH_STUB_ENGINE="tests.stub_engine", DV_STUB_LOG=log, PYTHONPATH=ROOT, OMP_NUM_THREADS="1")
        for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
            env.pop(k, None)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
                            "--dump-outputs", out], capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")]
        assert len(lines) == 1, r.stdout
        d = json.loads(lines[0])
        assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 2 and d["ms_per_step"] >= 5.0
        assert abs(d["value"] - 256 / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
        assert d["higher_is_better"] is True and d["unit"] == "stamps/s" and d["dtype"] == "f32"
        ev = [json.loads(ln) for ln in open(log + ".0")]
        assert [e["steps"] for e in ev if e["event"] == "train_steps"] == [2, 3]
        files = sorted(os.listdir(out))
        assert {"loss.npy", "nll_mean.npy", "kl_reg.npy", "mse.npy", "dec.convt3.kernel.npy"} <= set(files)
        arrs = {f: np.load(os.path.join(out, f)) for f in files}
        assert all(a.dtype == np.float32 for a in arrs.values())
        assert arrs["dec.convt3.kernel.npy"].ndim == 4 and float(arrs["loss.npy"]) == 1.0
        assert sum(os.path.getsize(os.path.join(out, f)) for f in files) <= 64 * 10**6
        dumps.append(arrs)
    assert dumps[0].keys() == dumps[1].keys() and all(np.array_equal(dumps[0][f], dumps[1][f]) for f in dumps[0])


def test_dump_outputs_keeps_a_fixed_sample_of_outputs_over_the_limit(tmp_path):
    """Outputs over the limit are cut to a seeded sample of each array, the same elements on every call; float64 stays
    float64, everything else is written as float32."""
    import bench

    big = np.arange(9 * 10**6, dtype=np.float64)              # 72 MB
    small = np.arange(1000, dtype=np.int32).reshape(10, 100)
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), {"big": big, "small": small, "loss": np.float32(2.5)})
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["big.npy", "loss.npy", "small.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 * 10**6
    a, b = (np.load(tmp_path / run / "big.npy") for run in ("a", "b"))
    assert a.dtype == np.float64 and 0 < a.size < big.size and np.array_equal(a, b)
    assert np.all(np.diff(a) > 0) and a[0] >= 0 and a[-1] < big.size      # distinct elements of `big`, in index order
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float32 and s.ndim == 1 and np.isin(s, np.arange(1000)).all()
    assert np.load(tmp_path / "a" / "loss.npy").size == 1
