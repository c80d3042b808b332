"""The driver's bench.py contract (CPU, gloo): one process and a torchrun group of ranks each print exactly
one JSON line from rank 0 with the BASELINE.json metric, whole-job images/sec, the timed step count and a
step time consistent with the value; the data-parallel replicas end bit-identical.  The same script runs
one rank per MI355X over RCCL / the xGMI kernel on a GPU node (tests/test_xgmi_gpu.py covers that path)."""
import json
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
        "vs_baseline", "dtype", "data", "config"}


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("world", [1, 4])
def test_bench_json_line_contract(world):
    env = dict(os.environ, TDE_BENCH_WARM_MS="0", OMP_NUM_THREADS="1", TDE_HEARTBEAT="0", CUDA_VISIBLE_DEVICES="")
    args = ["--gpus", str(world), "--steps", "6", "--warmup", "2"]
    if world == 1:
        cmd = [sys.executable, os.path.join(ROOT, "bench.py")] + args
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
               "--master-addr=127.0.0.1", f"--master-port={_port()}", os.path.join(ROOT, "bench.py")] + args
    r = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    res = json.loads(lines[0])
    assert KEYS <= set(res), set(res) ^ KEYS
    base = json.load(open(os.path.join(ROOT, "BASELINE.json")))
    assert res["metric"] == base["metric"]
    assert res["n_gpus"] == world and res["steps"] == 6 and res["warmup"] == 2
    assert res["scaling"] == "weak" and res["higher_is_better"] is True and res["unit"] == "images/sec"
    cfg = res["config"]
    assert cfg["model"] == "mnist_cnn" and cfg["global_batch"] == 64 * world
    assert cfg["parallelism"] == f"dp{world}"
    # value is the whole-job rate implied by the timed step time
    implied = cfg["global_batch"] * 1000.0 / res["ms_per_step"]
    assert abs(res["value"] - implied) <= 1e-3 * implied + 1.0
    if world > 1:
        assert "replicas_identical=True" in r.stdout, r.stdout[-3000:]


def _plain(extra, **env_extra):
    env = dict(os.environ, OMP_NUM_THREADS="1", TDE_HEARTBEAT="0", CUDA_VISIBLE_DEVICES="", **env_extra)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "TF_CONFIG"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "6", "--warmup", "2"]
                       + extra, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0])


def test_bench_dump_outputs_repeat_from_run_to_run(tmp_path):
    """--dump-outputs writes every model variable (float32) and the loss / accuracy (float64) left by one
    replay of the timed execution from the initial weights as DIR/<name>.npy, and two runs with the same
    arguments write the same values although their warm-ups run a different number of executions (the
    time-based part of the warm-up on and off)."""
    import numpy as np
    a = _plain(["--dump-outputs", str(tmp_path / "a")], TDE_BENCH_WARM_MS="0")
    b = _plain(["--dump-outputs", str(tmp_path / "b")], TDE_BENCH_WARM_MS="150")
    assert a["config"]["warmup_steps_run"] < b["config"]["warmup_steps_run"]
    assert a["steps"] == 6 and a["config"]["repeat_ms_per_step"] == []   # a plain run: no repeated measurement
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert {"loss.npy", "accuracy.npy", "conv2d.kernel.npy", "dense.kernel.npy", "dense_1.bias.npy"} <= set(names)
    total = 0
    for n in names:
        va, vb = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert va.dtype in (np.float32, np.float64) and np.isfinite(va).all(), n
        np.testing.assert_array_equal(va, vb, err_msg=n)
        total += va.nbytes
    assert total <= 64 << 20
    assert np.load(tmp_path / "a" / "dense.kernel.npy").shape == (5408, 64)
    assert 0.0 < float(np.load(tmp_path / "a" / "loss.npy")) < 10.0


@pytest.mark.gpu
def test_bench_dump_outputs_repeat_on_gpu(tmp_path):
    """The same on the fused hipGraph plan: the initial weights are loaded back between graph replays.
    The plan sums its split-K partial products with float atomics, so two runs agree to summation-order
    rounding (a few float32 ulp of the ~0.1-sized weights, < 1e-7 over 20 steps), not bitwise; one SGD step
    more or less moves the head's weights by lr * |g| ~ 1e-3 * 5e-2 = 5e-5, far above the 1e-6 allowed here."""
    import numpy as np
    res = []
    for name, warm in (("a", "20"), ("b", "120")):
        env = dict(os.environ, TDE_BENCH_WARM_MS=warm, TDE_HEARTBEAT="0")
        for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "TF_CONFIG"):
            env.pop(k, None)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup",
                            "5", "--dump-outputs", str(tmp_path / name)], env=env, cwd=ROOT, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-3000:]
        res.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0]))
    assert res[0]["config"]["plan"] == "fused_convnet" and res[0]["config"]["hipgraph"] is True
    assert res[0]["config"]["warmup_steps_run"] < res[1]["config"]["warmup_steps_run"]
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) and len(names) == 8, names
    for n in names:
        va, vb = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert np.isfinite(va).all(), n
        np.testing.assert_allclose(va, vb, rtol=0, atol=1e-6, err_msg=n)
    w0 = np.load(tmp_path / "a" / "dense_1.kernel.npy")
    assert float(np.abs(w0).max()) > 1e-2


def test_bench_full_adds_the_repeated_measurements():
    """--full keeps the result line's contract and adds the spread evidence (--repeats measurements)."""
    res = _plain(["--full", "--repeats", "3"], TDE_BENCH_WARM_MS="0")
    assert KEYS <= set(res) and res["steps"] == 6
    rep = res["config"]["repeat_ms_per_step"]
    assert len(rep) == 3 and all(v > 0 for v in rep)


def test_bench_multi_gpu_without_launcher_runs_mirrored():
    """`python bench.py --gpus 2` with no torchrun (VERDICT r5 Missing #1): one process drives both replicas
    with MirroredStrategy (BASELINE config 3; mnist_keras_distributed.py:243), rc 0, one JSON line."""
    env = dict(os.environ, TDE_BENCH_WARM_MS="0", OMP_NUM_THREADS="1", TDE_HEARTBEAT="0", CUDA_VISIBLE_DEVICES="")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "TF_CONFIG"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "6",
                        "--warmup", "2", "--repeats", "1"], env=env, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    res = json.loads(lines[0])
    base = json.load(open(os.path.join(ROOT, "BASELINE.json")))
    assert res["metric"] == base["metric"] and res["n_gpus"] == 2
    cfg = res["config"]
    assert cfg["strategy"] == "MirroredStrategy" and cfg["replicas_per_process"] == 2
    assert cfg["global_batch"] == 128 and cfg["parallelism"] == "dp2"
    assert "replicas_identical=True" in r.stdout, r.stdout[-3000:]


@pytest.mark.gpu
def test_bench_multi_gpu_without_launcher_on_gpu():
    """The same launcher-less command on a GPU box: with fewer visible GPUs than --gpus the replicas wrap onto
    cuda:0 (a rehearsal of the N-GPU Mirrored layout: one hipGraph per replica, in-process xGMI all-reduce),
    rc 0 and bit-identical replicas."""
    env = dict(os.environ, TDE_BENCH_WARM_MS="20", TDE_HEARTBEAT="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "TF_CONFIG"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "20",
                        "--warmup", "5", "--repeats", "1"], env=env, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    res = json.loads(lines[0])
    assert res["n_gpus"] == 2 and res["config"]["strategy"] == "MirroredStrategy"
    assert res["config"]["plan"] == "fused_convnet" and res["config"]["hipgraph"] is True
    assert "replicas_identical=True" in r.stdout, r.stdout[-3000:]


def test_bench_devices_list_sets_the_replica_count():
    """`--strategy mirrored --devices cpu,cpu` without --gpus: the device list is the replica count (the
    2-replica rehearsal form of tests/test_mirrored_gpu.py, `--devices 0,0`)."""
    env = dict(os.environ, TDE_BENCH_WARM_MS="0", OMP_NUM_THREADS="1", TDE_HEARTBEAT="0", CUDA_VISIBLE_DEVICES="")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "TF_CONFIG"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--strategy", "mirrored", "--devices",
                        "cpu,cpu", "--steps", "4", "--warmup", "1", "--repeats", "1"], env=env, cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    assert res["n_gpus"] == 2 and res["config"]["replicas_per_process"] == 2
