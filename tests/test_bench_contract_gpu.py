"""bench.py's output contract, on the reduced `mini` architecture (development workload: seconds, not a reportable number):
one JSON line from rank 0 with the keys the driver reads, at N = 1 and -- both ranks on the one GPU, over RCCL with a real
peer (each rank claims its own NCCL_HOSTID: tests/test_distributed_gpu.py) -- at N = 2."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUICK = ["--workload", "mini", "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-reference-loop", "--no-nested",
         "--no-nested1024", "--no-sampling"]
KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
        "dtype", "data", "config", "roofline"}


def _line(cmd, env):
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert out.returncode == 0 and len(lines) == 1, (out.returncode, out.stdout[-2000:], out.stderr[-3000:])
    return json.loads(lines[0])


def _env(**kw):
    env = dict(os.environ, BENCH_SETTLE_STEPS="1", HSA_ENABLE_IPC_MODE_LEGACY="0", **kw)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    return env


def test_one_rank_line_has_the_contract_keys():
    d = _line([sys.executable, "bench.py", "--gpus", "1", "--full"] + QUICK, _env())
    assert KEYS <= set(d), sorted(KEYS - set(d))
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["scaling"] == "weak" and d["vs_baseline"] is None and d["dtype"] == "bf16" and "synthetic" in d["data"]
    assert d["value"] > 0 and abs(d["value"] * d["ms_per_step"] / 1e3 - 1.0) < 1e-3      # N x steps/s, N = 1
    assert "workload" in d["config"] and "model" not in d["config"]
    r = d["roofline"]
    assert {"bound", "achieved", "peak", "unit", "frac", "traffic"} <= set(r) and r["bound"] in ("mfma", "hbm")
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    assert "cpu_baseline" not in d          # --no-cpu-baseline (a --full run carries it: profiles/r06_bench_unet64_b64_line.json)
    assert len(d["binary"]["sha256"]) == 64


def test_two_ranks_on_one_gpu_over_rccl():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29547", "bench.py", "--gpus", "2", "--no-roofline"] + QUICK
    d = _line(cmd, _env(MDM_BENCH_DEVICE="0"))
    assert d["n_gpus"] == 2 and d["scaling"] == "weak"
    comm = d["config"]["comm"]
    assert comm["backend"] == "nccl" and comm["world_size"] == 2 and len(comm["bucket_timeline_ms"]) >= 1
    assert abs(d["value"] * d["ms_per_step"] / 1e3 - 2.0) < 2e-3                           # whole job: 2 x steps/s


def test_plain_run_times_only_the_step_and_dumps_its_outputs(tmp_path):
    """without --full the line carries the headline figure alone; --dump-outputs writes the last timed step's results, and
    a second run with the same arguments starts from the same inputs"""
    import numpy as np

    runs = []
    for k in range(2):
        out = tmp_path / ("run%d" % k)
        d = _line([sys.executable, "bench.py", "--gpus", "1", "--workload", "mini", "--steps", "3", "--warmup", "1",
                   "--dump-outputs", str(out)], _env())
        assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0
        assert abs(d["value"] * d["ms_per_step"] / 1e3 - 1.0) < 1e-3
        for leg in ("roofline", "sampling", "nested256", "reference_loop", "nested1024_sampling"):
            assert d[leg] is None, leg
        assert "cpu_baseline" not in d
        files = {p.name: np.load(p) for p in out.glob("*.npy")}
        assert {"loss.npy", "losses.npy", "times.npy", "x_t.npy", "means.npy", "targets.npy", "params_sample.npy",
                "ema_params_sample.npy"} <= set(files)
        assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in files.values())
        assert sum(p.stat().st_size for p in out.glob("*.npy")) <= 64 << 20
        runs.append(files)
    assert np.array_equal(runs[0]["times.npy"], runs[1]["times.npy"])
    for name in ("x_t.npy", "targets.npy"):
        assert np.allclose(runs[0][name], runs[1][name], rtol=0, atol=1e-6), name
