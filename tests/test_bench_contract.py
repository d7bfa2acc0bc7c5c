"""bench.py prints ONE JSON line with the fields the driver reads (metric / value / unit / n_gpus / steps / warmup /
ms_per_step / higher_is_better / scaling / vs_baseline / dtype / data / config.workload); with --full also the `roofline`
and `cpu_baseline` objects. A plain run writes the outputs of its last timed step with --dump-outputs. Checked here on
short runs so that a broken bench shows up in the GPU suite."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
@pytest.mark.parametrize("workload", ["resnet18", "conv3x3", "mobilenet"])
def test_bench_prints_the_contract_line(workload):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--workload", workload, "--full"], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["value"] > 0
    assert d["vs_baseline"] is None and d["dtype"] == "f32" and d["data"] == "synthetic" and d["scaling"] == "weak"
    assert "workload" in d["config"] and "model" not in d["config"]
    roof = d["roofline"]
    assert roof["bound"] in ("hbm", "mfma") and roof["unit"] in ("GB/s", "TFLOP/s")
    assert roof["peak"] in (8000.0, 157.3) and abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-3
    assert "traffic" in roof and "traffic_source" in roof   # null unless a PMC summary of THESE kernel sources is on file
    if workload == "resnet18":   # the default run also times configs[1] and configs[4] briefly
        side = d["workloads"]
        assert set(side) == {"conv3x3", "mobilenet"}
        for w in side.values():
            assert w["images_per_s"] > 0 and w["roofline"]["bound"] in ("hbm", "mfma") and w["kernel_classes"]
            assert w["cpu_baseline"]["kind"] == "reference" and w["cpu_baseline"]["value"] > 0  # per workload
    else:
        assert "workloads" not in d
    cpu = d["cpu_baseline"]
    assert cpu["kind"] in ("reference", "port") and cpu["value"] > 0 and cpu["cores"] >= 1 and cpu["sample"]
    assert cpu["host_cores"] == os.cpu_count()
    if "winograd" in roof["kernel"]:
        assert 0 < roof["frac_unpadded"] <= roof["frac"]


def _plain_run(workload, dump_dir):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--workload", workload, "--dump-outputs", str(dump_dir)], cwd=ROOT, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
@pytest.mark.parametrize("workload,names", [("resnet18", {"prob", "params", "grad_arena"}), ("conv3x3", {"y", "dw", "db"})])
def test_plain_run_is_lean_and_dumps_the_same_outputs_every_time(tmp_path, workload, names):
    """without --full: the headline fields only (no profiling, side workloads or CPU baseline); --dump-outputs writes the
    last timed step's arrays as float .npy files, at most 64 MB in all, identical in two runs with the same arguments"""
    a = _plain_run(workload, tmp_path / "a")
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "n_gpus", "steps", "warmup"):
        assert key in a, key
    assert a["steps"] == 3 and a["warmup"] == 1 and a["warmup_extra"] == 0 and a["value"] > 0 and a["ms_per_step"] > 0
    assert a["metric"] == "images/sec fwd+bwd" and a["unit"] == "images/s" and a["higher_is_better"] is True
    assert abs(a["value"] - 3 * a["config"]["batch_per_gpu"] / (a["ms_per_step"] * 3e-3)) < 1e-2 * a["value"]
    for key in ("roofline", "kernel_classes", "kernel_classes_alone", "cpu_baseline", "workloads"):
        assert key not in a, key
    files = sorted(os.listdir(tmp_path / "a"))
    assert {f[:-4] for f in files} == names and all(f.endswith(".npy") for f in files)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 << 20
    _plain_run(workload, tmp_path / "b")
    for f in files:
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.dtype in (np.float32, np.float64) and x.size > 0 and np.isfinite(x).all(), f
        assert x.shape == y.shape and np.array_equal(x, y), f
