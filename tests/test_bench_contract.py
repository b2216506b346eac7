"""bench.py prints ONE JSON line with the keys the driver reads (task statement, section 4); `--full` adds the roofline, a plain run
times the headline steps only and can write what its last step computed (`--dump-outputs`)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_line_has_the_contract_keys():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--batch", "8",
                          "--no-cpu-baseline", "--full"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k, typ in (("metric", str), ("value", float), ("unit", str), ("n_gpus", int), ("steps", int), ("warmup", int),
                   ("ms_per_step", float), ("higher_is_better", bool), ("scaling", str), ("dtype", str), ("data", str),
                   ("config", dict), ("roofline", dict)):
        assert isinstance(d[k], typ), k
    assert d["vs_baseline"] is None and d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1
    assert d["metric"] == "denoising_steps_per_sec" and d["unit"] == "reaction-steps/s" and d["scaling"] == "weak"
    assert "workload" in d["config"] and "model" not in d["config"]
    r = d["roofline"]
    assert r["bound"] in ("hbm", "mfma") and r["unit"] in ("GB/s", "TFLOP/s")
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9 and 0 < r["frac"] < 1
    assert abs(d["value"] - 8 * 3 / (d["ms_per_step"] * 3e-3)) / d["value"] < 1e-6


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs(tmp_path):
    """A plain run carries the headline keys and none of the --full legs; --dump-outputs writes the last timed step's outputs (one
    float32 array of velocities and features per object), and two runs with the same arguments compute the same outputs."""
    dumps = []
    for k in range(2):
        d = tmp_path / f"run{k}"
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--batch", "8",
                              "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1
        line = json.loads(lines[0])
        assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["dtype"] == "f32"
        assert abs(line["value"] - 8 * 3 / (line["ms_per_step"] * 3e-3)) / line["value"] < 1e-6
        for leg in ("roofline", "sampler_loop", "train_step", "second_line", "config5", "general_edge_lists", "cpu_baseline"):
            assert line.get(leg) is None, leg
        dumps.append({f.name: np.load(f) for f in sorted(d.iterdir())})
    assert sorted(dumps[0]) == ["output_P.npy", "output_R.npy", "output_TS.npy"]
    for name, a in dumps[0].items():
        assert a.dtype == np.float32 and a.ndim == 2 and a.shape[0] == 8 * 23 and a.shape[1] > 3 and np.isfinite(a).all(), name
        np.testing.assert_allclose(dumps[1][name], a, rtol=1e-5, atol=1e-6)
