"""bench.py on the GPU: a plain run (the headline only) with --dump-outputs — the last timed step's image, radii and leaf gradients
as float32 .npy files, per-Gaussian arrays as the fixed, seeded sample of DUMP_ROWS rows when P is larger (c2: 100 k splats)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_bench_run_dumps_the_last_step(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    d = tmp_path / "out"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2", "--workload", "c2",
                        "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    assert out["steps"] == 4 and out["ms_per_step"] > 0 and out["unit"] == "Msplats/s" and out["dtype"] == "f32"
    assert "kernels" not in out and "cpu_baseline" not in out   # --full only
    rows = 65536   # bench.DUMP_ROWS < P = 100 k
    want = {"color": (3, 1080, 1920), "radii": (rows,), "grad_means3D": (rows, 3), "grad_opacities": (rows, 1),
            "grad_shs": (rows, 16, 3), "grad_scales": (rows, 3), "grad_rotations": (rows, 4), "grad_means2D": (rows, 3)}
    assert sorted(os.listdir(d)) == sorted(n + ".npy" for n in want)
    total = 0
    for name, shape in want.items():
        a = np.load(d / (name + ".npy"))
        assert a.dtype == np.float32 and a.shape == shape and np.isfinite(a).all(), name
        total += a.nbytes
    assert total <= 64 * 2 ** 20
    assert np.load(d / "color.npy").max() > 0 and np.abs(np.load(d / "grad_means3D.npy")).max() > 0
    assert (np.load(d / "radii.npy") > 0).any()
