"""bench.py refuses a step that produced non-finite numbers.

After the timed loop, outside the timing, bench.py reduces the last step's loss terms and every
optimizer's flat parameter buffer to one device-side isfinite verdict, writes it to the JSON line
as "finite", and exits 3 when it is false.  Round 5 showed why: a kernel whose epilogue corrupted
the data gradient's halo produced NaN from the second step on, and NaN operands draw less power, so
the clock rose and the bench read 12 % faster.  Here the bench runs a small full step (64x64, bs 2,
one residual block) once as is and once with a NaN injected into the synthetic inputs."""
import json
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT

SMALL = ["--img", "64", "--batch", "2", "--blocks", "1", "--steps", "2", "--warmup", "1", "--no-cpu-baseline"]


def _bench(*extra):
    env = dict(os.environ, PYTHONUNBUFFERED="1")
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *SMALL, *extra], cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=240)


def _record(out):
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    assert lines, out
    return json.loads(lines[-1])


def test_all_finite_helper_cpu():
    sys.path.insert(0, ROOT)
    import bench
    assert bench.all_finite([torch.zeros(3), torch.ones(2, 2), torch.empty(0)])
    assert not bench.all_finite([torch.zeros(3), torch.tensor([1.0, float("nan")])])
    assert not bench.all_finite([torch.tensor(float("inf"))])


def test_dump_outputs_helper_cpu(tmp_path):
    """dump_outputs writes float32 .npy files; an array above the per-array cap becomes the same fixed
    sample of it in every call."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    big = torch.arange(bench.DUMP_MAX_ELEMS + 5, dtype=torch.float64)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"loss": torch.tensor(1.5), "big": big, "m": torch.ones(2, 3)})
    a = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in ("loss", "big", "m")}
    assert all(v.dtype == np.float32 for v in a.values())
    assert a["loss"].shape == () and float(a["loss"]) == 1.5 and a["m"].shape == (2, 3)
    assert a["big"].shape == (bench.DUMP_MAX_ELEMS,) and len(np.unique(a["big"])) > bench.DUMP_MAX_ELEMS // 2
    assert np.array_equal(a["big"], np.load(tmp_path / "b" / "big.npy"))


@pytest.mark.gpu
def test_bench_plain_run_and_dump_outputs(tmp_path):
    """A plain run (no --full) has no cpu_baseline leg; --dump-outputs writes the last step's loss terms
    and the three optimizers' parameters, and the line keeps its headline fields."""
    import numpy as np
    args = [a for a in SMALL if a != "--no-cpu-baseline"]
    env = dict(os.environ, PYTHONUNBUFFERED="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args, "--dump-outputs",
                        str(tmp_path / "out")], cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = _record(r.stdout)
    assert "cpu_baseline" not in rec and rec["steps"] == 2 and rec["ms_per_step"] > 0
    assert abs(rec["value"] - 2 / (rec["ms_per_step"] * 1e-3)) <= 1e-2 * rec["value"]
    names = {p.name for p in (tmp_path / "out").iterdir()}
    assert {"loss_G.npy", "params_G.npy", "params_D_A.npy", "params_D_B.npy"} <= names, names
    total = 0
    for n in names:
        a = np.load(tmp_path / "out" / n)
        assert a.dtype == np.float32 and np.isfinite(a).all(), n
        total += a.nbytes
    assert total <= 64 << 20


@pytest.mark.gpu
def test_bench_reports_finite_step():
    r = _bench()
    assert r.returncode == 0, r.stderr[-3000:]
    rec = _record(r.stdout)
    assert rec["finite"] is True and rec["value"] > 0


@pytest.mark.gpu
def test_bench_exits_nonzero_on_nan_step():
    r = _bench("--inject-nan")
    assert r.returncode == 3, (r.returncode, r.stderr[-3000:])
    rec = _record(r.stdout)
    assert rec["finite"] is False
    assert "non-finite" in r.stderr
