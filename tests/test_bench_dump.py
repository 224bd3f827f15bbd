"""bench.py --dump-outputs: the sampling rule (CPU) and the files a
single-GPU run writes when the iterate exceeds the budget (GPU)."""

import importlib.util
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent


def _bench():
    spec = importlib.util.spec_from_file_location("acg_bench", REPO / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("n,cap", [(11, 10), (1000, 7), (16_777_216, 1 << 16)])
def test_dump_sample_distinct_sorted_seeded(n, cap):
    bench = _bench()
    a = bench.dump_sample(n, cap, 777)
    assert a.shape == (cap,) and a.dtype == np.int64
    assert a[0] >= 0 and a[-1] < n
    assert np.all(np.diff(a) > 0)  # sorted, no duplicates
    np.testing.assert_array_equal(a, bench.dump_sample(n, cap, 777))
    if cap > 100:
        assert not np.array_equal(a, bench.dump_sample(n, cap, 778))


@pytest.mark.gpu
def test_bench_dump_outputs_sampled(tmp_path):
    """192^3 Poisson rows (7.08M) exceed the 48 MB iterate budget: x.npy is
    the capped float64 sample, identical across two runs with a pinned
    solver, and solver.txt names that solver."""
    bench = _bench()
    cap = bench.DUMP_X_BYTES // 8
    assert 192 ** 3 > cap
    outs = []
    for name in ("a", "b"):
        d = tmp_path / name
        r = subprocess.run(
            [sys.executable, "bench.py", "--gpus", "1", "--config", "poisson7",
             "--grid", "192", "--steps", "3", "--warmup", "1",
             "--solver", "classic", "--dump-outputs", str(d)],
            capture_output=True, text=True, cwd=REPO, timeout=300)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
        line = next(l for l in r.stdout.splitlines() if l.startswith("{"))
        res = json.loads(line)
        assert res["steps"] == 3 and res["ms_per_step"] > 0
        assert sorted(p.name for p in d.iterdir()) == [
            "residual_norms.npy", "solver.txt", "x.npy"]
        assert (d / "solver.txt").read_text().strip() == "cg-classic"
        x = np.load(d / "x.npy")
        nrm = np.load(d / "residual_norms.npy")
        assert x.dtype == np.float64 and x.shape == (cap,)
        assert nrm.dtype == np.float64 and nrm.shape == (3,)
        assert np.isfinite(x).all() and np.isfinite(nrm).all()
        assert x.nbytes + nrm.nbytes <= 64 << 20
        outs.append((x, nrm))
    np.testing.assert_array_equal(outs[0][0], outs[1][0])
    np.testing.assert_array_equal(outs[0][1], outs[1][1])
