"""Multi-process GPU-solver tests on ONE GPU (gloo, world_size=2).

The gpurun pool has single-GPU boxes and RCCL refuses two ranks on one
device ("Duplicate GPU detected"), so real multi-rank RCCL only runs on
the driver's 8-GPU node.  This file closes the remaining test-matrix cell
before that: the *GPU* solver (HIP kernels, streams, lag pipeline,
overlapped allreduce) under *real* multi-process torch.distributed comm,
using the CPU-staged gloo path in dist/comm.py + dist/halo.py.  Only the
backend differs from production (gloo staging vs RCCL device-direct);
every solver branch taken is the world_size>1 code the driver will run.
"""

import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from acg_amd.gen import queen_like_spec, stencil_global

pytestmark = pytest.mark.gpu


def _worker(rank, world, port, fn_name, q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        os.environ["RANK"] = str(rank)
        os.environ["WORLD_SIZE"] = str(world)
        from acg_amd.dist.comm import Comm

        comm = Comm("gloo")
        result = globals()[fn_name](comm)
        q.put((rank, "ok", result))
        comm.finalize()
    except Exception:  # pragma: no cover
        import traceback

        q.put((rank, "err", traceback.format_exc()))
        raise


def _run_dist(fn_name, world=2, port=29610):
    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, fn_name, q))
             for r in range(world)]
    for p in procs:
        p.start()
    results = {}
    for _ in range(world):
        rank, status, payload = q.get()
        assert status == "ok", f"rank {rank} failed:\n{payload}"
        results[rank] = payload
    for p in procs:
        p.join(timeout=120)
    return results


# -- worker bodies (module-level for spawn picklability) -------------------

def _body_halo_gpu(comm):
    from acg_amd.dist.halo import HaloExchange
    from acg_amd.gen import STENCIL_27PT_3D, stencil_local_slab

    S = stencil_local_slab(6, 6, 8, STENCIL_27PT_3D, comm.rank, comm.size)
    x = torch.zeros(S.nowned + S.nghost, dtype=torch.float64, device="cuda:0")
    x[:S.nowned] = torch.from_numpy(S.owned_global.astype(np.float64)).cuda()
    hx = HaloExchange(S.halo, S.nowned, "cuda:0", comm)
    hx.exchange(x)
    torch.cuda.synchronize()
    got = x[S.nowned:].cpu().numpy()
    np.testing.assert_array_equal(got, S.ghost_global.astype(np.float64))
    return True


def _solve_gpu(comm, method):
    from acg_amd.gen import stencil_local_slab
    from acg_amd.solvers.hip import CGSolverHIP

    spec = queen_like_spec(3)
    S = stencil_local_slab(5, 5, 8, spec, comm.rank, comm.size)
    rng = np.random.default_rng(42)
    b_global = rng.standard_normal(S.n_global)
    b = torch.from_numpy(b_global[S.owned_global]).cuda()
    solver = CGSolverHIP(S, comm=comm, device="cuda:0")
    x = torch.zeros(S.nowned + S.nghost, dtype=torch.float64, device="cuda:0")
    res = getattr(solver, method)(b, x, maxits=500, res_rtol=1e-10)
    assert res.converged, res.summary()
    return (S.owned_global, x[:S.nowned].cpu().numpy(), res.niterations)


def _body_cg_gpu(comm):
    return _solve_gpu(comm, "solve")


def _body_cg_gpu_pipelined(comm):
    return _solve_gpu(comm, "solve_pipelined")


def _body_cg_gpu_jacobi(comm):
    return _solve_gpu(comm, "solve_jacobi")


def _check_vs_direct(results):
    spec = queen_like_spec(3)
    A = stencil_global(5, 5, 8, spec)
    rng = np.random.default_rng(42)
    b_global = rng.standard_normal(A.n)
    import scipy.sparse.linalg as spla

    x_ref = spla.spsolve(A.to_scipy_full().tocsc(), b_global)
    covered = np.zeros(A.n, dtype=bool)
    for _, (owned_global, xloc, _nit) in results.items():
        np.testing.assert_allclose(xloc, x_ref[owned_global], rtol=1e-6, atol=1e-8)
        covered[owned_global] = True
    assert covered.all()


def _body_cg_gpu_matfree(comm):
    """2-rank matrix-free pipelined solve: halo + generic matO ghost pass
    + column-walk matA under real multi-process comm."""
    from acg_amd.gen import STENCIL_7PT_3D
    from acg_amd.gen.device_slab import device_stencil_slab
    from acg_amd.solvers.hip import CGSolverHIP

    S = device_stencil_slab(6, 6, 10, dict(STENCIL_7PT_3D), comm.rank,
                            comm.size, "cuda:0", operator=False)
    rng = np.random.default_rng(21)
    b_global = rng.standard_normal(S.n_global)
    # slab owned rows are plane-reordered: recover global ids from the host
    # generator (layout equality is covered by CPU tests)
    from acg_amd.gen import stencil_local_slab

    H = stencil_local_slab(6, 6, 10, dict(STENCIL_7PT_3D), comm.rank, comm.size)
    b = torch.from_numpy(b_global[H.owned_global]).cuda()
    solver = CGSolverHIP(S, comm=comm, device="cuda:0", matfree=True)
    x = torch.zeros(S.nowned + S.nghost, dtype=torch.float64, device="cuda:0")
    res = solver.solve_pipelined(b, x, maxits=500, res_rtol=1e-10)
    assert res.converged, res.summary()
    return (H.owned_global, x[:S.nowned].cpu().numpy(), res.niterations)


def _body_cg_gpu_ws4(comm):
    """4 ranks on one GPU, generic rgb partition: multi-neighbour halos
    through the full extract_subdomains path with the HIP solver."""
    from acg_amd.gen import STENCIL_27PT_3D
    from acg_amd.part import extract_subdomains, partition_rows
    from acg_amd.solvers.hip import CGSolverHIP

    A = stencil_global(6, 6, 6, STENCIL_27PT_3D)
    part = partition_rows(A, comm.size, method="rgb", seed=1)
    S = extract_subdomains(A, part, comm.size)[comm.rank]
    rng = np.random.default_rng(7)
    b_global = rng.standard_normal(A.n)
    b = torch.from_numpy(b_global[S.owned_global]).cuda()
    solver = CGSolverHIP(S, comm=comm, device="cuda:0")
    x = torch.zeros(S.nowned + S.nghost, dtype=torch.float64, device="cuda:0")
    res = solver.solve_pipelined(b, x, maxits=800, res_rtol=1e-10)
    assert res.converged, res.summary()
    return (S.owned_global, x[:S.nowned].cpu().numpy(), res.niterations)


def test_gpu_halo_exchange_2proc():
    _run_dist("_body_halo_gpu", world=2, port=29610)


def test_gpu_cg_classic_2proc():
    _check_vs_direct(_run_dist("_body_cg_gpu", world=2, port=29611))


def test_gpu_cg_jacobi_2proc():
    """2-process Jacobi-PCG on one GPU (gloo-staged): multi-rank
    (r,z)/(p,t) allreduces + the fused PCG epilogue."""
    _check_vs_direct(_run_dist("_body_cg_gpu_jacobi", world=2, port=29647))


def test_gpu_cg_pipelined_2proc():
    _check_vs_direct(_run_dist("_body_cg_gpu_pipelined", world=2, port=29612))


def test_gpu_cg_matfree_2proc():
    from acg_amd.gen import STENCIL_7PT_3D

    results = _run_dist("_body_cg_gpu_matfree", world=2, port=29614)
    A = stencil_global(6, 6, 10, dict(STENCIL_7PT_3D))
    rng = np.random.default_rng(21)
    b_global = rng.standard_normal(A.n)
    import scipy.sparse.linalg as spla

    x_ref = spla.spsolve(A.to_scipy_full().tocsc(), b_global)
    for _, (owned_global, xloc, _nit) in results.items():
        np.testing.assert_allclose(xloc, x_ref[owned_global], rtol=1e-6, atol=1e-8)


def test_gpu_cg_ws4_rgb():
    from acg_amd.gen import STENCIL_27PT_3D

    results = _run_dist("_body_cg_gpu_ws4", world=4, port=29613)
    A = stencil_global(6, 6, 6, STENCIL_27PT_3D)
    rng = np.random.default_rng(7)
    b_global = rng.standard_normal(A.n)
    import scipy.sparse.linalg as spla

    x_ref = spla.spsolve(A.to_scipy_full().tocsc(), b_global)
    for _, (owned_global, xloc, _nit) in results.items():
        np.testing.assert_allclose(xloc, x_ref[owned_global], rtol=1e-6, atol=1e-8)


def test_bench_2proc_end_to_end(tmp_path):
    """The driver-facing bench contract at world_size=2 on one GPU
    (ACG_BENCH_COMM=gloo test override): full flow -- slab generation per
    rank, multi-rank solve, MAX-over-ranks timing, nnz SUM, one JSON line
    from rank 0."""
    import json
    import subprocess
    import sys as _sys
    from pathlib import Path

    repo = Path(__file__).resolve().parent.parent
    env = dict(__import__("os").environ)
    env["ACG_BENCH_COMM"] = "gloo"
    cmd = [_sys.executable, "-m", "torch.distributed.run", "--nnodes", "1",
           "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29640", "bench.py", "--gpus", "2",
           "--steps", "5", "--warmup", "2", "--grid", "14", "--full",
           "--dump-outputs", str(tmp_path / "dump")]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=repo,
                       env=env, timeout=420)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = next(l for l in r.stdout.splitlines() if l.startswith("{"))
    d = json.loads(line)
    assert d["n_gpus"] == 2 and d["steps"] == 5
    assert d["value"] > 0
    assert d["config"]["solver"] in ("cg-pipelined", "cg-classic")  # auto probes
    assert d["config"]["rows"] == 3 * 14 ** 3
    # --full extras: integrity check and one span record per rank
    assert np.isfinite(d["config"]["rel_residual_true"])
    assert set(d["config"]["rank_spans_us_per_call"]) == {"r0", "r1"}
    # --dump-outputs: per-rank float64 files, owned rows add up, the norms
    # are allreduced (equal on both ranks), solver.txt names the solver
    dump = tmp_path / "dump"
    assert sorted(p.name for p in dump.iterdir()) == [
        "residual_norms_rank0.npy", "residual_norms_rank1.npy",
        "solver.txt", "x_rank0.npy", "x_rank1.npy"]
    xs = [np.load(dump / f"x_rank{r}.npy") for r in range(2)]
    nr = [np.load(dump / f"residual_norms_rank{r}.npy") for r in range(2)]
    assert all(a.dtype == np.float64 and a.ndim == 1 for a in xs)
    assert sum(a.size for a in xs) == 3 * 14 ** 3
    assert all(np.isfinite(a).all() for a in xs)
    assert nr[0].dtype == np.float64 and nr[0].shape == (3,)
    # two-term fp64 sums: ranks agree to a few ulp whatever the order
    np.testing.assert_allclose(nr[0], nr[1], rtol=1e-12, atol=0)
    assert (dump / "solver.txt").read_text().strip() == d["config"]["solver"]


@pytest.mark.gpu
def test_run_poisson2048_script_smoke(tmp_path):
    """The config-5 push-button script works end-to-end at a toy grid
    (1 proc, GRID=64): torchrun launch, preflight assert, one JSON line."""
    import json
    import subprocess
    from pathlib import Path

    repo = Path(__file__).resolve().parent.parent
    env = dict(os.environ)
    env.update(GRID="64", STEPS="3", WARMUP="1", NGPUS="1",
               MASTER_PORT="29650")
    r = subprocess.run(["bash", str(repo / "tools/run_poisson2048.sh")],
                       capture_output=True, text=True, cwd=repo, env=env,
                       timeout=420)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    line = next(l for l in r.stdout.splitlines() if l.startswith("{"))
    d = json.loads(line)
    assert d["config"]["model"] == "poisson3d-7pt-G64"
    assert d["steps"] == 3 and d["value"] > 0
    assert "preflight" in r.stderr
