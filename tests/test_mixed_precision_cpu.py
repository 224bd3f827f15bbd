"""fp32-stored operator SpMV and mixed-precision refined CG, CPU side:
torch_ref kernel semantics against the high-precision oracle, the op-layer
constant, CGSolverCPU.solve_mixed, the CLI and a 2-rank gloo run.

Kernel level.  fp32 -> fp64 conversion is exact and all arithmetic is
fp64, so the oracle of an fp32 run is the existing one evaluated on the
case with ``vals`` replaced by ``vals.astype(float32).astype(float64)``;
the existing bound (L+48) * 2^-53 * M applies unchanged.  The same
expectation must REJECT a result computed from the original fp64 values:
that is what shows the fp32 path is the one that ran."""

import copy
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import kernel_oracle as ko
import mixed_systems as ms
from acg_amd.ops import torch_ref

SELL_ACCEPT = [(1, False), (2, False), (7, False), (1, True), (2, True),
               (7, True)]
# sell_case(1, short=True) is one all-empty slice (y == 0): accept only
SELL_REJECT = [c for c in SELL_ACCEPT if c != (1, True)]
BSELL_CASES = [(dof, n) for dof in (2, 3, 4) for n in (1, 65, 130)]


def rounded(case):
    """The case the fp32-stored operator represents."""
    c = copy.copy(case)
    c.vals = case.vals.astype(np.float32).astype(np.float64)
    return c


def sell_packed32(case, col64=False, sigma=1):
    out = torch_ref.sell_from_csr(
        case.rowptr, case.cols.astype(np.int64 if col64 else np.int32),
        case.vals, sigma=sigma)
    return (out[0], out[1], out[2].astype(np.float32)) + tuple(out[3:])


def bsell_packed32(case, dev):
    bptr, bcol, bvals = ko.pack_bsell(case, dev)
    return bptr, bcol, bvals.to(torch.float32)


# -- torch_ref kernel level -------------------------------------------------

@pytest.mark.parametrize("ns,short", SELL_ACCEPT)
def test_ref_sell_fp32_accepts(ns, short):
    case = ko.sell_case(ns, short=short)
    e = ko.sell_spmv_expect(rounded(case))
    got = ko.run_sell_spmv(torch_ref, case, "cpu", packed=sell_packed32(case))
    ko.assert_accepts(e, got, f"ref-f32 ns={ns} short={short}")


@pytest.mark.parametrize("ns,short", SELL_REJECT)
def test_ref_sell_fp32_expectation_rejects_fp64_values(ns, short):
    case = ko.sell_case(ns, short=short)
    e = ko.sell_spmv_expect(rounded(case))
    assert not ko.accepts(e, ko.run_sell_spmv(torch_ref, case, "cpu"))


@pytest.mark.parametrize("dof,n", BSELL_CASES)
def test_ref_bsell_fp32_accepts_and_rejects_fp64_values(dof, n):
    case = ko.bsell_case(dof, n, True)
    e = ko.bsell_spmv_expect(rounded(case), dotslot=ko.S_PT)
    got = ko.run_bsell_spmv(torch_ref, case, "cpu", dotslot=ko.S_PT,
                            packed=bsell_packed32(case, "cpu"))
    ko.assert_accepts(e, got, f"ref-f32 dof={dof} n={n}")
    assert not ko.accepts(e, ko.run_bsell_spmv(torch_ref, case, "cpu",
                                               dotslot=ko.S_PT))


# -- op layer -----------------------------------------------------------------

def test_operator_value_dtypes_constant():
    assert torch_ref.OPERATOR_VALUE_DTYPES == (torch.float64, torch.float32)
    try:
        from acg_amd.ops import gpu_ops
    except ImportError:  # extension not built on this machine
        return
    assert gpu_ops.OPERATOR_VALUE_DTYPES == (torch.float64, torch.float32)


def test_ref_rejects_other_value_dtypes():
    case = ko.sell_case(1)
    sp, sc, sv = sell_packed32(case)
    with pytest.raises(TypeError):
        ko.run_sell_spmv(torch_ref, case, "cpu",
                         packed=(sp, sc, sv.astype(np.float16)))


# -- CGSolverCPU.solve_mixed -------------------------------------------------

cpu_solves = ms.cpu_solves


@pytest.mark.parametrize("name", list(ms.SYSTEMS))
def test_solve_mixed_reaches_fp64_tolerance(name):
    s = cpu_solves(name)
    res = s["mixed"]
    rn = ms.true_residual(s["A"], s["b"], s["x"])
    print(f"MIXED_CPU {name}: nouter={res.nouter} inner={res.niterations} "
          f"plain={s['plain'].niterations} true/tol={rn / s['tol']:.3f} "
          f"rnrm2/tol={res.rnrm2 / s['tol']:.3f}")
    assert s["plain"].converged
    assert res.converged and res.solver == "cg-cpu-mixed"
    assert rn <= 1.1 * s["tol"]
    assert res.rnrm2 <= s["tol"]
    assert res.nouter >= 2
    assert res.niterations <= 1.5 * s["plain"].niterations
    assert f"outer refinement sweeps: {res.nouter}" in res.summary()


@pytest.mark.parametrize("name", list(ms.SYSTEMS))
def test_single_sweep_stalls_at_fp32_operator_accuracy(name):
    """One sweep asked to go all the way down (target = 0.5 * tol): with the
    fp32-rounded operator the TRUE residual stalls near kappa * 2^-24; had
    the inner solve used the fp64 values it would meet the tolerance."""
    s = cpu_solves(name)
    x = torch.zeros_like(torch.from_numpy(s["b"]))
    res = s["solver"].solve_mixed(s["bt"], x, maxits=ms.MAXITS,
                                  res_rtol=ms.RES_RTOL, inner_rtol=1e-13,
                                  max_outer=1)
    rel = ms.true_residual(s["A"], s["b"], x.numpy()) / np.linalg.norm(s["b"])
    print(f"MIXED_CPU {name}: single-sweep relative residual {rel:.3e}")
    assert res.nouter == 1 and not res.converged
    assert rel > 1e-9
    assert res.rnrm2 == pytest.approx(rel * np.linalg.norm(s["b"]), rel=1e-3)


def test_budget_spent_is_not_converged():
    s = cpu_solves("poisson32")
    x = torch.zeros_like(s["bt"])
    res = s["solver"].solve_mixed(s["bt"], x, maxits=40,
                                  res_rtol=ms.RES_RTOL)
    assert not res.converged and res.niterations == 40


def test_refinement_stagnation_stops():
    """2x2 SPD matrix whose small eigenvalue is 1.735 * 2^-23 in fp64 but
    2^-23 after fp32 rounding (a = 1 + 1.49 * 2^-23 rounds to 1 + 2^-23,
    c = 1 - 0.245 * 2^-23 rounds to 1): along that eigenvector each sweep
    leaves |1 - 1.735| = 0.735 of the residual, which is more than half, so
    refinement must give up after ONE sweep instead of looping."""
    from acg_amd.core.symcsr import SymCSRMatrix
    from acg_amd.solvers.cpu import CGSolverCPU

    u = 2.0 ** -23
    a, c = 1.0 + 1.49 * u, 1.0 - 0.245 * u
    assert np.float32(a) == np.float32(1.0 + u) and np.float32(c) == 1.0
    A = SymCSRMatrix.from_coo(2, [0, 0, 1], [0, 1, 1], [a, c, a])
    solver = CGSolverCPU(ms.local(A))
    b = torch.tensor([1.0, -1.0], dtype=torch.float64)
    x = torch.zeros(2, dtype=torch.float64)
    res = solver.solve_mixed(b, x, maxits=100, res_rtol=1e-12, max_outer=20)
    assert not res.converged
    assert res.nouter == 1
    assert 0.5 * res.r0nrm2 < res.rnrm2 < res.r0nrm2


# -- CLI ----------------------------------------------------------------------

def _poisson_mtx(tmp_path):
    from acg_amd.gen import STENCIL_5PT_2D, stencil_global
    from acg_amd.io.mtx import MtxFile, write_mtx

    A = stencil_global(16, 16, 1, STENCIL_5PT_2D)
    rows = np.repeat(np.arange(A.n), np.diff(A.rowptr))
    m = MtxFile(object="matrix", format="coordinate", field_="real",
                symmetry="symmetric", nrows=A.n, ncols=A.n,
                nnz=A.nnz_stored, rowidx=rows, colidx=A.colidx, a=A.vals)
    path = tmp_path / "A.mtx"
    write_mtx(path, m)
    return path


def test_cli_cpu_mixed(tmp_path, capsys, monkeypatch):
    from acg_amd import cli

    path = _poisson_mtx(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("RANK", raising=False)
    rc = cli.main([str(path), "--solver", "cpu-mixed", "--jacobi-scale",
                   "--manufactured-solution", "--max-iterations", "2000",
                   "--residual-rtol", "1e-10", "--inner-rtol", "1e-3", "-q"])
    out = capsys.readouterr()
    assert rc == 0, out.err
    assert "solver: cg-cpu-mixed" in out.err
    assert "outer refinement sweeps:" in out.err
    assert "manufactured solution" in out.err


def test_cli_cpu_mixed_missed_criterion_exits_2(tmp_path, capsys, monkeypatch):
    from acg_amd import cli

    path = _poisson_mtx(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("RANK", raising=False)
    rc = cli.main([str(path), "--solver", "cpu-mixed", "--max-iterations",
                   "5", "--residual-rtol", "1e-30", "-q"])
    assert rc == 2, capsys.readouterr().err


# -- 2 ranks over gloo ----------------------------------------------------------

def _worker(rank, world, port, q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        os.environ["RANK"] = str(rank)
        os.environ["WORLD_SIZE"] = str(world)
        from acg_amd.dist.comm import Comm
        from acg_amd.solvers.cpu import CGSolverCPU

        comm = Comm("gloo")
        A = ms.queen6()
        S = ms.local(A, world, rank)
        b = torch.from_numpy(ms.rhs(A)[S.owned_global])
        x = torch.zeros(S.nowned + S.nghost, dtype=torch.float64)
        res = CGSolverCPU(S, comm=comm).solve_mixed(
            b, x, **ms.MIXED_KW)
        q.put((rank, "ok", (S.owned_global, x[:S.nowned].numpy(), res.nouter,
                            res.niterations, res.converged)))
        comm.finalize()
    except Exception:  # pragma: no cover
        import traceback

        q.put((rank, "err", traceback.format_exc()))
        raise


def test_distributed_mixed_matches_serial():
    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    procs = [ctx.Process(target=_worker, args=(r, 2, 29660, q))
             for r in range(2)]
    for p in procs:
        p.start()
    results = {}
    for _ in range(2):
        rank, status, payload = q.get()
        assert status == "ok", f"rank {rank} failed:\n{payload}"
        results[rank] = payload
    for p in procs:
        p.join(timeout=60)
    serial = cpu_solves("queen6")
    assert results[0][2:] == results[1][2:]  # same nouter / inner / verdict
    assert results[0][4] and results[0][2] >= 2
    for _, (owned_global, xloc, *_r) in results.items():
        np.testing.assert_allclose(xloc, serial["x"][owned_global],
                                   rtol=1e-6, atol=1e-8)
