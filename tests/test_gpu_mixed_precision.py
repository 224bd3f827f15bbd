"""fp32-stored operator SpMV kernels and CGSolverHIP.solve_mixed on the GPU.

Kernel level: same oracle and bound as tests/test_gpu_kernel_oracle.py,
evaluated on the case with the values rounded to fp32 (the conversion back
is exact and all arithmetic is fp64; tests/test_mixed_precision_cpu.py shows
that this expectation rejects results computed from the fp64 values).
Solver level: the CPU solver's solve_mixed is the oracle."""

import copy
import os
from functools import lru_cache

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import kernel_oracle as ko
import mixed_systems as ms

pytestmark = pytest.mark.gpu

DOFS = (2, 3, 4)
BSELL_NODES = (1, 63, 65, 130)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gpu_ops():
    from acg_amd.ops import gpu_ops

    # before ANY launch: without fp32 support a float32 buffer would be read
    # as doubles past its end
    assert torch.float32 in getattr(gpu_ops, "OPERATOR_VALUE_DTYPES", ())
    assert gpu_ops.MAXG == ko.MAXG and gpu_ops.S_NSLOTS == ko.S_NSLOTS
    return gpu_ops


def rounded(case):
    c = copy.copy(case)
    c.vals = case.vals.astype(np.float32).astype(np.float64)
    return c


@lru_cache(maxsize=None)
def _bsell(dof, nnodes, ghost):
    case = ko.bsell_case(dof, nnodes, ghost)
    return case, rounded(case)


@lru_cache(maxsize=None)
def _sell(ns, short):
    case = ko.sell_case(ns, short=short)
    return case, rounded(case)


def sell_packed(case, col64=False, sigma=1, f32=True):
    from acg_amd.ops import torch_ref

    out = torch_ref.sell_from_csr(
        case.rowptr, case.cols.astype(np.int64 if col64 else np.int32),
        case.vals, sigma=sigma)
    vals = out[2].astype(np.float32) if f32 else out[2]
    return (out[0], out[1], vals) + tuple(out[3:])


# ---------------------------------------------------------------------------
# kernels

@pytest.mark.parametrize("ghost", [False, True])
@pytest.mark.parametrize("nnodes", BSELL_NODES)
@pytest.mark.parametrize("dof", DOFS)
def test_spmv_bsell_fp32(dev, gpu_ops, dof, nnodes, ghost):
    case, rcase = _bsell(dof, nnodes, ghost)
    bptr, bcol, bvals = ko.pack_bsell(case, dev)
    packed = (bptr, bcol, bvals.to(torch.float32))
    for dotslot, acc in ((-1, False), (ko.S_PT, False), (ko.S_PT, True)):
        got = ko.run_bsell_spmv(gpu_ops, case, dev, dotslot=dotslot,
                                dot_accum=acc, packed=packed)
        ko.assert_accepts(ko.bsell_spmv_expect(rcase, dotslot, acc), got,
                          f"f32 dof{dof} n{nnodes} ghost{ghost} slot{dotslot} acc{acc}")
        ko.check_partials(got, halves=1)


@pytest.mark.parametrize("col64", [False, True])
@pytest.mark.parametrize("ns,short", [(1, False), (2, False), (7, False),
                                      (1, True), (2, True), (7, True)])
def test_spmv_sell_fp32(dev, gpu_ops, ns, short, col64):
    case, rcase = _sell(ns, short)
    packed = sell_packed(case, col64=col64)
    for acc in (False, True):
        got = ko.run_sell_spmv(gpu_ops, case, dev, dot_accum=acc, packed=packed)
        ko.assert_accepts(ko.sell_spmv_expect(rcase, dot_accum=acc), got,
                          f"f32 ns{ns} short{short} col64={col64} acc{acc}")
        ko.check_partials(got, halves=1)


@pytest.mark.parametrize("ns,short", [(7, False), (7, True)])
def test_spmv_sell_fp32_sigma_perm(dev, gpu_ops, ns, short):
    case, rcase = _sell(ns, short)
    packed = sell_packed(case, sigma=4096)
    assert len(packed) == 4
    for acc in (False, True):
        got = ko.run_sell_spmv(gpu_ops, case, dev, dot_accum=acc, packed=packed)
        ko.assert_accepts(ko.sell_spmv_expect(rcase, perm=packed[3],
                                              dot_accum=acc), got,
                          f"f32 sigma ns{ns} short{short} acc{acc}")
        ko.check_partials(got, halves=1)


@pytest.mark.parametrize("col64", [False, True])
def test_spmv_sell_fp32_accum_rowbase(dev, gpu_ops, col64):
    """y[rowbase:rowbase+n] += A32 x with the dot accumulated on top of the
    slot (the matO pass), rows outside the window untouched."""
    case, rcase = _sell(2, False)
    n, rowbase = case.nrows, 5
    assert case.ncols >= rowbase + n
    sp, sc, sv = sell_packed(case, col64=col64)
    y = ko._nan(n + 2 * rowbase, dev)
    y[rowbase:rowbase + n] = ko._t(ko.csr_y0(case), dev)
    scal = ko._t(ko.SENTINELS, dev)
    partials = ko._nan(2 * ko.MAXG, dev)
    gpu_ops.spmv_sell(ko._t(sp, dev), ko._t(sc, dev), ko._t(sv, dev), n,
                      ko._t(case.x, dev), y, rowbase=rowbase, accum=True,
                      partials=partials, scal=scal, dotslot=ko.S_PT,
                      dot_accum=True)
    yy = ko._np(y)
    got = {"y": yy[rowbase:rowbase + n],
           "y_outside": np.concatenate([yy[:rowbase], yy[rowbase + n:]])}
    ko._partials_out(got, partials, ko.sell_blocks(case.nslices))
    ko._scal_out(got, scal)
    e = ko.Expect("k_spmv_sell")
    xh = ko.hp(case.x)
    c, M = ko.spmv(rcase.rowptr, rcase.cols, rcase.vals, xh)
    L = ko.sell_padded_len(case.rowptr)
    y0 = ko.hp(ko.csr_y0(case))
    e.add("y", y0 + c, ko.habs(y0) + M, L)
    e.add_exact("y_outside", np.full(2 * rowbase, np.nan))
    d, tol = ko.dot(xh[rowbase:rowbase + n], c, tb=ko.bound(M, L),
                    add=ko.SENTINELS[ko.S_PT])
    e.add_tol(f"scal{ko.S_PT}", d, tol)
    e.scalars(ko.SENTINELS, touched=(ko.S_PT,))
    ko.assert_accepts(e, got, f"f32 accum rowbase col64={col64}")
    ko.check_partials(got, halves=1)


def _all_nan(t):
    return bool(torch.isnan(t).all())


def test_guards_raise_before_launch(dev, gpu_ops):
    case, _ = _sell(2, False)
    sp, sc, sv = sell_packed(case)
    y = ko._nan(case.nrows, dev)
    partials = ko._nan(2 * ko.MAXG, dev)
    scal = ko._nan(ko.S_NSLOTS, dev)
    args = (ko._t(sp, dev), ko._t(sc, dev))
    kw = dict(partials=partials, scal=scal, dotslot=ko.S_PT)
    x = ko._t(case.x, dev)
    with pytest.raises(TypeError):
        gpu_ops.spmv_sell(*args, ko._t(sv.astype(np.float16), dev),
                          case.nrows, x, y, **kw)
    with pytest.raises(TypeError):
        gpu_ops.spmv_sell(*args, ko._t(sv, dev), case.nrows, x, y,
                          variant=gpu_ops.SELL_SWZ, **kw)
    bcase, _ = _bsell(3, 65, False)
    bptr, bcol, bvals = ko.pack_bsell(bcase, dev)
    yb = ko._nan(bcase.nrows, dev)
    with pytest.raises(TypeError):
        gpu_ops.spmv_bsell(bptr, bcol, bvals.to(torch.float16), bcase.nnodes,
                           bcase.dof, ko._t(bcase.x, dev), yb, **kw)
    torch.cuda.synchronize()
    assert _all_nan(y) and _all_nan(yb) and _all_nan(partials) and _all_nan(scal)


def test_fp64_values_unchanged(dev, gpu_ops):
    """fp64 values through the same dispatch still meet the fp64-value
    expectations (and those reject the fp32 results)."""
    case, rcase = _bsell(3, 130, True)
    got = ko.run_bsell_spmv(gpu_ops, case, dev, dotslot=ko.S_PT)
    ko.assert_accepts(ko.bsell_spmv_expect(case, ko.S_PT), got, "f64 bsell")
    assert not ko.accepts(ko.bsell_spmv_expect(rcase, ko.S_PT), got)
    case, rcase = _sell(7, False)
    got = ko.run_sell_spmv(gpu_ops, case, dev,
                           packed=sell_packed(case, f32=False))
    ko.assert_accepts(ko.sell_spmv_expect(case), got, "f64 sell")
    assert not ko.accepts(ko.sell_spmv_expect(rcase), got)


# ---------------------------------------------------------------------------
# solver

def _x0(S, dev):
    return torch.zeros(S.nowned + S.nghost, dtype=torch.float64, device=dev)


@pytest.mark.parametrize("name,fmt", [("poisson32", "sell"),
                                      ("poisson32", "sigma"),
                                      ("queen6", "sell"), ("queen6", "sigma"),
                                      ("queen6", "bsell")])
def test_solve_mixed(dev, gpu_ops, name, fmt):
    from acg_amd.solvers.hip import CGSolverHIP

    ref = ms.cpu_solves(name)
    A, bn, S, tol = ref["A"], ref["b"], ref["S"], ref["tol"]
    b = torch.from_numpy(bn).to(dev)
    solver = CGSolverHIP(S, device=dev, force_format=fmt)
    assert solver._format_name() == fmt
    x = _x0(S, dev)
    res = solver.solve_mixed(b, x, **ms.MIXED_KW)
    xn = x[:S.nowned].cpu().numpy()
    rn = ms.true_residual(A, bn, xn)
    cpu = ref["mixed"]
    print(f"MIXED_GPU {name}/{fmt}: nouter={res.nouter} (cpu {cpu.nouter}) "
          f"inner={res.niterations} (cpu {cpu.niterations}) "
          f"true/tol={rn / tol:.3f} rnrm2/tol={res.rnrm2 / tol:.3f}")
    assert res.converged and res.solver == "cg-hip-mixed"
    assert rn <= 1.1 * tol
    assert res.rnrm2 == pytest.approx(rn, rel=0.1)
    assert res.nouter == cpu.nouter
    assert abs(res.niterations - cpu.niterations) <= 2 * cpu.nouter
    # the fp32 copy exists next to the fp64 values, which stay in place
    assert solver._vals32.dtype == torch.float32
    src = solver.bsell[2] if fmt == "bsell" else solver.sell[2]
    assert src.dtype == torch.float64 and src.numel() == solver._vals32.numel()

    # repeat on the same instance: workspaces (and graphs) are reused
    x2 = _x0(S, dev)
    res2 = solver.solve_mixed(b, x2, **ms.MIXED_KW)
    assert torch.equal(x, x2)
    assert (res2.nouter, res2.niterations) == (res.nouter, res.niterations)

    # one sweep asked to go all the way stalls at the fp32 operator's accuracy
    x1 = _x0(S, dev)
    res1 = solver.solve_mixed(b, x1, maxits=ms.MAXITS, res_rtol=ms.RES_RTOL,
                              inner_rtol=1e-13, max_outer=1)
    rel = ms.true_residual(A, bn, x1[:S.nowned].cpu().numpy()) / np.linalg.norm(bn)
    print(f"MIXED_GPU {name}/{fmt}: single-sweep relative residual {rel:.3e}")
    assert res1.nouter == 1 and not res1.converged and rel > 1e-9

    # a plain solve afterwards still uses the fp64 operator only
    xa = _x0(S, dev)
    ra = solver.solve(b, xa, maxits=ms.MAXITS, res_rtol=ms.RES_RTOL)
    xb = _x0(S, dev)
    rb = CGSolverHIP(S, device=dev, force_format=fmt).solve(
        b, xb, maxits=ms.MAXITS, res_rtol=ms.RES_RTOL)
    assert ra.converged and ra.niterations == rb.niterations
    assert torch.equal(xa, xb)


def test_solve_mixed_graph_keys_per_value_set(dev, gpu_ops):
    """With graph replay on, the fp64 and the fp32 iteration each capture
    their own graph; neither replays the other's."""
    from acg_amd.solvers.hip import CGSolverHIP

    ref = ms.cpu_solves("queen6")
    S = ref["S"]
    b = torch.from_numpy(ref["b"]).to(dev)
    solver = CGSolverHIP(S, device=dev, force_format="bsell")
    xa = _x0(S, dev)
    solver.solve(b, xa, maxits=ms.MAXITS, res_rtol=ms.RES_RTOL, use_graph=True)
    x = _x0(S, dev)
    res = solver.solve_mixed(b, x, **ms.MIXED_KW)
    assert "classic" in solver._graphs and "classic:f32" not in solver._graphs
    assert res.converged
    rn = ms.true_residual(ref["A"], ref["b"], x[:S.nowned].cpu().numpy())
    assert rn <= 1.1 * ref["tol"]
    # the inner iteration with replay on records under its own key ...
    xl = _x0(S, dev)
    solver._solve_classic(b, xl, ms.MAXITS, 0.0, ms.RES_RTOL, use_graph=True,
                          lowprec=True)
    assert "classic:f32" in solver._graphs
    assert solver._graphs["classic:f32"] is not solver._graphs["classic"]
    assert not torch.equal(xa, xl)  # A32 x = b is a different system
    xl2 = _x0(S, dev)
    solver._solve_classic(b, xl2, ms.MAXITS, 0.0, ms.RES_RTOL, use_graph=True,
                          lowprec=True)
    assert torch.equal(xl, xl2)
    # ... and the fp64 replay still solves the fp64 system
    xb = _x0(S, dev)
    solver.solve(b, xb, maxits=ms.MAXITS, res_rtol=ms.RES_RTOL, use_graph=True)
    assert torch.equal(xa, xb)


@pytest.mark.parametrize("fmt", ["hybrid", "csr"])
def test_solve_mixed_rejects_other_formats(dev, gpu_ops, fmt):
    from acg_amd.solvers.hip import CGSolverHIP

    ref = ms.cpu_solves("poisson32")
    S = ref["S"]
    solver = CGSolverHIP(S, device=dev, force_format=fmt)
    x = _x0(S, dev)
    with pytest.raises(ValueError, match=fmt):
        solver.solve_mixed(torch.from_numpy(ref["b"]).to(dev), x, maxits=10)
    assert not bool(x.any())


# ---------------------------------------------------------------------------
# two processes on one GPU over gloo

def _worker(rank, world, port, q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        os.environ["RANK"] = str(rank)
        os.environ["WORLD_SIZE"] = str(world)
        from acg_amd.dist.comm import Comm
        from acg_amd.ops import gpu_ops
        from acg_amd.solvers.hip import CGSolverHIP

        assert torch.float32 in gpu_ops.OPERATOR_VALUE_DTYPES
        comm = Comm("gloo")
        A = ms.queen6()
        S = ms.local(A, world, rank)
        b = torch.from_numpy(ms.rhs(A)[S.owned_global]).cuda()
        x = torch.zeros(S.nowned + S.nghost, dtype=torch.float64,
                        device="cuda:0")
        solver = CGSolverHIP(S, comm=comm, device="cuda:0")
        res = solver.solve_mixed(b, x, **ms.MIXED_KW)
        q.put((rank, "ok", (S.owned_global, x[:S.nowned].cpu().numpy(),
                            res.nouter, res.niterations, res.converged)))
        comm.finalize()
    except Exception:  # pragma: no cover
        import traceback

        q.put((rank, "err", traceback.format_exc()))
        raise


def test_gpu_solve_mixed_2proc(gpu_ops):
    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    procs = [ctx.Process(target=_worker, args=(r, 2, 29661, q))
             for r in range(2)]
    for p in procs:
        p.start()
    results = {}
    for _ in range(2):
        rank, status, payload = q.get()
        assert status == "ok", f"rank {rank} failed:\n{payload}"
        results[rank] = payload
    for p in procs:
        p.join(timeout=120)
    serial = ms.cpu_solves("queen6")
    assert results[0][2:] == results[1][2:]  # same nouter / inner / verdict
    assert results[0][4] and results[0][2] >= 2
    covered = np.zeros(serial["A"].n, dtype=bool)
    for _, (owned_global, xloc, *_r) in results.items():
        np.testing.assert_allclose(xloc, serial["x"][owned_global],
                                   rtol=1e-6, atol=1e-8)
        covered[owned_global] = True
    assert covered.all()
