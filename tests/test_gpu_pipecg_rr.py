"""Residual replacement of the pipelined CG on the GPU: the dual SpMV
kernels and the replacement finalize against the high-precision oracle
(tests/pipecg_rr_oracle.py), the wrappers' argument checks, and
``CGSolverHIP.solve_pipelined(rr_period=...)`` on SELL, megafused SELL,
BSELL, the four-SpMV fallback, graph replay and two gloo ranks on one GPU.

Solver figures (printed as RR_GPU lines) are relative to ||b||; the bounds
are the issue's: true residual <= 10 * rtol * ||b|| with replacement, the
plain solve at least 10x (SELL) / 100x (BSELL) worse."""

import os
from functools import lru_cache

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import kernel_oracle as ko
import mixed_systems as ms
import pipecg_rr_oracle as po
from acg_amd.gen import STENCIL_5PT_2D, stencil_global

pytestmark = pytest.mark.gpu

RTOL = 1e-13
PERIOD = 50
FLAGS = [(r, f) for r in (False, True) for f in (False, True)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gpu_ops():
    from acg_amd.ops import gpu_ops

    assert gpu_ops.MAXG == ko.MAXG and gpu_ops.S_NSLOTS == ko.S_NSLOTS
    assert gpu_ops.S_GAMMA == ko.S_GAMMA and gpu_ops.S_DELTA == ko.S_DELTA
    return gpu_ops


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64))


# ---------------------------------------------------------------------------
# kernels

@pytest.mark.parametrize("sigma", [1, 4])
@pytest.mark.parametrize("col64", [False, True])
@pytest.mark.parametrize("nslices,short", [(1, False), (1, True), (3, False),
                                           (3, True)])
def test_spmv2_sell(dev, gpu_ops, nslices, short, col64, sigma):
    case = po.sell_case2(nslices, short)
    for resid, fuse in FLAGS:
        got = po.run_sell_spmv2(gpu_ops, case, dev, resid=resid, fuse=fuse,
                                col64=col64, sigma=sigma)
        if sigma > 1 and not short:
            assert not np.array_equal(got["perm"][:case.nrows],
                                      np.arange(case.nrows)), "sigma must permute"
        e = po.sell_spmv2_expect(case, resid, fuse, perm=got["perm"])
        ko.assert_accepts(e, got, f"ns{nslices} short={short} col64={col64} "
                                  f"sigma{sigma} resid={resid} fuse={fuse}")
        ko.check_partials(got, halves=2)
        again = po.run_sell_spmv2(gpu_ops, case, dev, resid=resid, fuse=fuse,
                                  col64=col64, sigma=sigma)
        for k in ("y1", "y2", "partials"):
            assert _same_bits(np.nan_to_num(got[k]), np.nan_to_num(again[k])), k
    for fuse in (False, True):
        twin = po.run_sell_spmv2(gpu_ops, case, dev, resid=False, fuse=fuse,
                                 col64=col64, sigma=sigma, x2=case.x)
        assert _same_bits(twin["y1"], twin["y2"])


@pytest.mark.parametrize("ghost", [False, True])
@pytest.mark.parametrize("nnodes", (1, 63, 65, 130))
@pytest.mark.parametrize("dof", (2, 3, 4))
def test_spmv2_bsell(dev, gpu_ops, dof, nnodes, ghost):
    case = po.bsell_case2(dof, nnodes, ghost)
    packed = ko.pack_bsell(case, dev)
    for resid, fuse in FLAGS:
        got = po.run_bsell_spmv2(gpu_ops, case, dev, resid=resid, fuse=fuse,
                                 packed=packed)
        e = po.bsell_spmv2_expect(case, resid, fuse)
        ko.assert_accepts(e, got, f"dof{dof} n{nnodes} ghost={ghost} "
                                  f"resid={resid} fuse={fuse}")
        ko.check_partials(got, halves=2)
        again = po.run_bsell_spmv2(gpu_ops, case, dev, resid=resid, fuse=fuse,
                                   packed=packed)
        for k in ("y1", "y2", "partials"):
            assert _same_bits(np.nan_to_num(got[k]), np.nan_to_num(again[k])), k
    for fuse in (False, True):
        twin = po.run_bsell_spmv2(gpu_ops, case, dev, resid=False, fuse=fuse,
                                  packed=packed, x2=case.x)
        assert _same_bits(twin["y1"], twin["y2"])


@pytest.mark.parametrize("dof,size,sigma", [(1, 1, 1), (1, 3, 1), (1, 3, 4),
                                            (2, 65, 1), (3, 130, 1), (4, 63, 1)])
def test_dot2_slices_repeats_the_fused_partials(dev, gpu_ops, dof, size, sigma):
    """The matrix-free dot of the four-SpMV replacement: within the oracle
    bound, and bit for bit the partials the fused dual SpMV wrote for the
    same (x1, y1)."""
    if dof == 1:
        case = po.sell_case2(size)
        fused = po.run_sell_spmv2(gpu_ops, case, dev, resid=True, fuse=True,
                                  sigma=sigma)
        perm, nunits = fused["perm"], case.nrows
        blocks = po.block_rows(case.nrows, case.nslices, perm=perm)
    else:
        case = po.bsell_case2(dof, size, True)
        fused = po.run_bsell_spmv2(gpu_ops, case, dev, resid=True, fuse=True)
        perm, nunits = None, case.nnodes
        blocks = po.block_rows(case.nrows, (size + 63) // 64, dof)
    got = po.run_dot2_slices(gpu_ops, case.x, fused["y1"], nunits, dof, dev, perm)
    e = po.dot2_slices_expect(case.nrows, case.x, fused["y1"], blocks)
    ko.assert_accepts(e, got, f"dof{dof} size{size} sigma{sigma}")
    ko.check_partials(got, halves=2)
    assert got["nblocks"] == fused["nblocks"]
    assert _same_bits(got["pg"], fused["pg"]) and _same_bits(got["pd"], fused["pd"])


@pytest.mark.parametrize("nblocks", [1, 5, 257, 1000])
def test_replace_finalize(dev, gpu_ops, nblocks):
    case = po.finalize_case(nblocks)
    ko.assert_accepts(po.finalize_expect(case),
                      po.run_finalize(gpu_ops, case, dev), f"nb{nblocks}")


# ---------------------------------------------------------------------------
# wrappers refuse bad arguments before any launch

def _sell_args(dev, case):
    from acg_amd.ops import torch_ref

    sp, sc, sv = torch_ref.sell_from_csr(case.rowptr, case.cols.astype(np.int32),
                                         case.vals)
    t = lambda a: ko._t(a, dev)  # noqa: E731
    return dict(sp=t(sp), sc=t(sc), sv=t(sv), x1=t(case.x), x2=t(case.x2),
                b=t(case.b), y1=ko._nan(case.nrows, dev),
                y2=ko._nan(case.nrows, dev))


def _untouched(*vs):
    torch.cuda.synchronize()
    return all(bool(torch.isnan(v).all()) for v in vs)


def test_wrappers_refuse_before_launch(dev, gpu_ops):
    case = po.sell_case2(3)
    a = _sell_args(dev, case)
    n, nc = case.nrows, case.ncols

    def call(**kw):
        d = dict(a, **kw)
        return gpu_ops.spmv2_sell(d["sp"], d["sc"], d["sv"], n, d["x1"], d["x2"],
                                  d["y1"], d["y2"], ncols=d.get("ncols", nc),
                                  b=d.get("b"))

    with pytest.raises(TypeError, match="float64"):
        call(sv=a["sv"].to(torch.float32))
    # short gathered vector (the ghost tail is missing), short output, short b
    with pytest.raises(ValueError, match="x2"):
        call(x2=a["x2"][:n])
    with pytest.raises(ValueError, match="x1"):
        call(x1=a["x1"][:nc - 1])
    with pytest.raises(ValueError, match="y2"):
        call(y2=a["y2"][:n - 1])
    with pytest.raises(ValueError, match="b"):
        call(b=a["b"][:n - 1])
    # aliasing, full and partial overlap
    with pytest.raises(ValueError, match="share memory"):
        call(y1=a["y2"])
    with pytest.raises(ValueError, match="share memory"):
        call(x2=a["x1"])
    big = ko._nan(2 * nc, dev)
    with pytest.raises(ValueError, match="share memory"):
        call(x1=big[:nc], y1=big[nc - 1:nc - 1 + n])
    with pytest.raises(ValueError, match="share memory"):
        call(b=a["x2"][:n])
    assert _untouched(a["y1"], a["y2"], big)

    bc = po.bsell_case2(3, 65, True)
    bptr, bcol, bvals = ko.pack_bsell(bc, dev)
    x1, x2 = ko._t(bc.x, dev), ko._t(bc.x2, dev)
    y1, y2 = ko._nan(bc.nrows, dev), ko._nan(bc.nrows, dev)
    with pytest.raises(TypeError, match="float64"):
        gpu_ops.spmv2_bsell(bptr, bcol, bvals.to(torch.float32), bc.nnodes, 3,
                            x1, x2, y1, y2, ncols=bc.ncols)
    with pytest.raises(ValueError, match="x1"):
        gpu_ops.spmv2_bsell(bptr, bcol, bvals, bc.nnodes, 3, x1[:bc.nrows], x2,
                            y1, y2, ncols=bc.ncols)
    with pytest.raises(ValueError, match="share memory"):
        gpu_ops.spmv2_bsell(bptr, bcol, bvals, bc.nnodes, 3, x1, x2, y1, y1,
                            ncols=bc.ncols)
    with pytest.raises(ValueError, match="dof"):
        gpu_ops.spmv2_bsell(bptr, bcol, bvals, bc.nnodes, 5, x1, x2, y1, y2,
                            ncols=bc.ncols)
    assert _untouched(y1, y2)


# ---------------------------------------------------------------------------
# solver

def _x0(S, dev):
    return torch.zeros(S.nowned + S.nghost, dtype=torch.float64, device=dev)


@lru_cache(maxsize=None)
def _p48():
    A = ms.scaled(stencil_global(48, 48, 1, dict(STENCIL_5PT_2D)))
    return A, ms.rhs(A), ms.local(A)


def _run(solver, S, bn, dev, method="solve_pipelined", **kw):
    x = _x0(S, dev)
    res = getattr(solver, method)(torch.from_numpy(bn).to(dev), x, **kw)
    return res, x[:S.nowned].cpu().numpy()


@pytest.mark.parametrize("mega", [False, True])
def test_sell_solve_reaches_the_true_residual(dev, mega):
    from acg_amd.solvers.hip import CGSolverHIP

    A, bn, S = _p48()
    bnrm = float(np.linalg.norm(bn))
    solver = CGSolverHIP(S, device=dev)
    assert solver._format_name() == "sell" and solver.can_megafuse
    kw = dict(maxits=1500, res_rtol=RTOL, megafuse=mega)
    rr, xr = _run(solver, S, bn, dev, rr_period=PERIOD, **kw)
    plain, xp = _run(solver, S, bn, dev, **kw)
    tr, tp = ms.true_residual(A, bn, xr), ms.true_residual(A, bn, xp)
    print(f"RR_GPU p48 mega={mega}: rr its={rr.niterations} conv={rr.converged} "
          f"true={tr / bnrm:.3e} nrepl={rr.nreplacements} | plain "
          f"its={plain.niterations} conv={plain.converged} true={tp / bnrm:.3e}")
    assert rr.converged
    assert tr <= 10 * RTOL * bnrm
    assert rr.niterations < plain.niterations
    assert tp >= 10 * tr
    assert rr.nreplacements == rr.niterations // PERIOD


def test_bsell_solve_reaches_the_classic_floor(dev):
    from acg_amd.solvers.hip import CGSolverHIP

    A = ms.queen6()
    bn, S = ms.rhs(A), ms.local(A)
    bnrm = float(np.linalg.norm(bn))
    solver = CGSolverHIP(S, device=dev, force_format="bsell")
    assert solver._format_name() == "bsell"
    kw = dict(maxits=300, res_rtol=0.0)
    _, xc = _run(solver, S, bn, dev, method="solve", **kw)
    rr, xr = _run(solver, S, bn, dev, rr_period=PERIOD, **kw)
    _, xp = _run(solver, S, bn, dev, **kw)
    tc, tr, tp = (ms.true_residual(A, bn, v) for v in (xc, xr, xp))
    print(f"RR_GPU queen6 bsell: classic={tc / bnrm:.3e} rr={tr / bnrm:.3e} "
          f"plain={tp / bnrm:.3e} nrepl={rr.nreplacements}")
    assert rr.niterations == 300 and rr.nreplacements == 6
    assert tr <= 100 * tc
    assert tp >= 100 * tr


@pytest.mark.parametrize("fmt", ["sell", "sigma", "bsell"])
def test_fast_path_matches_fallback(dev, fmt):
    from acg_amd.solvers.hip import CGSolverHIP

    if fmt == "bsell":
        A = ms.queen6()
        bn, S = ms.rhs(A), ms.local(A)
        kw = dict(maxits=600, res_rtol=1e-12, rr_period=PERIOD)
    else:
        A, bn, S = _p48()
        kw = dict(maxits=1500, res_rtol=RTOL, rr_period=PERIOD, megafuse=False)
    solver = CGSolverHIP(S, device=dev, force_format=fmt)
    assert solver._format_name() == fmt
    fast, xf = _run(solver, S, bn, dev, **kw)
    solver._rr_fast = False
    slow, xs = _run(solver, S, bn, dev, **kw)
    print(f"RR_GPU {fmt}: fast its={fast.niterations} fallback its={slow.niterations} "
          f"|dx|/|x|={np.linalg.norm(xf - xs) / np.linalg.norm(xs):.3e}")
    assert fast.converged and slow.converged
    assert fast.niterations == slow.niterations
    assert np.linalg.norm(xf - xs) <= 10 * kw["res_rtol"] * np.linalg.norm(xs)


@pytest.mark.parametrize("mega", [False, True])
def test_graph_replay_keeps_the_iteration_count(dev, mega):
    from acg_amd.solvers.hip import CGSolverHIP

    A, bn, S = _p48()
    solver = CGSolverHIP(S, device=dev)
    kw = dict(maxits=1500, res_rtol=RTOL, rr_period=PERIOD, megafuse=mega)
    eager, _ = _run(solver, S, bn, dev, use_graph=False, **kw)
    graph, xg = _run(solver, S, bn, dev, use_graph=True, **kw)
    key = "pipelined_mega_rr" if mega else "pipelined_rr"
    assert key in solver._graphs, "the replay path did not run"
    assert eager.converged and graph.converged
    assert graph.niterations == eager.niterations
    assert ms.true_residual(A, bn, xg) <= 10 * RTOL * float(np.linalg.norm(bn))


@pytest.mark.parametrize("name,fmt", [("poisson32", "sell"), ("queen6", "bsell")])
def test_period_zero_is_the_plain_solve(dev, name, fmt):
    from acg_amd.solvers.hip import CGSolverHIP

    A = ms.SYSTEMS[name]()
    bn, S = ms.rhs(A), ms.local(A)
    solver = CGSolverHIP(S, device=dev, force_format=fmt)
    kw = dict(maxits=150, res_rtol=1e-10)
    r0, x0 = _run(solver, S, bn, dev, **kw)
    keys = set(solver._ws)
    r1, x1 = _run(solver, S, bn, dev, rr_period=0, **kw)
    assert set(solver._ws) == keys, "rr_period=0 must use the plain workspace"
    assert r0.niterations == r1.niterations and r1.nreplacements == 0
    assert _same_bits(x0, x1)
    with pytest.raises(ValueError, match="rr_period"):
        _run(solver, S, bn, dev, rr_period=-1, **kw)


# ---------------------------------------------------------------------------
# two processes on one GPU over gloo: the ghost-tailed t / p

def _worker(rank, world, port, q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        os.environ["RANK"] = str(rank)
        os.environ["WORLD_SIZE"] = str(world)
        from acg_amd.dist.comm import Comm
        from acg_amd.solvers.hip import CGSolverHIP

        comm = Comm("gloo")
        A = ms.poisson32()
        S = ms.local(A, nparts=world, rank=rank)
        assert S.nghost > 0
        b = torch.from_numpy(ms.rhs(A)[S.owned_global]).cuda()
        solver = CGSolverHIP(S, comm=comm, device="cuda:0")
        out = []
        for mega in (False, True):
            x = torch.zeros(S.nowned + S.nghost, dtype=torch.float64,
                            device="cuda:0")
            res = solver.solve_pipelined(b, x, maxits=2000, res_rtol=RTOL,
                                         rr_period=PERIOD, megafuse=mega)
            out.append((x[:S.nowned].cpu().numpy(), res.niterations,
                        res.converged, res.nreplacements))
        q.put((rank, "ok", (S.owned_global, out)))
        comm.finalize()
    except Exception:  # pragma: no cover
        import traceback

        q.put((rank, "err", traceback.format_exc()))
        raise


def test_two_ranks_on_one_gpu(dev):
    from acg_amd.solvers.hip import CGSolverHIP

    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    procs = [ctx.Process(target=_worker, args=(r, 2, 29682, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = {}
    for _ in procs:
        rank, status, payload = q.get()
        assert status == "ok", f"rank {rank} failed:\n{payload}"
        results[rank] = payload
    for p in procs:
        p.join(timeout=120)
    A = ms.poisson32()
    bn, S = ms.rhs(A), ms.local(A)
    bnrm = float(np.linalg.norm(bn))
    solver = CGSolverHIP(S, device=dev)
    for i, mega in enumerate((False, True)):
        one, _ = _run(solver, S, bn, dev, maxits=2000, res_rtol=RTOL,
                      rr_period=PERIOD, megafuse=mega)
        xg = np.full(A.n, np.nan)
        for owned, out in results.values():
            xloc, nit, conv, nrep = out[i]
            assert conv and nit == one.niterations, (mega, nit, one.niterations)
            assert nrep == nit // PERIOD
            xg[owned] = xloc
        true = ms.true_residual(A, bn, xg)
        print(f"RR_GPU 2 ranks mega={mega}: its={one.niterations} "
              f"true={true / bnrm:.3e}")
        assert one.converged
        assert true <= 10 * RTOL * bnrm
