"""Residual replacement of the pipelined CG on the host (no GPU needed):
the CPU solver that is the GPU's oracle, the torch reference of the dual
SpMV against the high-precision oracle, the 2-process gloo solve and the
CLI option."""

import os
from functools import lru_cache

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import kernel_oracle as ko
import mixed_systems as ms
import pipecg_rr_oracle as po
from acg_amd.io.mtx import MtxFile, write_mtx
from acg_amd.solvers.cpu import CGSolverCPU
from acg_amd.utils.errors import AcgError, ErrCode

RTOL = 1e-13
MAXITS = 2000
PERIOD = 50


def _solve(name, **kw):
    A = ms.SYSTEMS[name]()
    b = ms.rhs(A)
    S = ms.local(A)
    x = torch.zeros(S.nowned + S.nghost, dtype=torch.float64)
    res = CGSolverCPU(S).solve_pipelined(torch.from_numpy(b), x, **kw)
    return A, b, x[:S.nowned].numpy().copy(), res


@lru_cache(maxsize=None)
def _poisson(rr_period):
    return _solve("poisson32", maxits=MAXITS, res_rtol=RTOL, rr_period=rr_period)


# ---------------------------------------------------------------------------
# solver

@pytest.mark.parametrize("name,kw", [
    ("poisson32", dict(maxits=400, res_rtol=1e-10)),
    ("queen6", dict(maxits=120, res_rtol=0.0))])
def test_period_zero_is_the_plain_solve(name, kw):
    _, _, x0, r0 = _solve(name, **kw)
    _, _, x1, r1 = _solve(name, rr_period=0, **kw)
    assert r0.niterations == r1.niterations and r1.nreplacements == 0
    assert np.array_equal(x0.view(np.int64), x1.view(np.int64))


def test_negative_period_is_refused():
    with pytest.raises(ValueError, match="rr_period"):
        _solve("poisson32", maxits=5, rr_period=-1)


def test_replacement_reaches_the_true_residual():
    A, b, x, res = _poisson(PERIOD)
    _, _, _, plain = _poisson(0)
    bnrm = float(np.linalg.norm(b))
    true = ms.true_residual(A, b, x)
    print(f"RR_CPU poisson32 its={res.niterations} plain_its={plain.niterations} "
          f"true/(rtol*|b|)={true / (RTOL * bnrm):.3g} nrepl={res.nreplacements}")
    assert res.converged
    assert true <= 10 * RTOL * bnrm
    assert res.nreplacements == res.niterations // PERIOD
    assert plain.converged and res.niterations < plain.niterations


def test_plain_pipelined_reports_a_false_convergence():
    """The yardstick: without replacement the solve reports convergence
    while its true residual misses the bound used above by more than 10x."""
    A, b, x, plain = _poisson(0)
    bnrm = float(np.linalg.norm(b))
    true = ms.true_residual(A, b, x)
    print(f"RR_CPU plain poisson32 true/(10*rtol*|b|)={true / (10 * RTOL * bnrm):.3g}")
    assert plain.converged
    assert true > 10 * (10 * RTOL * bnrm)


# ---------------------------------------------------------------------------
# two processes over gloo

def _worker(rank, world, port, q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        os.environ["RANK"] = str(rank)
        os.environ["WORLD_SIZE"] = str(world)
        from acg_amd.dist.comm import Comm

        comm = Comm("gloo")
        A = ms.poisson32()
        b = ms.rhs(A)
        S = ms.local(A, nparts=world, rank=rank)
        x = torch.zeros(S.nowned + S.nghost, dtype=torch.float64)
        res = CGSolverCPU(S, comm=comm).solve_pipelined(
            torch.from_numpy(b[S.owned_global]), x, maxits=MAXITS,
            res_rtol=RTOL, rr_period=PERIOD)
        q.put((rank, "ok", (S.owned_global, x[:S.nowned].numpy().copy(),
                            res.niterations, res.converged, res.nreplacements)))
        comm.finalize()
    except Exception:  # pragma: no cover
        import traceback

        q.put((rank, "err", traceback.format_exc()))
        raise


def test_two_ranks_match_the_serial_solve():
    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    procs = [ctx.Process(target=_worker, args=(r, 2, 29681, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = {}
    for _ in procs:
        rank, status, payload = q.get()
        assert status == "ok", f"rank {rank} failed:\n{payload}"
        results[rank] = payload
    for p in procs:
        p.join(timeout=60)
    _, _, xs, serial = _poisson(PERIOD)
    xg = np.full(xs.size, np.nan)
    for owned, xloc, nit, conv, nrep in results.values():
        assert conv and nit == serial.niterations
        assert nrep == serial.nreplacements
        xg[owned] = xloc
    np.testing.assert_allclose(xg, xs, rtol=1e-6, atol=1e-8)


# ---------------------------------------------------------------------------
# torch reference of the dual SpMV against the long-double oracle

FLAGS = [(r, f) for r in (False, True) for f in (False, True)]


@pytest.mark.parametrize("resid,fuse", FLAGS)
@pytest.mark.parametrize("sigma", [1, 4])
@pytest.mark.parametrize("nslices,short", [(1, False), (3, True), (5, False)])
def test_torch_ref_spmv2_sell(nslices, short, sigma, resid, fuse):
    from acg_amd.ops import torch_ref

    case = po.sell_case2(nslices, short)
    got = po.run_sell_spmv2(torch_ref, case, "cpu", resid=resid, fuse=fuse,
                            sigma=sigma)
    e = po.sell_spmv2_expect(case, resid, fuse, perm=got["perm"])
    ko.assert_accepts(e, got, f"ns{nslices} short={short} sigma{sigma}")
    # the expectation can reject: the same run on perturbed values
    vals = case.vals * (1.0 + 1e-12)
    bad = po.run_sell_spmv2(torch_ref, case, "cpu", resid=resid, fuse=fuse,
                            sigma=sigma, vals=vals)
    if case.vals.size:
        assert not ko.accepts(e, bad)


@pytest.mark.parametrize("resid,fuse", FLAGS)
@pytest.mark.parametrize("dof,nnodes,ghost", [(2, 65, True), (3, 130, False),
                                              (4, 63, True), (3, 1, False)])
def test_torch_ref_spmv2_bsell(dof, nnodes, ghost, resid, fuse):
    from acg_amd.ops import torch_ref

    case = po.bsell_case2(dof, nnodes, ghost)
    got = po.run_bsell_spmv2(torch_ref, case, "cpu", resid=resid, fuse=fuse)
    e = po.bsell_spmv2_expect(case, resid, fuse)
    ko.assert_accepts(e, got, f"dof{dof} n{nnodes} ghost={ghost}")
    bptr, bcol, bvals = ko.pack_bsell(case, "cpu")
    bad = po.run_bsell_spmv2(torch_ref, case, "cpu", resid=resid, fuse=fuse,
                             packed=(bptr, bcol, bvals * (1.0 + 1e-12)))
    assert not ko.accepts(e, bad)


def test_torch_ref_spmv2_rejects_crossed_columns():
    """Swapping the two gathered vectors must be caught."""
    from acg_amd.ops import torch_ref

    case = po.sell_case2(3)
    e = po.sell_spmv2_expect(case, False, True)
    got = po.run_sell_spmv2(torch_ref, case, "cpu", resid=False, fuse=True)
    assert ko.accepts(e, got)
    swapped = dict(got, y1=got["y2"], y2=got["y1"])
    assert not ko.accepts(e, swapped)


@pytest.mark.parametrize("dof,size,sigma", [(1, 3, 1), (1, 3, 4), (3, 130, 1)])
def test_torch_ref_dot2_slices(dof, size, sigma):
    from acg_amd.ops import torch_ref

    if dof == 1:
        case = po.sell_case2(size)
        fused = po.run_sell_spmv2(torch_ref, case, "cpu", resid=True, fuse=True,
                                  sigma=sigma)
        perm, nunits = fused["perm"], case.nrows
        blocks = po.block_rows(case.nrows, case.nslices, perm=perm)
    else:
        case = po.bsell_case2(dof, size, True)
        fused = po.run_bsell_spmv2(torch_ref, case, "cpu", resid=True, fuse=True)
        perm, nunits = None, case.nnodes
        blocks = po.block_rows(case.nrows, (size + 63) // 64, dof)
    e = po.dot2_slices_expect(case.nrows, case.x, fused["y1"], blocks)
    got = po.run_dot2_slices(torch_ref, case.x, fused["y1"], nunits, dof, "cpu", perm)
    ko.assert_accepts(e, got, f"dof{dof} size{size} sigma{sigma}")
    # rejects the other vector pairing
    bad = po.run_dot2_slices(torch_ref, case.x, fused["y2"], nunits, dof, "cpu", perm)
    assert not ko.accepts(e, bad)


def test_torch_ref_replace_finalize():
    from acg_amd.ops import torch_ref

    for nb in (1, 5, 300):
        case = po.finalize_case(nb)
        ko.assert_accepts(po.finalize_expect(case),
                          po.run_finalize(torch_ref, case, "cpu"), f"nb{nb}")


def test_torch_ref_refuses_float32_values():
    from acg_amd.ops import torch_ref

    case = po.sell_case2(1)
    with pytest.raises(TypeError, match="float64"):
        po.run_sell_spmv2(torch_ref, case, "cpu", resid=False, fuse=False,
                          vals=case.vals.astype(np.float32))


# ---------------------------------------------------------------------------
# CLI

def _mtx(tmp_path):
    A = ms.poisson32()
    rows = np.repeat(np.arange(A.n), np.diff(A.rowptr))
    path = tmp_path / "A.mtx"
    write_mtx(path, MtxFile(object="matrix", format="coordinate", field_="real",
                            symmetry="symmetric", nrows=A.n, ncols=A.n,
                            nnz=A.nnz_stored, rowidx=rows, colidx=A.colidx,
                            a=A.vals))
    return path


def _cli(monkeypatch, capsys, argv):
    from acg_amd import cli

    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("RANK", raising=False)
    rc = cli.main([str(a) for a in argv])
    return rc, capsys.readouterr()


def test_cli_runs_and_reports_replacements(tmp_path, monkeypatch, capsys):
    rc, out = _cli(monkeypatch, capsys, [
        _mtx(tmp_path), "--solver", "cpu-pipelined", "--residual-replacement",
        str(PERIOD), "--max-iterations", str(MAXITS), "--residual-rtol",
        str(RTOL), "-q", "-v"])
    assert rc == 0
    assert f"residual replacement every {PERIOD} iterations" in out.err
    line = next(l for l in out.err.splitlines()
                if l.startswith("residual replacements:"))
    assert int(line.split(":")[1]) >= 1


def test_cli_refuses_other_solvers(tmp_path, monkeypatch, capsys):
    path = _mtx(tmp_path)
    with pytest.raises(AcgError, match="--residual-replacement") as ei:
        _cli(monkeypatch, capsys, [path, "--solver", "cpu",
                                   "--residual-replacement", str(PERIOD)])
    assert ei.value.code == ErrCode.NOT_SUPPORTED
    # 0 stays accepted everywhere
    rc, _ = _cli(monkeypatch, capsys, [path, "--solver", "cpu",
                                       "--residual-replacement", "0", "-q",
                                       "--max-iterations", str(MAXITS)])
    assert rc == 0
