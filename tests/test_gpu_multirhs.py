"""Multiple right-hand sides on the GPU: the SpMM / multi-vector kernels
against the single-vector oracle expectation of every column
(tests/multirhs_oracle.py), through gpu_ops, on NaN-poisoned buffers; then
CGSolverHIP.solve_multi and the CLI.

Inputs are the ones tests/test_multirhs_cpu.py proves discriminating.
Every kernel runs twice: the two results must be bitwise equal."""

import numpy as np
import pytest
import torch

import kernel_oracle as ko
import multirhs_oracle as mo

pytestmark = pytest.mark.gpu

VEC_N = (1, 257, 300_001)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gpu_ops():
    from acg_amd.ops import gpu_ops

    assert gpu_ops.MAXG == ko.MAXG and gpu_ops.S_NSLOTS == ko.S_NSLOTS
    assert tuple(gpu_ops.MULTI_K) == mo.KS
    return gpu_ops


def _accept_all(expect_of, gots, tag):
    for c, got in enumerate(gots):
        ko.assert_accepts(expect_of(c), got, f"{tag} col{c}")


def _same_bits(ex1, ex2, names):
    for nm in names:
        a, b = np.ascontiguousarray(ex1[nm]), np.ascontiguousarray(ex2[nm])
        assert np.array_equal(a.view(np.int64), b.view(np.int64)), \
            f"{nm}: two runs differ"


# ---------------------------------------------------------------------------
# SpMM

@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("col64", [False, True])
@pytest.mark.parametrize("nslices", [3, 37])
@pytest.mark.parametrize("k", mo.KS)
def test_spmm_sell(dev, gpu_ops, k, nslices, col64, fused):
    gots, ex = mo.run_spmm_sell(gpu_ops, nslices, False, k, dev, col64=col64,
                                fused=fused)
    s0 = mo.slab(k)
    _accept_all(lambda c: mo.sell_expect(nslices, False, c, s0[c], fused), gots,
                f"K{k} ns{nslices} col64={col64} fused{fused}")
    mo.check_untouched(ex, k, on_gpu=True)
    _, ex2 = mo.run_spmm_sell(gpu_ops, nslices, False, k, dev, col64=col64,
                              fused=fused)
    _same_bits(ex, ex2, ("Y", "scal", "partials"))


@pytest.mark.parametrize("k", mo.KS)
def test_spmm_sell_short_slices(dev, gpu_ops, k):
    """Slice lengths 0, 1, 7, 9: empty, below the unroll depth, and full
    unrolled steps plus a one-entry tail."""
    case, _ = mo.sell_multi_case(5, True)
    assert set(ko.sell_padded_len(case.rowptr)) == {0, 1, 7, 9}
    s0 = mo.slab(k)
    for fused in (False, True):
        gots, ex = mo.run_spmm_sell(gpu_ops, 5, True, k, dev, fused=fused)
        _accept_all(lambda c: mo.sell_expect(5, True, c, s0[c], fused), gots,
                    f"short K{k} fused{fused}")
        mo.check_untouched(ex, k, on_gpu=True)


@pytest.mark.parametrize("k", mo.KS)
def test_spmm_sell_sigma_perm(dev, gpu_ops, k):
    gots, ex = mo.run_spmm_sell(gpu_ops, 37, False, k, dev, sigma=4)
    s0 = mo.slab(k)
    _accept_all(lambda c: mo.sell_expect(37, False, c, s0[c], True, sigma=4),
                gots, f"sigma4 K{k}")
    mo.check_untouched(ex, k, on_gpu=True)


@pytest.mark.parametrize("ghost", [False, True])
@pytest.mark.parametrize("nnodes", [1, 65, 130])
@pytest.mark.parametrize("k", mo.KS)
@pytest.mark.parametrize("dof", (2, 3, 4))
def test_spmm_bsell(dev, gpu_ops, dof, k, nnodes, ghost):
    assert gpu_ops.spmm_bsell_supported(dof, k)
    s0 = mo.slab(k)
    for fused in (False, True):
        gots, ex = mo.run_spmm_bsell(gpu_ops, dof, nnodes, ghost, None, k, dev,
                                     fused=fused)
        _accept_all(lambda c: mo.bsell_expect(dof, nnodes, ghost, None, c, s0[c], fused),
                    gots, f"dof{dof} K{k} n{nnodes} ghost{ghost} fused{fused}")
        mo.check_untouched(ex, k, on_gpu=True)
        _, ex2 = mo.run_spmm_bsell(gpu_ops, dof, nnodes, ghost, None, k, dev,
                                   fused=fused)
        _same_bits(ex, ex2, ("Y", "scal", "partials"))


def test_spmm_bsell_empty_slice(dev, gpu_ops):
    gots, ex = mo.run_spmm_bsell(gpu_ops, 3, 130, True, 1, 4, dev)
    s0 = mo.slab(4)
    _accept_all(lambda c: mo.bsell_expect(3, 130, True, 1, c, s0[c], True), gots,
                "empty slice")
    mo.check_untouched(ex, 4, on_gpu=True)


# ---------------------------------------------------------------------------
# vector kernels

@pytest.mark.parametrize("n", VEC_N)
@pytest.mark.parametrize("k", mo.KS)
def test_cg_update_and_finalize_multi(dev, gpu_ops, k, n):
    mc = mo.vec_multi_case(n)
    s0 = mo.slab(k, rr=True, pt_zero_col=k - 1)
    gots, ex = mo.run_cg_update(gpu_ops, mc, k, dev, s0)
    assert ex["nblocks"] == mo.multi_blocks(n, k)
    _accept_all(lambda c: mo.cg_update_expect(mc, c, s0[c]), gots, f"K{k} n{n}")
    mo.check_rr_out(ex, k)
    mo.check_untouched(ex, k, on_gpu=True)
    # S_PT = 0: safe_div gives alpha = 0, r and x keep their bits
    assert np.array_equal(ex["R"][:, k - 1], mc.r[:, k - 1])
    assert np.array_equal(ex["X"][:, k - 1], mc.x[:, k - 1])
    _, ex2 = mo.run_cg_update(gpu_ops, mc, k, dev, s0)
    _same_bits(ex, ex2, ("R", "X", "scal", "partials", "rr_out"))


@pytest.mark.parametrize("n", VEC_N)
@pytest.mark.parametrize("k", mo.KS)
def test_daypx_ratio_multi(dev, gpu_ops, k, n):
    mc = mo.vec_multi_case(n)
    s0 = mo.slab(k, rr=True)
    s0[k - 1, ko.S_RR_PREV] = 0.0  # beta = 0 in one column
    for n_act in {n, n - 3 if n > 3 else n}:
        gots, ex = mo.run_daypx(gpu_ops, mc, k, dev, s0, n_act)
        _accept_all(lambda c: mo.daypx_expect(mc, c, s0[c], n_act), gots,
                    f"K{k} n{n} act{n_act}")
        assert np.array_equal(ex["P"][:n_act, k - 1], mc.x[:n_act, k - 1])
        _, ex2 = mo.run_daypx(gpu_ops, mc, k, dev, s0, n_act)
        _same_bits(ex, ex2, ("P", "scal"))


@pytest.mark.parametrize("n", VEC_N)
@pytest.mark.parametrize("k", mo.KS)
def test_dot_multi(dev, gpu_ops, k, n):
    mc = mo.vec_multi_case(n)
    for acc in (False, True):
        s0 = mo.slab(k)
        s0[:, ko.S_PT] = ko.SENTINELS[ko.S_PT]
        gots, ex = mo.run_dot(gpu_ops, mc, k, dev, s0, ko.S_PT, acc)
        _accept_all(lambda c: mo.dot_expect(mc, c, s0[c], ko.S_PT, acc), gots,
                    f"K{k} n{n} acc{acc}")
        mo.check_untouched(ex, k, on_gpu=True)
        _, ex2 = mo.run_dot(gpu_ops, mc, k, dev, s0, ko.S_PT, acc)
        _same_bits(ex, ex2, ("scal", "partials"))


@pytest.mark.parametrize("nb", [1, 255, 257, 4096])
@pytest.mark.parametrize("k", mo.KS)
def test_reduce_partials_multi(dev, gpu_ops, k, nb):
    pvals = mo.columns(nb, 14000 + nb, k).T.copy()
    for acc in (False, True):
        s0 = mo.slab(k)
        gots, ex = mo.run_reduce(gpu_ops, pvals, k, dev, s0, ko.S_GAMMA, acc)
        _accept_all(lambda c: mo.reduce_expect(pvals[c], s0[c], ko.S_GAMMA, acc),
                    gots, f"K{k} nb{nb} acc{acc}")
        _, ex2 = mo.run_reduce(gpu_ops, pvals, k, dev, s0, ko.S_GAMMA, acc)
        _same_bits(ex, ex2, ("scal",))


def test_wrappers_refuse_bad_arguments(dev, gpu_ops):
    X = torch.zeros(10, 4, dtype=torch.float64, device=dev)
    s = gpu_ops.alloc_scalars_multi(dev, 4)
    p = gpu_ops.alloc_partials_multi(dev, 4)
    assert s.shape == (4, ko.S_NSLOTS) and p.shape == (4, ko.MAXG)
    X3 = torch.zeros(10, 3, dtype=torch.float64, device=dev)
    with pytest.raises(ValueError):
        gpu_ops.dot_multi(X3, X3, p, s, 0)
    with pytest.raises(ValueError):
        gpu_ops.dot_multi(X[:, ::2], X[:, ::2], p, s, 0)
    with pytest.raises(TypeError):
        gpu_ops.dot_multi(X.float(), X.float(), p, s, 0)
    with pytest.raises(ValueError):
        gpu_ops.dot_multi(X, X, p, s, 0, n=11)
    with pytest.raises(ValueError):
        gpu_ops.dot_multi(X, X, p, s[:2], 0)
    case, Xc = mo.bsell_multi_case(3, 65, False)
    bptr, bcol, bvals = ko.pack_bsell(case, dev)
    Xm = ko._t(Xc[:, :4], dev)
    with pytest.raises(TypeError):
        gpu_ops.spmm_bsell(bptr, bcol, bvals.float(), case.nnodes, 3, Xm,
                           torch.zeros_like(Xm))


# ---------------------------------------------------------------------------
# solver

def _csr_apply(S, X, absval=False):
    vals = np.abs(S.A_vals) if absval else S.A_vals
    rows = ko.csr_rows(S.A_rowptr)
    Y = np.zeros((S.nowned, X.shape[1]))
    np.add.at(Y, rows, vals[:, None] * X[np.asarray(S.A_colidx, np.int64)])
    return Y


@pytest.fixture(scope="module", params=["sell7", "bsell3"])
def system(request):
    from acg_amd.gen import STENCIL_7PT_3D, queen_like_spec, stencil_local_slab

    if request.param == "sell7":
        S = stencil_local_slab(12, 12, 12, dict(STENCIL_7PT_3D), 0, 1)
    else:
        S = stencil_local_slab(8, 8, 9, queen_like_spec(3), 0, 1)
    assert S.nowned == 1728 and S.nghost == 0
    rng = np.random.default_rng(77)
    rand = rng.standard_normal((S.nowned, 10))
    a1 = _csr_apply(S, np.ones((S.nowned, 1)))[:, 0]
    cols = [a1, rand[:, 0], np.zeros(S.nowned), 4.0 * rand[:, 0]]
    B = np.column_stack(cols + [rand[:, i] for i in range(1, 8)])  # 11 columns
    return request.param, S, B


MAXITS, RTOL = 600, 1e-10


@pytest.fixture(scope="module")
def single_solves(dev, system):
    """Reference: one solve() per column, computed once."""
    from acg_amd.solvers.hip import CGSolverHIP

    name, S, B = system
    solver = CGSolverHIP(S, device=dev)
    out = []
    for c in range(B.shape[1]):
        x = torch.zeros(S.nowned, dtype=torch.float64, device=dev)
        if c == 2:  # zero column: nothing to iterate on
            out.append((x.cpu(), None))
            continue
        res = solver.solve(torch.from_numpy(B[:, c].copy()).to(dev), x,
                           maxits=MAXITS, res_rtol=RTOL)
        assert res.converged
        out.append((x.cpu(), res))
    return out


@pytest.mark.parametrize("k", [5, 11])
def test_solve_multi(dev, system, single_solves, k):
    """k = 5: one group padded to 8; k = 11: 8 + a group of 3 padded to 4."""
    from acg_amd.solvers.hip import CGSolverHIP

    name, S, B = system
    solver = CGSolverHIP(S, device=dev)
    assert solver._format_name() == ("sell" if name == "sell7" else "bsell")
    assert solver._multi_fast_path()
    Bk = torch.from_numpy(B[:, :k].copy()).to(dev)
    X = torch.zeros(S.nowned, k, dtype=torch.float64, device=dev)
    res = solver.solve_multi(Bk, X, maxits=MAXITS, res_rtol=RTOL)
    assert len(res) == k
    Xh = X.cpu()
    assert torch.isfinite(Xh).all()
    AX = _csr_apply(S, Xh.numpy())
    reach = _csr_apply(S, 1e-8 + 1e-6 * np.abs(Xh.numpy()), absval=True)
    for c in range(k):
        assert res[c].converged, (c, res[c].summary())
        assert res[c].solver == "cg-hip-multi"
        x1, r1 = single_solves[c]
        torch.testing.assert_close(Xh[:, c], x1, rtol=1e-6, atol=1e-8)
        # true residual, fp64 on the host: the target plus what the
        # comparison criterion above allows x to be off by
        bn = np.linalg.norm(B[:, c])
        rn = np.linalg.norm(B[:, c] - AX[:, c])
        print(f"MULTI_RHS {name} k{k} col{c}: it={res[c].niterations} "
              f"true_rel_res={rn / bn if bn else rn:.3e}")
        assert rn <= RTOL * bn + np.linalg.norm(reach[:, c])
        if r1 is not None:
            assert abs(res[c].niterations - r1.niterations) <= 2
            assert res[c].bnrm2 == pytest.approx(bn, rel=1e-12)
    # the zero column: converged at iteration 0, exact zeros
    assert res[2].niterations == 0 and res[2].bnrm2 == 0.0
    assert not Xh[:, 2].any()
    # 4 x a column is bitwise 4 x its solution (same group): a power-of-two
    # scaling commutes with every operation, any cross-column scalar mix-up
    # breaks it
    assert torch.equal(Xh[:, 3], 4.0 * Xh[:, 1])
    assert res[3].niterations == res[1].niterations


def test_solve_multi_repeat_and_x0(dev, system):
    """A second call on the same solver (workspace reuse) is bitwise the
    first; starting from the solution converges at iteration 0."""
    from acg_amd.solvers.hip import CGSolverHIP

    name, S, B = system
    solver = CGSolverHIP(S, device=dev)
    Bk = torch.from_numpy(B[:, :3].copy()).to(dev)
    X1 = torch.zeros(S.nowned, 3, dtype=torch.float64, device=dev)
    solver.solve_multi(Bk, X1, maxits=MAXITS, res_rtol=RTOL)
    X2 = torch.zeros_like(X1)
    solver.solve_multi(Bk, X2, maxits=MAXITS, res_rtol=RTOL)
    assert torch.equal(X1, X2)
    res = solver.solve_multi(Bk, X2, maxits=MAXITS, res_rtol=1e-8)
    assert all(r.converged and r.niterations == 0 for r in res)
    assert torch.equal(X1, X2)
    with pytest.raises(ValueError):
        solver.solve_multi(Bk, X2[:, :2].contiguous())


def test_solve_multi_groups_of_four(dev, system, single_solves):
    """multi_group = 4: k = 11 runs as 4 + 4 + 3 (padded to 4)."""
    from acg_amd.solvers.hip import CGSolverHIP

    name, S, B = system
    solver = CGSolverHIP(S, device=dev)
    solver.multi_group = 4
    assert solver._multi_kmax() == 4
    Bk = torch.from_numpy(B.copy()).to(dev)
    X = torch.zeros(S.nowned, 11, dtype=torch.float64, device=dev)
    res = solver.solve_multi(Bk, X, maxits=MAXITS, res_rtol=RTOL)
    Xh = X.cpu()
    for c in range(11):
        assert res[c].converged
        torch.testing.assert_close(Xh[:, c], single_solves[c][0], rtol=1e-6, atol=1e-8)
    assert torch.equal(Xh[:, 3], 4.0 * Xh[:, 1]) and not Xh[:, 2].any()
    solver.multi_group = 3
    with pytest.raises(ValueError):
        solver.solve_multi(Bk, X)


@pytest.mark.parametrize("maxits", mo.SHORT_MAXITS)
def test_solve_multi_stopped_within_the_lag(dev, maxits):
    """maxits <= 3: the lag-2 host test reads everything in its tail drain
    (maxits <= 2) or one value in the loop and the rest in the drain."""
    mo.check_short_run("solve_multi", maxits, dev)


def test_solve_multi_csr_falls_back(dev, system, single_solves):
    from acg_amd.solvers.hip import CGSolverHIP

    name, S, B = system
    solver = CGSolverHIP(S, device=dev, force_format="csr")
    assert solver._format_name() == "csr" and not solver._multi_fast_path()
    cols = [0, 1, 3, 4]  # without the zero column
    Bk = torch.from_numpy(B[:, cols].copy()).to(dev)
    X = torch.zeros(S.nowned, len(cols), dtype=torch.float64, device=dev)
    res = solver.solve_multi(Bk, X, maxits=MAXITS, res_rtol=RTOL)
    assert [r.solver for r in res] == ["cg-hip"] * len(cols)
    for i, c in enumerate(cols):
        assert res[i].converged
        torch.testing.assert_close(X[:, i].cpu(), single_solves[c][0],
                                   rtol=1e-6, atol=1e-8)


# ---------------------------------------------------------------------------
# CLI

def test_cli_multi_rhs_gpu_matches_cpu(tmp_path, capsys, monkeypatch):
    from acg_amd import cli
    from acg_amd.gen import STENCIL_5PT_2D, stencil_global
    from acg_amd.io.mtx import MtxFile, write_mtx

    A = stencil_global(24, 24, 1, STENCIL_5PT_2D)
    rows = np.repeat(np.arange(A.n), np.diff(A.rowptr))
    path = tmp_path / "p.mtx"
    write_mtx(path, MtxFile(object="matrix", format="coordinate", field_="real",
                            symmetry="symmetric", nrows=A.n, ncols=A.n,
                            nnz=A.nnz_stored, rowidx=rows, colidx=A.colidx,
                            a=A.vals))
    Bm = np.random.default_rng(9).standard_normal((A.n, 3))
    bpath = tmp_path / "b.mtx"
    write_mtx(bpath, MtxFile(object="matrix", format="array", field_="real",
                             symmetry="general", nrows=A.n, ncols=3,
                             nnz=3 * A.n, a=np.ascontiguousarray(Bm.T).reshape(-1)))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("RANK", raising=False)
    outs = {}
    for solver in ("acg", "cpu"):
        rc = cli.main([str(path), str(bpath), "--solver", solver,
                       "--max-iterations", "2000", "--residual-rtol", "1e-10"])
        out = capsys.readouterr()
        assert rc == 0, out.err
        lines = out.out.strip().splitlines()
        assert lines[0].startswith("%%MatrixMarket matrix array real general")
        assert lines[1].split() == [str(A.n), "3"]
        vals = np.array([float(v) for v in lines[2:]])
        assert len(vals) == 3 * A.n
        outs[solver] = vals.reshape(3, A.n).T
        assert out.err.count("true residual") == 3
        assert out.err.count("solver: cg-hip-multi" if solver == "acg"
                             else "solver: cg-cpu") == 3
    for c in range(3):
        np.testing.assert_allclose(outs["acg"][:, c], outs["cpu"][:, c],
                                   rtol=1e-6, atol=1e-8)
