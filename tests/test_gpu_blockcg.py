"""Block CG on the GPU: the block-CG kernels through gpu_ops against the
long-double oracle of tests/blockcg_oracle.py on NaN-poisoned buffers (the
inputs tests/test_blockcg_cpu.py proves discriminating), then
CGSolverHIP.solve_block against CGSolverCPU.solve_block and per-column
solves, and the CLI."""

import numpy as np
import pytest
import torch

import blockcg_oracle as bo
import kernel_oracle as ko
import multirhs_oracle as mo

pytestmark = pytest.mark.gpu

KG = [(k, kg) for k in bo.KS for kg in sorted({1, k - 1, k})]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gpu_ops():
    from acg_amd.ops import gpu_ops

    bo.check_layout(gpu_ops)
    assert gpu_ops.alloc_block_state("cuda:0").shape == (bo.BS_SIZE,)
    return gpu_ops


def _same(ex1, ex2, names):
    for nm in names:
        a, b = ex1[nm], ex2[nm]
        if isinstance(a, dict):
            _same(a, b, a.keys())
        else:
            assert bo.same_bits(a, b), f"{nm}: two runs differ"


# ---------------------------------------------------------------------------
# row kernels

@pytest.mark.parametrize("n", bo.ROW_N)
@pytest.mark.parametrize("k", bo.KS)
def test_gram_multi(dev, gpu_ops, k, n):
    got, ex = bo.run_gram(gpu_ops, n, k, dev)
    assert ex["nblocks"] == bo.row_blocks(n)
    ko.assert_accepts(bo.gram_expectation(n, k), got, f"K{k} n{n}")
    bo.check_partials_untouched(ex["partials"], ex["nblocks"], k)
    _same(ex, bo.run_gram(gpu_ops, n, k, dev)[1], ("partials",))


@pytest.mark.parametrize("n", bo.ROW_N)
@pytest.mark.parametrize("k,kg", KG)
def test_block_update(dev, gpu_ops, k, kg, n):
    got, ex = bo.run_update(gpu_ops, n, k, kg, dev)
    bo.check_update(n, k, kg, got, ex, f"K{k} kg{kg} n{n}", on_gpu=True)
    _same(ex, bo.run_update(gpu_ops, n, k, kg, dev)[1], ("out", "partials"))


@pytest.mark.parametrize("n", bo.ROW_N)
@pytest.mark.parametrize("k,kg", KG)
def test_block_ortho(dev, gpu_ops, k, kg, n):
    for s_zero in (False, True):
        got, ex = bo.run_ortho(gpu_ops, n, k, kg, dev, s_zero=s_zero)
        bo.check_ortho(n, k, kg, got, ex, f"K{k} kg{kg} n{n} s0{s_zero}", s_zero)
        _same(ex, bo.run_ortho(gpu_ops, n, k, kg, dev, s_zero=s_zero)[1], ("out",))


@pytest.mark.parametrize("k", bo.KS)
def test_row_kernels_second_grid_stride_trip(dev, gpu_ops, k):
    """The block cap times the block size plus a tail: the first 77 threads
    of block 0 take a second trip."""
    n = bo.second_trip_n()
    assert bo.row_blocks(n) == gpu_ops.BLOCK_MAXG and n > gpu_ops.BLOCK_MAXG * 256
    got, ex = bo.run_gram(gpu_ops, n, k, dev)
    assert ex["nblocks"] == gpu_ops.BLOCK_MAXG
    ko.assert_accepts(bo.gram_expectation(n, k), got, f"K{k} n{n}")
    got, ex = bo.run_update(gpu_ops, n, k, k, dev)
    bo.check_update(n, k, k, got, ex, f"K{k} n{n}", on_gpu=True)
    got, ex = bo.run_ortho(gpu_ops, n, k, k, dev)
    bo.check_ortho(n, k, k, got, ex, f"K{k} n{n}")


@pytest.mark.parametrize("k", bo.KS)
def test_row_kernels_frozen_by_flag(dev, gpu_ops, k):
    _, ex = bo.run_update(gpu_ops, 65, k, k, dev, flag=True)
    bo.check_frozen_rows(ex)
    _, ex = bo.run_ortho(gpu_ops, 65, k, k, dev, flag=True)
    bo.check_frozen_rows(ex, "qs")


# ---------------------------------------------------------------------------
# coefficient kernels

@pytest.mark.parametrize("nb", bo.COEF_NB)
@pytest.mark.parametrize("k,kg", KG)
def test_coef_alpha(dev, gpu_ops, k, kg, nb):
    P8 = bo.gram_partials("spd", nb)
    ex = bo.run_coef_alpha(gpu_ops, P8, k, kg, dev)
    bo.check_coef_alpha(P8, k, kg, ex, f"K{k} kg{kg} nb{nb}")
    _same(ex, bo.run_coef_alpha(gpu_ops, P8, k, kg, dev), ("state",))


@pytest.mark.parametrize("init", [False, True])
@pytest.mark.parametrize("nb", bo.COEF_NB)
@pytest.mark.parametrize("k,kg", KG)
def test_coef_beta(dev, gpu_ops, k, kg, nb, init):
    P8 = bo.gram_partials("spd", nb)
    ex = bo.run_coef_beta(gpu_ops, P8, k, kg, dev, init=init)
    bo.check_coef_beta(P8, k, kg, ex, f"K{k} kg{kg} nb{nb} init{init}", init)
    _same(ex, bo.run_coef_beta(gpu_ops, P8, k, kg, dev, init=init),
          ("state", "rr_out"))


@pytest.mark.parametrize("k", bo.KS)
def test_coef_small_scale_is_no_breakdown(dev, gpu_ops, k):
    P8 = bo.gram_partials("spd", 5, 2.0 ** -16)
    bo.check_coef_beta(P8, k, k, bo.run_coef_beta(gpu_ops, P8, k, k, dev),
                       f"scaled K{k}")
    bo.check_coef_alpha(P8, k, k, bo.run_coef_alpha(gpu_ops, P8, k, k, dev),
                        f"scaled K{k}")


@pytest.mark.parametrize("kind", ["dup", "zero", "nan"])
@pytest.mark.parametrize("k", bo.KS)
def test_coef_breakdown(dev, gpu_ops, k, kind):
    P8 = bo.gram_partials(kind, 5)
    ex = bo.run_coef_alpha(gpu_ops, P8, k, k, dev, it=9)
    bo.check_breakdown(ex, k, 9, "M", beta=False)
    for init, it in ((False, 9), (True, 0)):
        ex = bo.run_coef_beta(gpu_ops, P8, k, k, dev, it=it, init=init)
        bo.check_breakdown(ex, k, it, "G", beta=True)
    if k > 2:
        ex = bo.run_coef_beta(gpu_ops, P8, k, 1, dev)
        bo.check_coef_beta(P8, k, 1, ex, f"{kind} kg1")


@pytest.mark.parametrize("k", bo.KS)
def test_coef_flag_on_entry(dev, gpu_ops, k):
    P8 = bo.gram_partials("spd", 5)
    bo.check_flag_on_entry(bo.run_coef_alpha(gpu_ops, P8, k, k, dev, flag=True),
                           k, beta=False)
    bo.check_flag_on_entry(bo.run_coef_beta(gpu_ops, P8, k, k, dev, flag=True),
                           k, beta=True)


def test_wrappers_refuse_bad_arguments(dev, gpu_ops):
    X = torch.zeros(10, 4, dtype=torch.float64, device=dev)
    p = gpu_ops.alloc_partials_multi(dev, 4)
    st = gpu_ops.alloc_block_state(dev)
    rr = torch.zeros(6, dtype=torch.float64, device=dev)
    X3 = torch.zeros(10, 3, dtype=torch.float64, device=dev)
    with pytest.raises(ValueError):
        gpu_ops.gram_multi(X3, X3, p)
    with pytest.raises(ValueError):
        gpu_ops.gram_multi(X[:, ::2], X[:, ::2], p)
    with pytest.raises(TypeError):
        gpu_ops.gram_multi(X.float(), X.float(), p)
    with pytest.raises(ValueError):
        gpu_ops.gram_multi(X, X, p, n=11)
    with pytest.raises(ValueError):
        gpu_ops.gram_multi(X, X, p[:1, :100])
    with pytest.raises(ValueError):
        gpu_ops.block_update(X, X, X, X, st[:100], p, 10)
    with pytest.raises(ValueError):
        gpu_ops.block_ortho(X, X, st.float(), 10)
    with pytest.raises(ValueError):
        gpu_ops.block_coef_alpha(p, 1, st, 3, 1, 1)
    with pytest.raises(ValueError):
        gpu_ops.block_coef_alpha(p, 1, st, 4, 5, 1)
    with pytest.raises(ValueError):
        gpu_ops.block_coef_alpha(p, 0, st, 4, 4, 1)
    with pytest.raises(ValueError):
        gpu_ops.block_coef_beta(p, gpu_ops.BLOCK_MAXG + 1, st, rr, 4, 4, 1)
    with pytest.raises(ValueError):
        gpu_ops.block_coef_beta(p, 1, st, rr[:5], 4, 4, 1)
    with pytest.raises(ValueError):
        gpu_ops.block_coef_beta(p, 1, st.cpu(), rr, 4, 4, 1)


# ---------------------------------------------------------------------------
# solver

@pytest.fixture(scope="module", params=["sell7", "bsell3"])
def system(request):
    S, B = bo.solver_system(request.param)
    return request.param, S, B


@pytest.fixture(scope="module")
def single_solves(dev, system):
    """Reference: one CGSolverHIP.solve() per column, computed once."""
    from acg_amd.solvers.hip import CGSolverHIP

    name, S, B = system
    solver = CGSolverHIP(S, device=dev)
    out = []
    for c in range(B.shape[1]):
        x = torch.zeros(S.nowned, dtype=torch.float64, device=dev)
        res = solver.solve(torch.from_numpy(B[:, c].copy()).to(dev), x,
                           maxits=bo.MAXITS, res_rtol=bo.RTOL)
        assert res.converged
        out.append((x.cpu(), res.niterations))
    return out


def _hip(S, dev, **kw):
    from acg_amd.solvers.hip import CGSolverHIP

    return CGSolverHIP(S, device=dev, **kw)


def _solve_block(solver, S, Bk, dev, x0=None, **kw):
    X = torch.zeros(S.nowned, Bk.shape[1], dtype=torch.float64, device=dev)
    if x0 is not None:
        X[:] = torch.from_numpy(x0).to(dev)
    kw = {"maxits": bo.MAXITS, "res_rtol": bo.RTOL, **kw}
    res = solver.solve_block(torch.from_numpy(np.array(Bk, order="C")).to(dev),
                             X, **kw)
    Xh = X.cpu().numpy()
    assert np.isfinite(Xh).all()
    return Xh, res


def _agrees_with_single(S, Bk, X, solver, dev):
    for c in range(Bk.shape[1]):
        x = torch.zeros(S.nowned, dtype=torch.float64, device=dev)
        r = solver.solve(torch.from_numpy(Bk[:, c].copy()).to(dev), x,
                         maxits=bo.MAXITS, res_rtol=bo.RTOL)
        assert r.converged
        torch.testing.assert_close(torch.from_numpy(X[:, c].copy()), x.cpu(),
                                   rtol=1e-6, atol=1e-8)


@pytest.mark.parametrize("k", [2, 3, 5, 8])
def test_solve_block(dev, system, single_solves, k):
    name, S, B = system
    solver = _hip(S, dev)
    assert solver._format_name() == ("sell" if name == "sell7" else "bsell")
    assert solver._multi_fast_path()
    X, res = _solve_block(solver, S, B[:, :k], dev)
    Xc, resc = bo.cpu_block_solves(name, k)
    assert len(res) == k
    for c in range(k):
        assert res[c].converged and res[c].block_breakdown == -1, res[c].summary()
        assert res[c].solver == "cg-hip-block"
        assert res[c].bnrm2 == pytest.approx(np.linalg.norm(B[:, c]), rel=1e-12)
        torch.testing.assert_close(torch.from_numpy(X[:, c].copy()),
                                   single_solves[c][0], rtol=1e-6, atol=1e-8)
    torch.testing.assert_close(torch.from_numpy(X), torch.from_numpy(Xc.copy()),
                               rtol=1e-6, atol=1e-8)
    bo.check_true_residual(S, B[:, :k], X, f"{name} k{k}")
    nit = max(r.niterations for r in res)
    nit_cpu = max(r.niterations for r in resc)
    nit_single = max(s[1] for s in single_solves[:k])
    print(f"BLOCK_CG {name} k{k}: block its {nit}, cpu block {nit_cpu}, "
          f"single max {nit_single}")
    assert abs(nit - nit_cpu) <= 2
    assert nit <= nit_single


def test_group_splitting(dev, system):
    name, S, B = system
    solver = _hip(S, dev)
    B11 = np.column_stack([B, B[:, 1] + B[:, 2], B[:, 3] - B[:, 4], B[:, 5] + 1.0])
    for group, shapes in ((8, [(8, 8), (4, 3)]), (4, [(4, 4), (4, 4), (4, 3)])):
        solver.multi_group = group
        calls = []
        real = solver._block_iterate
        solver._block_iterate = lambda ws, K, kg, *a: (calls.append((K, kg)),
                                                       real(ws, K, kg, *a))[1]
        X, res = _solve_block(solver, S, B11, dev)
        del solver._block_iterate
        assert calls == shapes and len(res) == 11
        assert all(r.converged and r.block_breakdown == -1 for r in res)
        bo.check_true_residual(S, B11, X, f"{name} group{group}")
        assert f"block{shapes[0][0]}" in solver._ws
    solver.multi_group = 3
    with pytest.raises(ValueError):
        _solve_block(solver, S, B11, dev)


def test_zero_column_and_x0(dev, system):
    name, S, B = system
    solver = _hip(S, dev)
    Bz = np.column_stack([B[:, 1], np.zeros(S.nowned), B[:, 2]])
    X, res = _solve_block(solver, S, Bz, dev)
    assert res[1].converged and res[1].niterations == 0 and res[1].bnrm2 == 0.0
    assert not X[:, 1].any()
    assert res[0].converged and res[2].converged
    bo.check_true_residual(S, Bz[:, [0, 2]], X[:, [0, 2]], f"{name} zero")
    X2, res2 = _solve_block(solver, S, Bz, dev, x0=X, res_rtol=1e-8)
    assert all(r.converged and r.niterations == 0 for r in res2)
    assert np.array_equal(X2, X)
    with pytest.raises(ValueError):
        solver.solve_block(torch.from_numpy(Bz.copy()).to(dev),
                           torch.zeros(S.nowned, 2, dtype=torch.float64, device=dev))


def test_handover_at_initialisation(dev, system):
    name, S, B = system
    solver = _hip(S, dev)
    Bd = bo.special_rhs(name, "dependent")
    X, res = _solve_block(solver, S, Bd, dev)
    assert all(r.converged and r.block_breakdown == 0 for r in res)
    assert all(r.solver == "cg-hip-block" for r in res)
    bo.check_true_residual(S, Bd, X, f"{name} dependent")
    _agrees_with_single(S, Bd, X, solver, dev)


def test_near_dependence_both_sides_of_tau(dev, system):
    name, S, B = system
    solver = _hip(S, dev)
    for eps, want in ((1e-2, -1), (1e-4, 0)):
        Bn = bo.special_rhs(name, "near", eps)
        X, res = _solve_block(solver, S, Bn, dev)
        assert all(r.converged and r.block_breakdown == want for r in res), \
            [(r.converged, r.block_breakdown) for r in res]
        bo.check_true_residual(S, Bn, X, f"{name} eps{eps}")
        _agrees_with_single(S, Bn, X, solver, dev)


def test_handover_in_the_first_iteration(dev, system):
    name, S, B = system
    solver = _hip(S, dev)
    Be = bo.special_rhs(name, "exact")
    X1, res1 = _solve_block(solver, S, Be, dev, maxits=1)
    assert all(r.block_breakdown == 1 for r in res1)
    r1 = np.linalg.norm(Be[:, 1] - bo.csr_apply(S, X1)[:, 1]) / np.linalg.norm(Be[:, 1])
    print(f"BLOCK_CG {name} exact column: rel res at hand-over {r1:.3e}")
    assert r1 <= bo.RTOL
    X, res = _solve_block(solver, S, Be, dev)
    assert all(r.converged and r.block_breakdown == 1 for r in res)
    bo.check_true_residual(S, Be, X, f"{name} exact")
    _agrees_with_single(S, Be, X, solver, dev)


@pytest.mark.parametrize("maxits", mo.SHORT_MAXITS)
def test_solve_block_stopped_within_the_lag(dev, maxits):
    """maxits <= 3: the lag-2 host test reads everything in its tail drain
    (maxits <= 2) or one state in the loop and the rest in the drain."""
    mo.check_short_run("solve_block", maxits, dev)


def test_csr_and_k1_are_solve_multi(dev, system):
    name, S, B = system
    Bk = torch.from_numpy(B[:, :4].copy()).to(dev)
    solver = _hip(S, dev, force_format="csr")
    assert not solver._multi_fast_path()
    Xb = torch.zeros(S.nowned, 4, dtype=torch.float64, device=dev)
    rb = solver.solve_block(Bk, Xb, maxits=bo.MAXITS, res_rtol=bo.RTOL)
    Xm = torch.zeros_like(Xb)
    rm = solver.solve_multi(Bk, Xm, maxits=bo.MAXITS, res_rtol=bo.RTOL)
    assert torch.equal(Xb, Xm)
    assert [r.solver for r in rb] == [r.solver for r in rm] == ["cg-hip"] * 4
    assert [r.niterations for r in rb] == [r.niterations for r in rm]
    solver = _hip(S, dev)
    X1 = torch.zeros(S.nowned, 1, dtype=torch.float64, device=dev)
    r1 = solver.solve_block(Bk[:, 1:2].contiguous(), X1, maxits=bo.MAXITS,
                            res_rtol=bo.RTOL)
    Xm1 = torch.zeros_like(X1)
    rm1 = solver.solve_multi(Bk[:, 1:2].contiguous(), Xm1, maxits=bo.MAXITS,
                             res_rtol=bo.RTOL)
    assert torch.equal(X1, Xm1) and r1[0].solver == rm1[0].solver == "cg-hip"
    assert r1[0].niterations == rm1[0].niterations and r1[0].block_breakdown == -1


def test_deterministic(dev, system):
    name, S, B = system
    solver = _hip(S, dev)
    Xa, ra = _solve_block(solver, S, B[:, :5], dev)
    Xb, rb = _solve_block(solver, S, B[:, :5], dev)
    assert np.array_equal(Xa, Xb)
    assert [r.niterations for r in ra] == [r.niterations for r in rb]
    Xc, _ = _solve_block(_hip(S, dev), S, B[:, :5], dev)
    assert np.array_equal(Xa, Xc)


# ---------------------------------------------------------------------------
# CLI

def test_cli_block_gpu_matches_cpu(tmp_path, capsys, monkeypatch):
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
    for solver in ("acg-block", "cpu-block"):
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
        assert out.err.count("solver: cg-hip-block" if solver == "acg-block"
                             else "solver: cg-block") == 3
    for c in range(3):
        np.testing.assert_allclose(outs["acg-block"][:, c], outs["cpu-block"][:, c],
                                   rtol=1e-6, atol=1e-8)
