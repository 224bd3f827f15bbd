"""Block CG without a GPU: the torch_ref counterparts of the block-CG
kernels against the long-double oracle of tests/blockcg_oracle.py, mutants
that prove the inputs discriminate, and CGSolverCPU.solve_block (the
oracle of the GPU solver) against per-column solve() and a scipy residual."""

import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import blockcg_oracle as bo
import kernel_oracle as ko
from acg_amd.ops import torch_ref

CPU = torch.device("cpu")
KG = [(k, kg) for k in bo.KS for kg in sorted({1, k - 1, k})]


def test_layout_is_mirrored():
    bo.check_layout(torch_ref)
    assert torch_ref.alloc_block_state().shape == (bo.BS_SIZE,)


# ---------------------------------------------------------------------------
# row kernels

@pytest.mark.parametrize("n", bo.ROW_N)
@pytest.mark.parametrize("k", bo.KS)
def test_ref_gram_multi(k, n):
    got, ex = bo.run_gram(torch_ref, n, k, CPU)
    ko.assert_accepts(bo.gram_expectation(n, k), got, f"K{k} n{n}")
    bo.check_partials_untouched(ex["partials"], ex["nblocks"], k)


@pytest.mark.parametrize("n", bo.ROW_N)
@pytest.mark.parametrize("k,kg", KG)
def test_ref_block_update(k, kg, n):
    got, ex = bo.run_update(torch_ref, n, k, kg, CPU)
    _check_update_ref(n, k, kg, got, ex)


def _check_update_ref(n, k, kg, got, ex):
    bo.check_update(n, k, kg, got, ex, f"K{k} kg{kg} n{n}")


@pytest.mark.parametrize("n", bo.ROW_N)
@pytest.mark.parametrize("k,kg", KG)
def test_ref_block_ortho(k, kg, n):
    for s_zero in (False, True):
        got, ex = bo.run_ortho(torch_ref, n, k, kg, CPU, s_zero=s_zero)
        bo.check_ortho(n, k, kg, got, ex, f"K{k} kg{kg} n{n} s0{s_zero}", s_zero)


@pytest.mark.parametrize("k", bo.KS)
def test_ref_row_ops_second_trip_size(k):
    n = bo.second_trip_n()
    assert n > bo.BLOCK_MAXG * 256
    got, ex = bo.run_gram(torch_ref, n, k, CPU)
    ko.assert_accepts(bo.gram_expectation(n, k), got, f"K{k} n{n}")
    got, ex = bo.run_update(torch_ref, n, k, k, CPU)
    _check_update_ref(n, k, k, got, ex)
    got, ex = bo.run_ortho(torch_ref, n, k, k, CPU)
    bo.check_ortho(n, k, k, got, ex, f"K{k} n{n}")


@pytest.mark.parametrize("k", bo.KS)
def test_ref_row_ops_frozen_by_flag(k):
    _, ex = bo.run_update(torch_ref, 65, k, k, CPU, flag=True)
    bo.check_frozen_rows(ex)
    _, ex = bo.run_ortho(torch_ref, 65, k, k, CPU, flag=True)
    bo.check_frozen_rows(ex, "qs")


# ---------------------------------------------------------------------------
# coefficient kernels

@pytest.mark.parametrize("nb", bo.COEF_NB)
@pytest.mark.parametrize("k,kg", KG)
def test_ref_coef_alpha(k, kg, nb):
    P8 = bo.gram_partials("spd", nb)
    ex = bo.run_coef_alpha(torch_ref, P8, k, kg, CPU)
    bo.check_coef_alpha(P8, k, kg, ex, f"K{k} kg{kg} nb{nb}")


@pytest.mark.parametrize("init", [False, True])
@pytest.mark.parametrize("nb", bo.COEF_NB)
@pytest.mark.parametrize("k,kg", KG)
def test_ref_coef_beta(k, kg, nb, init):
    P8 = bo.gram_partials("spd", nb)
    ex = bo.run_coef_beta(torch_ref, P8, k, kg, CPU, init=init)
    bo.check_coef_beta(P8, k, kg, ex, f"K{k} kg{kg} nb{nb} init{init}", init)


@pytest.mark.parametrize("k", bo.KS)
def test_ref_coef_small_scale_is_no_breakdown(k):
    """Columns scaled by 2^-16: every Gram entry is far below tau in
    absolute terms, the relative pivot test is unaffected."""
    P8 = bo.gram_partials("spd", 5, 2.0 ** -16)
    assert P8[0].sum() < bo.TAU
    bo.check_coef_beta(P8, k, k, bo.run_coef_beta(torch_ref, P8, k, k, CPU),
                       f"scaled K{k}")
    bo.check_coef_alpha(P8, k, k, bo.run_coef_alpha(torch_ref, P8, k, k, CPU),
                        f"scaled K{k}")


@pytest.mark.parametrize("kind", ["dup", "zero", "nan"])
@pytest.mark.parametrize("k", bo.KS)
def test_ref_coef_breakdown(k, kind):
    """Two identical columns, a zero column, a NaN in the Gram: flag and
    iteration set, nothing else but the published Gram changes."""
    P8 = bo.gram_partials(kind, 5)
    ex = bo.run_coef_alpha(torch_ref, P8, k, k, CPU, it=9)
    bo.check_breakdown(ex, k, 9, "M", beta=False)
    for init, it in ((False, 9), (True, 0)):
        ex = bo.run_coef_beta(torch_ref, P8, k, k, CPU, it=it, init=init)
        bo.check_breakdown(ex, k, it, "G", beta=True)
    # the dependent column outside the real columns: no breakdown
    if k > 2:
        ex = bo.run_coef_beta(torch_ref, P8, k, 1, CPU)
        bo.check_coef_beta(P8, k, 1, ex, f"{kind} kg1")


@pytest.mark.parametrize("k", bo.KS)
def test_ref_coef_flag_on_entry(k):
    P8 = bo.gram_partials("spd", 5)
    bo.check_flag_on_entry(bo.run_coef_alpha(torch_ref, P8, k, k, CPU, flag=True),
                           k, beta=False)
    bo.check_flag_on_entry(bo.run_coef_beta(torch_ref, P8, k, k, CPU, flag=True),
                           k, beta=True)


# ---------------------------------------------------------------------------
# mutants: each must be rejected on at least one case

def _ops(**over):
    names = ("gram_multi", "block_update", "block_ortho", "block_coef_alpha",
             "block_coef_beta")
    d = {nm: getattr(torch_ref, nm) for nm in names}
    d.update(over)
    return SimpleNamespace(**d)


def _rejected(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


def _with_region(base, transform, op):
    """Run ``op`` with one state region replaced, then put it back."""
    def wrapped(*args):
        state = next(a for a in args if isinstance(a, torch.Tensor)
                     and a.numel() == bo.BS_SIZE)
        reg = state[base:base + 64].view(8, 8)
        keep = reg.clone()
        reg.copy_(transform(state))
        try:
            return op(*args)
        finally:
            reg.copy_(keep)
    return wrapped


def test_mutant_xi_transposed():
    mut = _ops(block_update=_with_region(
        bo.BS_XI, lambda st: st[bo.BS_XI:bo.BS_XI + 64].view(8, 8).T.clone(),
        torch_ref.block_update))
    hits = [_rejected(lambda: _check_update_ref(
        65, k, k, *bo.run_update(mut, 65, k, k, CPU))) for k in bo.KS]
    assert all(hits)


def test_mutant_zeta_transpose_for_inverse():
    mut = _ops(block_ortho=_with_region(
        bo.BS_ZINV, lambda st: st[bo.BS_ZETA:bo.BS_ZETA + 64].view(8, 8).T.clone(),
        torch_ref.block_ortho))
    hits = [_rejected(lambda: bo.check_ortho(
        65, k, k, *bo.run_ortho(mut, 65, k, k, CPU), "mutant")) for k in bo.KS]
    assert all(hits)


def test_mutant_mirror_from_the_wrong_side(monkeypatch):
    def sym_lower(partials, nblocks, k, kg):
        """Mirrors the triangle nobody summed into (still the identity it
        was initialised to) over the one that holds the sums."""
        good = real(partials, nblocks, k, kg)
        return torch.diag(torch.diag(good))

    real = torch_ref._block_sym
    monkeypatch.setattr(torch_ref, "_block_sym", sym_lower)
    P8 = bo.gram_partials("spd", 5)
    for check, run in ((bo.check_coef_alpha, bo.run_coef_alpha),
                       (bo.check_coef_beta, bo.run_coef_beta)):
        hits = [_rejected(lambda: check(P8, k, k, run(torch_ref, P8, k, k, CPU),
                                        "mutant")) for k in bo.KS]
        assert all(hits)


def test_mutant_c_times_zeta(monkeypatch):
    monkeypatch.setattr(torch_ref, "_block_newc", lambda zeta, C: C @ zeta)
    P8 = bo.gram_partials("spd", 5)
    hits = [_rejected(lambda: bo.check_coef_beta(
        P8, k, k, bo.run_coef_beta(torch_ref, P8, k, k, CPU), "mutant"))
        for k in bo.KS]
    assert all(hits)


def test_mutant_absolute_pivot_test(monkeypatch):
    def chol_abs(g, kg):
        """torch_ref._block_chol with d_j <= tau instead of d_j <= tau g_jj."""
        k = g.shape[0]
        l = [[1.0 if i == j else 0.0 for j in range(k)] for i in range(k)]
        for j in range(kg):
            d = float(g[j, j]) - sum(l[j][q] ** 2 for q in range(j))
            if not math.isfinite(d) or not d > torch_ref.BLOCK_TAU:
                return None
            l[j][j] = math.sqrt(d)
            for i in range(j + 1, kg):
                l[i][j] = (float(g[i, j]) - sum(l[i][q] * l[j][q]
                                                for q in range(j))) / l[j][j]
        return torch.tensor(l, dtype=torch.float64)

    monkeypatch.setattr(torch_ref, "_block_chol", chol_abs)
    P8 = bo.gram_partials("spd", 5, 2.0 ** -16)
    hits = [_rejected(lambda: bo.check_coef_beta(
        P8, k, k, bo.run_coef_beta(torch_ref, P8, k, k, CPU), "mutant"))
        for k in bo.KS]
    assert all(hits)
    # and it misses a real breakdown of large columns: sine^2 = 1e-8 < tau
    # while the pivot itself, 1e-8 * 2^40 * |v|^2, is far above tau
    V = bo.mo.columns(64, 4242, 2) * 2.0 ** 20
    V[:, 1] = V[:, 0] + 1e-4 * V[:, 1]
    G = V.T @ V
    P8 = np.zeros((len(bo.pairs(bo.KMAX)), 1))
    P8[[0, 1, 8], 0] = G[0, 0], G[0, 1], G[1, 1]
    ex = bo.run_coef_beta(torch_ref, P8, 2, 2, CPU, it=3)
    assert ex["state"][bo.BS_FLAG] == 0.0  # the mutant lets it through
    monkeypatch.undo()
    bo.check_breakdown(bo.run_coef_beta(torch_ref, P8, 2, 2, CPU, it=3), 2, 3,
                       "G", beta=True)


def test_mutant_update_ignores_the_flag():
    def update_anyway(X, S, Q, T, state, partials, n):
        keep = state[bo.BS_FLAG].clone()
        state[bo.BS_FLAG] = 0.0
        try:
            return torch_ref.block_update(X, S, Q, T, state, partials, n)
        finally:
            state[bo.BS_FLAG] = keep

    mut = _ops(block_update=update_anyway)
    hits = [_rejected(lambda: bo.check_frozen_rows(
        bo.run_update(mut, 65, k, k, CPU, flag=True)[1])) for k in bo.KS]
    assert all(hits)


# ---------------------------------------------------------------------------
# CGSolverCPU.solve_block

SYSTEMS = ["sell7", "bsell3"]


def _solver(name):
    from acg_amd.solvers.cpu import CGSolverCPU

    S, B = bo.solver_system(name)
    return S, B, CGSolverCPU(S)


def _solve_block(solver, S, Bk, x0=None, **kw):
    X = torch.zeros(S.nowned, Bk.shape[1], dtype=torch.float64)
    if x0 is not None:
        X[:] = torch.from_numpy(x0)
    kw = {"maxits": bo.MAXITS, "res_rtol": bo.RTOL, **kw}
    res = solver.solve_block(torch.from_numpy(np.array(Bk, order="C")), X, **kw)
    return X.numpy(), res


def _scipy_apply(S, X):
    import scipy.sparse as sp

    A = sp.csr_matrix((S.A_vals, S.A_colidx, S.A_rowptr),
                      shape=(S.nowned, S.nowned))
    return A @ X


def _agrees_with_single(S, Bk, X, solver):
    for c in range(Bk.shape[1]):
        x = torch.zeros(S.nowned, dtype=torch.float64)
        r = solver.solve(torch.from_numpy(Bk[:, c].copy()), x, maxits=bo.MAXITS,
                         res_rtol=bo.RTOL)
        assert r.converged
        torch.testing.assert_close(torch.from_numpy(X[:, c].copy()), x,
                                   rtol=1e-6, atol=1e-8)


@pytest.mark.parametrize("k", [2, 3, 5, 8])
@pytest.mark.parametrize("name", SYSTEMS)
def test_cpu_solve_block(name, k):
    S, B = bo.solver_system(name)
    X, res = bo.cpu_block_solves(name, k)
    X1, its1 = bo.cpu_single_solves(name)
    assert len(res) == k
    for c in range(k):
        assert res[c].converged and res[c].block_breakdown == -1
        assert res[c].solver == "cg-block"
        assert res[c].bnrm2 == pytest.approx(np.linalg.norm(B[:, c]), rel=1e-12)
    torch.testing.assert_close(torch.from_numpy(X), torch.from_numpy(X1[:, :k].copy()),
                               rtol=1e-6, atol=1e-8)
    bo.check_true_residual(S, B[:, :k], X, f"cpu {name} k{k}")
    # the same criterion with scipy's CSR product, an independent A x
    bo.check_true_residual(S, B[:, :k], X, f"cpu {name} k{k} scipy",
                           AX=_scipy_apply(S, X))
    nit = max(r.niterations for r in res)
    print(f"BLOCK_CG cpu {name} k{k}: block its {nit}, single max {max(its1[:k])}")
    assert nit <= max(its1[:k])


def test_cpu_block_counts_match_triage():
    """Iteration counts are arithmetic: the prototype's table holds up to
    the one iteration a different summation order can move."""
    want = {"sell7": ({2: 51, 3: 51, 5: 48, 8: 43}, 57),
            "bsell3": ({2: 20, 3: 19, 5: 17, 8: 16}, 22)}
    for name, (blk, single) in want.items():
        assert max(bo.cpu_single_solves(name)[1]) == single
        for k, w in blk.items():
            got = max(r.niterations for r in bo.cpu_block_solves(name, k)[1])
            assert abs(got - w) <= 1, (name, k, got, w)


@pytest.mark.parametrize("name", SYSTEMS)
def test_cpu_group_splitting(name):
    S, B, solver = _solver(name)
    B11 = np.column_stack([B, B[:, 1] + B[:, 2], B[:, 3] - B[:, 4], B[:, 5] + 1.0])
    for group, sizes in ((8, [8, 3]), (4, [4, 4, 3])):
        solver.multi_group = group
        calls = []
        real = solver._solve_block_group
        solver._solve_block_group = lambda Bg, Xg, *a: (calls.append(Bg.shape[1]),
                                                        real(Bg, Xg, *a))[1]
        X, res = _solve_block(solver, S, B11)
        assert calls == sizes and len(res) == 11
        assert all(r.converged and r.block_breakdown == -1 for r in res)
        bo.check_true_residual(S, B11, X, f"cpu {name} group{group}")
        del solver._solve_block_group
    solver.multi_group = 3
    with pytest.raises(ValueError):
        _solve_block(solver, S, B11)


@pytest.mark.parametrize("name", SYSTEMS)
def test_cpu_zero_column_and_x0(name):
    S, B, solver = _solver(name)
    Bz = np.column_stack([B[:, 1], np.zeros(S.nowned), B[:, 2]])
    X, res = _solve_block(solver, S, Bz)
    assert res[1].converged and res[1].niterations == 0 and res[1].bnrm2 == 0.0
    assert not X[:, 1].any()
    assert res[0].converged and res[2].converged
    bo.check_true_residual(S, Bz[:, [0, 2]], X[:, [0, 2]], f"cpu {name} zero")
    # x0 = the solution: 0 iterations, X keeps its bits
    X2, res2 = _solve_block(solver, S, Bz, x0=X, res_rtol=1e-8)
    assert all(r.converged and r.niterations == 0 for r in res2)
    assert np.array_equal(X2, X)
    with pytest.raises(ValueError):
        solver.solve_block(torch.from_numpy(Bz.copy()),
                           torch.zeros(S.nowned, 2, dtype=torch.float64))


@pytest.mark.parametrize("name", SYSTEMS)
def test_cpu_handover_at_initialisation(name):
    S, B, solver = _solver(name)
    Bd = bo.special_rhs(name, "dependent")
    X, res = _solve_block(solver, S, Bd)
    assert all(r.converged and r.block_breakdown == 0 for r in res)
    assert all(r.solver == "cg-block" for r in res)
    bo.check_true_residual(S, Bd, X, f"cpu {name} dependent")
    _agrees_with_single(S, Bd, X, solver)


@pytest.mark.parametrize("name", SYSTEMS)
def test_cpu_near_dependence_both_sides_of_tau(name):
    S, B, solver = _solver(name)
    for eps, want in ((1e-2, -1), (1e-4, 0)):
        Bn = bo.special_rhs(name, "near", eps)
        v, w = B[:, 1], B[:, 2]
        wperp = w - v * (v @ w) / (v @ v)
        sin2 = eps ** 2 * (wperp @ wperp) / (Bn[:, 1] @ Bn[:, 1])
        assert (sin2 > 50 * bo.TAU) if want < 0 else (sin2 < bo.TAU / 50), sin2
        X, res = _solve_block(solver, S, Bn)
        assert all(r.converged and r.block_breakdown == want for r in res), \
            [(r.converged, r.block_breakdown) for r in res]
        bo.check_true_residual(S, Bn, X, f"cpu {name} eps{eps}")
        _agrees_with_single(S, Bn, X, solver)


@pytest.mark.parametrize("name", SYSTEMS)
def test_cpu_handover_in_the_first_iteration(name):
    S, B, solver = _solver(name)
    Be = bo.special_rhs(name, "exact")
    # one block iteration only: column 1 is already solved at the hand-over
    X1, res1 = _solve_block(solver, S, Be, maxits=1)
    assert all(r.block_breakdown == 1 for r in res1)
    r1 = np.linalg.norm(Be[:, 1] - bo.csr_apply(S, X1)[:, 1]) / np.linalg.norm(Be[:, 1])
    print(f"BLOCK_CG cpu {name} exact column: rel res at hand-over {r1:.3e}")
    assert r1 <= bo.RTOL
    X, res = _solve_block(solver, S, Be)
    assert all(r.converged and r.block_breakdown == 1 for r in res)
    assert res[1].niterations == 1
    bo.check_true_residual(S, Be, X, f"cpu {name} exact")
    _agrees_with_single(S, Be, X, solver)


def test_cpu_k1_is_solve_multi():
    S, B, solver = _solver("sell7")
    X, res = _solve_block(solver, S, B[:, 1:2])
    Xm = torch.zeros(S.nowned, 1, dtype=torch.float64)
    rm = solver.solve_multi(torch.from_numpy(B[:, 1:2].copy()), Xm,
                            maxits=bo.MAXITS, res_rtol=bo.RTOL)
    assert np.array_equal(X, Xm.numpy())
    assert res[0].solver == rm[0].solver == "cg-cpu"
    assert res[0].niterations == rm[0].niterations


def test_cpu_deterministic():
    S, B, solver = _solver("bsell3")
    Xa, ra = _solve_block(solver, S, B[:, :5])
    Xb, rb = _solve_block(solver, S, B[:, :5])
    assert np.array_equal(Xa, Xb)
    assert [r.niterations for r in ra] == [r.niterations for r in rb]


def test_nonfinite_rhs_raises():
    S, B, solver = _solver("sell7")
    Bn = B[:, :2].copy()
    Bn[3, 1] = np.inf
    with pytest.raises(FloatingPointError):
        _solve_block(solver, S, Bn)


# -- 2 ranks over gloo: the fall-back to solve_multi -------------------------

def _worker(rank, world, port, q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        os.environ["RANK"] = str(rank)
        os.environ["WORLD_SIZE"] = str(world)
        from acg_amd.dist.comm import Comm
        from acg_amd.gen import queen_like_spec, stencil_local_slab
        from acg_amd.solvers.cpu import CGSolverCPU

        comm = Comm("gloo")
        S = stencil_local_slab(5, 5, 8, queen_like_spec(3), comm.rank, comm.size)
        Bg = np.random.default_rng(42).standard_normal((S.n_global, 3))
        Bl = torch.from_numpy(Bg[S.owned_global])
        out = []
        for meth in ("solve_block", "solve_multi"):
            X = torch.zeros(S.nowned + S.nghost, 3, dtype=torch.float64)
            res = getattr(CGSolverCPU(S, comm=comm), meth)(
                Bl, X, maxits=500, res_rtol=1e-10)
            out.append((X[:S.nowned].numpy(), [r.solver for r in res],
                        [r.niterations for r in res],
                        [r.converged for r in res],
                        [r.block_breakdown for r in res]))
        q.put((rank, "ok", out))
        comm.finalize()
    except Exception:  # pragma: no cover
        import traceback

        q.put((rank, "err", traceback.format_exc()))
        raise


def test_two_ranks_fall_back_to_solve_multi():
    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    procs = [ctx.Process(target=_worker, args=(r, 2, 29671, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = {}
    for _ in range(2):
        rank, status, payload = q.get()
        assert status == "ok", f"rank {rank} failed:\n{payload}"
        results[rank] = payload
    for p in procs:
        p.join(timeout=60)
    for rank, (blk, multi) in results.items():
        assert np.array_equal(blk[0], multi[0])
        assert blk[1:] == multi[1:]
        assert blk[1] == ["cg-cpu"] * 3 and all(blk[3]) and blk[4] == [-1] * 3
