"""CPU side of the multiple-right-hand-side kernel tests (multirhs_oracle.py).

* every torch_ref multi op against the single-vector oracle expectation of
  each of its columns, at the GPU tests' shapes;
* a discrimination self-check in the style of test_kernel_oracle_cpu.py:
  for the exact inputs of the GPU tests, results of deliberately wrong
  kernels are built in fp64 and must be REJECTED on every column where the
  defect can show;
* CGSolverCPU.solve_multi.
"""

import numpy as np
import pytest
import torch

import kernel_oracle as ko
import multirhs_oracle as mo
from acg_amd.ops import torch_ref

CPU = torch.device("cpu")
SELL_CASES = [(3, False), (37, False), (5, True)]
BSELL_NODES = (1, 65, 130)
VEC_N = (1, 257, 300_001)


def _accept_all(expect_of, gots, tag):
    for c, got in enumerate(gots):
        ko.assert_accepts(expect_of(c), got, f"{tag} col{c}")


# ---------------------------------------------------------------------------
# torch_ref vs oracle

@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("nslices,short", SELL_CASES)
@pytest.mark.parametrize("k", mo.KS)
def test_ref_spmm_sell(k, nslices, short, fused):
    for col64 in (False, True):
        gots, ex = mo.run_spmm_sell(torch_ref, nslices, short, k, CPU,
                                    col64=col64, fused=fused)
        _accept_all(lambda c: mo.sell_expect(nslices, short, c, mo.slab(k)[c], fused),
                    gots, f"K{k} ns{nslices} short{short} col64={col64} fused{fused}")
        mo.check_untouched(ex, k, on_gpu=False)


@pytest.mark.parametrize("k", mo.KS)
def test_ref_spmm_sell_sigma(k):
    gots, ex = mo.run_spmm_sell(torch_ref, 3, False, k, CPU, sigma=4)
    _accept_all(lambda c: mo.sell_expect(3, False, c, mo.slab(k)[c], True, sigma=4),
                gots, f"K{k} sigma4")
    mo.check_untouched(ex, k, on_gpu=False)


@pytest.mark.parametrize("ghost", [False, True])
@pytest.mark.parametrize("nnodes", BSELL_NODES)
@pytest.mark.parametrize("dof", (2, 3, 4))
def test_ref_spmm_bsell(dof, nnodes, ghost):
    for k in mo.KS:
        for fused in (False, True):
            gots, ex = mo.run_spmm_bsell(torch_ref, dof, nnodes, ghost, None, k,
                                         CPU, fused=fused)
            _accept_all(lambda c: mo.bsell_expect(dof, nnodes, ghost, None, c,
                                                  mo.slab(k)[c], fused),
                        gots, f"dof{dof} n{nnodes} ghost{ghost} K{k} fused{fused}")
            mo.check_untouched(ex, k, on_gpu=False)


def test_ref_spmm_bsell_empty_slice():
    gots, ex = mo.run_spmm_bsell(torch_ref, 3, 130, True, 1, 4, CPU)
    _accept_all(lambda c: mo.bsell_expect(3, 130, True, 1, c, mo.slab(4)[c], True),
                gots, "empty slice")
    mo.check_untouched(ex, 4, on_gpu=False)


@pytest.mark.parametrize("n", VEC_N)
@pytest.mark.parametrize("k", mo.KS)
def test_ref_vector_ops_multi(k, n):
    mc = mo.vec_multi_case(n)
    scal0 = mo.slab(k, rr=True, pt_zero_col=k - 1)
    gots, ex = mo.run_cg_update(torch_ref, mc, k, CPU, scal0)
    _accept_all(lambda c: mo.cg_update_expect(mc, c, scal0[c]), gots, f"upd K{k} n{n}")
    mo.check_rr_out(ex, k)
    # S_PT = 0: alpha = 0 leaves r and x bitwise alone
    assert np.array_equal(ex["R"][:, k - 1], mc.r[:, k - 1])
    assert np.array_equal(ex["X"][:, k - 1], mc.x[:, k - 1])
    n_act = n - 3 if n > 3 else n
    gots, _ = mo.run_daypx(torch_ref, mc, k, CPU, scal0, n_act)
    _accept_all(lambda c: mo.daypx_expect(mc, c, scal0[c], n_act), gots,
                f"daypx K{k} n{n}")
    for acc in (False, True):
        s0 = mo.slab(k)
        s0[:, ko.S_PT] = ko.SENTINELS[ko.S_PT]
        gots, _ = mo.run_dot(torch_ref, mc, k, CPU, s0, ko.S_PT, acc)
        _accept_all(lambda c: mo.dot_expect(mc, c, s0[c], ko.S_PT, acc), gots,
                    f"dot K{k} n{n} acc{acc}")


@pytest.mark.parametrize("nb", [1, 255, 257, 4096])
def test_ref_reduce_partials_multi(nb):
    for k in mo.KS:
        pvals = mo.columns(nb, 14000 + nb, k).T.copy()
        for acc in (False, True):
            s0 = mo.slab(k)
            gots, _ = mo.run_reduce(torch_ref, pvals, k, CPU, s0, ko.S_GAMMA, acc)
            _accept_all(lambda c: mo.reduce_expect(pvals[c], s0[c], ko.S_GAMMA, acc),
                        gots, f"reduce K{k} nb{nb} acc{acc}")


def test_wrappers_validate():
    X = torch.zeros(10, 4, dtype=torch.float64)
    s, p = torch_ref.alloc_scalars_multi(CPU, 4), torch_ref.alloc_partials_multi(CPU, 4)
    assert s.shape == (4, torch_ref.S_NSLOTS) and p.shape == (4, torch_ref.MAXG)
    with pytest.raises(ValueError):
        torch_ref.dot_multi(X[:, :3].contiguous(), X[:, :3].contiguous(), p, s, 0)
    with pytest.raises(ValueError):
        torch_ref.dot_multi(X[:, ::2], X[:, ::2], p, s, 0)  # not contiguous
    with pytest.raises(TypeError):
        torch_ref.dot_multi(X.float(), X.float(), p, s, 0)
    with pytest.raises(ValueError):
        torch_ref.dot_multi(X, X, p, s, 0, n=11)
    assert torch_ref.spmm_bsell_supported(3, 8)
    assert not torch_ref.spmm_bsell_supported(5, 4)
    assert not torch_ref.spmm_bsell_supported(3, 3)


# ---------------------------------------------------------------------------
# discrimination: wrong kernels the acceptance helper must reject

def _sell_rows_mv(case, xof):
    """y[row] = sum_j a_j * xof(col_j), plain fp64."""
    prod = case.vals * xof(case.cols)
    y = np.zeros(case.nrows)
    np.add.at(y, ko.csr_rows(case.rowptr), prod)
    return y


def _emulate_spmm_sell(case, X, k, scal0, mutant=None):
    """fp64 emulation of k_spmm_sell + k_reduce_partials_multi with one
    defect switched on.  Partials a defect reads without having written
    them hold zeros -- the most forgiving garbage there is."""
    Xk = np.ascontiguousarray(X[:, :k])
    flat = Xk.reshape(-1)
    nb = ko.sell_blocks(case.nslices)
    part = np.zeros(mo.KMAX * mo.MAXG + mo.KMAX * nb)
    scal = scal0.copy()
    gots = []
    for c in range(k):
        if mutant == "next_column":
            y = _sell_rows_mv(case, lambda ci: Xk[ci, (c + 1) % k])
        elif mutant == "unscaled_index":
            y = _sell_rows_mv(case, lambda ci: flat[ci + c])
        else:
            y = _sell_rows_mv(case, lambda ci: Xk[ci, c])
        rows = np.arange(case.nrows)
        for b in range(nb):
            sl = rows[b * 256:(b + 1) * 256]
            base = c * nb if mutant == "partials_griddim" else c * mo.MAXG
            part[base + b] = float(Xk[sl, c] @ y[sl])
        gots.append({"y": y})
    for c in range(k):
        scal[c, ko.S_PT] = part[c * mo.MAXG:c * mo.MAXG + nb].sum()
        mo._scal_got(gots[c], scal[c])
    return gots


@pytest.mark.parametrize("nslices,short", SELL_CASES)
@pytest.mark.parametrize("k", mo.KS)
def test_mutants_spmm_sell(k, nslices, short):
    case, X = mo.sell_multi_case(nslices, short)
    s0 = mo.slab(k)
    es = [mo.sell_expect(nslices, short, c, s0[c], True) for c in range(k)]
    good = _emulate_spmm_sell(case, X, k, s0)
    assert all(ko.accepts(e, g) for e, g in zip(es, good)), "emulator itself is off"
    for m in ("next_column", "unscaled_index"):
        bad = _emulate_spmm_sell(case, X, k, s0, m)
        for c in range(k):
            assert not ko.accepts(es[c], bad[c]), (m, c)
    bad = _emulate_spmm_sell(case, X, k, s0, "partials_griddim")
    assert ko.accepts(es[0], bad[0])  # column 0's range is the same
    for c in range(1, k):
        assert not ko.accepts(es[c], bad[c]), ("partials_griddim", c)


def _transpose_blocks(dense, dof):
    nn, ncn = dense.shape[0] // dof, dense.shape[1] // dof
    return (dense.reshape(nn, dof, ncn, dof).transpose(0, 3, 2, 1)
            .reshape(nn * dof, ncn * dof))


@pytest.mark.parametrize("ghost", [False, True])
@pytest.mark.parametrize("nnodes", BSELL_NODES)
@pytest.mark.parametrize("dof", (2, 3, 4))
def test_mutants_spmm_bsell(dof, nnodes, ghost):
    """Block applied transposed; column c gathering column c+1."""
    case, X = mo.bsell_multi_case(dof, nnodes, ghost)
    dense = ko.csr_dense(case.rowptr, case.cols, case.vals, case.ncols)
    dense_t = _transpose_blocks(dense, dof)
    for k in mo.KS:
        s0 = mo.slab(k)
        gots, _ = mo.run_spmm_bsell(torch_ref, dof, nnodes, ghost, None, k, CPU,
                                    fused=False)
        for c in range(k):
            e = mo.bsell_expect(dof, nnodes, ghost, None, c, s0[c], False)
            assert ko.accepts(e, gots[c])
            assert ko.accepts(e, dict(gots[c], y=dense @ X[:, c]))
            assert not ko.accepts(e, dict(gots[c], y=dense_t @ X[:, c])), ("transposed", c)
            assert not ko.accepts(e, dict(gots[c], y=dense @ X[:, (c + 1) % k])), \
                ("next_column", c)


def _emulate_update(mc, k, scal0, mutant=None):
    """fp64 emulation of k_cg_fused_update_multi + k_cg_finalize_multi."""
    scal = scal0.copy()
    alpha = np.array([torch_ref._sdiv(scal[c, ko.S_RR], scal[c, ko.S_PT])
                      for c in range(k)])
    if mutant == "alpha_swapped":
        alpha[[0, 1]] = alpha[[1, 0]]
    gots, sums = [], []
    for c in range(k):
        r = mc.r[:, c] - alpha[c] * mc.t[:, c]
        x = mc.x[:, c] + alpha[c] * mc.p[:, c]
        gots.append({"r": r, "x": x})
        sums.append(float(r @ r))
    for c in range(k):
        sc = scal[0] if mutant == "finalize_col0" else scal[c]
        sc[ko.S_RR_PREV] = sc[ko.S_RR]
        sc[ko.S_RR] = sums[c]
    for c in range(k):
        mo._scal_got(gots[c], scal[c])
    return gots


@pytest.mark.parametrize("n", VEC_N)
@pytest.mark.parametrize("k", mo.KS)
def test_mutants_update_finalize(k, n):
    mc = mo.vec_multi_case(n)
    s0 = mo.slab(k, rr=True, pt_zero_col=k - 1)
    es = [mo.cg_update_expect(mc, c, s0[c]) for c in range(k)]
    good = _emulate_update(mc, k, s0)
    assert all(ko.accepts(e, g) for e, g in zip(es, good)), "emulator itself is off"
    bad = _emulate_update(mc, k, s0, "alpha_swapped")
    for c in (0, 1):
        assert not ko.accepts(es[c], bad[c]), ("alpha_swapped", c)
    bad = _emulate_update(mc, k, s0, "finalize_col0")
    for c in range(1, k):
        assert not ko.accepts(es[c], bad[c]), ("finalize_col0", c)


# ---------------------------------------------------------------------------
# CPU solver

def test_cpu_solve_multi_is_the_loop_over_solve():
    from acg_amd.gen import STENCIL_7PT_3D, stencil_local_slab
    from acg_amd.solvers.cpu import CGSolverCPU

    S = stencil_local_slab(6, 6, 6, dict(STENCIL_7PT_3D), 0, 1)
    solver = CGSolverCPU(S)
    rng = np.random.default_rng(5)
    n = S.nowned
    B = torch.from_numpy(rng.standard_normal((n, 3)))
    B[:, 1] = 0.0
    X = torch.zeros(n + S.nghost, 3, dtype=torch.float64)
    res = solver.solve_multi(B, X, maxits=200, res_rtol=1e-10)
    assert len(res) == 3
    for c in range(3):
        x1 = torch.zeros(n + S.nghost, dtype=torch.float64)
        r1 = solver.solve(B[:, c].contiguous(), x1, maxits=200, res_rtol=1e-10)
        assert torch.equal(X[:, c], x1)
        assert res[c].niterations == r1.niterations
        assert res[c].converged
    assert res[1].niterations == 0 and not X[:, 1].any()
    with pytest.raises(ValueError):
        solver.solve_multi(B, X[:, :2].contiguous(), maxits=5)
