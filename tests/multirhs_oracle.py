"""Oracle helpers for the multiple-right-hand-side kernels.

Plain helper module (not a conftest), built on tests/kernel_oracle.py.

Expectation rule: column c of any multi kernel must satisfy the EXISTING
single-vector expectation (``ko.sell_spmv_expect``, ``ko.bsell_spmv_expect``,
``ko.cg_update_expect``, ``ko.dot_expect``, ``ko.ratio_update_expect``) built
from column c of the inputs -- the derived bound (L + 48) * 2^-53 * M, no new
constant.  On top of that, everything a kernel must not touch is compared
bitwise: the other slots of every column's slab, the partials beyond the
block count and in other columns' ranges, the ghost rows of Y.

Inputs: the columns of a multivector are ``ko.rand_values`` drawn from
different seeds (pairwise distinct, checked); the column scalars rr, pt,
rr_prev differ per column and so do the sentinels of the untouched slots.
The same ``run_*`` drivers serve the CPU tests (torch_ref, mutants) and the
GPU tests (gpu_ops).
"""

from __future__ import annotations

import copy
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

import kernel_oracle as ko

KS = (2, 4, 8)
KMAX = 8
MAXG = ko.MAXG
NS = ko.S_NSLOTS
GHOST_ROWS = 5  # extra NaN rows behind Y that no kernel may write
_NANBITS = np.array([np.nan]).view(np.int64)[0]


def multi_blocks(n, k):
    """Grid of the element-wise multi kernels: one 16-byte pair per thread
    per stride (n*k/2 pairs), capped at 4096 blocks."""
    return max(1, min(4096, (n * k // 2 + 255) // 256))


def columns(n, seed, k=KMAX):
    """(n, k) array whose columns are rand_values from different seeds;
    column c is the same for every k (prefix property)."""
    X = np.empty((n, k))
    for c in range(k):
        X[:, c] = ko.rand_values(n, np.random.default_rng(seed + 7919 * (c + 1)))
    for c in range(k):
        for d in range(c):
            assert not np.any(X[:, c] == X[:, d]), "columns must differ everywhere"
    return X


def slab(k, rr=False, pt_zero_col=None):
    """(k, 8) slab: column c holds SENTINELS + 1000*c (exact, distinct per
    column); ``rr`` fills distinct S_RR / S_PT / S_RR_PREV per column, with
    S_PT = 0 in ``pt_zero_col``."""
    s = np.stack([ko.SENTINELS + 1000.0 * c for c in range(k)])
    if rr:
        for c in range(k):
            s[c, ko.S_RR] = 1.3719 + 0.37 * c
            s[c, ko.S_PT] = 2.9131 + 0.53 * c
            s[c, ko.S_RR_PREV] = 0.7717 + 0.29 * c
        if pt_zero_col is not None:
            s[pt_zero_col, ko.S_PT] = 0.0
    return s


def _col(case, **repl):
    c = copy.copy(case)
    for k, v in repl.items():
        setattr(c, k, v)
    return c


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def all_nan_bits(a):
    return bool(np.all(_bits(a) == _NANBITS))


def _scal_got(got, slab_row):
    for i in range(NS):
        got[f"scal{i}"] = slab_row[i:i + 1].copy()
    return got


# ---------------------------------------------------------------------------
# cases (cached: references are computed once and shared)

@lru_cache(maxsize=None)
def sell_multi_case(nslices, short=False):
    case = ko.sell_case(nslices, short=short)
    X = columns(case.ncols, 11000 + nslices + (500 if short else 0))
    return case, X


@lru_cache(maxsize=None)
def bsell_multi_case(dof, nnodes, ghost, empty_slice=None):
    case = ko.bsell_case(dof, nnodes, ghost, empty_slice=empty_slice)
    X = columns(case.ncols, 12000 + 100 * dof + nnodes + (7 if ghost else 0))
    return case, X


@lru_cache(maxsize=None)
def vec_multi_case(n):
    """r, x, p, t, w multivectors of n rows (8 columns)."""
    return SimpleNamespace(n=n, **{nm: columns(n, 13000 + 1000 * i + n)
                                   for i, nm in enumerate("rxptw")})


# ---------------------------------------------------------------------------
# expectations, one per column

@lru_cache(maxsize=None)
def _sell_expect_cached(nslices, short, c, sigma):
    case, X = sell_multi_case(nslices, short)
    perm = None
    if sigma > 1:
        from acg_amd.ops import torch_ref

        perm = torch_ref.sell_from_csr(case.rowptr, case.cols.astype(np.int32),
                                       case.vals, sigma=sigma)[3]
    return ko.sell_spmv_expect(_col(case, x=X[:, c]), perm=perm,
                               dotslot=ko.S_PT, dot_accum=False)


def sell_expect(nslices, short, c, slab_row, fused, sigma=1):
    e = copy.deepcopy(_sell_expect_cached(nslices, short, c, sigma))
    e.kernel = "k_spmm_sell"
    if not fused:
        del e.close[f"scal{ko.S_PT}"]
    e.scalars(slab_row, touched=(ko.S_PT,) if fused else ())
    return e


@lru_cache(maxsize=None)
def _bsell_expect_cached(dof, nnodes, ghost, empty_slice, c, fused):
    case, X = bsell_multi_case(dof, nnodes, ghost, empty_slice)
    return ko.bsell_spmv_expect(_col(case, x=X[:, c]),
                                dotslot=ko.S_PT if fused else -1)


def bsell_expect(dof, nnodes, ghost, empty_slice, c, slab_row, fused):
    e = copy.deepcopy(_bsell_expect_cached(dof, nnodes, ghost, empty_slice, c, fused))
    e.kernel = "k_spmm_bsell"
    e.scalars(slab_row, touched=(ko.S_PT,) if fused else ())
    return e


def _vec_col(mc, c, scal_row):
    return SimpleNamespace(n=mc.n, scal=scal_row.copy(),
                           **{nm: getattr(mc, nm)[:, c] for nm in "rxptw"})


def cg_update_expect(mc, c, scal_row):
    e = ko.cg_update_expect(_vec_col(mc, c, scal_row))
    e.kernel = "k_cg_fused_update_multi"
    return e


def daypx_expect(mc, c, scal_row, n_act):
    """ko.ratio_update_expect divides S_RR by S_PT; k_daypx_ratio_multi
    divides S_RR by S_RR_PREV, so the expectation is built from a slab with
    rr_prev in the S_PT slot and the untouched-slot check from the real one."""
    fake = scal_row.copy()
    fake[ko.S_PT] = scal_row[ko.S_RR_PREV]
    e = ko.ratio_update_expect(_vec_col(mc, c, fake), "daypx_ratio", n_act)
    e.kernel = "k_daypx_ratio_multi"
    e.scalars(scal_row)
    return e


def dot_expect(mc, c, scal_row, slot, accumulate):
    if accumulate:
        assert scal_row[slot] == ko.SENTINELS[slot]
    e = ko.dot_expect(_vec_col(mc, c, scal_row), slot, accumulate)
    e.kernel = "k_dot_multi"
    e.scalars(scal_row, touched=(slot,))
    return e


def reduce_expect(pvals, scal_row, slot, accumulate):
    """Sum of the first nblocks partials of one column: the dot bound with
    a vector of ones."""
    e = ko.Expect("k_reduce_partials_multi")
    d, tol = ko.dot(ko.hp(pvals), ko.hp(np.ones(len(pvals))),
                    add=scal_row[slot] if accumulate else None)
    e.add_tol(f"scal{slot}", d, tol)
    e.scalars(scal_row, touched=(slot,))
    return e


# ---------------------------------------------------------------------------
# runners: drive ``ops`` on NaN-poisoned buffers.  Each returns
# (per-column got dicts, extras); extras carry what is checked bitwise.

def _nan2(rows, k, dev):
    import torch

    return torch.full((rows, k), float("nan"), dtype=torch.float64, device=dev)


def check_untouched(extras, k, on_gpu):
    """Ghost rows of Y keep their NaN bits; on the GPU the partials beyond
    each column's block count (hence every other column's range) do too and
    the owned ones are finite."""
    if "y_tail" in extras:
        assert all_nan_bits(extras["y_tail"]), "ghost rows of Y written"
    if not on_gpu:
        return
    part, nb = extras["partials"].reshape(-1, MAXG), extras["nblocks"]
    assert part.shape[0] == KMAX
    for c in range(KMAX):
        lo = nb if c < k else 0
        assert all_nan_bits(part[c, lo:]), f"partials of column {c} beyond {lo} written"
        assert np.all(np.isfinite(part[c, :lo]))


def _finish_spmm(Y, nrows, k, scal, partials, nblocks):
    yy, ss = ko._np(Y), ko._np(scal)
    gots = [_scal_got({"y": yy[:nrows, c].copy()}, ss[c]) for c in range(k)]
    return gots, {"y_tail": yy[nrows:], "partials": ko._np(partials),
                  "nblocks": nblocks, "Y": yy, "scal": ss}


def run_spmm_sell(ops, nslices, short, k, dev, *, col64=False, sigma=1,
                  fused=True):
    from acg_amd.ops import torch_ref

    case, X = sell_multi_case(nslices, short)
    packed = torch_ref.sell_from_csr(
        case.rowptr, case.cols.astype(np.int64 if col64 else np.int32),
        case.vals, sigma=sigma)
    sp, sc, sv = packed[:3]
    kw = {"perm": ko._t(packed[3], dev)} if len(packed) == 4 else {}
    Y = _nan2(case.nrows + GHOST_ROWS, k, dev)
    scal = ko._t(slab(k), dev)
    partials = _nan2(KMAX, MAXG, dev)
    if fused:
        kw.update(partials=partials, scal=scal, dotslot=ko.S_PT)
    ops.spmm_sell(ko._t(sp, dev), ko._t(sc, dev), ko._t(sv, dev), case.nrows,
                  ko._t(X[:, :k], dev), Y, **kw)
    return _finish_spmm(Y, case.nrows, k, scal, partials,
                        ko.sell_blocks(case.nslices) if fused else 0)


def run_spmm_bsell(ops, dof, nnodes, ghost, empty_slice, k, dev, *, fused=True):
    case, X = bsell_multi_case(dof, nnodes, ghost, empty_slice)
    bptr, bcol, bvals = ko.pack_bsell(case, dev)
    Y = _nan2(case.nrows + GHOST_ROWS, k, dev)
    scal = ko._t(slab(k), dev)
    partials = _nan2(KMAX, MAXG, dev)
    kw = dict(partials=partials, scal=scal, dotslot=ko.S_PT) if fused else {}
    ops.spmm_bsell(bptr, bcol, bvals, case.nnodes, dof, ko._t(X[:, :k], dev), Y, **kw)
    return _finish_spmm(Y, case.nrows, k, scal, partials,
                        ko.sell_blocks(bptr.numel() - 1) if fused else 0)


def run_cg_update(ops, mc, k, dev, scal0):
    """cg_fused_update_multi + cg_finalize_multi."""
    R, X = ko._t(mc.r[:, :k], dev), ko._t(mc.x[:, :k], dev)
    scal = ko._t(scal0, dev)
    partials = _nan2(KMAX, MAXG, dev)
    rr_out = ko._nan(KMAX, dev)
    nb = ops.cg_fused_update_multi(R, X, ko._t(mc.p[:, :k], dev),
                                   ko._t(mc.t[:, :k], dev), scal, partials, mc.n)
    ops.cg_finalize_multi(partials, nb, scal, rr_out)
    rr, xx, ss = ko._np(R), ko._np(X), ko._np(scal)
    gots = [_scal_got({"r": rr[:, c].copy(), "x": xx[:, c].copy()}, ss[c])
            for c in range(k)]
    return gots, {"partials": ko._np(partials), "nblocks": nb,
                  "rr_out": ko._np(rr_out), "scal": ss, "R": rr, "X": xx}


def check_rr_out(extras, k):
    """rr_out[c] is bitwise the published S_RR of column c; the rest of the
    buffer is untouched."""
    assert np.array_equal(_bits(extras["rr_out"][:k]),
                          _bits(extras["scal"][:k, ko.S_RR]))
    assert all_nan_bits(extras["rr_out"][k:])


def run_daypx(ops, mc, k, dev, scal0, n_act):
    P = ko._t(mc.r[:, :k], dev)
    scal = ko._t(scal0, dev)
    ops.daypx_ratio_multi(P, ko._t(mc.x[:, :k], dev), scal, n=n_act)
    pp, ss = ko._np(P), ko._np(scal)
    gots = [_scal_got({"y": pp[:n_act, c].copy(), "y_tail": pp[n_act:, c].copy()},
                      ss[c]) for c in range(k)]
    return gots, {"P": pp, "scal": ss}


def run_dot(ops, mc, k, dev, scal0, slot, accumulate):
    scal = ko._t(scal0, dev)
    partials = _nan2(KMAX, MAXG, dev)
    ops.dot_multi(ko._t(mc.r[:, :k], dev), ko._t(mc.w[:, :k], dev), partials,
                  scal, slot, accumulate=accumulate)
    ss = ko._np(scal)
    return ([_scal_got({}, ss[c]) for c in range(k)],
            {"partials": ko._np(partials), "nblocks": multi_blocks(mc.n, k), "scal": ss})


def run_reduce(ops, pvals, k, dev, scal0, slot, accumulate):
    """pvals: (k, nblocks) block sums placed at partials[c, :nblocks]."""
    nb = pvals.shape[1]
    part = np.full((KMAX, MAXG), np.nan)
    part[:k, :nb] = pvals
    scal = ko._t(scal0, dev)
    partials = ko._t(part, dev)
    ops.reduce_partials_multi(partials, nb, scal, slot, accumulate=accumulate)
    ss = ko._np(scal)
    assert np.array_equal(_bits(ko._np(partials)), _bits(part)), "partials modified"
    return [_scal_got({}, ss[c]) for c in range(k)], {"scal": ss}


# ---------------------------------------------------------------------------
# solver level: runs shorter than the host test's lag

SHORT_MAXITS = (0, 1, 2, 3)


@lru_cache(maxsize=None)
def short_run_system():
    """(S, B) for solves that stop at maxits <= 3, where the lag-2 host test
    reads everything in its tail drain: the 648-row 6x6x6 queen_like_spec(3)
    system (one rank: the SpMM fast path) and three default_rng(5) columns,
    a group that is padded to K = 4."""
    from acg_amd.gen import queen_like_spec, stencil_local_slab

    S = stencil_local_slab(6, 6, 6, queen_like_spec(3), 0, 1)
    assert S.nowned == 648 and S.nghost == 0
    B = np.random.default_rng(5).standard_normal((S.nowned, 3))
    B.setflags(write=False)
    return S, B


@lru_cache(maxsize=None)
def short_run_cpu(method, maxits):
    """CGSolverCPU.solve_multi / solve_block on short_run_system with
    res_rtol = 0, so that only maxits stops it: (X, results)."""
    import torch

    from acg_amd.solvers.cpu import CGSolverCPU

    S, B = short_run_system()
    X = torch.zeros(S.nowned, B.shape[1], dtype=torch.float64)
    res = getattr(CGSolverCPU(S), method)(torch.from_numpy(B.copy()), X,
                                          maxits=maxits, res_rtol=0.0)
    return X, res


def check_short_run(method, maxits, dev):
    """CGSolverHIP.<method> stopped by maxits <= 3 against the CPU oracle:
    every column reports exactly maxits iterations, unconverged, without a
    breakdown, and X agrees to the criterion of the longer solver tests."""
    import torch

    from acg_amd.solvers.hip import CGSolverHIP

    S, B = short_run_system()
    Xc, resc = short_run_cpu(method, maxits)
    assert all(r.niterations == maxits and not r.converged
               and r.block_breakdown == -1 for r in resc)
    solver = CGSolverHIP(S, device=dev)
    assert solver._multi_fast_path()
    X = torch.zeros(S.nowned, B.shape[1], dtype=torch.float64, device=dev)
    res = getattr(solver, method)(torch.from_numpy(B.copy()).to(dev), X,
                                  maxits=maxits, res_rtol=0.0)
    assert len(res) == B.shape[1]
    for c, r in enumerate(res):
        assert r.niterations == maxits, (c, r.summary())
        assert r.converged is False, (c, r.summary())
        assert r.block_breakdown == -1, (c, r.summary())
    torch.testing.assert_close(X.cpu(), Xc, rtol=1e-6, atol=1e-8)
