"""Oracle helpers for the dual SpMV and the residual replacement of the
pipelined CG (plain helper module, not a conftest).  Extends
``kernel_oracle``: the same cases, the same high-precision arithmetic and
``Expect`` / ``bound`` acceptance, for two gathered vectors at once.

Bounds.  ``y2 = A x2`` and ``y1 = A x1`` are the single-vector sums: L
products, bound ``(L + 48) u M``.  With RESID the subtraction ``b - A x1``
adds one rounding relative to ``|b| + M``: bound ``(L + 1 + 48) u (|b| + M)``.
A block's partial of (x1,x1) is a plain dot of exact inputs; its partial of
(y1,x1) carries the element bounds of y1 through ``kernel_oracle.dot``.
The kernels launch one 256-thread block per 4 slices, so block ``g`` owns
SELL rows ``[256 g, 256 g + 256)`` (matrix rows through ``perm``)."""

from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import kernel_oracle as ko

ROWS_PER_BLOCK = 4 * ko.C


def with_second_vector(case, seed):
    """The case plus a second gathered vector ``x2`` and a right-hand side
    ``b``, both distinct random values of magnitude [0.5, 2)."""
    rng = np.random.default_rng(7000 + seed)
    d = dict(vars(case))
    d["x2"] = ko.rand_values(case.ncols, rng)
    d["b"] = ko.rand_values(case.nrows, rng)
    return SimpleNamespace(**d)


def sell_case2(nslices, short=False):
    return with_second_vector(ko.sell_case(nslices, short), nslices + (50 if short else 0))


def bsell_case2(dof, nnodes, ghost):
    return with_second_vector(ko.bsell_case(dof, nnodes, ghost),
                              100 * dof + nnodes + (7 if ghost else 0))


def block_rows(nrows, nslices, rows_per_sell_row=1, perm=None):
    """List of matrix-row index arrays, one per launched block."""
    nsell = nslices * ko.C
    rowof = np.arange(nsell) if perm is None else np.asarray(perm, np.int64)
    out = []
    for g0 in range(0, nsell, ROWS_PER_BLOCK):
        r = rowof[g0:g0 + ROWS_PER_BLOCK]
        r = r[r < nrows // rows_per_sell_row]
        if rows_per_sell_row > 1:  # BSELL: node -> its dof scalar rows
            r = (r[:, None] * rows_per_sell_row
                 + np.arange(rows_per_sell_row)[None, :]).reshape(-1)
        out.append(r)
    return out


def spmv2_expect(case, L, blocks, resid, fuse, kernel, x2=None):
    """Expectation of one dual SpMV: ``L`` products per row, ``blocks`` from
    :func:`block_rows`."""
    e = ko.Expect(kernel)
    x1h = ko.hp(case.x)
    x2h = ko.hp(case.x2 if x2 is None else x2)
    a1, M1 = ko.spmv(case.rowptr, case.cols, case.vals, x1h)
    a2, M2 = ko.spmv(case.rowptr, case.cols, case.vals, x2h)
    if resid:
        bh = ko.hp(case.b)
        y1, My1, L1 = bh - a1, ko.habs(bh) + M1, L + 1
    else:
        y1, My1, L1 = a1, M1, L
    e.add("y1", y1, My1, L1)
    e.add("y2", a2, M2, L)
    if fuse:
        ty1 = ko.bound(My1, L1)
        pg, pgt, pd, pdt = [], [], [], []
        for rows in blocks:
            xr = x1h[rows]
            g, gt = ko.dot(xr, xr)
            d, dt = ko.dot(xr, y1[rows], tb=ty1[rows])
            pg.append(g), pgt.append(gt), pd.append(d), pdt.append(dt)
        e.add_tol("pg", np.array(pg), np.array(pgt))
        e.add_tol("pd", np.array(pd), np.array(pdt))
    return e


def sell_spmv2_expect(case, resid, fuse, perm=None, x2=None):
    return spmv2_expect(case, ko.sell_padded_len(case.rowptr, perm),
                        block_rows(case.nrows, case.nslices, perm=perm),
                        resid, fuse, "k_spmv2_sell", x2)


def bsell_spmv2_expect(case, resid, fuse, x2=None):
    nslices = (case.nnodes + ko.C - 1) // ko.C
    return spmv2_expect(case, ko.bsell_padded_len(case.rowptr, case.cols, case.dof),
                        block_rows(case.nrows, nslices, case.dof),
                        resid, fuse, "k_spmv2_bsell", x2)


def _collect(y1, y2, partials, nb, fuse):
    got = {"y1": ko._np(y1), "y2": ko._np(y2)}
    ko._partials_out(got, partials, nb if fuse else 0)
    if fuse:
        got["pg"] = got["partials"][:nb]
        got["pd"] = got["partials"][ko.MAXG:ko.MAXG + nb]
    return got


def run_sell_spmv2(ops, case, dev, *, resid, fuse, col64=False, sigma=1,
                   x2=None, vals=None):
    """Drive ``ops.spmv2_sell`` on NaN-prefilled outputs and partials."""
    from acg_amd.ops import torch_ref

    packed = torch_ref.sell_from_csr(
        case.rowptr, case.cols.astype(np.int64 if col64 else np.int32),
        case.vals if vals is None else vals, sigma=sigma)
    sp, sc, sv = packed[:3]
    if vals is not None:  # the packer always returns fp64: keep the dtype asked for
        sv = sv.astype(np.asarray(vals).dtype)
    perm = ko._t(packed[3], dev) if len(packed) == 4 else None
    y1, y2 = ko._nan(case.nrows, dev), ko._nan(case.nrows, dev)
    partials = ko._nan(2 * ko.MAXG, dev)
    nb = ops.spmv2_sell(ko._t(sp, dev), ko._t(sc, dev), ko._t(sv, dev),
                        case.nrows, ko._t(case.x, dev),
                        ko._t(case.x2 if x2 is None else x2, dev), y1, y2,
                        ncols=case.ncols,
                        b=ko._t(case.b, dev) if resid else None,
                        partials=partials if fuse else None, perm=perm)
    assert nb == ko.sell_blocks(case.nslices)
    got = _collect(y1, y2, partials, nb, fuse)
    got["perm"] = packed[3] if len(packed) == 4 else None
    return got


def run_bsell_spmv2(ops, case, dev, *, resid, fuse, x2=None, packed=None):
    bptr, bcol, bvals = packed if packed is not None else ko.pack_bsell(case, dev)
    y1, y2 = ko._nan(case.nrows, dev), ko._nan(case.nrows, dev)
    partials = ko._nan(2 * ko.MAXG, dev)
    nb = ops.spmv2_bsell(bptr, bcol, bvals, case.nnodes, case.dof,
                         ko._t(case.x, dev),
                         ko._t(case.x2 if x2 is None else x2, dev), y1, y2,
                         ncols=case.ncols,
                         b=ko._t(case.b, dev) if resid else None,
                         partials=partials if fuse else None)
    assert nb == ko.sell_blocks(bptr.numel() - 1)
    return _collect(y1, y2, partials, nb, fuse)


# ---------------------------------------------------------------------------
# dot2_slices: the same partials without a matrix

def dot2_slices_expect(n, r, w, blocks):
    e = ko.Expect("k_dot2_slices")
    rh, wh = ko.hp(r[:n]), ko.hp(w[:n])
    pg, pgt, pd, pdt = [], [], [], []
    for rows in blocks:
        g, gt = ko.dot(rh[rows], rh[rows])
        d, dt = ko.dot(wh[rows], rh[rows])
        pg.append(g), pgt.append(gt), pd.append(d), pdt.append(dt)
    e.add_tol("pg", np.array(pg), np.array(pgt))
    e.add_tol("pd", np.array(pd), np.array(pdt))
    return e


def run_dot2_slices(ops, r, w, nunits, dof, dev, perm=None):
    partials = ko._nan(2 * ko.MAXG, dev)
    nb = ops.dot2_slices(ko._t(r, dev), ko._t(w, dev), nunits, dof, partials,
                         perm=None if perm is None else ko._t(perm, dev))
    got = ko._partials_out({}, partials, nb)
    got["pg"] = got["partials"][:nb]
    got["pd"] = got["partials"][ko.MAXG:ko.MAXG + nb]
    return got


# ---------------------------------------------------------------------------
# pipelined_replace_finalize

def finalize_case(nblocks):
    rng = np.random.default_rng(9000 + nblocks)
    part = np.full(2 * ko.MAXG, np.nan)
    part[:nblocks] = ko.rand_values(nblocks, rng)
    part[ko.MAXG:ko.MAXG + nblocks] = ko.rand_values(nblocks, rng)
    return SimpleNamespace(nblocks=nblocks, partials=part)


def finalize_expect(case):
    """Sums of nblocks values: bound (nblocks + 48) u sum|p|; every other
    slab slot keeps its sentinel bits."""
    e = ko.Expect("k_pipelined_replace_finalize")
    nb = case.nblocks
    for slot, lo in ((ko.S_GAMMA, 0), (ko.S_DELTA, ko.MAXG)):
        ph = ko.hp(case.partials[lo:lo + nb])
        e.add(f"scal{slot}", ko.hsum(ph), ko.hsum(ko.habs(ph)), nb)
    e.scalars(ko.SENTINELS, touched=(ko.S_GAMMA, ko.S_DELTA))
    return e


def run_finalize(ops, case, dev):
    scal = ko._t(ko.SENTINELS, dev)
    ops.pipelined_replace_finalize(ko._t(case.partials, dev), case.nblocks, scal)
    return ko._scal_out({}, scal)
