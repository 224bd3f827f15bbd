"""Tensor-level wrappers around the gfx950 HIP kernels (_acg_kernels.so).

Reference analog: the BLAS/SpMV call layer of acg/cghip.c (hipsparse
SpMV setup :463-585, hipblas dot/axpy wrappers) -- here every hot op is
one of our own kernels (ops/kernels.hip cites the per-kernel analogs).

Raw pointers + the caller's current HIP stream are passed to the
extension; all type/shape checks happen here.  If the extension is
missing on a machine with a GPU, import fails loudly (no eager fallback).

Reductions are two-phase (per-block partials + finalize kernel): callers
pass a ``partials`` scratch tensor of size 2*MAXG allocated once via
:func:`alloc_partials`.
"""

from __future__ import annotations

import torch

try:
    from . import _acg_kernels as K
except ImportError as e:  # pragma: no cover
    raise ImportError(
        "acg_amd HIP kernel extension (_acg_kernels) is not built. "
        "Run `python -m acg_amd.ops.build` (hipcc --offload-arch=gfx950). "
        f"Original error: {e}"
    ) from e

# scalar-slab slot indices (shared with kernels.hip)
S_RR = K.S_RR
S_PT = K.S_PT
S_RR_PREV = K.S_RR_PREV
S_BNRM2 = K.S_BNRM2
S_GAMMA = K.S_GAMMA
S_DELTA = K.S_DELTA
S_GAMMA_PREV = K.S_GAMMA_PREV
S_ALPHA_PREV = K.S_ALPHA_PREV
S_NSLOTS = K.S_NSLOTS
MAXG = K.MAXG
K_ST_TILE = K.ST_TILE  # nodes per BSELL-ST tile = one workgroup of k_spmv_bsell_st


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def alloc_scalars(device) -> torch.Tensor:
    return torch.zeros(S_NSLOTS, dtype=torch.float64, device=device)


def alloc_partials(device) -> torch.Tensor:
    return torch.zeros(2 * MAXG, dtype=torch.float64, device=device)


def pick_lanes(mean_nnz_per_row: float) -> int:
    """Lanes-per-row heuristic for the CSR vector kernel (CDNA4: wave=64).

    MEASURED mapping (tools/lanes_sweep.py, fixed-length rows, 30M nnz):
    the optimum sits near 1-2 nnz/lane, NOT the round-1 ~6 rule-of-thumb
    (len-24 rows: 32 lanes 372 us vs 4 lanes 557; len-16: 16 lanes 432
    vs 4 lanes 588).  len<=8 -> 8, <=16 -> 16, <=96 -> 32, else 64."""
    if mean_nnz_per_row <= 4.0:
        return 4
    if mean_nnz_per_row <= 8.0:
        return 8
    if mean_nnz_per_row <= 16.0:
        return 16
    if mean_nnz_per_row <= 96.0:
        return 32
    return 64


def spmv(rowptr: torch.Tensor, colidx: torch.Tensor, vals: torch.Tensor,
         x: torch.Tensor, y: torch.Tensor, *, rowbase: int = 0,
         lanes: int = 16, accum: bool = False,
         partials: torch.Tensor | None = None,
         scal: torch.Tensor | None = None, dotslot: int = -1,
         dot_accum: bool = True) -> None:
    """CSR-vector SpMV: y[rowbase:+nrows] (=|+=) A x; optional fused
    dot(x,y) finalized into scal[dotslot]."""
    nrows = rowptr.numel() - 1
    if nrows <= 0:
        return
    fuse = scal is not None and dotslot >= 0
    K.spmv(nrows, rowbase, rowptr.data_ptr(), colidx.data_ptr(),
           1 if colidx.dtype == torch.int64 else 0,
           vals.data_ptr(), x.data_ptr(), y.data_ptr(), lanes, accum,
           partials.data_ptr() if fuse else 0,
           scal.data_ptr() if fuse else 0, dotslot, dot_accum, _stream())


def build_row_bins(rowptr, max_lanes: int = 64):
    """Sort rows into lane-count bins by length for the hybrid binned SpMV.

    Returns (rowlist int32 numpy, bins [(start, count, lanes)]).  Bin
    thresholds follow the pick_lanes rule (~6 nnz per lane); rows inside
    a bin are ordered longest-first so grid-stride waves retire the
    heavy tail early."""
    import numpy as np

    rowptr = np.asarray(rowptr)
    lens = np.diff(rowptr)
    order = np.argsort(-lens, kind="stable").astype(np.int32)
    slens = lens[order.astype(np.int64)]
    bins = []
    lo = 0
    # descending order: long rows first; thresholds from the high end
    # (measured mapping, see pick_lanes: >96 -> 64, >16 -> 32, >8 -> 16,
    # >4 -> 8, rest 4)
    for lanes, thresh in ((64, 96), (32, 16), (16, 8), (8, 4), (4, None)):
        if lanes > max_lanes:
            continue
        if thresh is None:
            hi = len(slens)
        else:
            hi = int(np.searchsorted(-slens, -thresh - 1, side="right"))
        if hi > lo:
            bins.append((lo, hi - lo, lanes))
            lo = hi
    return order, bins


def build_sellcsr_hybrid(rowptr, colidx, vals, cut: int = 192,
                         window: int = 0, bucket: int = 8):
    """Host prep for the SELL+CSR hybrid: short rows (len <= cut) as
    sigma-sorted SELL, long rows as a longest-first 64/32-lane binned CSR
    list.  Returns (sellptr, cols, svals, perm, rowlist_long, bins) numpy
    arrays (sellptr None when every row is long)."""
    import numpy as np

    from .torch_ref import sellcsr_split

    sellptr, cols, svals, perm, long_rows, nshort = sellcsr_split(
        rowptr, colidx, vals, cut=cut, window=window, bucket=bucket)
    lens = np.diff(np.asarray(rowptr))
    longlens = lens[long_rows.astype(np.int64)]  # descending
    bins = []
    lo = 0
    for lanes, thresh in ((64, 96), (32, 16), (16, 8), (8, 4), (4, None)):
        if thresh is None:
            hi = len(longlens)
        else:
            hi = int(np.searchsorted(-longlens, -thresh - 1, side="right"))
        if hi > lo:
            bins.append((lo, hi - lo, lanes))
            lo = hi
        if lo >= len(longlens):
            break
    if nshort == 0:
        sellptr = None
    return sellptr, cols, svals, perm, long_rows, bins


def spmv_binned(rowptr: torch.Tensor, colidx: torch.Tensor, vals: torch.Tensor,
                rowlist: torch.Tensor, bins, x: torch.Tensor, y: torch.Tensor,
                *, rowbase: int = 0, accum: bool = False,
                partials: torch.Tensor | None = None,
                scal: torch.Tensor | None = None, dotslot: int = -1,
                dot_accum: bool = True) -> None:
    """Row-binned hybrid CSR SpMV (load balance for power-law rows).
    ``rowlist`` int32 rows sorted longest-first; ``bins`` from
    :func:`build_row_bins`."""
    if rowlist.numel() == 0:
        return
    assert rowlist.dtype == torch.int32
    fuse = scal is not None and dotslot >= 0
    K.spmv_binned(rowbase, rowptr.data_ptr(), colidx.data_ptr(),
                  1 if colidx.dtype == torch.int64 else 0,
                  vals.data_ptr(), x.data_ptr(), y.data_ptr(),
                  rowlist.data_ptr(), [list(b) for b in bins], accum,
                  partials.data_ptr() if fuse else 0,
                  scal.data_ptr() if fuse else 0, dotslot, dot_accum,
                  _stream())


# SELL kernel variant bits (see kernels.hip): +1 non-temporal vals/cols,
# +2 XCD-aware block swizzle, +4 unroll-8.
SELL_NT, SELL_SWZ, SELL_U8 = K.SELL_NT, K.SELL_SWZ, K.SELL_U8
# A/B on MI355X (tools/spmv_bench.py, Queen-shaped 326M nnz): base 5.53,
# NT 5.66, NT+U8 5.78 TB/s (92% of the ~6.3 TB/s achievable); SWZ slightly
# negative (x is L3-resident, natural slice order already L2-local).
DEFAULT_SELL_VARIANT = SELL_NT | SELL_U8

# Storage types the SELL / BSELL operator values may have.  fp32 values
# keep the fp64 element order (``vals.to(torch.float32)`` is the pack
# step); the kernels widen them on load and compute in fp64.
OPERATOR_VALUE_DTYPES = (torch.float64, torch.float32)


def _val32(vals: torch.Tensor, what: str) -> bool:
    """True for fp32-stored values; TypeError (before any launch) for a
    dtype the kernels would misread."""
    if vals.dtype not in OPERATOR_VALUE_DTYPES:
        raise TypeError(f"{what}: operator values must be float64 or "
                        f"float32, got {vals.dtype}")
    return vals.dtype == torch.float32


def spmv_sell(sellptr: torch.Tensor, cols: torch.Tensor, vals: torch.Tensor,
              nrows: int, x: torch.Tensor, y: torch.Tensor, *,
              rowbase: int = 0, accum: bool = False,
              partials: torch.Tensor | None = None,
              scal: torch.Tensor | None = None, dotslot: int = -1,
              dot_accum: bool = True, variant: int | None = None,
              perm: torch.Tensor | None = None) -> None:
    """SELL-C-64(-sigma) SpMV.  ``perm`` (int32) maps SELL row -> matrix
    row for sigma-sorted irregular matrices.  ``vals`` may be stored in
    fp32 (see OPERATOR_VALUE_DTYPES); only the default ``variant`` exists
    for fp32 values."""
    if variant is None:
        variant = DEFAULT_SELL_VARIANT
    val32 = _val32(vals, "spmv_sell")
    if val32 and (variant & (SELL_NT | SELL_SWZ | SELL_U8)) != DEFAULT_SELL_VARIANT:
        raise TypeError("spmv_sell: float32 values support only the default "
                        f"variant {DEFAULT_SELL_VARIANT}, got {variant}")
    nslices = sellptr.numel() - 1
    if nslices <= 0:
        return
    fuse = scal is not None and dotslot >= 0
    K.spmv_sell(nslices, nrows, rowbase, sellptr.data_ptr(), cols.data_ptr(),
                1 if cols.dtype == torch.int64 else 0,
                vals.data_ptr(), x.data_ptr(), y.data_ptr(), accum,
                partials.data_ptr() if fuse else 0,
                scal.data_ptr() if fuse else 0, dotslot, dot_accum,
                variant, perm.data_ptr() if perm is not None else 0, val32,
                _stream())


def spmv_bsell(bptr: torch.Tensor, bcol: torch.Tensor, bvals: torch.Tensor,
               nnodes: int, dof: int, x: torch.Tensor, y: torch.Tensor, *,
               partials: torch.Tensor | None = None,
               scal: torch.Tensor | None = None, dotslot: int = -1,
               dot_accum: bool = True) -> None:
    """Block-SELL SpMV (dense dof x dof blocks; one int32 index per block).
    ``bvals`` may be stored in fp32 (see OPERATOR_VALUE_DTYPES)."""
    val32 = _val32(bvals, "spmv_bsell")
    nslices = bptr.numel() - 1
    if nslices <= 0:
        return
    fuse = scal is not None and dotslot >= 0
    K.spmv_bsell(nslices, nnodes, dof, bptr.data_ptr(), bcol.data_ptr(),
                 bvals.data_ptr(), x.data_ptr(), y.data_ptr(),
                 partials.data_ptr() if fuse else 0,
                 scal.data_ptr() if fuse else 0, dotslot, dot_accum, val32,
                 _stream())


def _spmv2_check(what: str, vals: torch.Tensor, nrows: int, ncols: int,
                 x1, x2, y1, y2, b, partials) -> None:
    """Argument checks shared by the dual SpMV wrappers, all before any
    launch: fp64 operator values only, fp64 contiguous vectors on the
    operator's GPU, gathered vectors ``ncols`` long (owned rows plus the
    ghost tail), outputs and ``b`` ``nrows`` long, no two of
    y1/y2/x1/x2/b sharing memory."""
    if vals.dtype != torch.float64:
        raise TypeError(f"{what}: operator values must be float64, got "
                        f"{vals.dtype} (no dual kernel for fp32-stored values)")
    if ncols < nrows:
        raise ValueError(f"{what}: ncols={ncols} is less than nrows={nrows}")
    vecs = [("x1", x1, ncols), ("x2", x2, ncols), ("y1", y1, nrows),
            ("y2", y2, nrows)]
    if b is not None:
        vecs.append(("b", b, nrows))
    for nm, v, need in vecs:
        if v.dtype != torch.float64:
            raise TypeError(f"{what}: {nm} must be float64, got {v.dtype}")
        if v.dim() != 1 or not v.is_contiguous() or v.numel() < need:
            raise ValueError(f"{what}: {nm} must be a contiguous vector of at "
                             f"least {need} entries, got {tuple(v.shape)}")
        if v.device != vals.device:
            raise ValueError(f"{what}: {nm} lives on {v.device}, the operator "
                             f"on {vals.device}")
    spans = [(nm, v.data_ptr(), v.data_ptr() + 8 * v.numel()) for nm, v, _ in vecs]
    for i, (na, a0, a1) in enumerate(spans):
        for nb_, b0, b1 in spans[i + 1:]:
            if a0 < b1 and b0 < a1:
                raise ValueError(f"{what}: {na} and {nb_} share memory")
    if partials is not None and (
            partials.dtype != torch.float64 or not partials.is_contiguous()
            or partials.numel() < 2 * MAXG or partials.device != vals.device):
        raise ValueError(f"{what}: partials must be contiguous float64 with "
                         f"{2 * MAXG} entries on {vals.device}")


def spmv2_sell(sellptr: torch.Tensor, cols: torch.Tensor, vals: torch.Tensor,
               nrows: int, x1: torch.Tensor, x2: torch.Tensor,
               y1: torch.Tensor, y2: torch.Tensor, *, ncols: int,
               b: torch.Tensor | None = None,
               partials: torch.Tensor | None = None,
               perm: torch.Tensor | None = None) -> int:
    """Dual SELL-C-64(-sigma) SpMV, one pass over the matrix:
    ``y1 = A x1`` (``b - A x1`` when ``b`` is given) and ``y2 = A x2``.
    ``ncols`` is the length the gathered vectors need (owned rows plus
    ghosts).  With ``partials`` the block partials of (x1,x1) and (y1,x1)
    land in ``partials[:nb]`` and ``partials[MAXG:MAXG + nb]`` for
    :func:`pipelined_replace_finalize`; returns nb, the blocks launched."""
    _spmv2_check("spmv2_sell", vals, nrows, ncols, x1, x2, y1, y2, b, partials)
    if cols.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"spmv2_sell: cols must be int32 or int64, got {cols.dtype}")
    if perm is not None and perm.dtype != torch.int32:
        raise TypeError("spmv2_sell: perm must be int32")
    nslices = sellptr.numel() - 1
    if nslices <= 0 or nrows <= 0:
        return 0
    if nslices != (nrows + 63) // 64:
        raise ValueError(f"spmv2_sell: {nslices} slices do not hold {nrows} rows")
    if perm is not None and perm.numel() < nslices * 64:
        raise ValueError(f"spmv2_sell: perm has {perm.numel()} entries, "
                         f"needs {nslices * 64}")
    if cols.numel() != vals.numel():
        raise ValueError(f"spmv2_sell: cols and vals differ in length: "
                         f"{cols.numel()} vs {vals.numel()}")
    return int(K.spmv2_sell(
        nslices, nrows, sellptr.data_ptr(), cols.data_ptr(),
        1 if cols.dtype == torch.int64 else 0, vals.data_ptr(),
        x1.data_ptr(), x2.data_ptr(), b.data_ptr() if b is not None else 0,
        y1.data_ptr(), y2.data_ptr(),
        partials.data_ptr() if partials is not None else 0,
        perm.data_ptr() if perm is not None else 0, _stream()))


def spmv2_bsell(bptr: torch.Tensor, bcol: torch.Tensor, bvals: torch.Tensor,
                nnodes: int, dof: int, x1: torch.Tensor, x2: torch.Tensor,
                y1: torch.Tensor, y2: torch.Tensor, *, ncols: int,
                b: torch.Tensor | None = None,
                partials: torch.Tensor | None = None) -> int:
    """Dual Block-SELL SpMV (dof 2/3/4); see :func:`spmv2_sell`."""
    if dof not in (2, 3, 4):
        raise ValueError(f"spmv2_bsell: dof must be 2, 3 or 4, got {dof}")
    _spmv2_check("spmv2_bsell", bvals, nnodes * dof, ncols, x1, x2, y1, y2, b,
                 partials)
    if bcol.dtype != torch.int32:
        raise TypeError(f"spmv2_bsell: bcol must be int32, got {bcol.dtype}")
    nslices = bptr.numel() - 1
    if nslices <= 0 or nnodes <= 0:
        return 0
    if nslices != (nnodes + 63) // 64:
        raise ValueError(f"spmv2_bsell: {nslices} slices do not hold {nnodes} nodes")
    if bvals.numel() != bcol.numel() * dof * dof:
        raise ValueError(f"spmv2_bsell: {bcol.numel()} block columns do not "
                         f"match {bvals.numel()} values of dof {dof}")
    return int(K.spmv2_bsell(
        nslices, nnodes, dof, bptr.data_ptr(), bcol.data_ptr(),
        bvals.data_ptr(), x1.data_ptr(), x2.data_ptr(),
        b.data_ptr() if b is not None else 0, y1.data_ptr(), y2.data_ptr(),
        partials.data_ptr() if partials is not None else 0, _stream()))


def dot2_slices(r: torch.Tensor, w: torch.Tensor, nunits: int, dof: int,
                partials: torch.Tensor, *,
                perm: torch.Tensor | None = None) -> int:
    """Block partials of (r,r) and (w,r) over ``nunits * dof`` rows in the
    row order and block partition of the fused dual SpMV (dof 1: SELL rows,
    optional sigma ``perm``; dof 2/3/4: BSELL nodes), for
    :func:`pipelined_replace_finalize`.  Returns the blocks launched."""
    what = "dot2_slices"
    if dof not in (1, 2, 3, 4) or (perm is not None and dof != 1):
        raise ValueError(f"{what}: dof must be 1..4 (perm only with dof 1), "
                         f"got dof={dof}")
    n = nunits * dof
    for nm, v in (("r", r), ("w", w)):
        if v.dtype != torch.float64:
            raise TypeError(f"{what}: {nm} must be float64, got {v.dtype}")
        if v.dim() != 1 or not v.is_contiguous() or v.numel() < n:
            raise ValueError(f"{what}: {nm} must be a contiguous vector of at "
                             f"least {n} entries, got {tuple(v.shape)}")
    if (partials.dtype != torch.float64 or not partials.is_contiguous()
            or partials.numel() < 2 * MAXG):
        raise ValueError(f"{what}: partials must be contiguous float64 with "
                         f"{2 * MAXG} entries")
    nslices = (nunits + 63) // 64
    if perm is not None and (perm.dtype != torch.int32
                             or perm.numel() < nslices * 64):
        raise ValueError(f"{what}: perm must be int32 with {nslices * 64} entries")
    if nunits <= 0:
        return 0
    return int(K.dot2_slices(nslices, nunits, dof, r.data_ptr(), w.data_ptr(),
                             perm.data_ptr() if perm is not None else 0,
                             partials.data_ptr(), _stream()))


def pipelined_replace_finalize(partials: torch.Tensor, nblocks: int,
                               scal: torch.Tensor) -> None:
    """scal[GAMMA], scal[DELTA] = sums of the two partial halves of a fused
    dual SpMV.  No other slot is written (GAMMA_PREV / ALPHA_PREV keep the
    rotation of the iteration just finished)."""
    what = "pipelined_replace_finalize"
    if not 0 <= nblocks <= MAXG:
        raise ValueError(f"{what}: nblocks must be in 0..{MAXG}, got {nblocks}")
    _bj_slab(what, scal, partials, scal.device)
    K.pipelined_replace_finalize(partials.data_ptr(), nblocks, scal.data_ptr(),
                                 _stream())


def spmv_bsell_st(st, x: torch.Tensor, y: torch.Tensor, *,
                  partials: torch.Tensor | None = None,
                  scal: torch.Tensor | None = None, dotslot: int = -1,
                  dot_accum: bool = True, max_blocks: int = 0) -> int:
    """Tile-symmetric Block-SELL SpMV; ``st`` from
    :func:`acg_amd.ops.symtile.bsell_st_build`, ``x`` and ``y`` in its
    permuted node order.  ``max_blocks`` > 0 caps the grid.  Returns the
    number of blocks launched."""
    if st.tile != K_ST_TILE:
        raise ValueError(f"spmv_bsell_st: the kernel's tile is {K_ST_TILE} "
                         f"nodes, this operator was built with {st.tile}")
    n = st.nnodes * st.dof
    if x.numel() < n or y.numel() < n:
        raise ValueError("spmv_bsell_st: x and y must hold nnodes * dof values")
    if x.dtype != torch.float64 or y.dtype != torch.float64:
        raise TypeError("spmv_bsell_st: x and y must be float64")
    fuse = scal is not None and dotslot >= 0
    return K.spmv_bsell_st(st.ntiles, st.nslices, st.nnodes, st.dof, st.qmax,
                           st.sptr.data_ptr(), st.spl.data_ptr(),
                           st.scol.data_ptr(), st.sq.data_ptr(),
                           st.svals.data_ptr(), st.nrecv.data_ptr(),
                           x.data_ptr(), y.data_ptr(),
                           partials.data_ptr() if fuse else 0,
                           scal.data_ptr() if fuse else 0, dotslot, dot_accum,
                           max_blocks, _stream())


def stencil_spmv(mf, nrows_nodes: int, row0_node: int, x: torch.Tensor,
                 y: torch.Tensor, *, mato: bool = False,
                 partials: torch.Tensor | None = None,
                 scal: torch.Tensor | None = None, dotslot: int = -1,
                 dot_accum: bool = True) -> None:
    """Matrix-free stencil SpMV (dof=1 constant-coefficient operators).
    ``mf`` = gen.device_slab mf_tables dict.  7-pt matA passes take the
    z-column-walk kernel (w_old read exactly once)."""
    if nrows_nodes <= 0:
        return
    fuse = scal is not None and dotslot >= 0
    pp = partials.data_ptr() if fuse else 0
    sp = scal.data_ptr() if fuse else 0
    if not mato and mf["w7"] is not None:
        K.stencil_spmv7(mf["gx"] * mf["gy"], mf["gx"], mf["z0"], mf["z1"],
                        mf["gz"], mf["nown_nodes"], mf["pb"].data_ptr(),
                        mf["diag"], *mf["w7"], x.data_ptr(), y.data_ptr(),
                        pp, sp, dotslot, dot_accum, _stream())
        return
    K.stencil_spmv(nrows_nodes, row0_node, mf["gx"], mf["gy"], mf["gz"],
                   mf["nown_nodes"], mf["zs"].data_ptr(),
                   mf["pb"].data_ptr(), mf["offs"].data_ptr(), mf["ksten"],
                   mf["diag"], x.data_ptr(), y.data_ptr(), mato,
                   pp, sp, dotslot, dot_accum, _stream())


def stencil_pipe(mf, nrows_nodes: int, row0_node: int, border_base: int,
                 w_old, qpart, z, t, p, x, r, w_new, scal, first: bool,
                 partials, partials_off: int, mato: bool) -> int:
    """Megafused matrix-free pipelined iteration pass (stencil SpMV +
    6-vector update + dots); same protocol as sell_pipe."""
    if nrows_nodes <= 0:
        return 0
    qp = qpart.data_ptr() if qpart is not None else 0
    if not mato and mf["w7"] is not None:
        return K.stencil_pipe7(mf["gx"] * mf["gy"], mf["gx"], mf["z0"],
                               mf["z1"], mf["gz"], border_base,
                               mf["nown_nodes"], mf["pb"].data_ptr(),
                               mf["diag"], *mf["w7"], w_old.data_ptr(), qp,
                               z.data_ptr(), t.data_ptr(), p.data_ptr(),
                               x.data_ptr(), r.data_ptr(), w_new.data_ptr(),
                               scal.data_ptr(), 1 if first else 0,
                               partials.data_ptr(), partials_off, _stream())
    return K.stencil_pipe(nrows_nodes, row0_node, border_base, mf["gx"],
                          mf["gy"], mf["gz"], mf["nown_nodes"],
                          mf["zs"].data_ptr(), mf["pb"].data_ptr(),
                          mf["offs"].data_ptr(), mf["ksten"], mf["diag"],
                          w_old.data_ptr(), qp,
                          z.data_ptr(), t.data_ptr(), p.data_ptr(),
                          x.data_ptr(), r.data_ptr(), w_new.data_ptr(),
                          scal.data_ptr(), 1 if first else 0,
                          partials.data_ptr(), partials_off, mato, _stream())


def spmv_bsell_daypx(bptr, bcol, bvals, nnodes: int, dof: int,
                     pold: torch.Tensor, rvec: torch.Tensor,
                     pnew: torch.Tensor, y: torch.Tensor,
                     scal: torch.Tensor, partials: torch.Tensor,
                     dotslot: int) -> None:
    """Classic-CG fold: p_new = beta*p_old + r materialised inside the
    BSELL SpMV (gather computes it on the fly), (p_new, t) dot fused.
    beta = scal[RR]/scal[RR_PREV]; serial matA-only (no matO pass)."""
    nslices = bptr.numel() - 1
    if nslices <= 0:
        return
    K.spmv_bsell_daypx(nslices, nnodes, dof, bptr.data_ptr(), bcol.data_ptr(),
                       bvals.data_ptr(), pold.data_ptr(), rvec.data_ptr(),
                       pnew.data_ptr(), y.data_ptr(), scal.data_ptr(),
                       partials.data_ptr(), dotslot, _stream())


def zero_scalars(scal: torch.Tensor, i0: int = 0, count: int | None = None) -> None:
    K.zero_scalars(scal.data_ptr(), i0, count if count is not None else scal.numel() - i0,
                   _stream())


def cg_prep_pt(scal: torch.Tensor) -> None:
    K.cg_prep_pt(scal.data_ptr(), _stream())


def cg_prep_rr(scal: torch.Tensor) -> None:
    K.cg_prep_rr(scal.data_ptr(), _stream())


def dot(x: torch.Tensor, y: torch.Tensor, partials: torch.Tensor,
        scal: torch.Tensor, slot: int, n: int | None = None,
        accumulate: bool = False) -> None:
    n = x.numel() if n is None else n
    K.dot(x.data_ptr(), y.data_ptr(), n, partials.data_ptr(), scal.data_ptr(),
          slot, accumulate, _stream())


def dot2(r: torch.Tensor, w: torch.Tensor, partials: torch.Tensor,
         scal: torch.Tensor, n: int, accumulate: bool = False) -> None:
    """scal[GAMMA] (=|+=) (r,r); scal[DELTA] (=|+=) (w,r): one pass."""
    K.dot2(r.data_ptr(), w.data_ptr(), n, partials.data_ptr(), scal.data_ptr(),
           accumulate, _stream())


def axpy_ratio(y: torch.Tensor, x: torch.Tensor, scal: torch.Tensor,
               num: int, den: int, sign: float = 1.0, n: int | None = None) -> None:
    K.axpy_ratio(y.data_ptr(), x.data_ptr(), y.numel() if n is None else n,
                 scal.data_ptr(), num, den, sign, _stream())


def daypx_ratio(y: torch.Tensor, x: torch.Tensor, scal: torch.Tensor,
                num: int, den: int, n: int | None = None) -> None:
    K.daypx_ratio(y.data_ptr(), x.data_ptr(), y.numel() if n is None else n,
                  scal.data_ptr(), num, den, _stream())


def cg_fused_update(r: torch.Tensor, x: torch.Tensor, p: torch.Tensor,
                    t: torch.Tensor, scal: torch.Tensor,
                    partials: torch.Tensor, n: int) -> None:
    """alpha = rr_prev/pt (device); r -= alpha t; x += alpha p;
    scal[RR] = (r,r) (finalized)."""
    K.cg_fused_update(r.data_ptr(), x.data_ptr(), p.data_ptr(), t.data_ptr(),
                      n, scal.data_ptr(), partials.data_ptr(), _stream())


def pcg_fused_update(r, x, p, t, z, dinv, scal, partials, n: int) -> None:
    """Jacobi-PCG fused epilogue: alpha = rz/pt (device); r -= alpha t;
    x += alpha p; z = dinv*r; rotates rz -> RR_PREV and publishes the new
    rz in S_RR plus the TRUE (r,r) in S_GAMMA."""
    K.pcg_fused_update(r.data_ptr(), x.data_ptr(), p.data_ptr(), t.data_ptr(),
                       z.data_ptr(), dinv.data_ptr(), n, scal.data_ptr(),
                       partials.data_ptr(), _stream())


# -- block-Jacobi PCG on Block-SELL operators --------------------------------

BJ_DOFS = (2, 3, 4)


def block_inv_len(nnodes: int, dof: int) -> int:
    """Length of the packed inverse-block buffer: dof(dof+1)/2 components
    per node, laid out [slice][component][64]."""
    return ((nnodes + 63) // 64) * (dof * (dof + 1) // 2) * 64


def _bj_check(what: str, n: int, dof: int, minv: torch.Tensor, *vecs) -> int:
    """Validate the arguments shared by the block-Jacobi ops (before any
    launch); returns nnodes."""
    if dof not in BJ_DOFS:
        raise ValueError(f"{what}: dof must be one of {BJ_DOFS}, got {dof}")
    if n < 0 or n % dof:
        raise ValueError(f"{what}: n={n} is not a multiple of dof={dof}")
    nnodes = n // dof
    for v in (minv, *vecs):
        if v.dtype != torch.float64:
            raise TypeError(f"{what}: vectors must be float64, got {v.dtype}")
        if not v.is_cuda or v.device != minv.device:
            raise ValueError(f"{what}: tensors must live on one GPU")
        if not v.is_contiguous():
            raise ValueError(f"{what}: tensors must be contiguous")
    for v in vecs:
        if v.dim() != 1 or v.numel() < n:
            raise ValueError(f"{what}: vector has shape {tuple(v.shape)}, "
                             f"needs at least {n} entries")
    if minv.numel() != block_inv_len(nnodes, dof):
        raise ValueError(f"{what}: inverse buffer has {minv.numel()} entries, "
                         f"needs {block_inv_len(nnodes, dof)} for "
                         f"{nnodes} nodes of dof {dof}")
    return nnodes


def _bj_slab(what: str, scal: torch.Tensor, partials: torch.Tensor,
             device) -> None:
    for v, need in ((scal, S_NSLOTS), (partials, 2 * MAXG)):
        if (v.dtype != torch.float64 or v.device != device
                or not v.is_contiguous() or v.numel() < need):
            raise ValueError(f"{what}: scal/partials must be contiguous "
                             f"float64 on {device} with >= {S_NSLOTS} / "
                             f"{2 * MAXG} entries")


def bsell_diag_inv(bptr: torch.Tensor, bcol: torch.Tensor,
                   bvals: torch.Tensor, nnodes: int, dof: int):
    """Inverse of every node's dof x dof diagonal block of a Block-SELL
    matrix, by Cholesky, as packed upper triangles (see block_inv_len).
    Returns (minv, nbad); nbad counts the nodes without a diagonal block
    or with a pivot that is <= 0 or not finite (their inverse is zero).
    One launch plus one host read of the status word."""
    what = "bsell_diag_inv"
    if dof not in BJ_DOFS:
        raise ValueError(f"{what}: dof must be one of {BJ_DOFS}, got {dof}")
    if bvals.dtype != torch.float64:
        raise TypeError(f"{what}: reads the float64 block values, "
                        f"got {bvals.dtype}")
    if bptr.dtype != torch.int64 or bcol.dtype != torch.int32:
        raise TypeError(f"{what}: bptr must be int64 and bcol int32")
    for v in (bptr, bcol, bvals):
        if not v.is_cuda or v.device != bvals.device:
            raise ValueError(f"{what}: tensors must live on one GPU")
        if not v.is_contiguous():
            raise ValueError(f"{what}: tensors must be contiguous")
    nslices = bptr.numel() - 1
    if nnodes < 0 or nslices != (nnodes + 63) // 64:
        raise ValueError(f"{what}: {nslices} slices do not hold {nnodes} nodes")
    if (bvals.numel() != bcol.numel() * dof * dof
            or (nslices > 0 and bcol.numel() % 64)):
        raise ValueError(f"{what}: {bcol.numel()} block columns do not match "
                         f"{bvals.numel()} values of dof {dof}")
    if nslices > 0 and int(bptr[-1]) != bcol.numel():  # setup-time read
        raise ValueError(f"{what}: bptr ends at {int(bptr[-1])}, but there "
                         f"are {bcol.numel()} block columns")
    minv = torch.zeros(block_inv_len(nnodes, dof), dtype=torch.float64,
                       device=bvals.device)
    status = torch.zeros(1, dtype=torch.int32, device=bvals.device)
    if nnodes > 0:
        K.bsell_diag_inv(nslices, nnodes, dof, bptr.data_ptr(),
                         bcol.data_ptr(), bvals.data_ptr(), minv.data_ptr(),
                         status.data_ptr(), _stream())
    return minv, int(status.item())


def bjacobi_apply(minv: torch.Tensor, r: torch.Tensor, z: torch.Tensor,
                  partials: torch.Tensor, scal: torch.Tensor, n: int,
                  dof: int) -> None:
    """z = M^-1 r with the packed inverse blocks of bsell_diag_inv; rotates
    S_RR -> S_RR_PREV and publishes (r,z) in S_RR and (r,r) in S_GAMMA
    (the finalize of pcg_fused_update)."""
    nnodes = _bj_check("bjacobi_apply", n, dof, minv, r, z)
    _bj_slab("bjacobi_apply", scal, partials, minv.device)
    K.bjacobi_apply(minv.data_ptr(), r.data_ptr(), z.data_ptr(), nnodes, dof,
                    scal.data_ptr(), partials.data_ptr(), _stream())


def bpcg_fused_update(r, x, p, t, z, minv, scal, partials, n: int,
                      dof: int) -> None:
    """Block-Jacobi PCG fused epilogue: alpha = rz/pt (device); r -= alpha t;
    x += alpha p; z = M^-1 r node by node; rotates rz -> RR_PREV and
    publishes the new rz in S_RR plus the TRUE (r,r) in S_GAMMA."""
    nnodes = _bj_check("bpcg_fused_update", n, dof, minv, r, x, p, t, z)
    _bj_slab("bpcg_fused_update", scal, partials, minv.device)
    K.bpcg_fused_update(r.data_ptr(), x.data_ptr(), p.data_ptr(),
                        t.data_ptr(), z.data_ptr(), minv.data_ptr(), nnodes,
                        dof, scal.data_ptr(), partials.data_ptr(), _stream())


def sell_pipe(sellptr, cols, vals, nrows_pass: int, rowbase: int,
              border_base: int, w_old, qpart, z, t, p, x, r, w_new,
              scal, first: bool, partials, partials_off: int,
              mato: bool) -> int:
    """Megafused pipelined iteration pass (SpMV + 6-vector update + dots).
    Returns the number of partial blocks written."""
    nslices = sellptr.numel() - 1
    assert cols.dtype == torch.int32
    return K.sell_pipe(nslices, nrows_pass, rowbase, border_base,
                       sellptr.data_ptr(), cols.data_ptr(), vals.data_ptr(),
                       w_old.data_ptr(),
                       qpart.data_ptr() if qpart is not None else 0,
                       z.data_ptr(), t.data_ptr(), p.data_ptr(), x.data_ptr(),
                       r.data_ptr(), w_new.data_ptr(), scal.data_ptr(),
                       1 if first else 0, partials.data_ptr(), partials_off,
                       mato, _stream())


def pipelined_finalize(partials, nblocks: int, scal, first: bool) -> None:
    K.pipelined_finalize(partials.data_ptr(), nblocks, scal.data_ptr(),
                         1 if first else 0, _stream())


def pipelined_fused(z, t, p, x, r, w, q, scal: torch.Tensor,
                    partials: torch.Tensor, n: int, first: bool,
                    nt_update: bool = True) -> None:
    """Fused pipelined update + next gamma/delta + scalar rotation."""
    K.pipelined_fused(z.data_ptr(), t.data_ptr(), p.data_ptr(), x.data_ptr(),
                      r.data_ptr(), w.data_ptr(), q.data_ptr(), n,
                      scal.data_ptr(), 1 if first else 0, partials.data_ptr(),
                      nt_update, _stream())


BAR_STATE_WORDS = K.BAR_STATE_WORDS  # flat + hierarchical v3 barrier state


def cg_device(sellptr: torch.Tensor, cols: torch.Tensor, vals: torch.Tensor,
              nrows: int, b: torch.Tensor, x: torch.Tensor, r: torch.Tensor,
              p: torch.Tensor, t: torch.Tensor, scal: torch.Tensor,
              partials: torch.Tensor, out2: torch.Tensor,
              barrier_state: torch.Tensor, maxits: int,
              res_atol: float, res_rtol: float,
              hier: bool | None = None) -> int:
    """Monolithic device-side CG: one cooperative launch runs the whole
    solve.  ``barrier_state``: BAR_STATE_WORDS zeroed uint32 words (must
    be zeroed before EVERY launch).  ``hier`` selects the hierarchical
    (per-XCD then global) grid barrier; default = env ACG_DEVCG_HIER
    ("auto": hierarchical from 64 blocks up -- measured crossover,
    tools/devcg_barrier_ab.py).  Returns the grid size used."""
    what = "cg_device"
    nslices = sellptr.numel() - 1
    if sellptr.dtype != torch.int64 or nslices < 1:
        raise ValueError(f"{what}: sellptr must be int64 with at least 2 "
                         f"entries, got {sellptr.dtype}[{sellptr.numel()}]")
    if cols.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{what}: cols must be int32 or int64, got {cols.dtype}")
    if vals.dtype != torch.float64:
        raise ValueError(f"{what}: operator values must be float64, got "
                         f"{vals.dtype} (the fp32-stored operator is not supported)")
    nrows, maxits = int(nrows), int(maxits)
    if not 0 < nrows <= nslices * 64:
        raise ValueError(f"{what}: nrows={nrows} does not fit {nslices} slices")
    # sellptr[-1] lives on the device: reading it would cost a sync
    if cols.numel() != vals.numel():
        raise ValueError(f"{what}: cols and vals differ in length: "
                         f"{cols.numel()} vs {vals.numel()}")
    for nm, v in (("b", b), ("x", x), ("r", r), ("p", p), ("t", t)):
        if (v.dtype != torch.float64 or not v.is_contiguous()
                or v.numel() < nrows):
            raise ValueError(f"{what}: {nm} must be a contiguous float64 "
                             f"vector of at least {nrows} elements")
    for nm, v, need in (("scal", scal, S_NSLOTS), ("partials", partials, MAXG)):
        if (v.dtype != torch.float64 or not v.is_contiguous()
                or v.numel() < need):
            raise ValueError(f"{what}: {nm} must be contiguous float64 with "
                             f"at least {need} elements")
    if (out2.dtype != torch.int32 or not out2.is_contiguous()
            or out2.numel() < 2):
        raise ValueError(f"{what}: out2 must be contiguous int32 with at "
                         "least 2 elements")
    if (barrier_state.dtype not in (torch.int32, torch.uint32)
            or not barrier_state.is_contiguous()
            or barrier_state.numel() < BAR_STATE_WORDS):
        raise ValueError(f"{what}: barrier_state must hold at least "
                         f"{BAR_STATE_WORDS} contiguous 4-byte integer words")
    for nm, v in (("sellptr", sellptr), ("cols", cols), ("vals", vals),
                  ("b", b), ("x", x), ("r", r), ("p", p), ("t", t),
                  ("scal", scal), ("partials", partials), ("out2", out2),
                  ("barrier_state", barrier_state)):
        if not v.is_cuda or v.device != x.device:
            raise ValueError(f"{what}: {nm} must live on the GPU of x, got "
                             f"{v.device}")
    if not cols.is_contiguous() or not vals.is_contiguous() \
            or not sellptr.is_contiguous():
        raise ValueError(f"{what}: sellptr, cols and vals must be contiguous")
    if maxits < 0:
        raise ValueError(f"{what}: maxits must not be negative, got {maxits}")
    if hier is None:
        import os

        v = os.environ.get("ACG_DEVCG_HIER", "auto")
        ih = -1 if v == "auto" else (0 if v == "0" else 1)
    else:
        ih = 1 if hier else 0
    return K.cg_device(nslices, nrows, sellptr.data_ptr(), cols.data_ptr(),
                       1 if cols.dtype == torch.int64 else 0, vals.data_ptr(),
                       b.data_ptr(), x.data_ptr(), r.data_ptr(), p.data_ptr(),
                       t.data_ptr(), scal.data_ptr(), partials.data_ptr(),
                       out2.data_ptr(), barrier_state.data_ptr(),
                       maxits, res_atol, res_rtol, _stream(), ih)


# ---------------------------------------------------------------------------
# Multiple right-hand sides.  A multivector is a contiguous fp64 (n, K)
# tensor, element (i, c) at i*K + c, K in MULTI_K at kernel level; the
# scalar slab is (K, S_NSLOTS) and the partials scratch (K, MAXG).

MULTI_K = (2, 4, 8)


def alloc_scalars_multi(device, k: int) -> torch.Tensor:
    return torch.zeros(k, S_NSLOTS, dtype=torch.float64, device=device)


def alloc_partials_multi(device, k: int) -> torch.Tensor:
    return torch.zeros(k, MAXG, dtype=torch.float64, device=device)


def _multi_k(what: str, *mvs: torch.Tensor, rows: int | None = None) -> int:
    """Validate multivectors (fp64, 2-D, contiguous, 16 B aligned, same K in
    MULTI_K, at least ``rows`` rows); returns K."""
    k = mvs[0].shape[1] if mvs[0].dim() == 2 else -1
    if k not in MULTI_K:
        raise ValueError(f"{what}: multivectors must have shape (n, K) with K "
                         f"in {MULTI_K}, got {tuple(mvs[0].shape)}")
    for v in mvs:
        if v.dtype != torch.float64:
            raise TypeError(f"{what}: multivectors must be float64, got {v.dtype}")
        if v.dim() != 2 or v.shape[1] != k:
            raise ValueError(f"{what}: multivector shapes disagree: "
                             f"{[tuple(m.shape) for m in mvs]}")
        if not v.is_contiguous():
            raise ValueError(f"{what}: multivectors must be contiguous")
        if v.data_ptr() % 16:
            raise ValueError(f"{what}: multivectors must be 16-byte aligned")
        if rows is not None and v.shape[0] < rows:
            raise ValueError(f"{what}: multivector has {v.shape[0]} rows, "
                             f"needs at least {rows}")
    return k


def _multi_slab(what: str, k: int, scal: torch.Tensor,
                partials: torch.Tensor | None) -> None:
    for t, cols, nm in ((scal, S_NSLOTS, "scal"), (partials, MAXG, "partials")):
        if t is None:
            continue
        if (t.dtype != torch.float64 or not t.is_contiguous()
                or t.numel() < k * cols):
            raise ValueError(f"{what}: {nm} must be a contiguous float64 "
                             f"({k}, {cols}) tensor")


def spmm_bsell_supported(dof: int, k: int) -> bool:
    """True where a register-resident k_spmm_bsell<dof, k> exists."""
    return bool(K.spmm_bsell_supported(dof, k))


def spmm_sell(sellptr: torch.Tensor, cols: torch.Tensor, vals: torch.Tensor,
              nrows: int, X: torch.Tensor, Y: torch.Tensor, *,
              partials: torch.Tensor | None = None,
              scal: torch.Tensor | None = None, dotslot: int = -1,
              dot_accum: bool = False,
              perm: torch.Tensor | None = None) -> None:
    """SELL-C-64(-sigma) SpMM: Y[:nrows] = A X for K interleaved vectors;
    optional fused per-column dot (X_c, Y_c) into slot ``dotslot`` of every
    column's slab.  fp64 operator values only."""
    k = _multi_k("spmm_sell", X, Y, rows=nrows)
    if vals.dtype != torch.float64:
        raise TypeError(f"spmm_sell: operator values must be float64, got {vals.dtype}")
    if cols.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"spmm_sell: cols must be int32 or int64, got {cols.dtype}")
    if perm is not None and perm.dtype != torch.int32:
        raise TypeError("spmm_sell: perm must be int32")
    nslices = sellptr.numel() - 1
    if nslices <= 0:
        return
    fuse = scal is not None and dotslot >= 0
    if fuse:
        _multi_slab("spmm_sell", k, scal, partials)
    K.spmm_sell(nslices, nrows, k, sellptr.data_ptr(), cols.data_ptr(),
                1 if cols.dtype == torch.int64 else 0, vals.data_ptr(),
                X.data_ptr(), Y.data_ptr(),
                partials.data_ptr() if fuse else 0,
                scal.data_ptr() if fuse else 0, dotslot, dot_accum,
                perm.data_ptr() if perm is not None else 0, _stream())


def spmm_bsell(bptr: torch.Tensor, bcol: torch.Tensor, bvals: torch.Tensor,
               nnodes: int, dof: int, X: torch.Tensor, Y: torch.Tensor, *,
               partials: torch.Tensor | None = None,
               scal: torch.Tensor | None = None, dotslot: int = -1,
               dot_accum: bool = False) -> None:
    """Block-SELL SpMM (dof in 2/3/4), same fused dot as :func:`spmm_sell`."""
    k = _multi_k("spmm_bsell", X, Y, rows=nnodes * dof)
    if bvals.dtype != torch.float64:
        raise TypeError(f"spmm_bsell: operator values must be float64, got {bvals.dtype}")
    if not spmm_bsell_supported(dof, k):
        raise ValueError(f"spmm_bsell: no kernel for dof={dof}, K={k}")
    nslices = bptr.numel() - 1
    if nslices <= 0:
        return
    fuse = scal is not None and dotslot >= 0
    if fuse:
        _multi_slab("spmm_bsell", k, scal, partials)
    K.spmm_bsell(nslices, nnodes, dof, k, bptr.data_ptr(), bcol.data_ptr(),
                 bvals.data_ptr(), X.data_ptr(), Y.data_ptr(),
                 partials.data_ptr() if fuse else 0,
                 scal.data_ptr() if fuse else 0, dotslot, dot_accum, _stream())


def dot_multi(X: torch.Tensor, Y: torch.Tensor, partials: torch.Tensor,
              scal: torch.Tensor, slot: int, n: int | None = None,
              accumulate: bool = False) -> None:
    """scal[c, slot] (=|+=) (X[:n, c], Y[:n, c]) for every column c."""
    n = X.shape[0] if n is None else n
    k = _multi_k("dot_multi", X, Y, rows=n)
    _multi_slab("dot_multi", k, scal, partials)
    K.dot_multi(X.data_ptr(), Y.data_ptr(), n, k, partials.data_ptr(),
                scal.data_ptr(), slot, accumulate, _stream())


def reduce_partials_multi(partials: torch.Tensor, nblocks: int,
                          scal: torch.Tensor, slot: int,
                          accumulate: bool = False) -> None:
    """scal[c, slot] (=|+=) sum(partials[c, :nblocks]) for every column."""
    k = scal.numel() // S_NSLOTS
    _multi_slab("reduce_partials_multi", k, scal, partials)
    K.reduce_partials_multi(partials.data_ptr(), nblocks, k, scal.data_ptr(),
                            slot, accumulate, _stream())


def cg_fused_update_multi(R: torch.Tensor, X: torch.Tensor, P: torch.Tensor,
                          T: torch.Tensor, scal: torch.Tensor,
                          partials: torch.Tensor, n: int) -> int:
    """Per column c: alpha_c = scal[c, RR]/scal[c, PT]; R -= alpha_c T;
    X += alpha_c P on the first n rows.  Leaves the block partials of the
    new (r, r) in ``partials[c, :nblocks]`` for :func:`cg_finalize_multi`
    and returns nblocks."""
    k = _multi_k("cg_fused_update_multi", R, X, P, T, rows=n)
    _multi_slab("cg_fused_update_multi", k, scal, partials)
    return int(K.cg_fused_update_multi(R.data_ptr(), X.data_ptr(), P.data_ptr(),
                                       T.data_ptr(), n, k, scal.data_ptr(),
                                       partials.data_ptr(), _stream()))


def cg_finalize_multi(partials: torch.Tensor, nblocks: int, scal: torch.Tensor,
                      rr_out: torch.Tensor) -> None:
    """Per column c: rotate RR -> RR_PREV, publish sum(partials[c, :nblocks])
    as the new RR and as ``rr_out[c]`` (contiguous, for the host test)."""
    k = scal.numel() // S_NSLOTS
    _multi_slab("cg_finalize_multi", k, scal, partials)
    if (rr_out.dtype != torch.float64 or not rr_out.is_contiguous()
            or rr_out.numel() < k):
        raise ValueError(f"cg_finalize_multi: rr_out must be float64[{k}]")
    K.cg_finalize_multi(partials.data_ptr(), nblocks, k, scal.data_ptr(),
                        rr_out.data_ptr(), _stream())


def daypx_ratio_multi(P: torch.Tensor, R: torch.Tensor, scal: torch.Tensor,
                      num: int = S_RR, den: int = S_RR_PREV,
                      n: int | None = None) -> None:
    """P[:n, c] = (scal[c, num]/scal[c, den]) P[:n, c] + R[:n, c]."""
    n = R.shape[0] if n is None else n
    k = _multi_k("daypx_ratio_multi", P, R, rows=n)
    _multi_slab("daypx_ratio_multi", k, scal, None)
    K.daypx_ratio_multi(P.data_ptr(), R.data_ptr(), n, k, scal.data_ptr(),
                        num, den, _stream())


# ---------------------------------------------------------------------------
# Block CG (Dubrulle, orthonormalised residuals).  The block state is one
# fp64 tensor of BS_SIZE slots (layout in kernels.hip next to the S_*
# slots); the Gram partials live in an alloc_partials_multi(device, K)
# tensor, pair p = (a <= b) of block g at p*BLOCK_MAXG + g.

BS_LD = K.BS_LD
BS_M = K.BS_M
BS_XI = K.BS_XI
BS_XIC = K.BS_XIC
BS_G = K.BS_G
BS_ZETA = K.BS_ZETA
BS_ZINV = K.BS_ZINV
BS_C = K.BS_C
BS_FLAG = K.BS_FLAG
BS_ITER = K.BS_ITER
BS_SIZE = K.BS_SIZE
BLOCK_MAXG = K.BLOCK_MAXG
BLOCK_TAU = K.BLOCK_TAU


def alloc_block_state(device) -> torch.Tensor:
    return torch.zeros(BS_SIZE, dtype=torch.float64, device=device)


def _block_bufs(what: str, k: int, kg: int | None, state: torch.Tensor | None,
                partials: torch.Tensor | None, nblocks: int | None = None,
                rr_out: torch.Tensor | None = None) -> None:
    if k not in MULTI_K:
        raise ValueError(f"{what}: K must be in {MULTI_K}, got {k}")
    if kg is not None and not 1 <= kg <= k:
        raise ValueError(f"{what}: kg must be in 1..{k}, got {kg}")
    npairs = k * (k + 1) // 2
    for t, need, nm in ((state, BS_SIZE, "state"),
                        (partials, npairs * BLOCK_MAXG, "partials"),
                        (rr_out, k + 2, "rr_out")):
        if t is None:
            continue
        if (t.dtype != torch.float64 or not t.is_contiguous()
                or t.numel() < need or not t.is_cuda):
            raise ValueError(f"{what}: {nm} must be a contiguous float64 "
                             f"device tensor of at least {need} elements")
    if nblocks is not None and not 1 <= nblocks <= BLOCK_MAXG:
        raise ValueError(f"{what}: nblocks must be in 1..{BLOCK_MAXG}, "
                         f"got {nblocks}")


def gram_multi(X: torch.Tensor, Y: torch.Tensor, partials: torch.Tensor,
               n: int | None = None) -> int:
    """Block partials of the upper triangle (a <= b) of X[:n]^T Y[:n] into
    ``partials[p*BLOCK_MAXG + g]``; returns the number of blocks."""
    n = X.shape[0] if n is None else n
    k = _multi_k("gram_multi", X, Y, rows=n)
    _block_bufs("gram_multi", k, None, None, partials)
    return int(K.gram_multi(X.data_ptr(), Y.data_ptr(), n, k,
                            partials.data_ptr(), _stream()))


def block_update(X: torch.Tensor, S: torch.Tensor, Q: torch.Tensor,
                 T: torch.Tensor, state: torch.Tensor, partials: torch.Tensor,
                 n: int) -> int:
    """X += S (xi C); Q <- W = Q - T xi on the first n rows; block partials
    of the upper triangle of W^T W; returns the number of blocks.  Does
    nothing when the breakdown flag of ``state`` is set."""
    k = _multi_k("block_update", X, S, Q, T, rows=n)
    _block_bufs("block_update", k, None, state, partials)
    return int(K.block_update(X.data_ptr(), S.data_ptr(), Q.data_ptr(),
                              T.data_ptr(), n, k, state.data_ptr(),
                              partials.data_ptr(), _stream()))


def block_ortho(Q: torch.Tensor, S: torch.Tensor, state: torch.Tensor,
                n: int) -> None:
    """Q <- Q zeta^-1; S <- Q + S zeta^T on the first n rows (ghost rows of
    S are not written).  Does nothing when the breakdown flag is set."""
    k = _multi_k("block_ortho", Q, S, rows=n)
    _block_bufs("block_ortho", k, None, state, None)
    K.block_ortho(Q.data_ptr(), S.data_ptr(), n, k, state.data_ptr(), _stream())


def block_coef_alpha(partials: torch.Tensor, nblocks: int, state: torch.Tensor,
                     k: int, kg: int, it: int) -> None:
    """M = sum of the Gram partials (mirrored, identity beyond kg),
    pivot-tested Cholesky, xi = M^-1, xi C.  A failed pivot sets the sticky
    flag and records ``it``."""
    _block_bufs("block_coef_alpha", k, kg, state, partials, nblocks)
    K.block_coef_alpha(partials.data_ptr(), nblocks, state.data_ptr(), k, kg,
                       it, _stream())


def block_coef_beta(partials: torch.Tensor, nblocks: int, state: torch.Tensor,
                    rr_out: torch.Tensor, k: int, kg: int, it: int,
                    init: bool = False) -> None:
    """G = sum of the Gram partials, zeta = chol(G)^T, zeta^-1, C <- zeta C
    (``init``: C = zeta); rr_out[c] = ||C[:, c]||^2 for c < kg, rr_out[k] the
    breakdown flag and rr_out[k+1] the iteration it was set at (-1: never)."""
    _block_bufs("block_coef_beta", k, kg, state, partials, nblocks, rr_out)
    K.block_coef_beta(partials.data_ptr(), nblocks, state.data_ptr(),
                      rr_out.data_ptr(), k, kg, it, bool(init), _stream())


def pack_gather(sendbuf: torch.Tensor, x: torch.Tensor, idx: torch.Tensor) -> None:
    K.pack_gather(sendbuf.data_ptr(), x.data_ptr(), idx.data_ptr(),
                  1 if idx.dtype == torch.int64 else 0,
                  sendbuf.numel(), _stream())
