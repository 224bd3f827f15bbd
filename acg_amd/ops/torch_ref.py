"""Plain-PyTorch fp64 reference implementations of every HIP op.

Used (a) as the oracle in kernel numerics tests (GPU kernel vs torch fp64,
same semantics), (b) as the compute engine of the CPU solver path
(reference analog: acg/cg.c host solver).  Mirrors the device-scalar
convention: coefficients live in a small fp64 "scal" tensor; ``partials``
arguments are accepted for API parity but unused (torch reduces directly).
"""

from __future__ import annotations

import math

import torch

# keep slot numbering identical to kernels.hip
S_RR, S_PT, S_RR_PREV, S_BNRM2 = 0, 1, 2, 3
S_GAMMA, S_DELTA, S_GAMMA_PREV, S_ALPHA_PREV = 4, 5, 6, 7
S_NSLOTS = 8
# half-size of the two-phase reduction scratch (shared with kernels.hip);
# only sell_pipe/pipelined_finalize stage partial sums in this module
MAXG = 16384
# storage types of the SELL / BSELL operator values (same as gpu_ops):
# fp32 values are upcast (exact) and then take the fp64 arithmetic below
OPERATOR_VALUE_DTYPES = (torch.float64, torch.float32)


def _vals64(vals, what: str):
    if vals.dtype not in OPERATOR_VALUE_DTYPES:
        raise TypeError(f"{what}: operator values must be float64 or "
                        f"float32, got {vals.dtype}")
    return vals.to(torch.float64)


def alloc_scalars(device="cpu") -> torch.Tensor:
    return torch.zeros(S_NSLOTS, dtype=torch.float64, device=device)


def alloc_partials(device="cpu") -> torch.Tensor:
    return torch.zeros(1, dtype=torch.float64, device=device)


def spmv(rowptr, colidx, vals, x, y, *, rowbase: int = 0, accum: bool = False,
         partials=None, scal=None, dotslot: int = -1, dot_accum: bool = True) -> None:
    nrows = rowptr.numel() - 1
    if nrows <= 0:
        return
    counts = rowptr[1:] - rowptr[:-1]
    rows = torch.repeat_interleave(torch.arange(nrows, dtype=torch.int64,
                                                device=rowptr.device), counts)
    prod = vals * x[colidx.long()]
    contrib = torch.zeros(nrows, dtype=torch.float64, device=x.device)
    contrib.index_add_(0, rows, prod)
    sl = slice(rowbase, rowbase + nrows)
    if accum:
        y[sl] += contrib
    else:
        y[sl] = contrib
    if scal is not None and dotslot >= 0:
        d = torch.dot(x[sl], contrib)
        scal[dotslot] = scal[dotslot] + d if dot_accum else d


def spmv_binned(rowptr, colidx, vals, rowlist, bins, x, y, *, rowbase: int = 0,
                accum: bool = False, partials=None, scal=None,
                dotslot: int = -1, dot_accum: bool = True) -> None:
    """Row-binned CSR SpMV: ``bins`` only schedule the rows on the GPU;
    every row of ``rowlist`` is computed exactly once and no other row (or
    its share of the dot) is touched -- the hybrid's long-row list."""
    if rowlist.numel() == 0:
        return
    nrows = rowptr.numel() - 1
    if rowlist.numel() == nrows:
        return spmv(rowptr, colidx, vals, x, y, rowbase=rowbase, accum=accum,
                    partials=partials, scal=scal, dotslot=dotslot,
                    dot_accum=dot_accum)
    ysub = torch.zeros(nrows, dtype=torch.float64, device=x.device)
    spmv(rowptr, colidx, vals, x, ysub)
    rl = rowlist.long()
    y[rowbase + rl] = y[rowbase + rl] + ysub[rl] if accum else ysub[rl]
    if scal is not None and dotslot >= 0:
        d = torch.dot(x[rowbase + rl], ysub[rl])
        scal[dotslot] = scal[dotslot] + d if dot_accum else d


def zero_scalars(scal, i0: int = 0, count=None) -> None:
    scal[i0:i0 + (count if count is not None else scal.numel() - i0)] = 0.0


def sell_from_csr(rowptr, colidx, vals, C: int = 64, sigma: int = 1):
    """Convert CSR -> SELL-C-sigma (vectorized numpy host prep).

    Element j of SELL row (s*C+lane) lives at sellptr[s] + j*C + lane.
    ``sigma`` > 1 sorts rows by descending length within windows of
    sigma*C rows, shrinking padding for irregular matrices; the returned
    ``perm`` (or None for sigma=1) maps SELL row -> matrix row (pad lanes
    hold nrows as a sentinel).  Padding entries point at a valid row with
    value 0.  Returns (sellptr int64, cols, vals f64[, perm int32])."""
    import numpy as np

    rowptr = np.asarray(rowptr)
    colidx = np.asarray(colidx)
    vals = np.asarray(vals)
    nrows = len(rowptr) - 1
    nslices = (nrows + C - 1) // C
    counts = np.diff(rowptr)
    perm = None
    rowof = np.arange(nslices * C, dtype=np.int64)  # SELL row -> matrix row
    if sigma > 1 and nrows:
        win = sigma * C
        order = np.empty(nrows, dtype=np.int64)
        for w0 in range(0, nrows, win):
            w1 = min(w0 + win, nrows)
            sub = np.argsort(-counts[w0:w1], kind="stable")
            order[w0:w1] = w0 + sub
        rowof = np.full(nslices * C, nrows, dtype=np.int64)
        rowof[:nrows] = order
        perm = rowof.astype(np.int32)
    cpad = np.zeros(nslices * C, dtype=np.int64)
    valid = rowof < nrows
    cpad[valid] = counts[rowof[valid]]
    slice_len = cpad.reshape(nslices, C).max(axis=1)
    sellptr = np.zeros(nslices + 1, dtype=np.int64)
    np.cumsum(slice_len * C, out=sellptr[1:])
    total = int(sellptr[-1])
    # defaults: col = first valid row's own col target (clipped), val = 0
    slice_of_p = np.repeat(np.arange(nslices, dtype=np.int64), slice_len * C)
    lane = (np.arange(total, dtype=np.int64) - sellptr[slice_of_p]) % C
    defrow = np.minimum(rowof[np.minimum(slice_of_p * C + lane,
                                         nslices * C - 1)], nrows - 1)
    cols = defrow.astype(colidx.dtype)
    svals = np.zeros(total, dtype=np.float64)
    # scatter real entries: matrix row r sits at SELL row invperm[r]
    nnz = len(colidx)
    if perm is not None:
        invperm = np.empty(nslices * C, dtype=np.int64)
        invperm[rowof] = np.arange(nslices * C, dtype=np.int64)
        sellrow = invperm[:nrows]
    else:
        sellrow = np.arange(nrows, dtype=np.int64)
    rows = np.repeat(sellrow, counts)
    within = np.arange(nnz, dtype=np.int64) - rowptr[np.repeat(
        np.arange(nrows, dtype=np.int64), counts)]
    dst = sellptr[rows // C] + within * C + rows % C
    cols[dst] = colidx
    svals[dst] = vals
    if perm is not None:
        return sellptr, cols, svals, perm
    return sellptr, cols, svals


def sellcsr_split(rowptr, colidx, vals, cut: int = 192, C: int = 64,
                  window: int = 0, bucket: int = 8):
    """Split a CSR matrix by row length for the SELL+CSR hybrid format.

    Rows with len <= ``cut`` (the regular majority) go into a sigma-SELL
    structure; rows with len > cut (the power-law tail) stay CSR and are
    listed longest-first for the 64-lane vector kernel.  MEASURED motive
    (MI355X, 1M-row power-law): the pure binned hybrid spends 241 us/it
    in its 4-lane short-row bin -- 4-lane groups issue 16 scattered row
    streams per wave, while SELL's 64-lane slices load one contiguous
    512 B line set per step.

    ``window``: 0 = short rows globally length-descending (minimal
    padding, longest slices first).  W > 0 = sort by length only WITHIN
    windows of W consecutive short rows (original index order preserved
    across windows): slightly more padding, but the x gather keeps the
    source ordering's column locality -- the lever when the gather, not
    the vals/cols stream, bounds the SELL part.

    Returns (sellptr i64, cols, svals f64, perm int32 [sentinel n],
    rowlist_long int32 desc, nshort).  SELL part empty => sellptr len 1.
    """
    import numpy as np

    rowptr = np.asarray(rowptr)
    colidx = np.asarray(colidx)
    vals = np.asarray(vals)
    n = len(rowptr) - 1
    lens = np.diff(rowptr)
    order = np.argsort(-lens, kind="stable")
    slens = lens[order]
    nlong = int(np.searchsorted(-slens, -int(cut) - 1, side="right"))
    long_rows = order[:nlong].astype(np.int32)
    short_rows = order[nlong:].astype(np.int64)  # descending lengths
    if bucket and nlong and cut >= 96:
        # same line-sharing ordering for the tail.  Only when every long
        # row gets 64 lanes (cut >= 96): the bin builder derives bin
        # boundaries by searchsorted on descending lengths, which this
        # reorder would break for multi-bin tails.
        ll = lens[long_rows.astype(np.int64)]
        fc = colidx[rowptr[long_rows.astype(np.int64)]]
        bw = max(bucket * 8, 64)
        long_rows = long_rows[np.lexsort((fc, -((ll + bw - 1) // bw)))]
    if window and len(short_rows):
        sr = np.sort(short_rows)  # original index order
        out = np.empty_like(sr)
        for w0 in range(0, len(sr), window):
            w1 = min(w0 + window, len(sr))
            sub = np.argsort(-lens[sr[w0:w1]], kind="stable")
            out[w0:w1] = sr[w0:w1][sub]
        short_rows = out
    elif bucket and len(short_rows):
        # (length-bucket desc, first column asc): padding bounded by the
        # bucket width while rows inside a slice share nearby columns --
        # their 128 B x-line fetches overlap (the gather is the measured
        # bound: 50% L2 miss with 8-of-128-byte line use, see
        # profiles/irr_pmc_tcc_r02.txt)
        sl = lens[short_rows]
        firstcol = np.where(sl > 0, colidx[rowptr[short_rows]], 0)
        bkt = (sl + bucket - 1) // bucket
        order2 = np.lexsort((firstcol, -bkt))
        short_rows = short_rows[order2]
    nshort = len(short_rows)
    nslices = (nshort + C - 1) // C
    # SELL arrays over the short subset, slice lengths from the sorted order
    padlens = np.zeros(nslices * C, dtype=np.int64)
    padlens[:nshort] = lens[short_rows]
    slice_len = padlens.reshape(nslices, C).max(axis=1) if nslices else \
        np.zeros(0, np.int64)
    sellptr = np.zeros(nslices + 1, dtype=np.int64)
    np.cumsum(slice_len * C, out=sellptr[1:])
    total = int(sellptr[-1])
    perm = np.full(nslices * C, n, dtype=np.int32)
    perm[:nshort] = short_rows
    # defaults: pad cols point at a valid x slot, pad vals 0
    slice_of_p = np.repeat(np.arange(nslices, dtype=np.int64), slice_len * C)
    lane = (np.arange(total, dtype=np.int64) - sellptr[slice_of_p]) % C
    defrow = np.minimum(perm[np.minimum(slice_of_p * C + lane,
                                        max(nslices * C - 1, 0))], n - 1)
    cols = defrow.astype(colidx.dtype)
    svals = np.zeros(total, dtype=np.float64)
    # scatter the short rows' entries (vectorised: no per-row python loop)
    counts = lens[short_rows]
    rows_rep = np.repeat(np.arange(nshort, dtype=np.int64), counts)
    excl = np.zeros(nshort, dtype=np.int64)
    if nshort:
        np.cumsum(counts[:-1], out=excl[1:])
    within = np.arange(int(counts.sum()), dtype=np.int64) - excl[rows_rep]
    src = np.repeat(rowptr[short_rows], counts) + within
    dst = sellptr[rows_rep // C] + within * C + rows_rep % C
    cols[dst] = colidx[src]
    svals[dst] = vals[src]
    return sellptr, cols, svals, perm, long_rows, nshort


def bsell_from_csr(rowptr, colidx, vals, dof: int, C: int = 64):
    """Convert CSR -> Block-SELL (dense dof x dof blocks per node pair).

    Returns (bptr int64[nslices+1] in block units, bcol int32, bvals f64
    laid out [slice][j][k][64], density) or None when the matrix shape is
    not divisible by dof.  Blocks missing entries are zero-filled; the
    caller decides (via density) whether the 4->4/dof^2 B/nnz index saving
    beats the zero-fill cost."""
    import numpy as np

    rowptr = np.asarray(rowptr)
    colidx = np.asarray(colidx, dtype=np.int64)
    vals = np.asarray(vals)
    nrows = len(rowptr) - 1
    if dof < 2 or nrows % dof:
        return None
    nnodes = nrows // dof
    nnz = len(colidx)
    rows = np.repeat(np.arange(nrows, dtype=np.int64), np.diff(rowptr))
    try:
        from ..host import _acg_host as H

        blocks_per_node, bcols, inv = (np.asarray(a) for a in
                                       H.bsell_blocks(rowptr, colidx, dof))
        nblocks = len(bcols)
        bnode = np.repeat(np.arange(nnodes, dtype=np.int64), blocks_per_node)
    except ImportError:  # numpy fallback: O(nnz log nnz) unique
        node = rows // dof
        bcol_of_entry = colidx // dof
        key = node * (np.int64(1) << 32) | bcol_of_entry.astype(np.int64)
        uk, inv = np.unique(key, return_inverse=True)
        nblocks = len(uk)
        bnode = (uk >> 32).astype(np.int64)
        bcols = (uk & 0xFFFFFFFF).astype(np.int64)
        blocks_per_node = np.bincount(bnode, minlength=nnodes)
    density = nnz / (nblocks * dof * dof)
    nslices = (nnodes + C - 1) // C
    padlen = np.zeros(nslices * C, dtype=np.int64)
    padlen[:nnodes] = blocks_per_node
    slice_len = padlen.reshape(nslices, C).max(axis=1)
    bptr = np.zeros(nslices + 1, dtype=np.int64)
    np.cumsum(slice_len * C, out=bptr[1:])
    btotal = int(bptr[-1])
    # default: self block col (in-bounds), zero values
    slice_of_p = np.repeat(np.arange(nslices, dtype=np.int64), slice_len * C)
    lane = (np.arange(btotal, dtype=np.int64) - bptr[slice_of_p]) % C
    bcol = np.minimum(slice_of_p * C + lane, nnodes - 1).astype(np.int32)
    bvals = np.zeros(btotal * dof * dof, dtype=np.float64)
    # position of block b within its node's list (blocks sorted by key =>
    # grouped by node, ascending bcol)
    starts = np.zeros(nnodes + 1, dtype=np.int64)
    np.cumsum(blocks_per_node, out=starts[1:])
    within = np.arange(nblocks, dtype=np.int64) - starts[bnode]
    bdst = bptr[bnode // C] + within * C + bnode % C
    bcol[bdst] = bcols.astype(np.int32)
    # scatter entries into their block slots
    entry_block_dst = bdst[inv]
    k = (rows % dof) * dof + colidx % dof
    # bvals index, PAIR-major (see kernels.hip bval_off): element (j,k,lane)
    # at base_p*dof^2 + (k//2)*2C + lane*2 + k%2 for paired k, odd tail at
    # (dof^2-1)*C + lane
    lane_p = entry_block_dst % C
    base_p = entry_block_dst - lane_p
    D2 = dof * dof
    even = D2 & ~1
    off = np.where(k < even, (k >> 1) * (2 * C) + lane_p * 2 + (k & 1),
                   even * C + lane_p)
    vdst = base_p * D2 + off
    bvals[vdst] = vals
    return bptr, bcol, bvals, density


def spmv_sell(sellptr, cols, vals, nrows, x, y, *, rowbase: int = 0,
              accum: bool = False, partials=None, scal=None,
              dotslot: int = -1, dot_accum: bool = True, C: int = 64,
              variant=None, perm=None) -> None:
    """``variant`` only selects a kernel flavour on the GPU (same result);
    ``perm`` maps SELL row -> matrix row (sentinel nrows on pad lanes)."""
    vals = _vals64(vals, "spmv_sell")
    nslices = sellptr.numel() - 1
    assert (nrows + C - 1) // C == nslices, \
        f"SELL structure was built with a different chunk size than C={C}"
    contrib = torch.zeros(nrows, dtype=torch.float64, device=x.device)
    for s in range(nslices):
        base = int(sellptr[s])
        L = (int(sellptr[s + 1]) - base) // C
        block = (vals[base:base + L * C].view(L, C)
                 * x[cols[base:base + L * C].long()].view(L, C)).sum(dim=0)
        if perm is not None:
            rowof = perm[s * C:(s + 1) * C].long()
            ok = rowof < nrows
            contrib[rowof[ok]] = block[ok]
            continue
        hi = min(C, nrows - s * C)
        contrib[s * C:s * C + hi] = block[:hi]
    sl = slice(rowbase, rowbase + nrows)
    if accum:
        y[sl] += contrib
    else:
        y[sl] = contrib
    if scal is not None and dotslot >= 0:
        d = torch.dot(x[sl], contrib)
        scal[dotslot] = scal[dotslot] + d if dot_accum else d


def _bsell_contrib(bptr, bcol, bvals, nnodes: int, dof: int, xg, C: int = 64):
    """A @ xg for a Block-SELL matrix, decoding the pair-major bvals layout
    (kernels.hip bval_off): element (j, k, lane) of a slice sits at
    (k//2)*2C + lane*2 + k%2 inside block-column group j, the odd tail
    k = dof^2-1 at (dof^2-1)*C + lane; k = row_in_block*dof + col_in_block."""
    D2 = dof * dof
    even = D2 & ~1
    nslices = bptr.numel() - 1
    assert (nnodes + C - 1) // C == nslices, \
        f"BSELL structure was built with a different chunk size than C={C}"
    contrib = torch.zeros(nnodes * dof, dtype=torch.float64, device=xg.device)
    for s in range(nslices):
        b0 = int(bptr[s])
        L = (int(bptr[s + 1]) - b0) // C
        acc = torch.zeros(C, dof, dtype=torch.float64, device=xg.device)
        if L:
            cb = bcol[b0:b0 + L * C].view(L, C).long()
            v = bvals[b0 * D2:(b0 + L * C) * D2].view(L, D2 * C)
            for k in range(D2):
                if k < even:
                    lo = (k >> 1) * 2 * C + (k & 1)
                    a = v[:, lo:(k >> 1) * 2 * C + 2 * C:2]
                else:
                    a = v[:, even * C:even * C + C]
                acc[:, k // dof] += (a * xg[cb * dof + k % dof]).sum(dim=0)
        hi = min(C, nnodes - s * C)
        contrib[s * C * dof:(s * C + hi) * dof] = acc[:hi].reshape(-1)
    return contrib


def spmv_bsell(bptr, bcol, bvals, nnodes: int, dof: int, x, y, *,
               partials=None, scal=None, dotslot: int = -1,
               dot_accum: bool = True) -> None:
    bvals = _vals64(bvals, "spmv_bsell")
    if bptr.numel() - 1 <= 0:
        return
    n = nnodes * dof
    contrib = _bsell_contrib(bptr, bcol, bvals, nnodes, dof, x)
    y[:n] = contrib
    if scal is not None and dotslot >= 0:
        d = torch.dot(x[:n], contrib)
        scal[dotslot] = scal[dotslot] + d if dot_accum else d


def _spmv2_finish(c1, c2, owner_block, nblocks: int, n: int, x1, y1, y2, b,
                  partials) -> int:
    """Outputs and block partials of a dual SpMV from the two products;
    ``owner_block[row]`` is the 256-thread block (4 slices) that owns the
    row in the kernel, which fixes where its dot terms land."""
    o1 = b[:n] - c1 if b is not None else c1
    y1[:n] = o1
    y2[:n] = c2
    if partials is not None:
        xr = x1[:n]
        g = torch.zeros(nblocks, dtype=torch.float64, device=x1.device)
        d = torch.zeros(nblocks, dtype=torch.float64, device=x1.device)
        g.index_add_(0, owner_block, xr * xr)
        d.index_add_(0, owner_block, o1 * xr)
        partials[:nblocks] = g
        partials[MAXG:MAXG + nblocks] = d
    return nblocks


def spmv2_sell(sellptr, cols, vals, nrows, x1, x2, y1, y2, *, ncols: int,
               b=None, partials=None, perm=None, C: int = 64) -> int:
    """Dual SpMV (matches k_spmv2_sell): y1 = A x1 (b - A x1 with ``b``),
    y2 = A x2; with ``partials`` the per-block sums of (x1,x1) and (y1,x1)
    in partials[:nb] / partials[MAXG:MAXG + nb].  Returns nb."""
    if vals.dtype != torch.float64:
        raise TypeError(f"spmv2_sell: operator values must be float64, got {vals.dtype}")
    nslices = sellptr.numel() - 1
    if nslices <= 0 or nrows <= 0:
        return 0
    c1 = torch.zeros(nrows, dtype=torch.float64, device=x1.device)
    c2 = torch.zeros(nrows, dtype=torch.float64, device=x1.device)
    spmv_sell(sellptr, cols, vals, nrows, x1, c1, C=C, perm=perm)
    spmv_sell(sellptr, cols, vals, nrows, x2, c2, C=C, perm=perm)
    sellrow = torch.arange(nslices * C, device=x1.device)
    owner = torch.zeros(nrows, dtype=torch.int64, device=x1.device)
    if perm is not None:
        rowof = perm[:nslices * C].long()
        ok = rowof < nrows
        owner[rowof[ok]] = sellrow[ok] // (4 * C)
    else:
        owner[:] = sellrow[:nrows] // (4 * C)
    return _spmv2_finish(c1, c2, owner, (nslices + 3) // 4, nrows, x1, y1, y2,
                         b, partials)


def spmv2_bsell(bptr, bcol, bvals, nnodes: int, dof: int, x1, x2, y1, y2, *,
                ncols: int, b=None, partials=None, C: int = 64) -> int:
    """Dual Block-SELL SpMV (matches k_spmv2_bsell); see :func:`spmv2_sell`."""
    if bvals.dtype != torch.float64:
        raise TypeError(f"spmv2_bsell: operator values must be float64, got {bvals.dtype}")
    nslices = bptr.numel() - 1
    if nslices <= 0 or nnodes <= 0:
        return 0
    n = nnodes * dof
    c1 = _bsell_contrib(bptr, bcol, bvals, nnodes, dof, x1, C=C)
    c2 = _bsell_contrib(bptr, bcol, bvals, nnodes, dof, x2, C=C)
    owner = torch.arange(n, device=x1.device) // (dof * 4 * C)
    return _spmv2_finish(c1, c2, owner, (nslices + 3) // 4, n, x1, y1, y2, b,
                         partials)


def dot2_slices(r, w, nunits: int, dof: int, partials, *, perm=None,
                C: int = 64) -> int:
    """Block partials of (r,r) and (w,r) in the dual SpMV's block partition
    (matches k_dot2_slices).  Returns the number of blocks."""
    if nunits <= 0:
        return 0
    nslices = (nunits + C - 1) // C
    nblocks = (nslices + 3) // 4
    n = nunits * dof
    unit = torch.arange(nslices * C, device=r.device)
    owner = torch.zeros(nunits, dtype=torch.int64, device=r.device)
    if perm is not None:
        rowof = perm[:nslices * C].long()
        ok = rowof < nunits
        owner[rowof[ok]] = unit[ok] // (4 * C)
    else:
        owner[:] = unit[:nunits] // (4 * C)
    owner = owner.repeat_interleave(dof)
    g = torch.zeros(nblocks, dtype=torch.float64, device=r.device)
    d = torch.zeros(nblocks, dtype=torch.float64, device=r.device)
    g.index_add_(0, owner, r[:n] * r[:n])
    d.index_add_(0, owner, w[:n] * r[:n])
    partials[:nblocks] = g
    partials[MAXG:MAXG + nblocks] = d
    return nblocks


def pipelined_replace_finalize(partials, nblocks: int, scal) -> None:
    """scal[GAMMA] / scal[DELTA] from the two partial halves; nothing else
    (matches k_pipelined_replace_finalize)."""
    scal[S_GAMMA] = partials[:nblocks].sum()
    scal[S_DELTA] = partials[MAXG:MAXG + nblocks].sum()


def spmv_bsell_daypx(bptr, bcol, bvals, nnodes: int, dof: int, pold, rvec,
                     pnew, y, scal, partials, dotslot: int) -> None:
    """p_new = beta*p_old + r with beta = rr/rr_prev, y = A p_new, and
    scal[dotslot] = (p_new, y) (matches k_spmv_bsell_daypx + reduce)."""
    if bptr.numel() - 1 <= 0:
        return
    n = nnodes * dof
    beta = _sdiv(float(scal[S_RR]), float(scal[S_RR_PREV]))
    pn = beta * pold[:n] + rvec[:n]
    contrib = _bsell_contrib(bptr, bcol, bvals, nnodes, dof, pn)
    pnew[:n] = pn
    y[:n] = contrib
    scal[dotslot] = torch.dot(pn, contrib)


def spmv_bsell_st(st, x, y, *, partials=None, scal=None, dotslot: int = -1,
                  dot_accum: bool = True, max_blocks: int = 0) -> None:
    """y = A x on a BSELL-ST operator (ops/symtile.py), x and y in its
    permuted node order.  Follows k_spmv_bsell_st: own products first, the
    owner's A^T x_self lands in slot q of the partner, each node then adds
    its nrecv slots in slot order."""
    from .symtile import NOSEND, decode_st

    nn, dof = st.nnodes, st.dof
    n = nn * dof
    node, col, vals, q = decode_st(st)
    live = node < nn
    node, col, vals, q = node[live], col[live], vals[live], q[live]
    A = vals.view(-1, dof, dof)
    xb = x[:n].view(nn, dof)
    contrib = torch.zeros(nn, dof, dtype=torch.float64, device=x.device)
    contrib.index_add_(0, node, torch.einsum("brc,bc->br", A, xb[col]))
    snd = q != NOSEND
    slots = torch.zeros(max(st.qmax, 1), nn, dof, dtype=torch.float64,
                        device=x.device)
    slots[q[snd], col[snd]] = torch.einsum("brc,br->bc", A[snd], xb[node[snd]])
    nr = st.nrecv[:nn].long()
    for s in range(st.qmax):
        contrib += torch.where((nr > s)[:, None], slots[s], 0.0)
    contrib = contrib.reshape(-1)
    y[:n] = contrib
    if scal is not None and dotslot >= 0:
        d = torch.dot(x[:n], contrib)
        scal[dotslot] = scal[dotslot] + d if dot_accum else d


def cg_prep_pt(scal) -> None:
    scal[S_PT] = 0.0


def cg_prep_rr(scal) -> None:
    scal[S_RR_PREV] = scal[S_RR].clone()


def dot(x, y, partials, scal, slot, n=None, accumulate=False) -> None:
    n = x.numel() if n is None else n
    d = torch.dot(x[:n], y[:n])
    scal[slot] = scal[slot] + d if accumulate else d


def dot2(r, w, partials, scal, n, accumulate=False) -> None:
    g = torch.dot(r[:n], r[:n])
    d = torch.dot(w[:n], r[:n])
    if accumulate:
        scal[S_GAMMA] += g
        scal[S_DELTA] += d
    else:
        scal[S_GAMMA] = g
        scal[S_DELTA] = d


def _sdiv(a, b):
    # 0/0-safe coefficient division (see kernels.hip safe_div): a converged
    # solve driven past convergence underflows the recursion residual to
    # exact 0; dividing to 0 freezes the iterate instead of NaN-poisoning it
    return a / b if float(b) != 0.0 else torch.zeros_like(a) if torch.is_tensor(a) else 0.0


def axpy_ratio(y, x, scal, num, den, sign=1.0, n=None) -> None:
    n = y.numel() if n is None else n
    a = sign * _sdiv(float(scal[num]), float(scal[den]))
    y[:n] += a * x[:n]


def daypx_ratio(y, x, scal, num, den, n=None) -> None:
    n = y.numel() if n is None else n
    b = _sdiv(float(scal[num]), float(scal[den]))
    y[:n] = b * y[:n] + x[:n]


def cg_fused_update(r, x, p, t, scal, partials, n) -> None:
    """alpha = rr/pt; update r,x; then rotate rr->rr_prev and publish the
    new (r,r) (matches k_cg_fused_update + k_cg_finalize)."""
    alpha = _sdiv(float(scal[S_RR]), float(scal[S_PT]))
    r[:n] -= alpha * t[:n]
    x[:n] += alpha * p[:n]
    scal[S_RR_PREV] = scal[S_RR].clone()
    scal[S_RR] = torch.dot(r[:n], r[:n])


def pcg_fused_update(r, x, p, t, z, dinv, scal, partials, n) -> None:
    """Jacobi-PCG epilogue: alpha = rz/pt; update r,x; z = dinv*r; rotate
    rz -> rr_prev and publish the new rz in S_RR and the true (r,r) in
    S_GAMMA (matches k_pcg_fused_update + k_pcg_finalize)."""
    alpha = _sdiv(float(scal[S_RR]), float(scal[S_PT]))
    r[:n] -= alpha * t[:n]
    x[:n] += alpha * p[:n]
    z[:n] = dinv[:n] * r[:n]
    scal[S_RR_PREV] = scal[S_RR].clone()
    scal[S_RR] = torch.dot(r[:n], z[:n])
    scal[S_GAMMA] = torch.dot(r[:n], r[:n])


# -- block-Jacobi PCG on Block-SELL operators (same buffer layout as
# gpu_ops: dof(dof+1)/2 packed-upper components per node, row-major over
# (a <= b), stored [slice][component][64])

BJ_DOFS = (2, 3, 4)


def block_inv_len(nnodes: int, dof: int, C: int = 64) -> int:
    return ((nnodes + C - 1) // C) * (dof * (dof + 1) // 2) * C


def _bj_pairs(dof: int):
    return [(a, b) for a in range(dof) for b in range(a, dof)]


def unpack_block_inv(minv, nnodes: int, dof: int, C: int = 64):
    """Packed inverse blocks -> dense symmetric (nnodes, dof, dof)."""
    nc = dof * (dof + 1) // 2
    nslices = (nnodes + C - 1) // C
    if minv.numel() != nslices * nc * C:
        raise ValueError(f"unpack_block_inv: buffer has {minv.numel()} "
                         f"entries, needs {nslices * nc * C}")
    comp = minv.view(nslices, nc, C).permute(0, 2, 1).reshape(nslices * C, nc)
    out = torch.zeros(nnodes, dof, dof, dtype=minv.dtype, device=minv.device)
    for c, (a, b) in enumerate(_bj_pairs(dof)):
        out[:, a, b] = comp[:nnodes, c]
        out[:, b, a] = comp[:nnodes, c]
    return out


def pack_block_inv(blocks, C: int = 64):
    """Dense symmetric (nnodes, dof, dof) -> packed buffer (upper triangle
    taken); entries of the lanes past nnodes are zero."""
    nnodes, dof = blocks.shape[0], blocks.shape[1]
    nc = dof * (dof + 1) // 2
    nslices = (nnodes + C - 1) // C
    comp = torch.zeros(nslices * C, nc, dtype=blocks.dtype,
                       device=blocks.device)
    for c, (a, b) in enumerate(_bj_pairs(dof)):
        comp[:nnodes, c] = blocks[:, a, b]
    return comp.view(nslices, C, nc).permute(0, 2, 1).contiguous().view(-1)


def bsell_diag_blocks(bptr, bcol, bvals, nnodes: int, dof: int, C: int = 64):
    """(sum of every block of node i whose block column is i, how many
    such blocks there are) as (nnodes, dof, dof) and (nnodes,) tensors."""
    D2 = dof * dof
    even = D2 & ~1
    nslices = bptr.numel() - 1
    assert (nnodes + C - 1) // C == nslices, \
        f"BSELL structure was built with a different chunk size than C={C}"
    dev = bvals.device
    blocks = torch.zeros(nslices * C, D2, dtype=torch.float64, device=dev)
    found = torch.zeros(nslices * C, dtype=torch.int64, device=dev)
    lanes = torch.arange(C, device=dev)
    for s in range(nslices):
        b0 = int(bptr[s])
        L = (int(bptr[s + 1]) - b0) // C
        if not L:
            continue
        cb = bcol[b0:b0 + L * C].view(L, C).long()
        hit = cb == (s * C + lanes)[None, :]
        found[s * C:(s + 1) * C] = hit.sum(dim=0)
        v = bvals[b0 * D2:(b0 + L * C) * D2].view(L, D2 * C)
        for k in range(D2):
            if k < even:
                lo = (k >> 1) * 2 * C + (k & 1)
                a = v[:, lo:(k >> 1) * 2 * C + 2 * C:2]
            else:
                a = v[:, even * C:even * C + C]
            blocks[s * C:(s + 1) * C, k] = (a * hit).sum(dim=0)
    return blocks[:nnodes].view(nnodes, dof, dof), found[:nnodes]


def bsell_diag_inv(bptr, bcol, bvals, nnodes: int, dof: int):
    """Matches k_bsell_diag_inv: (packed inverse of every node's summed
    diagonal block, number of bad nodes).  A node is bad without a diagonal
    block or when a Cholesky pivot is <= 0 or not finite; its inverse is
    zero."""
    if dof not in BJ_DOFS:
        raise ValueError(f"bsell_diag_inv: dof must be one of {BJ_DOFS}, "
                         f"got {dof}")
    if bvals.dtype != torch.float64:
        raise TypeError(f"bsell_diag_inv: reads the float64 block values, "
                        f"got {bvals.dtype}")
    if nnodes == 0:
        return torch.zeros(0, dtype=torch.float64, device=bvals.device), 0
    D, found = bsell_diag_blocks(bptr, bcol, bvals, nnodes, dof)
    Lf, info = torch.linalg.cholesky_ex(D)
    ok = (found > 0) & (info == 0) & torch.isfinite(Lf).all(dim=(1, 2))
    eye = torch.eye(dof, dtype=torch.float64, device=D.device).expand_as(D)
    Lf = torch.where(ok[:, None, None], Lf, eye)
    inv = torch.cholesky_inverse(Lf)
    inv = torch.where(ok[:, None, None], inv, torch.zeros_like(inv))
    return pack_block_inv(inv), int((~ok).sum())


def _bj_mul(minv, v, n: int, dof: int):
    nnodes = n // dof
    if dof not in BJ_DOFS or n % dof:
        raise ValueError(f"block Jacobi: n={n} must be a multiple of dof "
                         f"in {BJ_DOFS}, got dof={dof}")
    if minv.numel() != block_inv_len(nnodes, dof):
        raise ValueError(f"block Jacobi: inverse buffer has {minv.numel()} "
                         f"entries, needs {block_inv_len(nnodes, dof)}")
    Mi = unpack_block_inv(minv, nnodes, dof)
    return torch.einsum("nab,nb->na", Mi, v[:n].view(nnodes, dof)).reshape(n)


def bjacobi_apply(minv, r, z, partials, scal, n: int, dof: int) -> None:
    """z = M^-1 r; rotate S_RR -> S_RR_PREV, publish (r,z) in S_RR and
    (r,r) in S_GAMMA (matches k_bjacobi_apply + k_pcg_finalize)."""
    z[:n] = _bj_mul(minv, r, n, dof)
    scal[S_RR_PREV] = scal[S_RR].clone()
    scal[S_RR] = torch.dot(r[:n], z[:n])
    scal[S_GAMMA] = torch.dot(r[:n], r[:n])


def bpcg_fused_update(r, x, p, t, z, minv, scal, partials, n: int,
                      dof: int) -> None:
    """Block-Jacobi PCG epilogue: alpha = rz/pt; update r,x; z = M^-1 r;
    rotate rz -> rr_prev and publish the new rz in S_RR and the true (r,r)
    in S_GAMMA (matches k_bpcg_fused_update + k_pcg_finalize)."""
    alpha = _sdiv(float(scal[S_RR]), float(scal[S_PT]))
    r[:n] -= alpha * t[:n]
    x[:n] += alpha * p[:n]
    z[:n] = _bj_mul(minv, r, n, dof)
    scal[S_RR_PREV] = scal[S_RR].clone()
    scal[S_RR] = torch.dot(r[:n], z[:n])
    scal[S_GAMMA] = torch.dot(r[:n], r[:n])


def _pipelined_coeffs(scal, first: bool):
    gamma = float(scal[S_GAMMA])
    delta = float(scal[S_DELTA])
    if first:
        return 0.0, _sdiv(gamma, delta)
    beta = _sdiv(gamma, float(scal[S_GAMMA_PREV]))
    alpha = _sdiv(gamma, delta - beta * _sdiv(gamma, float(scal[S_ALPHA_PREV])))
    return beta, alpha


def pipelined_fused(z, t, p, x, r, w, q, scal, partials, n, first: bool,
                    nt_update: bool = True) -> None:
    """Update the 6 vectors AND produce the next gamma/delta + rotate the
    scalar history (matches k_pipelined_fused + k_pipelined_finalize)."""
    beta, alpha = _pipelined_coeffs(scal, first)
    z[:n] = q[:n] + beta * z[:n]
    t[:n] = w[:n] + beta * t[:n]
    p[:n] = r[:n] + beta * p[:n]
    x[:n] += alpha * p[:n]
    r[:n] -= alpha * t[:n]
    w[:n] -= alpha * z[:n]
    scal[S_GAMMA_PREV] = scal[S_GAMMA].clone()
    scal[S_ALPHA_PREV] = alpha
    scal[S_GAMMA] = torch.dot(r[:n], r[:n])
    scal[S_DELTA] = torch.dot(w[:n], r[:n])


def sell_pipe(sellptr, cols, vals, nrows_pass: int, rowbase: int,
              border_base: int, w_old, qpart, z, t, p, x, r, w_new, scal,
              first: bool, partials, partials_off: int, mato: bool,
              C: int = 64) -> int:
    """One pass of the megafused pipelined iteration (matches k_sell_pipe).

    The matA pass (mato=False) updates rows below ``border_base`` and
    stores the partial q of the others into qpart[row - border_base]; the
    matO pass adds its ghost contributions to qpart and updates those rows.
    The pass's (r,r) and (w,r) sums go to partials[partials_off] and
    partials[MAXG + partials_off] for :func:`pipelined_finalize`, so
    ``partials`` needs 2*MAXG entries here; always one block per pass."""
    if nrows_pass == 0:
        return 0
    q = torch.zeros(rowbase + nrows_pass, dtype=torch.float64,
                    device=w_old.device)
    spmv_sell(sellptr, cols, vals, nrows_pass, w_old, q, rowbase=rowbase, C=C)
    beta, alpha = _pipelined_coeffs(scal, first)
    rows = torch.arange(rowbase, rowbase + nrows_pass, device=w_old.device)
    if mato:
        upd = rows
        qu = q[upd] + qpart[upd - border_base]
    else:
        defer = rows[rows >= border_base]
        qpart[defer - border_base] = q[defer]
        upd = rows[rows < border_base]
        qu = q[upd]
    zi = qu + beta * z[upd]
    ti = w_old[upd] + beta * t[upd]
    pi = r[upd] + beta * p[upd]
    z[upd] = zi
    t[upd] = ti
    p[upd] = pi
    x[upd] += alpha * pi
    rn = r[upd] - alpha * ti
    wn = w_old[upd] - alpha * zi
    r[upd] = rn
    w_new[upd] = wn
    partials[partials_off] = torch.dot(rn, rn)
    partials[MAXG + partials_off] = torch.dot(wn, rn)
    return 1


def _stencil_contrib(mf, nrows_nodes: int, row0_node: int, x, mato: bool):
    """Rows row0_node .. row0_node+nrows_nodes of the matrix-free stencil
    operator applied to the local vector ``x``: the owned couplings and the
    diagonal (mato=False) or the ghost-plane couplings alone (mato=True).
    Index arithmetic over the same pb/zs/offs tables the kernels read."""
    gx, gy, gz = mf["gx"], mf["gy"], mf["gz"]
    plane_nodes = gx * gy
    pb, zs = mf["pb"].long(), mf["zs"].long()
    offs = mf["offs"].view(-1, 4)
    node = torch.arange(row0_node, row0_node + nrows_nodes, dtype=torch.int64,
                        device=x.device)
    rem = node % plane_nodes
    xi, yi, zi = rem % gx, rem // gx, zs[node // plane_nodes]
    out = torch.zeros(nrows_nodes, dtype=torch.float64, device=x.device)
    if not mato:
        out += mf["diag"] * x[node]
    for o in range(mf["ksten"]):
        dx, dy, dz = (int(offs[o, k]) for k in range(3))
        nx, ny, nz = xi + dx, yi + dy, zi + dz
        ok = ((nx >= 0) & (nx < gx) & (ny >= 0) & (ny < gy)
              & (nz >= 0) & (nz < gz))
        base = pb[nz.clamp(0, gz - 1) + 1]
        ok &= base >= 0
        cn = base + nx + gx * ny
        ok &= (cn >= mf["nown_nodes"]) == mato
        out[ok] += offs[o, 3] * x[cn[ok]]
    return out


def stencil_spmv(mf, nrows_nodes: int, row0_node: int, x, y, *,
                 mato: bool = False, partials=None, scal=None,
                 dotslot: int = -1, dot_accum: bool = True) -> None:
    """Matrix-free stencil SpMV (matches k_stencil_spmv and, for 7-point
    stencils, the column walk k_stencil_spmv7): the matA pass stores the
    owned couplings, the matO pass adds the ghost couplings of its rows."""
    if nrows_nodes <= 0:
        return
    contrib = _stencil_contrib(mf, nrows_nodes, row0_node, x, mato)
    sl = slice(row0_node, row0_node + nrows_nodes)
    if mato:
        y[sl] += contrib
    else:
        y[sl] = contrib
    if scal is not None and dotslot >= 0:
        d = torch.dot(x[sl], contrib)
        scal[dotslot] = scal[dotslot] + d if dot_accum else d


def stencil_pipe(mf, nrows_nodes: int, row0_node: int, border_base: int,
                 w_old, qpart, z, t, p, x, r, w_new, scal, first: bool,
                 partials, partials_off: int, mato: bool) -> int:
    """One pass of the megafused matrix-free pipelined iteration (matches
    k_stencil_pipe / k_stencil_pipe7); same qpart / partials protocol as
    :func:`sell_pipe`, always one block per pass."""
    if nrows_nodes <= 0:
        return 0
    q = _stencil_contrib(mf, nrows_nodes, row0_node, w_old, mato)
    beta, alpha = _pipelined_coeffs(scal, first)
    rows = torch.arange(row0_node, row0_node + nrows_nodes, device=w_old.device)
    if mato:
        upd = rows
        qu = q + qpart[upd - border_base]
    else:
        defer = rows >= border_base
        qpart[rows[defer] - border_base] = q[defer]
        upd = rows[~defer]
        qu = q[~defer]
    zi = qu + beta * z[upd]
    ti = w_old[upd] + beta * t[upd]
    pi = r[upd] + beta * p[upd]
    z[upd] = zi
    t[upd] = ti
    p[upd] = pi
    x[upd] += alpha * pi
    rn = r[upd] - alpha * ti
    wn = w_old[upd] - alpha * zi
    r[upd] = rn
    w_new[upd] = wn
    partials[partials_off] = torch.dot(rn, rn)
    partials[MAXG + partials_off] = torch.dot(wn, rn)
    return 1


def pipelined_finalize(partials, nblocks: int, scal, first: bool) -> None:
    """Rotate gamma -> gamma_prev, store alpha -> alpha_prev, publish the
    summed partials as the new gamma/delta (matches k_pipelined_finalize)."""
    _, alpha = _pipelined_coeffs(scal, first)
    g = partials[:nblocks].sum()
    d = partials[MAXG:MAXG + nblocks].sum()
    scal[S_GAMMA_PREV] = scal[S_GAMMA].clone()
    scal[S_ALPHA_PREV] = alpha
    scal[S_GAMMA] = g
    scal[S_DELTA] = d


BAR_STATE_WORDS = 400  # same as gpu_ops; the reference needs no barrier


def cg_device(sellptr, cols, vals, nrows: int, b, x, r, p, t, scal, partials,
              out2, barrier_state, maxits: int, res_atol: float,
              res_rtol: float, hier=None) -> int:
    """Whole classic CG solve in one call (matches k_cg_device): bnrm2 =
    (b,b); r = p = b - A x; then alpha = rr/(p,t), x += alpha p,
    r -= alpha t, beta = rr'/rr, p = beta p + r until rr <= max(atol,
    rtol*|b|)^2 or ``maxits`` steps.  Publishes (b,b), (r0,r0), the last
    (p,t) and the final (r,r) in S_BNRM2, S_RR_PREV, S_PT and S_RR, and
    (niterations, converged) in ``out2``.  Every 256 rows form a block whose
    partial sum of the last reduction is left in ``partials`` when that has
    room; returns the number of blocks."""
    if vals.dtype != torch.float64:
        raise ValueError(f"cg_device: operator values must be float64, got {vals.dtype}")
    nslices = sellptr.numel() - 1
    n = nrows
    grid = (nslices * 64 + 255) // 256

    def gsum(v, slot):
        part = torch.stack([v[i:i + 256].sum() for i in range(0, grid * 256, 256)])
        if partials.numel() >= grid:
            partials[:grid] = part
        scal[slot] = part.sum()

    gsum(b[:n] * b[:n], S_BNRM2)
    spmv_sell(sellptr, cols, vals, n, x, t)
    r[:n] = b[:n] - t[:n]
    p[:n] = r[:n]
    gsum(r[:n] * r[:n], S_RR)
    scal[S_RR_PREV] = scal[S_RR].clone()
    rr = float(scal[S_RR])
    rt = max(res_rtol * math.sqrt(float(scal[S_BNRM2])), res_atol)
    rtol2 = rt * rt
    k = 0
    converged = rtol2 > 0.0 and rr <= rtol2
    while not converged and k < maxits:
        spmv_sell(sellptr, cols, vals, n, p, t)
        gsum(p[:n] * t[:n], S_PT)
        alpha = _sdiv(rr, float(scal[S_PT]))
        r[:n] -= alpha * t[:n]
        x[:n] += alpha * p[:n]
        gsum(r[:n] * r[:n], S_RR)
        rr_new = float(scal[S_RR])
        p[:n] = _sdiv(rr_new, rr) * p[:n] + r[:n]
        rr = rr_new
        k += 1
        converged = rtol2 > 0.0 and rr <= rtol2
    out2[0] = k
    out2[1] = 1 if converged else 0
    return grid


# ---------------------------------------------------------------------------
# Multiple right-hand sides (same layout as gpu_ops: (n, K) multivectors,
# (K, S_NSLOTS) slab, (K, MAXG) partials).  Every column is computed by the
# single-vector reference above, so a column of a multi op IS the single op.

MULTI_K = (2, 4, 8)


def alloc_scalars_multi(device, k: int) -> torch.Tensor:
    return torch.zeros(k, S_NSLOTS, dtype=torch.float64, device=device)


def alloc_partials_multi(device, k: int) -> torch.Tensor:
    return torch.zeros(k, MAXG, dtype=torch.float64, device=device)


def _multi_k(what: str, *mvs, rows=None) -> int:
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
        if rows is not None and v.shape[0] < rows:
            raise ValueError(f"{what}: multivector has {v.shape[0]} rows, "
                             f"needs at least {rows}")
    return k


def spmm_bsell_supported(dof: int, k: int) -> bool:
    return dof in (2, 3, 4) and k in MULTI_K


def spmm_sell(sellptr, cols, vals, nrows, X, Y, *, partials=None, scal=None,
              dotslot: int = -1, dot_accum: bool = False, perm=None) -> None:
    k = _multi_k("spmm_sell", X, Y, rows=nrows)
    if vals.dtype != torch.float64:
        raise TypeError(f"spmm_sell: operator values must be float64, got {vals.dtype}")
    if sellptr.numel() - 1 <= 0:
        return
    fuse = scal is not None and dotslot >= 0
    for c in range(k):
        y = torch.empty(nrows, dtype=torch.float64, device=X.device)
        spmv_sell(sellptr, cols, vals, nrows, X[:, c].contiguous(), y,
                  scal=scal.view(-1, S_NSLOTS)[c] if fuse else None,
                  dotslot=dotslot, dot_accum=dot_accum, perm=perm)
        Y[:nrows, c] = y


def spmm_bsell(bptr, bcol, bvals, nnodes: int, dof: int, X, Y, *,
               partials=None, scal=None, dotslot: int = -1,
               dot_accum: bool = False) -> None:
    n = nnodes * dof
    k = _multi_k("spmm_bsell", X, Y, rows=n)
    if bvals.dtype != torch.float64:
        raise TypeError(f"spmm_bsell: operator values must be float64, got {bvals.dtype}")
    if not spmm_bsell_supported(dof, k):
        raise ValueError(f"spmm_bsell: no kernel for dof={dof}, K={k}")
    if bptr.numel() - 1 <= 0:
        return
    fuse = scal is not None and dotslot >= 0
    for c in range(k):
        y = torch.empty(n, dtype=torch.float64, device=X.device)
        spmv_bsell(bptr, bcol, bvals, nnodes, dof, X[:, c].contiguous(), y,
                   scal=scal.view(-1, S_NSLOTS)[c] if fuse else None,
                   dotslot=dotslot, dot_accum=dot_accum)
        Y[:n, c] = y


def dot_multi(X, Y, partials, scal, slot, n=None, accumulate=False) -> None:
    n = X.shape[0] if n is None else n
    k = _multi_k("dot_multi", X, Y, rows=n)
    sc = scal.view(-1, S_NSLOTS)
    for c in range(k):
        d = torch.dot(X[:n, c], Y[:n, c])
        sc[c, slot] = sc[c, slot] + d if accumulate else d


def reduce_partials_multi(partials, nblocks: int, scal, slot,
                          accumulate=False) -> None:
    sc = scal.view(-1, S_NSLOTS)
    pp = partials.view(-1, MAXG)
    for c in range(sc.shape[0]):
        d = pp[c, :nblocks].sum()
        sc[c, slot] = sc[c, slot] + d if accumulate else d


def cg_fused_update_multi(R, X, P, T, scal, partials, n) -> int:
    """Matches k_cg_fused_update_multi: the new (r, r) of column c is left
    in partials[c, 0] (always one block here); returns 1."""
    k = _multi_k("cg_fused_update_multi", R, X, P, T, rows=n)
    sc = scal.view(-1, S_NSLOTS)
    pp = partials.view(-1, MAXG)
    for c in range(k):
        alpha = _sdiv(float(sc[c, S_RR]), float(sc[c, S_PT]))
        R[:n, c] -= alpha * T[:n, c]
        X[:n, c] += alpha * P[:n, c]
        pp[c, 0] = torch.dot(R[:n, c], R[:n, c])
    return 1


def cg_finalize_multi(partials, nblocks: int, scal, rr_out) -> None:
    sc = scal.view(-1, S_NSLOTS)
    pp = partials.view(-1, MAXG)
    for c in range(sc.shape[0]):
        v = pp[c, :nblocks].sum()
        sc[c, S_RR_PREV] = sc[c, S_RR].clone()
        sc[c, S_RR] = v
        rr_out[c] = v


def daypx_ratio_multi(P, R, scal, num: int = S_RR, den: int = S_RR_PREV,
                      n=None) -> None:
    n = R.shape[0] if n is None else n
    k = _multi_k("daypx_ratio_multi", P, R, rows=n)
    sc = scal.view(-1, S_NSLOTS)
    for c in range(k):
        b = _sdiv(float(sc[c, num]), float(sc[c, den]))
        P[:n, c] = b * P[:n, c] + R[:n, c]


# ---------------------------------------------------------------------------
# Block CG (same state layout as kernels.hip: every small matrix owns an
# 8 x 8 row-major region of the BS_SIZE-slot fp64 state tensor, a width-K
# op touches the leading K x K entries; Gram partials of pair p = (a <= b),
# row-major over the upper triangle, at partials[p*BLOCK_MAXG + block]).

BS_LD = 8
BS_M, BS_XI, BS_XIC, BS_G, BS_ZETA, BS_ZINV, BS_C = 0, 64, 128, 192, 256, 320, 384
BS_FLAG, BS_ITER, BS_SIZE = 448, 449, 456
BLOCK_MAXG = 2048
BLOCK_TAU = 1e-6


def alloc_block_state(device="cpu") -> torch.Tensor:
    return torch.zeros(BS_SIZE, dtype=torch.float64, device=device)


def _block_region(state, base: int, k: int):
    """Writable (k, k) view of one matrix of the state."""
    return state[base:base + BS_LD * BS_LD].view(BS_LD, BS_LD)[:k, :k]


def _block_pairs(k: int):
    return [(a, b) for a in range(k) for b in range(a, k)]


def _block_write_partials(G, partials, k: int) -> int:
    flat = partials.view(-1)
    for p, (a, b) in enumerate(_block_pairs(k)):
        flat[p * BLOCK_MAXG] = G[a, b]
    return 1


def _block_sym(partials, nblocks: int, k: int, kg: int):
    """Symmetric (k, k) Gram from the partials of its upper triangle; rows
    and columns >= kg are the identity."""
    flat = partials.view(-1)
    g = torch.eye(k, dtype=torch.float64)
    for p, (a, b) in enumerate(_block_pairs(k)):
        if b < kg:
            v = float(flat[p * BLOCK_MAXG:p * BLOCK_MAXG + nblocks].sum())
            g[a, b] = v
            g[b, a] = v
    return g


def _block_chol(g, kg: int):
    """Pivot-tested Cholesky g = l l^T of the leading kg x kg block, the
    rest of l the identity; None on breakdown (pivot d_j not finite or
    d_j <= BLOCK_TAU * g_jj)."""
    k = g.shape[0]
    l = [[1.0 if i == j else 0.0 for j in range(k)] for i in range(k)]
    for j in range(kg):
        d = float(g[j, j])
        for q in range(j):
            d -= l[j][q] * l[j][q]
        if not math.isfinite(d) or not d > BLOCK_TAU * float(g[j, j]):
            return None
        ljj = math.sqrt(d)
        l[j][j] = ljj
        for i in range(j + 1, kg):
            s = float(g[i, j])
            for q in range(j):
                s -= l[i][q] * l[j][q]
            l[i][j] = s / ljj
    return torch.tensor(l, dtype=torch.float64)


def _block_newc(zeta, C):
    return zeta @ C


def _block_flagged(state) -> bool:
    return float(state[BS_FLAG]) != 0.0


def gram_multi(X, Y, partials, n=None) -> int:
    """Upper triangle of X[:n]^T Y[:n] as ONE block of partials; returns 1."""
    n = X.shape[0] if n is None else n
    k = _multi_k("gram_multi", X, Y, rows=n)
    return _block_write_partials(X[:n].T @ Y[:n], partials, k)


def block_update(X, S, Q, T, state, partials, n) -> int:
    k = _multi_k("block_update", X, S, Q, T, rows=n)
    if _block_flagged(state):
        return 1
    xi = _block_region(state, BS_XI, k)
    xic = _block_region(state, BS_XIC, k)
    X[:n] += S[:n] @ xic
    Q[:n] -= T[:n] @ xi
    return _block_write_partials(Q[:n].T @ Q[:n], partials, k)


def block_ortho(Q, S, state, n) -> None:
    k = _multi_k("block_ortho", Q, S, rows=n)
    if _block_flagged(state):
        return
    Q[:n] = Q[:n] @ _block_region(state, BS_ZINV, k)
    S[:n] = Q[:n] + S[:n] @ _block_region(state, BS_ZETA, k).T


def block_coef_alpha(partials, nblocks: int, state, k: int, kg: int,
                     it: int) -> None:
    if _block_flagged(state):
        return
    m = _block_sym(partials, nblocks, k, kg)
    l = _block_chol(m, kg)
    _block_region(state, BS_M, k).copy_(m)
    if l is None:
        state[BS_FLAG] = 1.0
        state[BS_ITER] = float(it)
        return
    # column c: L y = e_c, L^T x = y (the kernel's order of operations)
    xi = torch.eye(k, dtype=torch.float64)
    for c in range(kg):
        for i in range(c, kg):
            s = 1.0 if i == c else 0.0
            for q in range(c, i):
                s -= float(l[i, q]) * float(xi[q, c])
            xi[i, c] = s / float(l[i, i])
        for i in range(kg - 1, -1, -1):
            s = float(xi[i, c])
            for q in range(i + 1, kg):
                s -= float(l[q, i]) * float(xi[q, c])
            xi[i, c] = s / float(l[i, i])
    C = _block_region(state, BS_C, k)
    _block_region(state, BS_XIC, k).copy_(xi @ C)
    _block_region(state, BS_XI, k).copy_(xi)


def block_coef_beta(partials, nblocks: int, state, rr_out, k: int, kg: int,
                    it: int, init: bool = False) -> None:
    if _block_flagged(state):
        rr_out[k] = state[BS_FLAG].clone()
        rr_out[k + 1] = state[BS_ITER].clone()
        return
    g = _block_sym(partials, nblocks, k, kg)
    l = _block_chol(g, kg)
    _block_region(state, BS_G, k).copy_(g)
    if l is None:
        state[BS_FLAG] = 1.0
        state[BS_ITER] = float(it)
        rr_out[k] = 1.0
        rr_out[k + 1] = float(it)
        return
    zeta = l.T.contiguous()
    zi = torch.eye(k, dtype=torch.float64)
    for c in range(kg):
        for i in range(c, -1, -1):
            s = 1.0 if i == c else 0.0
            for q in range(i + 1, c + 1):
                s -= float(zeta[i, q]) * float(zi[q, c])
            zi[i, c] = s / float(zeta[i, i])
    C = _block_region(state, BS_C, k)
    cn = zeta.clone() if init else _block_newc(zeta, C.clone())
    _block_region(state, BS_ZETA, k).copy_(zeta)
    _block_region(state, BS_ZINV, k).copy_(zi)
    C.copy_(cn)
    for c in range(kg):
        rr_out[c] = float((cn[:, c] * cn[:, c]).sum())
    rr_out[k] = 0.0
    rr_out[k + 1] = -1.0


def pack_gather(sendbuf, x, idx) -> None:
    torch.index_select(x, 0, idx.long(), out=sendbuf)
