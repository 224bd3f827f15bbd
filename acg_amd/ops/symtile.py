"""BSELL-ST: tile-symmetric Block-SELL, built from an existing BSELL.

A symmetric operator in Block-SELL stores ``A_ij`` and ``A_ji = A_ij^T``.
BSELL-ST keeps a pair once when both nodes fall into the same tile of
``tile`` consecutive nodes (one workgroup of ``k_spmv_bsell_st``): the
owner's block carries a slot number ``q``; the kernel hands ``A^T x_owner``
to the partner through LDS slot ``q`` and the partner adds its ``nrecv``
slots in slot order.  Everything here is torch index arithmetic and runs
on whichever device the BSELL arrays live on.

Steps (``new0`` = position in the caller's ``node_order``):

1. decode the BSELL into a block list, renumber to new0, sort by
   (row node, column node); a duplicated block refuses the build;
2. every in-tile block ``(i, j)``, ``i != j``, must have a partner that is
   its bitwise transpose, else the build refuses (returns ``None``);
3. ownership in synchronous rounds: a pair may be claimed by the endpoint
   that currently stores MORE blocks (ties: the lower index) -- the other
   endpoint, holding fewer, keeps the pair -- unless that endpoint has
   reached ``qmax`` receives, then by the other one; every node accepts at
   most one claim per round (smallest fixed pseudo-random priority), so
   receives stay balanced and the result does not depend on timing.  Pairs
   nobody may claim any more stay stored on both sides as plain blocks;
4. inside each tile nodes are sorted by stored-block count, descending
   (stable), before 64-lane slices are cut; the final permutation is the
   composition with ``node_order``;
5. a receiver's slots are numbered by ascending owner index;
6. per node: plain blocks, then sending blocks, each by ascending column.
   A slice's first ``spl[s]`` block columns are plain in every lane and
   are read without the slot byte; padding is a zero block with the
   node's own column and slot ``NOSEND``;
7. the byte gate: ``stored_bytes > gate * bsell_bytes`` refuses.
"""

from __future__ import annotations

from types import SimpleNamespace

import torch

C = 64
TILE = 256
QMAX = 8
GATE = 0.9
NOSEND = 255


def val_index(pos: torch.Tensor, lane: torch.Tensor, d2: int) -> torch.Tensor:
    """Index of element k of the block at storage position ``pos`` (lane
    ``lane`` of its slice) in the pair-major value array: shape
    (len(pos), d2).  Same formula as ``bval_off`` in kernels.hip."""
    k = torch.arange(d2, device=pos.device)[None, :]
    even = d2 & ~1
    lane = lane[:, None]
    off = torch.where(k < even, (k >> 1) * (2 * C) + lane * 2 + (k & 1),
                      even * C + lane)
    return (pos[:, None] - lane) * d2 + off


def stored_bytes(nblocks: int, nslot_bytes: int, nslices: int, d2: int) -> int:
    """Bytes one BSELL-ST SpMV reads of the operator: blocks (values + one
    int32 column each), slot bytes of the sending section, one receive
    count per lane, slice pointers and plain-section lengths."""
    return (nblocks * (8 * d2 + 4) + nslot_bytes + nslices * C
            + (nslices + 1) * 8 + nslices * 4)


def bsell_bytes(nblocks: int, nslices: int, d2: int) -> int:
    return nblocks * (8 * d2 + 4) + (nslices + 1) * 8


def _decode(ptr, col, vals, nnodes, d2):
    """(node, column, values[., d2], storage position) of every stored
    block of a BSELL-shaped array set, dead lanes included."""
    nsl = ptr.numel() - 1
    dev = ptr.device
    pos = torch.arange(int(ptr[-1]), device=dev)
    sl = torch.repeat_interleave(torch.arange(nsl, device=dev), ptr[1:] - ptr[:-1])
    lane = (pos - ptr[sl]) % C
    return sl * C + lane, col.long(), vals[val_index(pos, lane, d2)], pos, sl


def bsell_st_build(bptr, bcol, bvals, nnodes: int, dof: int, node_order=None,
                   *, tile: int = TILE, qmax: int = QMAX, gate: float = GATE):
    """Build BSELL-ST (module docstring) or return ``None`` when the
    operator is not pairwise transposed inside a tile, holds a block twice,
    or the byte gate fails.  ``node_order[new] = old`` is the caller's
    node order (default: the given one)."""
    if bvals.dtype != torch.float64:
        raise TypeError(f"bsell_st_build: float64 block values, got {bvals.dtype}")
    if not 0 <= qmax < NOSEND:
        raise ValueError(f"bsell_st_build: qmax must be in [0, {NOSEND})")
    if tile < 1 or (tile > C and tile % C):
        raise ValueError("bsell_st_build: tile must be a multiple of 64 (or < 64)")
    dev = bptr.device
    d2 = dof * dof
    nsl = bptr.numel() - 1
    if nnodes <= 0 or nsl != (nnodes + C - 1) // C:
        raise ValueError("bsell_st_build: bptr does not match nnodes")
    ar = torch.arange(nnodes, device=dev)
    if node_order is None:
        order = ar
    else:
        order = torch.as_tensor(node_order).to(dev).long()
        if order.shape != (nnodes,) or not torch.equal(order.sort().values, ar):
            raise ValueError("bsell_st_build: node_order is not a permutation")
    inv0 = torch.empty_like(order)
    inv0[order] = ar

    # 1. block list in new0 numbering, sorted by (row node, column node)
    node, col, vals, _, _ = _decode(bptr, bcol, bvals, nnodes, d2)
    real = (node < nnodes) & (vals != 0).any(dim=1)
    i0, j0, vals = inv0[node[real]], inv0[col[real]], vals[real]
    key, srt = torch.sort(i0 * nnodes + j0)
    if key.numel() > 1 and bool((key[1:] == key[:-1]).any()):
        return None
    i0, j0, vals = i0[srt], j0[srt], vals[srt]
    nb = key.numel()

    # 2. every in-tile off-diagonal block needs its bitwise transpose
    e = torch.nonzero((i0 // tile == j0 // tile) & (i0 != j0)).squeeze(1)
    if e.numel():
        pkey = j0[e] * nnodes + i0[e]
        pidx = torch.searchsorted(key, pkey).clamp_(max=nb - 1)
        if not bool((key[pidx] == pkey).all()):
            return None
        vt = vals[e].view(-1, dof, dof).transpose(1, 2).reshape(-1, d2).contiguous()
        if not torch.equal(vt.view(torch.int64),
                           vals[pidx].contiguous().view(torch.int64)):
            return None
        low = i0[e] < j0[e]
        blo, bhi = e[low], pidx[low]  # blocks (a, b) and (b, a), a < b
    else:
        blo = bhi = e
    a, b = i0[blo], j0[blo]
    npairs = blo.numel()

    # 3. ownership rounds
    stored = torch.bincount(i0, minlength=nnodes)
    got = torch.zeros(nnodes, dtype=torch.int64, device=dev)
    recv = torch.full((npairs,), -1, dtype=torch.int64, device=dev)
    pid = torch.arange(npairs, device=dev)
    prio = (((pid * 2654435761) & 0x7FFFFFFF) << 32) | pid
    big = torch.iinfo(torch.int64).max
    for _ in range(8 * qmax + 8 if npairs and qmax else 0):
        capa, capb = got[a] >= qmax, got[b] >= qmax
        sa, sb = stored[a], stored[b]
        a_claims = ~capa & ((sa >= sb) | capb)
        b_claims = ~capb & ((sb > sa) | capa)
        who = torch.where(a_claims, a, torch.where(b_claims, b, -1))
        cand = (recv < 0) & (who >= 0)
        if not bool(cand.any()):
            break
        best = torch.full((nnodes,), big, dtype=torch.int64, device=dev)
        best.scatter_reduce_(0, who[cand], prio[cand], "amin")
        win = cand & (best[who.clamp(min=0)] == prio)
        recv[win] = torch.where(who == a, 0, 1)[win]
        w = who[win]  # one claim per node and round: plain indexing is safe
        stored[w] -= 1
        got[w] += 1
    done = recv >= 0
    a_recv = recv == 0
    # the receiver's block is dropped, the owner's block sends
    drop_b = torch.where(a_recv, blo, bhi)[done]
    send_b = torch.where(a_recv, bhi, blo)[done]
    receiver0 = torch.where(a_recv, a, b)[done]
    owner0 = torch.where(a_recv, b, a)[done]

    # 4. in-tile sort by stored count, descending, stable
    cmax = int(stored.max())
    order1 = torch.sort((ar // tile) * (cmax + 1) + (cmax - stored),
                        stable=True).indices  # order1[new1] = new0
    inv1 = torch.empty_like(order1)
    inv1[order1] = ar
    perm = order[order1]  # perm[new1] = old
    iperm = torch.empty_like(perm)
    iperm[perm] = ar

    # 5. slot numbers: a receiver's owners in ascending (final) order
    q = torch.full((nb,), NOSEND, dtype=torch.int64, device=dev)
    nrecv = torch.zeros(nsl * C, dtype=torch.int64, device=dev)
    if send_b.numel():
        r1, o1 = inv1[receiver0], inv1[owner0]
        rk, rs = torch.sort(r1 * nnodes + o1)
        r1s = r1[rs]
        cnt = torch.bincount(r1s, minlength=nnodes)
        start = torch.cumsum(cnt, 0) - cnt
        q[send_b[rs]] = torch.arange(rs.numel(), device=dev) - start[r1s]
        nrecv[:nnodes] = cnt
    assert int(nrecv.max()) <= qmax

    # 6. kept blocks per node: plain, then sending, by ascending column
    keep = torch.ones(nb, dtype=torch.bool, device=dev)
    keep[drop_b] = False
    i1, j1, vals, q = inv1[i0[keep]], inv1[j0[keep]], vals[keep], q[keep]
    sends = (q != NOSEND).long()
    srt = torch.sort((i1 * 2 + sends) * nnodes + j1).indices
    i1, j1, vals, q, sends = i1[srt], j1[srt], vals[srt], q[srt], sends[srt]
    total = torch.bincount(i1, minlength=nnodes)
    nplain = total - torch.bincount(i1, weights=sends.double(),
                                    minlength=nnodes).long()
    within = torch.arange(i1.numel(), device=dev) - (torch.cumsum(total, 0) - total)[i1]
    pad = torch.zeros(nsl * C, dtype=torch.int64, device=dev)
    pad[:nnodes] = total
    blen = pad.view(nsl, C).max(dim=1).values
    pad.fill_(big)
    pad[:nnodes] = nplain
    spl = torch.minimum(pad.view(nsl, C).min(dim=1).values, blen)
    sptr = torch.zeros(nsl + 1, dtype=torch.int64, device=dev)
    torch.cumsum(blen * C, dim=0, out=sptr[1:])
    stotal = int(sptr[-1])
    pos = torch.arange(stotal, device=dev)
    sl = torch.repeat_interleave(torch.arange(nsl, device=dev), blen * C)
    lane = (pos - sptr[sl]) % C
    scol = torch.clamp(sl * C + lane, max=nnodes - 1).to(torch.int32)
    sq = torch.full((stotal,), NOSEND, dtype=torch.uint8, device=dev)
    svals = torch.zeros(stotal * d2, dtype=torch.float64, device=dev)
    dst = sptr[i1 // C] + within * C + i1 % C
    scol[dst] = j1.to(torch.int32)
    sq[dst] = q.to(torch.uint8)
    svals[val_index(dst, i1 % C, d2)] = vals
    # kernel invariants: a sending block sits in the slot-byte section and
    # targets a node of its own tile
    snd = q != NOSEND
    assert bool((within[snd] >= spl[i1[snd] // C]).all())
    assert bool((j1[snd] // tile == i1[snd] // tile).all())

    # 7. byte gate
    nslot = int(((blen - spl) * C).sum())
    sbytes = stored_bytes(stotal, nslot, nsl, d2)
    bbytes = bsell_bytes(int(bptr[-1]), nsl, d2)
    if sbytes > gate * bbytes:
        return None
    dofs = torch.arange(dof, device=dev)
    return SimpleNamespace(
        sptr=sptr, spl=spl.to(torch.int32), scol=scol, sq=sq, svals=svals,
        nrecv=nrecv.to(torch.uint8), perm=perm, iperm=iperm,
        vperm=(perm[:, None] * dof + dofs[None, :]).reshape(-1),
        nnodes=nnodes, dof=dof, tile=tile, qmax=qmax,
        ntiles=(nnodes + tile - 1) // tile, nslices=nsl,
        nblocks=stotal, nslot_bytes=nslot, stored_bytes=sbytes,
        bsell_bytes=bbytes, ratio=sbytes / bbytes,
        npairs=int(npairs), npaired=int(send_b.numel()))


def decode_st(st):
    """Stored blocks of a BSELL-ST: (node, column, values[., d2], slot)
    per storage position, dead lanes and padding included; slot is
    ``NOSEND`` in the plain section whatever the byte array holds there."""
    d2 = st.dof * st.dof
    node, col, vals, pos, sl = _decode(st.sptr, st.scol, st.svals, st.nnodes, d2)
    j = (pos - st.sptr[sl]) // C
    q = torch.where(j >= st.spl.long()[sl], st.sq.long(),
                    torch.full_like(j, NOSEND))
    return node, col, vals, q
