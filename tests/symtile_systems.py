"""Shared inputs, oracle and kernel emulation of the BSELL-ST tests.

Plain helper module (not a conftest).

* systems: the rotated-anisotropy ``A = L B L^T`` of tests/bjacobi_systems.py
  (its off-diagonal blocks are NOT symmetric, so a missing transpose shows)
  on G^3 grids, plus the same recipe on a 3 x 127 x 1 strip: 381 nodes = two
  256-node tiles with 61 live lanes in the last slice;
* oracle: ``A x`` from the ORIGINAL CSR in long double with the Block-SELL
  bound ``(L_i + 48) 2^-53 M_i`` of tests/kernel_oracle.py; ``L_i`` is the
  BSELL one -- BSELL-ST sums the same products in another order;
* ``run_spmv`` drives torch_ref on the CPU and gpu_ops on the GPU on
  NaN-poisoned ``y`` and ``partials``;
* ``emulate`` replays k_spmv_bsell_st step by step in numpy, with the
  mutants the CPU tests must see rejected.
"""

from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np
import torch

import bjacobi_systems as bs
import kernel_oracle as ko
from acg_amd.ops import symtile

NANBITS = np.array([np.nan]).view(np.int64)[0]
TAIL = 96  # NaN-prefilled doubles behind y that must stay untouched
CUBES = (3, 5, 12)  # 27, 125, 1728 nodes
STRIP = (3, 127, 1)  # 381 nodes
DOFS = (2, 3, 4)
ORDERS = ("brick", "natural")
MUTANTS = ("no_transpose", "slot_collision", "short_sum", "inverse_perm",
           "overcap_dropped")


@functools.lru_cache(maxsize=None)
def system(shape, dof):
    """Namespace (nnodes, n, dof, shape, S) of the rotated system on the
    grid ``shape`` (an int G means G^3)."""
    if isinstance(shape, int):
        s = bs.rotated_system(shape, dof)
        out = SimpleNamespace(nnodes=s.nnodes, n=s.n, dof=dof,
                              shape=(shape,) * 3, S=s.S, Af=s.Af, b=s.b)
    else:
        import scipy.sparse as sp

        from acg_amd.gen.stencil import queen_like_spec, stencil_global

        gx, gy, gz = shape
        rng = np.random.default_rng([9200, gx, gy, gz, dof])
        B = stencil_global(gx, gy, gz, queen_like_spec(dof)).to_scipy_full().tocsr()
        nnodes = gx * gy * gz
        Ls = []
        for _ in range(nnodes):
            Q, _r = np.linalg.qr(rng.standard_normal((dof, dof)))
            Ls.append(Q * 10.0 ** rng.uniform(-1.0, 1.0, size=dof)[None, :])
        Lm = sp.block_diag(Ls, format="csr")
        Af = (Lm @ B @ Lm.T).tocsr()
        Af = ((Af + Af.T) * 0.5).tocsr()
        A = bs._sym_from_full(Af, nnodes * dof)
        out = SimpleNamespace(nnodes=nnodes, n=nnodes * dof, dof=dof,
                              shape=shape, S=bs._local(A),
                              Af=A.to_scipy_full().tocsr(),
                              b=rng.standard_normal(nnodes * dof))
    # one rank: local order = global order, so the grid's brick order is a
    # valid hint for the LocalSystem's rows
    assert np.array_equal(out.S.owned_global, np.arange(out.n))
    return out


def node_order(shape, name):
    from acg_amd.gen.stencil import brick_order

    if name == "natural":
        return None
    gx, gy, gz = (shape,) * 3 if isinstance(shape, int) else shape
    return brick_order(gx, gy, gz)


def bsell(shape, dof, dev="cpu"):
    s = system(shape, dof)
    return tuple(torch.from_numpy(a).to(dev) for a in bs.bsell_arrays(s.S, dof))


def build(shape, dof, order, dev="cpu", arrays=None, **kw):
    """bsell_st_build of the system; the byte gate is off unless given, so
    every shape yields an operator to test."""
    s = system(shape, dof)
    kw.setdefault("gate", float("inf"))
    bptr, bcol, bvals = arrays if arrays is not None else bsell(shape, dof, dev)
    return symtile.bsell_st_build(bptr, bcol, bvals, s.nnodes, dof,
                                  node_order(shape, order), **kw)


@functools.lru_cache(maxsize=None)
def x_case(shape, dof):
    s = system(shape, dof)
    return ko.rand_values(s.n, np.random.default_rng([9300, s.nnodes, dof]))


@functools.lru_cache(maxsize=None)
def expect(shape, dof, dotslot=-1):
    """y = A x in the CALLER's row order, and the fused (x, y)."""
    s = system(shape, dof)
    S = s.S
    e = ko.Expect("k_spmv_bsell_st")
    xh = ko.hp(x_case(shape, dof))
    y, M = ko.spmv(S.A_rowptr, S.A_colidx, S.A_vals, xh)
    L = ko.bsell_padded_len(S.A_rowptr, S.A_colidx, dof)
    e.add("y", y, M, L)
    if dotslot >= 0:
        d, tol = ko.dot(xh, y, tb=ko.bound(M, L))
        e.add_tol(f"scal{dotslot}", d, tol)
    e.scalars(ko.SENTINELS, touched=(dotslot,))
    return e


def blocks_launched(st, max_blocks=0):
    nb = min(st.ntiles, ko.MAXG)
    return min(nb, max_blocks) if max_blocks > 0 else nb


def run_spmv(ops, st, shape, dof, dev, *, dotslot=-1, max_blocks=0):
    """One SpMV on NaN-poisoned outputs.  ``y`` comes back in the caller's
    row order; ``ytail`` is what lies behind the owned rows."""
    s = system(shape, dof)
    x = ko._t(x_case(shape, dof), dev)[st.vperm]
    ybuf = ko._nan(s.n + TAIL, dev)
    scal = ko._t(ko.SENTINELS, dev)
    partials = ko._nan(2 * ko.MAXG, dev)
    kw = dict(partials=partials, scal=scal, dotslot=dotslot,
              dot_accum=False) if dotslot >= 0 else {}
    ops.spmv_bsell_st(st, x, ybuf, max_blocks=max_blocks, **kw)
    y = torch.empty(s.n, dtype=torch.float64, device=dev)
    y[st.vperm] = ybuf[:s.n]
    got = {"y": ko._np(y), "yperm": ko._np(ybuf[:s.n]),
           "ytail": ko._np(ybuf[s.n:])}
    ko._partials_out(got, partials,
                     blocks_launched(st, max_blocks) if dotslot >= 0 else 0)
    return ko._scal_out(got, scal)


def check_untouched(got):
    """GPU only: nothing behind the owned rows and no partial beyond the
    launched blocks was written."""
    assert np.all(got["ytail"].view(np.int64) == NANBITS), "y tail written"
    ko.check_partials(got, halves=1)


# ---------------------------------------------------------------------------
# structure

def decode(st):
    node, col, vals, q = (t.cpu().numpy() for t in symtile.decode_st(st))
    live = node < st.nnodes
    return node[live], col[live], vals[live], q[live]


def dense_from_st(st):
    """The operator a BSELL-ST stores, in ITS node order: own blocks plus
    the transposes the sending blocks stand for."""
    dof, nn = st.dof, st.nnodes
    node, col, vals, q = decode(st)
    D = np.zeros((nn * dof, nn * dof))
    for i, j, v, qq in zip(node, col, vals, q):
        blk = v.reshape(dof, dof)
        D[i * dof:(i + 1) * dof, j * dof:(j + 1) * dof] += blk
        if qq != symtile.NOSEND:
            D[j * dof:(j + 1) * dof, i * dof:(i + 1) * dof] += blk.T
    return D


def overcap_pairs(st):
    """Indices (into decode(st)) of plain off-diagonal in-tile blocks whose
    partner block is stored as well: pairs left on both sides."""
    node, col, vals, q = decode(st)
    nz = (vals != 0).any(axis=1)
    key = node * st.nnodes + col
    have = set(key[nz & (q == symtile.NOSEND)].tolist())
    return [k for k in range(len(node))
            if nz[k] and q[k] == symtile.NOSEND and node[k] != col[k]
            and node[k] // st.tile == col[k] // st.tile
            and int(col[k] * st.nnodes + node[k]) in have]


# ---------------------------------------------------------------------------
# kernel emulation (fp64 numpy) and its mutants

def emulate(st, shape, dof, mutant=None):
    """What k_spmv_bsell_st computes, in the caller's row order."""
    assert mutant is None or mutant in MUTANTS
    nn = st.nnodes
    vperm = st.vperm.cpu().numpy()
    xb = x_case(shape, dof)[vperm].reshape(nn, dof)
    node, col, vals, q = decode(st)
    A = vals.reshape(-1, dof, dof)
    own = np.einsum("brc,bc->br", A, xb[col])
    if mutant == "overcap_dropped":
        own[overcap_pairs(st)[0]] = 0.0
    y = np.zeros((nn, dof))
    np.add.at(y, node, own)
    snd = q != symtile.NOSEND
    if mutant == "no_transpose":
        tr = np.einsum("brc,bc->br", A[snd], xb[node[snd]])
    else:
        tr = np.einsum("brc,br->bc", A[snd], xb[node[snd]])
    qs, recv = q[snd].copy(), col[snd]
    if mutant == "slot_collision":
        k = np.nonzero(qs == 1)[0][0]  # second sender of some receiver
        qs[k] = 0
    slots = np.zeros((max(st.qmax, 1), nn, dof))
    slots[qs, recv] = tr
    nr = st.nrecv.cpu().numpy()[:nn].astype(np.int64)
    if mutant == "short_sum":
        nr = np.maximum(nr - 1, 0)
    for k in range(st.qmax):
        y += np.where((nr > k)[:, None], slots[k], 0.0)
    y = y.reshape(-1)
    out = np.empty_like(y)
    if mutant == "inverse_perm":
        out = y[vperm]
    else:
        out[vperm] = y
    got = {"y": out}
    for i in range(ko.S_NSLOTS):
        got[f"scal{i}"] = ko.SENTINELS[i:i + 1]
    return got
