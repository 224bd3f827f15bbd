"""Shared inputs and oracles of the block-Jacobi PCG tests.

Plain helper module (not a conftest).  Two parts:

* the rotated-anisotropy systems ``A = L B L^T``: ``B`` is the Queen-shaped
  27-point block stencil on a G^3 grid and ``L = blockdiag(L_i)`` with
  ``L_i = Q_i diag(10^U(-1,1))``, ``Q_i`` the QR factor of a standard-normal
  dof x dof draw.  Every node's dofs are coupled by a rotated, badly scaled
  block (block condition numbers up to ~1e4), which point Jacobi cannot
  undo and block Jacobi removes exactly.  Seeds are fixed; each system and
  its direct solution are built once per process;
* long-double expectations (tests/kernel_oracle.py machinery) and runners
  for ``bjacobi_apply`` and ``bpcg_fused_update``; the same runners drive
  torch_ref on the CPU and gpu_ops on the GPU.  The packed inverse blocks
  are an exact fp64 INPUT of these two oracles, so inversion error does not
  enter; the inversion itself is checked per node against
  ``16 * dof * kappa_2(M) * 2^-53`` (:func:`diag_inv_ratio`).
"""

from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

import kernel_oracle as ko

RTOL = 1e-9  # residual tolerance of every block-Jacobi solve test


def bj_blocks(nnodes):
    """Blocks the block-Jacobi launchers start: one thread per node, two
    nodes per thread before the 4096-block cap."""
    return max(1, min(4096, (nnodes + 511) // 512))


# ---------------------------------------------------------------------------
# systems

def _sym_from_full(Af, n):
    from acg_amd.core.symcsr import SymCSRMatrix

    U = Af.tocoo()
    m = U.row <= U.col
    return SymCSRMatrix.from_coo(n, U.row[m], U.col[m], U.data[m])


def _local(A):
    from acg_amd.part import extract_subdomains, partition_rows

    return extract_subdomains(A, partition_rows(A, 1), 1)[0]


@functools.lru_cache(maxsize=None)
def rotated_system(G, dof):
    """The system of the module docstring on a G^3 grid: namespace with the
    SymCSRMatrix ``A``, its scipy form ``Af``, the one-rank LocalSystem
    ``S``, a right-hand side ``b`` and the dense diagonal blocks."""
    import scipy.sparse as sp

    from acg_amd.gen.stencil import queen_like_spec, stencil_global

    rng = np.random.default_rng([9000, G, dof])
    B = stencil_global(G, G, G, queen_like_spec(dof)).to_scipy_full().tocsr()
    nnodes = G ** 3
    n = nnodes * dof
    Ls = []
    for _ in range(nnodes):
        Q, _r = np.linalg.qr(rng.standard_normal((dof, dof)))
        Ls.append(Q * 10.0 ** rng.uniform(-1.0, 1.0, size=dof)[None, :])
    Lm = sp.block_diag(Ls, format="csr")
    Af = (Lm @ B @ Lm.T).tocsr()
    Af = ((Af + Af.T) * 0.5).tocsr()  # exactly symmetric
    A = _sym_from_full(Af, n)
    Af = A.to_scipy_full().tocsr()
    blocks = np.stack([Af[i * dof:(i + 1) * dof, i * dof:(i + 1) * dof].toarray()
                       for i in range(nnodes)])
    return SimpleNamespace(G=G, dof=dof, nnodes=nnodes, n=n, A=A, Af=Af,
                           S=_local(A), b=rng.standard_normal(n),
                           blocks=blocks)


@functools.lru_cache(maxsize=None)
def direct_solution(G, dof):
    import scipy.sparse.linalg as spla

    s = rotated_system(G, dof)
    return spla.spsolve(s.Af.tocsc(), s.b)


def modified_system(G, dof, kind, nodes):
    """``rotated_system`` with the diagonal blocks of ``nodes`` negated
    (``kind="indefinite"``), set to zero with their entries kept
    (``"zeroed"``) or removed from the structure (``"missing"``).
    Returns (SymCSRMatrix, LocalSystem)."""
    from acg_amd.core.symcsr import SymCSRMatrix

    s = rotated_system(G, dof)
    rows = np.repeat(np.arange(s.n, dtype=np.int64), np.diff(s.A.rowptr))
    cols, vals = s.A.colidx.copy(), s.A.vals.copy()
    hit = (rows // dof == cols // dof) & np.isin(rows // dof, nodes)
    if kind in ("indefinite", "zeroed"):
        vals[hit] = -vals[hit] if kind == "indefinite" else 0.0
        keep = np.ones(len(vals), dtype=bool)
    else:
        assert kind == "missing"
        keep = ~hit
    A = SymCSRMatrix.from_coo(s.n, rows[keep], cols[keep], vals[keep])
    return A, _local(A)


def bsell_arrays(S, dof):
    """Block-SELL arrays of the LocalSystem's matA with ``dof`` given."""
    from acg_amd.ops.torch_ref import bsell_from_csr

    bptr, bcol, bvals, density = bsell_from_csr(S.A_rowptr, S.A_colidx,
                                                S.A_vals, dof)
    return bptr, bcol, bvals


def write_mtx_file(path, A):
    from acg_amd.io.mtx import MtxFile, write_mtx

    rows = np.repeat(np.arange(A.n), np.diff(A.rowptr))
    write_mtx(path, MtxFile(object="matrix", format="coordinate",
                            field_="real", symmetry="symmetric", nrows=A.n,
                            ncols=A.n, nnz=A.nnz_stored, rowidx=rows,
                            colidx=A.colidx, a=A.vals))


# ---------------------------------------------------------------------------
# inversion acceptance

def diag_inv_ratio(blocks, inv):
    """Worst over the nodes of max|M M^-1 - I| / (16 dof kappa_2(M) 2^-53):
    the Cholesky-solve residual bound c*dof*u*kappa with c = 16 as slack
    for the back-substitutions.  <= 1 accepts."""
    blocks = np.asarray(blocks, dtype=np.float64)
    inv = np.asarray(inv, dtype=np.float64)
    dof = blocks.shape[1]
    if not np.all(np.isfinite(inv)):
        return float("inf")
    resid = np.abs(blocks @ inv - np.eye(dof)[None]).max(axis=(1, 2))
    kappa = np.linalg.cond(blocks, 2)
    return float((resid / (16.0 * dof * kappa * ko.U)).max())


# ---------------------------------------------------------------------------
# kernel cases, expectations, runners

def bj_case(nnodes, dof, pt_zero=False):
    rng = np.random.default_rng([9100, nnodes, dof])
    n = nnodes * dof
    scal = ko.SENTINELS.copy()
    scal[ko.S_RR] = 1.3719
    scal[ko.S_PT] = 0.0 if pt_zero else 2.9131
    return SimpleNamespace(nnodes=nnodes, dof=dof, n=n, scal=scal,
                           **{k: ko.rand_values(n, rng) for k in "rxpt"})


def _block_mul(Mi, r, Mr):
    """(M^-1 r, sum |M^-1| Mr) node by node in high precision; ``Mi`` the
    dense fp64 inverse blocks (nnodes, dof, dof)."""
    nnodes, dof = Mi.shape[0], Mi.shape[1]
    rb, Mb = r.reshape(nnodes, dof), Mr.reshape(nnodes, dof)
    z, Mz = ko.hzeros(nnodes * dof).reshape(nnodes, dof), \
        ko.hzeros(nnodes * dof).reshape(nnodes, dof)
    for a in range(dof):
        for b in range(dof):
            m = ko.hp(Mi[:, a, b])
            z[:, a] = z[:, a] + m * rb[:, b]
            Mz[:, a] = Mz[:, a] + ko.habs(m) * Mb[:, b]
    return z.reshape(-1), Mz.reshape(-1)


def _publish(e, case, r, Mr, z, Mz, exact_r):
    """(r,z) -> S_RR, (r,r) -> S_GAMMA, old S_RR -> S_RR_PREV; every other
    slot keeps its sentinel."""
    tr = None if exact_r else ko.bound(Mr)
    rz, rztol = ko.dot(r, z, ta=tr, tb=ko.bound(Mz, case.dof))
    rr, rrtol = ko.dot(r, r, ta=tr, tb=tr)
    e.add_exact(f"scal{ko.S_RR_PREV}", case.scal[ko.S_RR])
    e.add_tol(f"scal{ko.S_RR}", rz, rztol)
    e.add_tol(f"scal{ko.S_GAMMA}", rr, rrtol)
    e.scalars(case.scal, touched=(ko.S_RR, ko.S_RR_PREV, ko.S_GAMMA))


def bj_apply_expect(case, Mi):
    """z = M^-1 r from the unchanged input r: acceptance
    (dof + 48) 2^-53 sum|M^-1||r| per element."""
    e = ko.Expect("k_bjacobi_apply")
    r = ko.hp(case.r)
    z, Mz = _block_mul(Mi, r, ko.habs(r))
    e.add_exact("r", case.r)
    e.add("z", z, Mz, case.dof)
    _publish(e, case, r, ko.habs(r), z, Mz, exact_r=True)
    return e


def bj_update_expect(case, Mi):
    """Bounds of r' and x' as in kernel_oracle.pcg_expect; for z' the
    acceptance (dof + 48) 2^-53 sum|M^-1||r'|_M, |r'|_M the magnitude of
    the r' update."""
    e = ko.Expect("k_bpcg_fused_update")
    alpha = ko.ratio_coeff(case.scal[ko.S_RR], case.scal[ko.S_PT])
    aa = abs(alpha)
    r0, x0, p0, t0 = (ko.hp(getattr(case, k)) for k in "rxpt")
    r, Mr = r0 - alpha * t0, ko.habs(r0) + aa * ko.habs(t0)
    x, Mx = x0 + alpha * p0, ko.habs(x0) + aa * ko.habs(p0)
    exact = float(case.scal[ko.S_PT]) == 0.0
    if exact:
        e.add_exact("r", case.r)
        e.add_exact("x", case.x)
    else:
        e.add("r", r, Mr)
        e.add("x", x, Mx)
    z, Mz = _block_mul(Mi, r, Mr)
    e.add("z", z, Mz, case.dof)
    _publish(e, case, r, Mr, z, Mz, exact_r=exact)
    return e


def run_bj_apply(ops, case, minv, dev):
    r, z = ko._t(case.r, dev), ko._nan(case.n, dev)
    scal = ko._t(case.scal, dev)
    partials = ko._nan(2 * ko.MAXG, dev)
    ops.bjacobi_apply(minv, r, z, partials, scal, case.n, case.dof)
    got = {"r": ko._np(r), "z": ko._np(z)}
    ko._partials_out(got, partials, bj_blocks(case.nnodes))
    return ko._scal_out(got, scal)


def run_bj_update(ops, case, minv, dev):
    r, x, z = ko._t(case.r, dev), ko._t(case.x, dev), ko._nan(case.n, dev)
    scal = ko._t(case.scal, dev)
    partials = ko._nan(2 * ko.MAXG, dev)
    ops.bpcg_fused_update(r, x, ko._t(case.p, dev), ko._t(case.t, dev), z,
                          minv, scal, partials, case.n, case.dof)
    got = {"r": ko._np(r), "x": ko._np(x), "z": ko._np(z)}
    ko._partials_out(got, partials, bj_blocks(case.nnodes))
    return ko._scal_out(got, scal)
