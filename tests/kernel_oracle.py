"""High-precision oracle for the kernel-level exactness tests.

Plain helper module (not a conftest).  Three parts:

* oracle arithmetic: every operation is evaluated from the ORIGINAL CSR and
  the fp64 input vectors in ``np.longdouble`` (when it carries a 64-bit
  significand) or exact ``fractions.Fraction``; each value ``v`` comes with
  a magnitude ``M`` = the same expression with every term replaced by its
  absolute value.  The matrix-free stencil kernels have no CSR: their
  oracle (:func:`stencil_apply`) applies the stencil from global grid
  coordinates, and the slab generators are checked entry by entry against
  :func:`stencil_structure`;
* acceptance: ``|got_i - v_i| <= (L_i + 48) * 2^-53 * M_i`` element-wise
  (L_i = products summed into element i), propagated bounds for reduced
  scalars, bitwise equality where the result is exactly representable;
* the shared inputs and runners: the same ``case`` objects and the same
  ``run_*`` drivers serve the CPU tests (torch_ref, mutants) and the GPU
  tests (gpu_ops), so the CPU discrimination check speaks about exactly the
  inputs the kernels see.

Why the bound holds.  A length-L recursive (or pairwise, or FMA) sum of
products has running error <= L*u*sum|a_i b_i| (u = 2^-53, Higham 3.1; the
quadratic term is below 1e-13 of that here).  The vector-update chain adds
at most a handful of roundings on top, each relative to a partial result
that is bounded by M.  The coefficients alpha/beta are themselves rounded:
at most 4 operations, amplified by the cancellation factor of the
pipelined alpha denominator, which the inputs keep <= 8 (asserted by
:func:`pipe_expect`) -- 4*8 + the chain stays below the constant 48.
"""

from __future__ import annotations

from fractions import Fraction
from types import SimpleNamespace

import numpy as np

U = 2.0 ** -53
EXTRA_OPS = 48
C = 64
MAXG = 16384
USE_LONGDOUBLE = bool(np.finfo(np.longdouble).eps <= 2.0 ** -63)

S_RR, S_PT, S_RR_PREV, S_BNRM2 = 0, 1, 2, 3
S_GAMMA, S_DELTA, S_GAMMA_PREV, S_ALPHA_PREV = 4, 5, 6, 7
S_NSLOTS = 8
# distinct finite sentinels for scalar slots an operation must not touch
SENTINELS = np.array([101.5, 102.25, 103.125, 104.75, 105.5, 106.25,
                      107.125, 108.75])


# ---------------------------------------------------------------------------
# high-precision arithmetic

def hps(x):
    """fp64 scalar -> high-precision scalar (exact conversion)."""
    return np.longdouble(x) if USE_LONGDOUBLE else Fraction(float(x))


def hp(a):
    """fp64 array -> high-precision array (exact conversion)."""
    a = np.asarray(a, dtype=np.float64)
    if USE_LONGDOUBLE:
        return a.astype(np.longdouble)
    out = np.empty(a.size, dtype=object)
    for i, v in enumerate(a.ravel()):
        out[i] = Fraction(float(v))
    return out.reshape(a.shape)


def hzeros(n):
    return hp(np.zeros(n))


def to_f64(a):
    a = np.asarray(a)
    if a.dtype == object:
        return np.array([float(v) for v in a.ravel()]).reshape(a.shape)
    return a.astype(np.float64)


def habs(a):
    return np.abs(a)


def hsum(a):
    s = hps(0.0)
    return s + a.sum() if a.size else s


def ratio_coeff(num, den):
    """The kernels' safe_div in high precision: 0 when den == 0; a finite
    numerator over an infinite denominator is exactly 0 in fp64 too."""
    num, den = float(num), float(den)
    if den == 0.0 or np.isinf(den):
        return hps(0.0)
    return hps(num) / hps(den)


# ---------------------------------------------------------------------------
# oracle operations: each returns (value, magnitude)

def csr_rows(rowptr):
    rowptr = np.asarray(rowptr, dtype=np.int64)
    return np.repeat(np.arange(len(rowptr) - 1, dtype=np.int64), np.diff(rowptr))


def spmv(rowptr, colidx, vals, x, xM=None):
    """A x from the CSR.  ``x`` high-precision; ``xM`` its magnitude
    (default |x|)."""
    rows = csr_rows(rowptr)
    cols = np.asarray(colidx, dtype=np.int64)
    a = hp(vals)
    n = len(rowptr) - 1
    v, M = hzeros(n), hzeros(n)
    np.add.at(v, rows, a * x[cols])
    np.add.at(M, rows, habs(a) * (habs(x) if xM is None else xM)[cols])
    return v, M


def bound(M, L=0):
    """Element-wise acceptance bound (L + 48) * 2^-53 * M."""
    Lh = hp(np.broadcast_to(np.asarray(L, dtype=np.float64), np.shape(M)))
    return (Lh + hps(float(EXTRA_OPS))) * hps(U) * M


def dot(a, b, ta=None, tb=None, add=None):
    """sum a_i b_i with the propagated tolerance of the issue:
    sum(|a| tb + |b| ta + ta tb) + (n + 8) u sum|a b| (``add``: an old slot
    value accumulated into; its magnitude joins the sum).
    Returns (value, tolerance)."""
    n = a.size
    v = hsum(a * b)
    M = hsum(habs(a) * habs(b))
    tol = hps(0.0)
    if ta is not None:
        tol = tol + hsum(habs(b) * ta)
    if tb is not None:
        tol = tol + hsum(habs(a) * tb)
    if ta is not None and tb is not None:
        tol = tol + hsum(ta * tb)
    if add is not None:
        v = v + hps(add)
        M = M + abs(hps(add))
    return v, tol + hps(float(n + 8)) * hps(U) * M


def sell_padded_len(rowptr, perm=None):
    """Products per row in SELL-C-64: the slice's longest row.  ``perm``
    (SELL row -> matrix row, sentinel nrows) for sigma-sorted structures."""
    counts = np.diff(np.asarray(rowptr, dtype=np.int64))
    nrows = len(counts)
    nsl = (nrows + C - 1) // C
    rowof = np.arange(nsl * C) if perm is None else np.asarray(perm, np.int64)
    pad = np.zeros(nsl * C, dtype=np.int64)
    ok = rowof < nrows
    pad[ok] = counts[rowof[ok]]
    smax = pad.reshape(nsl, C).max(axis=1)
    L = np.zeros(nrows, dtype=np.int64)
    L[rowof[ok]] = np.repeat(smax, C)[ok]
    return L


def bsell_padded_len(rowptr, colidx, dof):
    """Products per scalar row in Block-SELL: dof * (most blocks of any node
    in the 64-node slice)."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    nrows = len(rowptr) - 1
    nnodes = nrows // dof
    key = (csr_rows(rowptr) // dof) * (1 << 32) + np.asarray(colidx, np.int64) // dof
    bnode = np.unique(key) >> 32
    per_node = np.bincount(bnode, minlength=nnodes)
    nsl = (nnodes + C - 1) // C
    pad = np.zeros(nsl * C, dtype=np.int64)
    pad[:nnodes] = per_node
    smax = pad.reshape(nsl, C).max(axis=1)
    return np.repeat(np.repeat(smax, C)[:nnodes], dof) * dof


def unpack_bsell(bptr, bcol, bvals, nnodes, dof, ncols):
    """Decode Block-SELL arrays into a dense (nnodes*dof, ncols) matrix.

    Written from the layout comment above ``bval_off`` in kernels.hip, not
    from the packer: per 64-node slice s (bptr in block units) the j-th
    block of lane's node has block-column bcol[bptr[s] + j*64 + lane]; its
    element k (row-major in the dof x dof block) sits at
    bptr[s]*dof^2 + j*dof^2*64 + off, off = (k//2)*128 + lane*2 + (k&1) for
    paired k and (dof^2-1)*64 + lane for the odd tail k = dof^2-1."""
    bptr = np.asarray(bptr, dtype=np.int64)
    bcol = np.asarray(bcol)
    bvals = np.asarray(bvals, dtype=np.float64)
    D2 = dof * dof
    odd = D2 % 2 == 1
    dense = np.zeros((nnodes * dof, ncols), dtype=np.float64)
    for s in range(len(bptr) - 1):
        assert (bptr[s + 1] - bptr[s]) % 64 == 0
        blen = (bptr[s + 1] - bptr[s]) // 64
        for j in range(blen):
            for lane in range(64):
                node = s * 64 + lane
                cb = int(bcol[bptr[s] + j * 64 + lane])
                assert 0 <= cb * dof and (cb + 1) * dof <= ncols, \
                    "block column (padding included) must stay in bounds"
                base = bptr[s] * D2 + j * D2 * 64
                for k in range(D2):
                    if odd and k == D2 - 1:
                        off = (D2 - 1) * 64 + lane
                    else:
                        off = (k // 2) * 128 + lane * 2 + (k & 1)
                    val = bvals[base + off]
                    if node >= nnodes:
                        assert val == 0.0, "padding lane holds a value"
                        continue
                    dense[node * dof + k // dof, cb * dof + k % dof] += val
    return dense


def csr_dense(rowptr, colidx, vals, ncols):
    dense = np.zeros((len(rowptr) - 1, ncols), dtype=np.float64)
    dense[csr_rows(rowptr), np.asarray(colidx, np.int64)] = vals
    return dense


def stencil_apply(gx, gy, gz, offsets, diag, xg, part=None):
    """Constant-coefficient stencil operator from GLOBAL grid coordinates
    (node id = x + gx*(y + gy*z)): y = diag*x + sum_o w_o * x[shifted by o],
    out-of-grid neighbours contributing nothing.  Knows nothing of slabs'
    local numbering, plane tables or any CSR the project builds.

    ``part = (which, z0, z1)`` restricts to the rows of planes [z0, z1) and
    keeps only the couplings into those planes plus the diagonal
    (``"owned"``, the matA part) or only the couplings into other planes
    (``"ghost"``, the matO part).  ``xg`` is an fp64 array of gx*gy*gz
    values.  Returns flat global (value, magnitude, products per row)."""
    X = hp(np.asarray(xg, dtype=np.float64)).reshape(gz, gy, gx)
    aX = habs(X)
    v = hzeros(gx * gy * gz).reshape(gz, gy, gx)
    M = hzeros(gx * gy * gz).reshape(gz, gy, gx)
    L = np.zeros((gz, gy, gx), dtype=np.int64)
    which, z0, z1 = part if part is not None else (None, 0, gz)
    if which != "ghost":
        d = hps(diag)
        v[z0:z1] += d * X[z0:z1]
        M[z0:z1] += abs(d) * aX[z0:z1]
        L[z0:z1] += 1
    for (dx, dy, dz, w) in offsets:
        dx, dy, dz = int(dx), int(dy), int(dz)
        wh = hps(w)
        ys = slice(max(0, -dy), min(gy, gy - dy))
        xs = slice(max(0, -dx), min(gx, gx - dx))
        yt = slice(ys.start + dy, ys.stop + dy)
        xt = slice(xs.start + dx, xs.stop + dx)
        if ys.start >= ys.stop or xs.start >= xs.stop:
            continue
        for z in range(z0, z1):
            tz = z + dz
            if not 0 <= tz < gz:
                continue
            if which is not None and (z0 <= tz < z1) != (which == "owned"):
                continue
            v[z, ys, xs] += wh * X[tz, yt, xt]
            M[z, ys, xs] += abs(wh) * aX[tz, yt, xt]
            L[z, ys, xs] += 1
    return v.reshape(-1), M.reshape(-1), L.reshape(-1)


def stencil_structure(gx, gy, gz, spec, rank, nranks):
    """Per-row structure oracle for the slab generators: for every owned
    local row (node, a) the dictionary {local column: value} of its owned
    couplings (``rowsA``) and, for the border rows, of its ghost couplings
    (``rowsO``, indexed from the first border row).  Built from global
    coordinates; value = D[a, b] for the node's own block and w_o * M[a, b]
    (ONE fp64 product, exactly reproducible) for neighbour o.  Local <->
    global goes through the host slab's owned_global / ghost_global."""
    from acg_amd.gen.stencil import stencil_local_slab

    H = stencil_local_slab(gx, gy, gz, spec, rank, nranks)
    dof = spec["dof"]
    Mb = np.asarray(spec.get("offblock", np.eye(dof)), dtype=np.float64)
    Db = np.asarray(spec.get("diagblock", spec.get("diag", 1.0) * np.eye(dof)),
                    dtype=np.float64)
    g2l = {int(g): i for i, g in enumerate(
        np.concatenate([H.owned_global, H.ghost_global]))}
    assert len(g2l) == H.nowned + H.nghost
    rowsA, rowsO = [], []
    for row in range(H.nowned):
        gnode, a = divmod(int(H.owned_global[row]), dof)
        x, y, z = gnode % gx, (gnode // gx) % gy, gnode // (gx * gy)
        dA = {g2l[gnode * dof + b]: float(Db[a, b]) for b in range(dof)}
        dO = {}
        for (dx, dy, dz, w) in spec["offsets"]:
            nx, ny, nz = x + int(dx), y + int(dy), z + int(dz)
            if not (0 <= nx < gx and 0 <= ny < gy and 0 <= nz < gz):
                continue
            nb = nx + gx * (ny + gy * nz)
            for b in range(dof):
                col = g2l[nb * dof + b]
                tgt = dA if col < H.nowned else dO
                assert col not in tgt
                tgt[col] = float(w) * float(Mb[a, b])
        rowsA.append(dA)
        if row >= H.ninterior:
            rowsO.append(dO)
        else:
            assert not dO, "an interior row couples to a ghost"
    return SimpleNamespace(dof=dof, rowsA=rowsA, rowsO=rowsO, nowned=H.nowned,
                           ninterior=H.ninterior, nborder=H.nborder,
                           nghost=H.nghost, nlocal=H.nowned + H.nghost,
                           nnzA=sum(map(len, rowsA)), nnzO=sum(map(len, rowsO)))


def rows_to_csr(rows):
    """[{col: value}] -> (rowptr, colidx, vals), columns ascending."""
    rowptr = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum([len(d) for d in rows], out=rowptr[1:])
    cols = np.array([c for d in rows for c in sorted(d)], dtype=np.int64)
    vals = np.array([d[c] for d in rows for c in sorted(d)], dtype=np.float64)
    return rowptr, cols, vals


def csr_to_rows(rowptr, colidx, vals):
    out = []
    for i in range(len(rowptr) - 1):
        sl = slice(int(rowptr[i]), int(rowptr[i + 1]))
        d = dict(zip(np.asarray(colidx[sl]).tolist(), np.asarray(vals[sl]).tolist()))
        assert len(d) == sl.stop - sl.start, "duplicate column in a row"
        out.append(d)
    return out


def sell_to_rows(sellptr, cols, vals, nrows):
    """Decode SELL-C-64 arrays (kernels.hip: element j of row s*64+lane at
    sellptr[s] + j*64 + lane) into per-row dictionaries of the NONZERO
    entries.  Returns (rows, entries per row incl. padding, the columns of
    every zero-valued entry)."""
    sellptr = np.asarray(sellptr, dtype=np.int64)
    cols, vals = np.asarray(cols), np.asarray(vals, dtype=np.float64)
    assert len(sellptr) - 1 == (nrows + C - 1) // C
    assert len(cols) == len(vals) == sellptr[-1]
    rows, lens, padcols = [], np.zeros(nrows, dtype=np.int64), []
    for s in range(len(sellptr) - 1):
        base, end = int(sellptr[s]), int(sellptr[s + 1])
        assert (end - base) % C == 0
        for lane in range(C):
            c, v = cols[base + lane:end:C], vals[base + lane:end:C]
            nz = v != 0.0
            padcols.extend(c[~nz].tolist())
            if s * C + lane >= nrows:
                assert not nz.any(), "padding lane holds a value"
                continue
            d = dict(zip(c[nz].tolist(), v[nz].tolist()))
            assert len(d) == int(nz.sum()), "duplicate column in a row"
            rows.append(d)
            lens[s * C + lane] = (end - base) // C
    return rows, lens, np.asarray(padcols, dtype=np.int64)


def rows_bits_equal(got, want):
    """Same columns and bit-identical values in every row."""
    if len(got) != len(want):
        return False
    for g, w in zip(got, want):
        if g.keys() != w.keys():
            return False
        ks = sorted(w)
        if not _bits_equal([g[k] for k in ks], [w[k] for k in ks]):
            return False
    return True


# ---------------------------------------------------------------------------
# acceptance

class Expect:
    """What one operation must produce: named arrays with element bounds,
    named arrays that must match bitwise, and pairs of outputs that must be
    bitwise equal to each other."""

    def __init__(self, kernel):
        self.kernel = kernel
        self.close = {}
        self.exact = {}
        self.same = []

    def add(self, name, v, M, L=0):
        self.close[name] = (np.atleast_1d(v), np.atleast_1d(bound(np.atleast_1d(M), L)))

    def add_tol(self, name, v, tol):
        self.close[name] = (np.atleast_1d(v), np.atleast_1d(tol))

    def add_exact(self, name, arr):
        self.exact[name] = np.atleast_1d(np.asarray(arr, dtype=np.float64)).copy()

    def add_same(self, a, b):
        self.same.append((a, b))

    def scalars(self, untouched_from, touched=()):
        """Every slab slot not in ``touched`` must keep its input bits."""
        for i in range(S_NSLOTS):
            if i not in touched:
                self.add_exact(f"scal{i}", untouched_from[i])


def _bits_equal(a, b):
    a = np.ascontiguousarray(np.atleast_1d(a), dtype=np.float64)
    b = np.ascontiguousarray(np.atleast_1d(b), dtype=np.float64)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.int64), b.view(np.int64)))


def ratios(expect, got):
    """name -> worst error/bound (0 = exact, inf = NaN, a broken bitwise
    check, or an error where the bound is 0)."""
    out = {}
    for name, (v, bnd) in expect.close.items():
        g = np.atleast_1d(np.asarray(got[name], dtype=np.float64))
        if g.shape != v.shape or not np.all(np.isfinite(g)):
            out[name] = float("inf")
            continue
        if g.size == 0:
            out[name] = 0.0
            continue
        err = habs(hp(g) - v)
        zero = np.asarray(bnd == 0, dtype=bool)
        safe = np.where(zero, hps(1.0), bnd)
        r = to_f64(err / safe)
        bad = zero & np.asarray(err != 0, dtype=bool)
        r[zero] = 0.0
        r[bad] = float("inf")
        out[name] = float(r.max())
    for name, want in expect.exact.items():
        out[name] = 0.0 if _bits_equal(got[name], want) else float("inf")
    for a, b in expect.same:
        out[f"{a}=={b}"] = 0.0 if _bits_equal(got[a], got[b]) else float("inf")
    return out


def accepts(expect, got):
    return all(r <= 1.0 for r in ratios(expect, got).values())


def assert_accepts(expect, got, tag=""):
    rs = ratios(expect, got)
    worst = max((r for r in rs.values()), default=0.0)
    print(f"ORACLE_RATIO kernel={expect.kernel} case={tag} worst={worst:.4g} "
          + " ".join(f"{k}={v:.3g}" for k, v in rs.items() if v > 0))
    bad = {k: v for k, v in rs.items() if not v <= 1.0}
    assert not bad, f"{expect.kernel} [{tag}]: error/bound > 1 for {bad}"
    return worst


# ---------------------------------------------------------------------------
# inputs

_BASE_LENS = (0, 1, 7, 8, 9, 15, 16, 17)


def rand_values(n, rng):
    """Distinct fp64 values with |v| in [0.5, 2): no entry is small enough
    to hide inside another entry's rounding error."""
    v = rng.uniform(0.5, 2.0, size=n) * rng.choice([-1.0, 1.0], size=n)
    assert len(np.unique(v)) == n
    return v


def ragged_counts(nrows, cap, rng):
    """Row lengths such that every 64-row slice holds one long row (40..47,
    cycling through every remainder mod 8) and rows of length
    0, 1, 7, 8, 9, 15, 16, 17 (as far as the slice has rows); capped at the
    number of columns."""
    counts = rng.choice(_BASE_LENS, size=nrows)
    for s0 in range(0, nrows, C):
        hi = min(s0 + C, nrows)
        counts[s0] = 40 + (3 * (s0 // C)) % 8
        k = min(hi - s0 - 1, len(_BASE_LENS))
        counts[s0 + 1:s0 + 1 + k] = _BASE_LENS[:k]
    return np.minimum(counts, cap).astype(np.int64)


def short_counts(nrows, rng):
    """Slices whose LONGEST row has 0, 1, 7, 9, 0, ... entries: the SELL
    kernels' main unrolled loop never runs (slice length < 8), runs exactly
    once with a one-entry tail, or the slice is entirely empty."""
    counts = np.zeros(nrows, dtype=np.int64)
    for s0 in range(0, nrows, C):
        hi = min(s0 + C, nrows)
        top = (0, 1, 7, 9)[(s0 // C) % 4]
        counts[s0:hi] = rng.integers(0, top + 1, size=hi - s0)
        counts[s0 + (hi - s0) // 2] = top
    return counts


def csr_from_counts(counts, col_lo, col_hi, rng):
    """Random CSR (sorted distinct columns in [col_lo, col_hi))."""
    rowptr = np.zeros(len(counts) + 1, dtype=np.int64)
    np.cumsum(counts, out=rowptr[1:])
    cols = np.empty(int(rowptr[-1]), dtype=np.int64)
    for i, c in enumerate(counts):
        cols[rowptr[i]:rowptr[i + 1]] = col_lo + np.sort(
            rng.choice(col_hi - col_lo, size=int(c), replace=False))
    return rowptr, cols, rand_values(len(cols), rng)


def sell_case(nslices, short=False):
    rng = np.random.default_rng(1000 + nslices + (500 if short else 0))
    nrows = nslices * C - 13
    ncols = nrows + 37
    counts = short_counts(nrows, rng) if short else ragged_counts(nrows, ncols, rng)
    rowptr, cols, vals = csr_from_counts(counts, 0, ncols, rng)
    return SimpleNamespace(nrows=nrows, ncols=ncols, rowptr=rowptr, cols=cols,
                           vals=vals, x=rand_values(ncols, rng), nslices=nslices)


def bsell_case(dof, nnodes, ghost, empty_slice=None):
    """Block matrix with ragged block-rows, random unsymmetric blocks with
    some off-diagonal entries missing, optional ghost block-columns and an
    optional all-empty 64-node slice."""
    rng = np.random.default_rng(2000 + 100 * dof + nnodes + (7 if ghost else 0)
                                + (3 if empty_slice is not None else 0))
    ncn = max(nnodes, 48) + 7 if ghost else nnodes
    bcounts = ragged_counts(nnodes, ncn, rng)
    if empty_slice is not None:
        bcounts[empty_slice * C:(empty_slice + 1) * C] = 0
    rows, cols = [], []
    for nd in range(nnodes):
        bcs = np.sort(rng.choice(ncn, size=int(bcounts[nd]), replace=False))
        for a in range(dof):
            for bc in bcs:
                for b in range(dof):
                    if a == b or rng.random() >= 0.25:
                        rows.append(nd * dof + a)
                        cols.append(bc * dof + b)
    rows = np.asarray(rows, dtype=np.int64)
    cols = np.asarray(cols, dtype=np.int64)
    nrows = nnodes * dof
    rowptr = np.zeros(nrows + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=nrows), out=rowptr[1:])
    vals = rand_values(len(cols), rng)
    ncols = ncn * dof
    return SimpleNamespace(dof=dof, nnodes=nnodes, nrows=nrows, ncols=ncols,
                           rowptr=rowptr, cols=cols, vals=vals,
                           x=rand_values(ncols, rng), pold=rand_values(ncols, rng),
                           r=rand_values(ncols, rng))


def pipe_case(nowned, split, nborder0=False, short=False):
    """Local system of one rank: interior | border rows, owned | ghost
    columns.  serial: no border, no ghosts.  ``nborder0``: ghosts exist but
    no row couples to them (border_base = nowned, no matO pass).
    ``short``: slice lengths 0/1/7/9 (see short_counts) in matA and matO."""
    rng = np.random.default_rng(3000 + nowned + (1 if split else 0)
                                + (2 if nborder0 else 0) + (500 if short else 0))
    if split and not nborder0:
        ninterior = {65: 37, 200: 131, 400: 150}.get(nowned, (nowned * 2) // 3 | 1)
        assert ninterior % C
    else:
        ninterior = nowned
    nborder = nowned - ninterior
    nghost = 45 if split else 0
    cntA = short_counts(nowned, rng) if short else ragged_counts(nowned, nowned, rng)
    A = csr_from_counts(cntA, 0, nowned, rng)
    if nborder:
        cntO = short_counts(nborder, rng) if short else ragged_counts(nborder, nghost, rng)
        O =csr_from_counts(cntO, nowned, nowned + nghost, rng)
    else:
        O = None
    # the original local matrix: row-wise union (owned cols sort first)
    cnt = cntA.copy()
    if nborder:
        cnt[ninterior:] += cntO
    rowptr = np.zeros(nowned + 1, dtype=np.int64)
    np.cumsum(cnt, out=rowptr[1:])
    cols = np.empty(int(rowptr[-1]), dtype=np.int64)
    vals = np.empty(int(rowptr[-1]))
    for i in range(nowned):
        a0, a1 = A[0][i], A[0][i + 1]
        k = rowptr[i]
        cols[k:k + a1 - a0] = A[1][a0:a1]
        vals[k:k + a1 - a0] = A[2][a0:a1]
        if i >= ninterior:
            o0, o1 = O[0][i - ninterior], O[0][i - ninterior + 1]
            cols[k + a1 - a0:rowptr[i + 1]] = O[1][o0:o1]
            vals[k + a1 - a0:rowptr[i + 1]] = O[2][o0:o1]
    vec = {k: rand_values(nowned, rng) for k in "ztpxr"}
    scal = SENTINELS.copy()
    scal[S_GAMMA], scal[S_DELTA] = 2.3719, 3.1427
    scal[S_GAMMA_PREV], scal[S_ALPHA_PREV] = 1.7353, 2.9131
    return SimpleNamespace(nowned=nowned, ninterior=ninterior, nborder=nborder,
                           nghost=nghost, nlocal=nowned + nghost,
                           border_base=ninterior if nborder else nowned,
                           A=A, O=O, rowptr=rowptr, cols=cols, vals=vals,
                           w_old=rand_values(nowned + nghost, rng), scal=scal,
                           **vec)


# Offset weights of the stencil cases: pairwise distinct in MAGNITUDE (so
# w(d) != w(-d) and any exchange of two weights changes the result), not
# dyadic, mixed signs, 0.25 <= |w| <= 2.
_STENCIL_W = (-1.37, 0.83, -0.61, 1.19, 0.47, -1.73, 0.29, -0.97, 1.53, -0.41,
              0.71, 1.91, -1.13, 0.37, -0.53, 1.67, -1.87, 0.59, 1.01, -0.31,
              0.89, -1.43, 1.27, -0.67, 0.43, -1.61)
# upper triangles (row-major) of the dense symmetric neighbour / self blocks
_STENCIL_M = (0.77, -0.35, 0.58, 1.21, -0.49, 0.93, 0.27, 1.45, -0.63, 1.09)
_STENCIL_D = (5.3, 0.45, -0.85, 6.1, 0.65, -0.39, 7.7, 0.55, 0.95, 4.9)
# deliberately NOT the (-x, +x, -y, +y, -z, +z) order of the walk kernels
_OFFS_7 = ((0, 0, 1), (-1, 0, 0), (0, 1, 0), (0, 0, -1), (1, 0, 0), (0, -1, 0))
_OFFS_5 = ((0, 1, 0), (-1, 0, 0), (1, 0, 0), (0, -1, 0))
_OFFS_27 = tuple((dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1)
                 for dx in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0))
STENCIL_KINDS = {"7pt": (_OFFS_7, 5.3), "27pt": (_OFFS_27, 7.9),
                 "5pt2d": (_OFFS_5, 3.7)}
assert len(set(map(abs, _STENCIL_W))) == len(_STENCIL_W) == len(_OFFS_27)


# (gx, gy, gz, nranks), every rank of each: a plane of 15 < one wave with an
# uneven split whose rank 1 owns two planes, both border (ninterior = 0);
# a plane of 63 with one plane per rank (rank 1's is both borders, two
# ghosts); a plane of 65; gx = 1; gy = 1; serial.
STENCIL_SHAPES_3D = ((5, 3, 7, 3), (9, 7, 3, 3), (13, 5, 7, 3), (1, 13, 4, 2),
                     (13, 1, 5, 5), (17, 16, 6, 1))
STENCIL_SHAPE_2D = (19, 11, 1, 1)
# the walk kernels' grid-stride loops start above (MAXG-1024)*256 and
# MAXG*256 = 4 194 304 columns: 2049 * 2048 = 4 196 352 is above both
STENCIL_LARGE = ("7pt", 2049, 2048, 2, 0, 1)


def stencil_case_ids(kinds=("7pt", "27pt")):
    """(kind, gx, gy, gz, rank, nranks) of every rank of every shape."""
    ids = [(k, gx, gy, gz, rank, nr) for k in kinds
           for (gx, gy, gz, nr) in STENCIL_SHAPES_3D for rank in range(nr)]
    return ids + [("5pt2d",) + STENCIL_SHAPE_2D[:3] + (0, 1)]


def _sym_block(tri, dof):
    B = np.zeros((dof, dof))
    it = iter(tri)
    for a in range(dof):
        for b in range(a, dof):
            B[a, b] = B[b, a] = next(it)
    return B


def stencil_spec(kind, dof=1):
    """Stencil with per-offset weights; dof > 1: dense symmetric blocks
    whose entries are pairwise distinct up to symmetry."""
    offs, diag = STENCIL_KINDS[kind]
    spec = {"offsets": [(dx, dy, dz, w) for (dx, dy, dz), w
                        in zip(offs, _STENCIL_W)], "diag": diag, "dof": dof}
    if dof > 1:
        spec["offblock"] = _sym_block(_STENCIL_M, dof)
        spec["diagblock"] = _sym_block(_STENCIL_D, dof)
    return spec


def stencil_case(kind, gx, gy, gz, rank, nranks, host_map=True):
    """Rank ``rank``'s slab of a dof=1 stencil system: a global input
    vector (SpMV input and w_old of the pipelined iteration) in local
    order, the five owned vectors and the scalar slab of pipe_case.
    ``host_map=False`` (serial only): local = global order, without
    building the host slab."""
    spec = stencil_spec(kind)
    rng = np.random.default_rng([7000, list(STENCIL_KINDS).index(kind),
                                 gx, gy, gz, rank, nranks])
    plane = gx * gy
    if host_map:
        from acg_amd.gen.stencil import stencil_local_slab

        H = stencil_local_slab(gx, gy, gz, spec, rank, nranks)
        owned, ghost = H.owned_global, H.ghost_global
        ninterior = H.ninterior
    else:
        assert nranks == 1
        owned, ghost = np.arange(plane * gz, dtype=np.int64), np.zeros(0, np.int64)
        ninterior = len(owned)
    nowned, nghost = len(owned), len(ghost)
    z0, z1 = int(owned.min()) // plane, int(owned.max()) // plane + 1
    assert nowned == (z1 - z0) * plane
    wg = rand_values(plane * gz, rng)
    vec = {k: rand_values(nowned, rng) for k in "ztpxr"}
    scal = SENTINELS.copy()
    scal[S_GAMMA], scal[S_DELTA] = 2.3719, 3.1427
    scal[S_GAMMA_PREV], scal[S_ALPHA_PREV] = 1.7353, 2.9131
    return SimpleNamespace(kind=kind, spec=spec, gx=gx, gy=gy, gz=gz, rank=rank,
                           nranks=nranks, z0=z0, z1=z1, plane=plane,
                           owned_global=owned, ghost_global=ghost,
                           nowned=nowned, ninterior=ninterior,
                           nborder=nowned - ninterior, nghost=nghost,
                           nlocal=nowned + nghost,
                           border_base=ninterior if nghost else nowned,
                           wg=wg, w_old=wg[np.concatenate([owned, ghost])],
                           scal=scal, _products=None, **vec)


def stencil_products(case):
    """The oracle's matA part, matO part and their sum on the owned rows
    (computed once per case): name -> (value, magnitude, products)."""
    if case._products is None:
        o = case.owned_global
        args = (case.gx, case.gy, case.gz, case.spec["offsets"],
                case.spec["diag"], case.wg)
        A = tuple(a[o] for a in stencil_apply(*args, part=("owned", case.z0, case.z1)))
        if case.nghost:
            O = tuple(a[o] for a in stencil_apply(*args, part=("ghost", case.z0, case.z1)))
            assert not O[2][:case.ninterior].any() and O[2][case.ninterior:].all()
            full = tuple(a + b for a, b in zip(A, O))
        else:
            O, full = None, A
        case._products = {"A": A, "O": O, "full": full}
    return case._products


def stencil_mf(case, dev):
    """The matrix-free operator tables of the case on ``dev``, from the
    host-side table builder (no GPU, no compiled extension needed)."""
    from acg_amd.gen.device_slab import mf_tables_from, stencil_slab_tables

    tab = stencil_slab_tables(case.gx, case.gy, case.gz, case.spec, case.rank,
                              case.nranks)
    return mf_tables_from(tab, tab["zs_own"].to(dev), tab["pb"].to(dev),
                          tab["offs"].to(dev))


def vec_case(n, pt_zero=False):
    rng = np.random.default_rng(4000 + n)
    scal = SENTINELS.copy()
    scal[S_RR] = 1.3719
    scal[S_PT] = 0.0 if pt_zero else 2.9131
    return SimpleNamespace(n=n, r=rand_values(n, rng), x=rand_values(n, rng),
                           p=rand_values(n, rng), t=rand_values(n, rng),
                           w=rand_values(n, rng),
                           dinv=rng.uniform(0.5, 2.0, size=n), scal=scal)


# ---------------------------------------------------------------------------
# expectations

def sell_blocks(nslices):
    return (nslices * C + 255) // 256


def elem_blocks(n):
    return max(1, min(4096, (n + 1023) // 1024))


def sell_spmv_expect(case, perm=None, dotslot=S_PT, dot_accum=False):
    e = Expect("k_spmv_sell")
    xh = hp(case.x)
    y, M = spmv(case.rowptr, case.cols, case.vals, xh)
    L = sell_padded_len(case.rowptr, perm)
    e.add("y", y, M, L)
    ty = bound(M, L)
    d, tol = dot(xh[:case.nrows], y, tb=ty,
                 add=SENTINELS[dotslot] if dot_accum else None)
    e.add_tol(f"scal{dotslot}", d, tol)
    e.scalars(SENTINELS, touched=(dotslot,))
    return e


def bsell_spmv_expect(case, dotslot=-1, dot_accum=False):
    e = Expect("k_spmv_bsell")
    xh = hp(case.x)
    y, M = spmv(case.rowptr, case.cols, case.vals, xh)
    L = bsell_padded_len(case.rowptr, case.cols, case.dof)
    e.add("y", y, M, L)
    if dotslot >= 0:
        d, tol = dot(xh[:case.nrows], y, tb=bound(M, L),
                     add=SENTINELS[dotslot] if dot_accum else None)
        e.add_tol(f"scal{dotslot}", d, tol)
    e.scalars(SENTINELS, touched=(dotslot,))
    return e


def bsell_daypx_scal(beta_zero):
    scal = SENTINELS.copy()
    scal[S_RR] = 1.3719
    scal[S_RR_PREV] = np.inf if beta_zero else 2.9131
    return scal


def bsell_daypx_expect(case, beta_zero):
    assert case.ncols == case.nrows
    e = Expect("k_spmv_bsell_daypx")
    scal = bsell_daypx_scal(beta_zero)
    beta = ratio_coeff(scal[S_RR], scal[S_RR_PREV])
    pn = beta * hp(case.pold) + hp(case.r)
    Mp = abs(beta) * habs(hp(case.pold)) + habs(hp(case.r))
    if beta_zero:
        e.add_exact("pnew", case.r)
    else:
        e.add("pnew", pn, Mp)
    y, My = spmv(case.rowptr, case.cols, case.vals, pn, xM=Mp)
    L = bsell_padded_len(case.rowptr, case.cols, case.dof)
    e.add("y", y, My, L)
    d, tol = dot(pn, y, ta=bound(Mp), tb=bound(My, L))
    e.add_tol(f"scal{S_PT}", d, tol)
    e.scalars(scal, touched=(S_PT,))
    return e


def pipe_coeffs(scal, first):
    """(beta, alpha, cancellation factor of alpha's denominator)."""
    if first:
        return hps(0.0), ratio_coeff(scal[S_GAMMA], scal[S_DELTA]), 1.0
    beta = ratio_coeff(scal[S_GAMMA], scal[S_GAMMA_PREV])
    sub = beta * ratio_coeff(scal[S_GAMMA], scal[S_ALPHA_PREV])
    den = hps(scal[S_DELTA]) - sub
    kappa = float((abs(hps(scal[S_DELTA])) + abs(sub)) / abs(den))
    return beta, hps(scal[S_GAMMA]) / den, kappa


def pipe_expect(case, first):
    """One full megafused iteration (all passes + finalize)."""
    e = Expect("k_sell_pipe")
    n = case.nowned
    w = hp(case.w_old)
    q, Mq = spmv(case.rowptr, case.cols, case.vals, w)
    L = sell_padded_len(case.A[0])
    if case.nborder:
        L[case.ninterior:] += sell_padded_len(case.O[0])
    _pipelined_update(e, case, first, q, Mq, L, w[:n], "w_new")
    if case.nghost:
        e.add_exact("w_new_tail", np.full(case.nghost, np.nan))
    if case.nborder:  # the matA pass alone must leave the border rows alone
        for k in "ztpxr":
            e.add_exact(f"matA/{k}_border", getattr(case, k)[case.ninterior:])
        e.add_exact("matA/w_new_border", np.full(case.nborder + case.nghost, np.nan))
    return e


def _pipelined_update(e, case, first, q, Mq, L, wo, wname):
    """Ghysels-Vanroose 6-vector update + next gamma/delta + rotation, given
    q = A w with magnitude Mq built from L products per element."""
    beta, alpha, kappa = pipe_coeffs(case.scal, first)
    assert kappa <= 8.0, f"alpha denominator cancels too much: {kappa}"
    ab, aa = abs(beta), abs(alpha)
    z0, t0, p0, x0, r0 = (hp(getattr(case, k)) for k in "ztpxr")
    z, Mz = q + beta * z0, Mq + ab * habs(z0)
    t, Mt = wo + beta * t0, habs(wo) + ab * habs(t0)
    p, Mp = r0 + beta * p0, habs(r0) + ab * habs(p0)
    x, Mx = x0 + alpha * p, habs(x0) + aa * Mp
    r, Mr = r0 - alpha * t, habs(r0) + aa * Mt
    wn, Mw = wo - alpha * z, habs(wo) + aa * Mz
    e.add("z", z, Mz, L)
    e.add("t", t, Mt)
    e.add("p", p, Mp)
    e.add("x", x, Mx)
    e.add("r", r, Mr)
    e.add(wname, wn, Mw, L)
    g, gtol = dot(r, r, ta=bound(Mr), tb=bound(Mr))
    d, dtol = dot(wn, r, ta=bound(Mw, L), tb=bound(Mr))
    e.add_exact(f"scal{S_GAMMA_PREV}", case.scal[S_GAMMA])
    e.add(f"scal{S_ALPHA_PREV}", alpha, aa)
    e.add_tol(f"scal{S_GAMMA}", g, gtol)
    e.add_tol(f"scal{S_DELTA}", d, dtol)
    e.scalars(case.scal, touched=(S_GAMMA, S_DELTA, S_GAMMA_PREV, S_ALPHA_PREV))


def stencil_spmv_expect(case, fused, kernel="k_stencil_spmv"):
    """matA pass (fused dot: set) and, on a rank with ghosts, the matO pass
    over the border rows (fused dot: accumulate).  The accumulated slot is
    the sum of two computed dots; the rounding of that one addition is
    covered by the 8 spare roundings each dot tolerance carries."""
    e = Expect(kernel)
    n, ni = case.nowned, case.ninterior
    P = stencil_products(case)
    xo = hp(case.w_old[:n])
    qA, MA, LA = P["A"]
    q, M, L = P["full"]
    tail = np.full(case.nghost, np.nan)
    e.add("matA/y", qA, MA, LA)
    e.add_exact("matA/y_tail", tail)
    e.add("y", q, M, L)
    e.add_exact("y_tail", tail)
    e.add_same("matA/y_interior", "y_interior")
    if fused:
        d, tol = dot(xo, qA, tb=bound(MA, LA))
        e.add_tol(f"matA/scal{S_PT}", d, tol)
        if case.nborder:
            qO, MO, LO = P["O"]
            dO, tolO = dot(xo[ni:], qO[ni:], tb=bound(MO[ni:], LO[ni:]))
            d, tol = d + dO, tol + tolO
        e.add_tol(f"scal{S_PT}", d, tol)
    for i in range(S_NSLOTS):
        if not (fused and i == S_PT):
            e.add_exact(f"matA/scal{i}", SENTINELS[i])
    e.scalars(SENTINELS, touched=(S_PT,) if fused else ())
    return e


def stencil_pipe_expect(case, first, kernel="k_stencil_pipe"):
    """One full megafused matrix-free iteration (matA pass, matO pass,
    finalize) plus the state after the matA pass alone."""
    e = Expect(kernel)
    n, ni = case.nowned, case.ninterior
    P = stencil_products(case)
    q, Mq, L = P["full"]
    _pipelined_update(e, case, first, q, Mq, L, hp(case.w_old[:n]), "w_new")
    e.add_exact("w_new_tail", np.full(case.nghost, np.nan))
    if case.nborder:
        for k in "ztpxr":
            e.add_exact(f"matA/{k}_border", getattr(case, k)[ni:])
        e.add_exact("matA/w_new_border", np.full(case.nborder + case.nghost, np.nan))
        qA, MA, LA = P["A"]
        e.add("matA/qpart", qA[ni:], MA[ni:], LA[ni:])
        e.add_same("matA/qpart", "qpart")  # the matO pass only reads it
    else:
        e.add_exact("qpart", np.full(1, np.nan))
    return e


def stencil_blocks(case, walk, n):
    """Blocks the launchers start for an n-row pass (before the megafused
    kernels' cap): elem_grid, or one thread per (x, y) column."""
    return (case.plane + 255) // 256 if walk else elem_blocks(n)


def run_stencil_spmv(ops, case, dev, mf, fused):
    n, ni = case.nowned, case.ninterior
    walk = mf["w7"] is not None
    x = _t(case.w_old, dev)
    y = _nan(case.nlocal, dev)
    scal = _t(SENTINELS, dev)
    partials = _nan(2 * MAXG, dev)
    kw = dict(partials=partials, scal=scal, dotslot=S_PT) if fused else {}
    ops.stencil_spmv(mf, n, 0, x, y, mato=False, dot_accum=False, **kw)
    yy = _np(y)
    got = {"matA/y": yy[:n], "matA/y_tail": yy[n:], "matA/y_interior": yy[:ni]}
    got.update({f"matA/{k}": v for k, v in _scal_out({}, scal).items()})
    nb = min(MAXG, stencil_blocks(case, walk, n))
    if case.nborder:
        ops.stencil_spmv(mf, case.nborder, ni, x, y, mato=True, dot_accum=True, **kw)
        nb = max(nb, stencil_blocks(case, False, case.nborder))
    yy = _np(y)
    got.update({"y": yy[:n], "y_tail": yy[n:], "y_interior": yy[:ni]})
    _partials_out(got, partials, nb if fused else 0)
    return _scal_out(got, scal)


def run_stencil_pipe(ops, case, dev, mf, first):
    """matA pass, (matO pass with partials_off = nbA,) finalize -- the call
    protocol of the solver."""
    n, ni = case.nowned, case.ninterior
    v = {k: _t(getattr(case, k), dev) for k in "ztpxr"}
    w_old = _t(case.w_old, dev)
    w_new = _nan(case.nlocal, dev)
    qpart = _nan(max(case.nborder, 1), dev)
    scal = _t(case.scal, dev)
    partials = _nan(2 * MAXG, dev)
    nbA = ops.stencil_pipe(mf, n, 0, case.border_base, w_old, qpart, v["z"],
                           v["t"], v["p"], v["x"], v["r"], w_new, scal, first,
                           partials, 0, mato=False)
    got, nbO = {}, 0
    if case.nborder:
        for k in "ztpxr":
            got[f"matA/{k}_border"] = _np(v[k][ni:])
        got["matA/w_new_border"] = _np(w_new[ni:])
        got["matA/qpart"] = _np(qpart)
        nbO = ops.stencil_pipe(mf, case.nborder, ni, ni, w_old, qpart, v["z"],
                               v["t"], v["p"], v["x"], v["r"], w_new, scal,
                               first, partials, nbA, mato=True)
    ops.pipelined_finalize(partials, nbA + nbO, scal, first)
    for k in "ztpxr":
        got[k] = _np(v[k])
    got["qpart"] = _np(qpart)
    got["w_new"] = _np(w_new[:n])
    got["w_new_tail"] = _np(w_new[n:])
    got["nbA"], got["nbO"] = int(nbA), int(nbO)
    _partials_out(got, partials, nbA + nbO)
    return _scal_out(got, scal)


def fused_case(n):
    """Inputs of the unfused pipelined update: q is a plain input vector."""
    rng = np.random.default_rng(5000 + n)
    scal = SENTINELS.copy()
    scal[S_GAMMA], scal[S_DELTA] = 2.3719, 3.1427
    scal[S_GAMMA_PREV], scal[S_ALPHA_PREV] = 1.7353, 2.9131
    return SimpleNamespace(n=n, scal=scal,
                           **{k: rand_values(n, rng) for k in "ztpxrwq"})


def fused_expect(case, first):
    e = Expect("k_pipelined_fused")
    q = hp(case.q)
    _pipelined_update(e, case, first, q, habs(q), 0, hp(case.w), "w")
    return e


def run_fused(ops, case, dev, first, **kw):
    v = {k: _t(getattr(case, k), dev) for k in "ztpxrwq"}
    scal = _t(case.scal, dev)
    partials = _nan(2 * MAXG, dev)
    ops.pipelined_fused(v["z"], v["t"], v["p"], v["x"], v["r"], v["w"], v["q"],
                        scal, partials, case.n, first, **kw)
    got = {k: _np(v[k]) for k in "ztpxrw"}
    _partials_out(got, partials, elem_blocks(case.n))
    return _scal_out(got, scal)


def csr_blocks(nrows, lanes):
    return min(MAXG, (nrows + 256 // lanes - 1) // (256 // lanes))


def csr_spmv_expect(case, rowbase=0, accum=False, dot_accum=False,
                    kernel="spmv_csr_vector"):
    """CSR SpMV into y[rowbase:rowbase+nrows] of a buffer with ``rowbase``
    extra rows on either side; ``accum`` adds to y0 = case.x[:nrows]
    reversed (any known finite vector does)."""
    e = Expect(kernel)
    xh = hp(case.x)
    c, M = spmv(case.rowptr, case.cols, case.vals, xh)
    L = np.diff(case.rowptr)
    y, My = c, M
    if accum:
        y0 = hp(csr_y0(case))
        y, My = y0 + c, habs(y0) + M
    e.add("y", y, My, L)
    e.add_exact("y_outside", np.full(2 * rowbase, np.nan))
    d, tol = dot(xh[rowbase:rowbase + case.nrows], c, tb=bound(M, L),
                 add=SENTINELS[S_PT] if dot_accum else None)
    e.add_tol(f"scal{S_PT}", d, tol)
    e.scalars(SENTINELS, touched=(S_PT,))
    return e


def csr_y0(case):
    return case.x[:case.nrows][::-1].copy()


def run_csr_spmv(ops, case, dev, *, rowbase=0, accum=False, dot_accum=False,
                 col64=False, lanes=None, binned=False):
    n = case.nrows
    y = _nan(n + 2 * rowbase, dev)
    if accum:
        y[rowbase:rowbase + n] = _t(csr_y0(case), dev)
    scal = _t(SENTINELS, dev)
    partials = _nan(2 * MAXG, dev)
    cols = _t(case.cols.astype(np.int64 if col64 else np.int32), dev)
    kw = dict(rowbase=rowbase, accum=accum, partials=partials, scal=scal,
              dotslot=S_PT, dot_accum=dot_accum)
    if binned:
        from acg_amd.ops.gpu_ops import build_row_bins  # host-side numpy prep

        rowlist, bins = build_row_bins(case.rowptr)
        ops.spmv_binned(_t(case.rowptr, dev), cols, _t(case.vals, dev),
                        _t(rowlist, dev), bins, _t(case.x, dev), y, **kw)
        nb = sum(csr_blocks(cnt, ln) for _, cnt, ln in bins)
    else:
        if lanes is not None:
            kw["lanes"] = lanes
        ops.spmv(_t(case.rowptr, dev), cols, _t(case.vals, dev),
                 _t(case.x, dev), y, **kw)
        nb = csr_blocks(n, lanes or 16)
    yy = _np(y)
    got = {"y": yy[rowbase:rowbase + n],
           "y_outside": np.concatenate([yy[:rowbase], yy[rowbase + n:]])}
    _partials_out(got, partials, nb)
    return _scal_out(got, scal)


def ratio_update_expect(case, op, n_act):
    """axpy_ratio (y += sign*(num/den)*x, sign = -1) or daypx_ratio
    (y = (num/den)*y + x) on the first n_act elements; num/den =
    scal[S_RR]/scal[S_PT]."""
    e = Expect(f"k_{op}")
    a = ratio_coeff(case.scal[S_RR], case.scal[S_PT])
    y0, x0 = hp(case.r[:n_act]), hp(case.x[:n_act])
    if op == "axpy_ratio":
        e.add("y", y0 - a * x0, habs(y0) + abs(a) * habs(x0))
    else:
        e.add("y", a * y0 + x0, abs(a) * habs(y0) + habs(x0))
    e.add_exact("y_tail", case.r[n_act:])
    e.scalars(case.scal)
    return e


def run_ratio_update(ops, case, dev, op, n_act):
    y, scal = _t(case.r, dev), _t(case.scal, dev)
    if op == "axpy_ratio":
        ops.axpy_ratio(y, _t(case.x, dev), scal, S_RR, S_PT, sign=-1.0, n=n_act)
    else:
        ops.daypx_ratio(y, _t(case.x, dev), scal, S_RR, S_PT, n=n_act)
    yy = _np(y)
    return _scal_out({"y": yy[:n_act], "y_tail": yy[n_act:]}, scal)


def run_exact_ops(ops, dev, idx64):
    """pack_gather, zero_scalars, cg_prep_pt, cg_prep_rr: pure data movement,
    every result is bitwise defined.  Returns (expect, got)."""
    rng = np.random.default_rng(6000)
    e, got = Expect("k_pack_gather/k_zero_scalars/k_cg_prep"), {}
    x = rand_values(1500, rng)
    idx = rng.integers(0, 1500, size=777).astype(np.int64 if idx64 else np.int32)
    send = _nan(777 + 5, dev)
    ops.pack_gather(send[:777], _t(x, dev), _t(idx, dev))
    e.add_exact("sendbuf", np.concatenate([x[idx], np.full(5, np.nan)]))
    got["sendbuf"] = _np(send)
    want = SENTINELS.copy()
    want[2:5] = 0.0
    scal = _t(SENTINELS, dev)
    ops.zero_scalars(scal, 2, 3)
    e.add_exact("zeroed", want)
    got["zeroed"] = _np(scal)
    scal = _t(SENTINELS, dev)
    ops.cg_prep_pt(scal)
    ops.cg_prep_rr(scal)
    want = SENTINELS.copy()
    want[S_PT], want[S_RR_PREV] = 0.0, SENTINELS[S_RR]
    e.add_exact("prepped", want)
    got["prepped"] = _np(scal)
    return e, got


def pcg_expect(case):
    e = Expect("k_pcg_fused_update")
    alpha = ratio_coeff(case.scal[S_RR], case.scal[S_PT])
    aa = abs(alpha)
    r0, x0, p0, t0 = (hp(getattr(case, k)) for k in "rxpt")
    dinv = hp(case.dinv)
    r, Mr = r0 - alpha * t0, habs(r0) + aa * habs(t0)
    x, Mx = x0 + alpha * p0, habs(x0) + aa * habs(p0)
    z, Mz = dinv * r, dinv * Mr
    if float(case.scal[S_PT]) == 0.0:
        e.add_exact("r", case.r)
        e.add_exact("x", case.x)
    else:
        e.add("r", r, Mr)
        e.add("x", x, Mx)
    e.add("z", z, Mz)
    e.add_same("z", "dinv*r")
    rz, rztol = dot(r, z, ta=bound(Mr), tb=bound(Mz))
    rr, rrtol = dot(r, r, ta=bound(Mr), tb=bound(Mr))
    e.add_exact(f"scal{S_RR_PREV}", case.scal[S_RR])
    e.add_tol(f"scal{S_RR}", rz, rztol)
    e.add_tol(f"scal{S_GAMMA}", rr, rrtol)
    e.scalars(case.scal, touched=(S_RR, S_RR_PREV, S_GAMMA))
    return e


def cg_update_expect(case):
    e = Expect("k_cg_fused_update")
    alpha = ratio_coeff(case.scal[S_RR], case.scal[S_PT])
    aa = abs(alpha)
    r0, x0, p0, t0 = (hp(getattr(case, k)) for k in "rxpt")
    r, Mr = r0 - alpha * t0, habs(r0) + aa * habs(t0)
    x, Mx = x0 + alpha * p0, habs(x0) + aa * habs(p0)
    e.add("r", r, Mr)
    e.add("x", x, Mx)
    rr, rrtol = dot(r, r, ta=bound(Mr), tb=bound(Mr))
    e.add_exact(f"scal{S_RR_PREV}", case.scal[S_RR])
    e.add_tol(f"scal{S_RR}", rr, rrtol)
    e.scalars(case.scal, touched=(S_RR, S_RR_PREV))
    return e


def dot_expect(case, slot, accumulate):
    e = Expect("k_dot")
    d, tol = dot(hp(case.r), hp(case.w),
                 add=SENTINELS[slot] if accumulate else None)
    e.add_tol(f"scal{slot}", d, tol)
    e.scalars(SENTINELS, touched=(slot,))
    return e


def dot2_expect(case, accumulate):
    e = Expect("k_dot2")
    g, gtol = dot(hp(case.r), hp(case.r),
                  add=SENTINELS[S_GAMMA] if accumulate else None)
    d, dtol = dot(hp(case.w), hp(case.r),
                  add=SENTINELS[S_DELTA] if accumulate else None)
    e.add_tol(f"scal{S_GAMMA}", g, gtol)
    e.add_tol(f"scal{S_DELTA}", d, dtol)
    e.scalars(SENTINELS, touched=(S_GAMMA, S_DELTA))
    return e


# ---------------------------------------------------------------------------
# runners: drive ``ops`` (torch_ref or gpu_ops) on poisoned buffers and
# collect everything the expectations name

def _t(a, dev):
    import torch

    return torch.from_numpy(np.array(a, copy=True, order="C")).to(dev)  # never alias the case


def _nan(n, dev):
    import torch

    return torch.full((n,), float("nan"), dtype=torch.float64, device=dev)


def _np(t):
    return t.detach().cpu().numpy().copy()


def _scal_out(got, scal):
    s = _np(scal)
    for i in range(S_NSLOTS):
        got[f"scal{i}"] = s[i:i + 1]
    return got


def _partials_out(got, partials, nblocks):
    got["partials"] = _np(partials)
    got["nblocks"] = int(nblocks)
    return got


def run_sell_spmv(ops, case, dev, *, col64=False, variant=None, sigma=1,
                  dotslot=S_PT, dot_accum=False, packed=None):
    from acg_amd.ops import torch_ref

    if packed is None:
        packed = torch_ref.sell_from_csr(
            case.rowptr, case.cols.astype(np.int64 if col64 else np.int32),
            case.vals, sigma=sigma)
    sp, sc, sv = packed[:3]
    kw = {}
    if len(packed) == 4:
        kw["perm"] = _t(packed[3], dev)
    if variant is not None:
        kw["variant"] = variant
    y = _nan(case.nrows, dev)
    scal = _t(SENTINELS, dev)
    partials = _nan(2 * MAXG, dev)
    ops.spmv_sell(_t(sp, dev), _t(sc, dev), _t(sv, dev), case.nrows,
                  _t(case.x, dev), y, partials=partials, scal=scal,
                  dotslot=dotslot, dot_accum=dot_accum, **kw)
    got = {"y": _np(y)}
    _partials_out(got, partials, sell_blocks(case.nslices))
    return _scal_out(got, scal)


def pack_bsell(case, dev):
    from acg_amd.ops import torch_ref

    bptr, bcol, bvals, _ = torch_ref.bsell_from_csr(case.rowptr, case.cols,
                                                    case.vals, case.dof)
    return _t(bptr, dev), _t(bcol, dev), _t(bvals, dev)


def run_bsell_spmv(ops, case, dev, *, dotslot=-1, dot_accum=False, packed=None):
    bptr, bcol, bvals = packed if packed is not None else pack_bsell(case, dev)
    y = _nan(case.nrows, dev)
    scal = _t(SENTINELS, dev)
    partials = _nan(2 * MAXG, dev)
    kw = dict(partials=partials, scal=scal, dotslot=dotslot,
              dot_accum=dot_accum) if dotslot >= 0 else {}
    ops.spmv_bsell(bptr, bcol, bvals, case.nnodes, case.dof, _t(case.x, dev),
                   y, **kw)
    got = {"y": _np(y)}
    _partials_out(got, partials, sell_blocks(bptr.numel() - 1) if dotslot >= 0 else 0)
    return _scal_out(got, scal)


def run_bsell_daypx(ops, case, dev, beta_zero, packed=None):
    bptr, bcol, bvals = packed if packed is not None else pack_bsell(case, dev)
    y, pnew = _nan(case.nrows, dev), _nan(case.nrows, dev)
    scal = _t(bsell_daypx_scal(beta_zero), dev)
    partials = _nan(2 * MAXG, dev)
    ops.spmv_bsell_daypx(bptr, bcol, bvals, case.nnodes, case.dof,
                         _t(case.pold, dev), _t(case.r, dev), pnew, y, scal,
                         partials, S_PT)
    got = {"y": _np(y), "pnew": _np(pnew)}
    _partials_out(got, partials, sell_blocks(bptr.numel() - 1))
    return _scal_out(got, scal)


def run_pipe(ops, case, dev, first):
    """matA pass, (matO pass with partials_off = nbA,) finalize."""
    from acg_amd.ops import torch_ref

    n = case.nowned

    def pack(csr):
        sp, sc, sv = torch_ref.sell_from_csr(csr[0], csr[1].astype(np.int32), csr[2])
        return _t(sp, dev), _t(sc, dev), _t(sv, dev)

    v = {k: _t(getattr(case, k), dev) for k in "ztpxr"}
    w_old = _t(case.w_old, dev)
    w_new = _nan(case.nlocal, dev)
    qpart = _nan(max(case.nborder, 1), dev)
    scal = _t(case.scal, dev)
    partials = _nan(2 * MAXG, dev)
    nb = ops.sell_pipe(*pack(case.A), n, 0, case.border_base, w_old, qpart,
                       v["z"], v["t"], v["p"], v["x"], v["r"], w_new, scal,
                       first, partials, 0, mato=False)
    got = {}
    if case.nborder:
        for k in "ztpxr":
            got[f"matA/{k}_border"] = _np(v[k][case.ninterior:])
        got["matA/w_new_border"] = _np(w_new[case.ninterior:])
        nb += ops.sell_pipe(*pack(case.O), case.nborder, case.ninterior,
                            case.ninterior, w_old, qpart, v["z"], v["t"],
                            v["p"], v["x"], v["r"], w_new, scal, first,
                            partials, nb, mato=True)
    ops.pipelined_finalize(partials, nb, scal, first)
    for k in "ztpxr":
        got[k] = _np(v[k])
    got["w_new"] = _np(w_new[:n])
    got["w_new_tail"] = _np(w_new[n:])
    _partials_out(got, partials, nb)
    return _scal_out(got, scal)


def run_pcg(ops, case, dev):
    r, x, z = _t(case.r, dev), _t(case.x, dev), _nan(case.n, dev)
    scal = _t(case.scal, dev)
    partials = _nan(2 * MAXG, dev)
    ops.pcg_fused_update(r, x, _t(case.p, dev), _t(case.t, dev), z,
                         _t(case.dinv, dev), scal, partials, case.n)
    got = {"r": _np(r), "x": _np(x), "z": _np(z)}
    got["dinv*r"] = case.dinv * got["r"]
    _partials_out(got, partials, elem_blocks(case.n))
    return _scal_out(got, scal)


def run_cg_update(ops, case, dev):
    r, x = _t(case.r, dev), _t(case.x, dev)
    scal = _t(case.scal, dev)
    partials = _nan(2 * MAXG, dev)
    ops.cg_fused_update(r, x, _t(case.p, dev), _t(case.t, dev), scal,
                        partials, case.n)
    got = {"r": _np(r), "x": _np(x)}
    _partials_out(got, partials, elem_blocks(case.n))
    return _scal_out(got, scal)


def run_dot(ops, case, dev, slot, accumulate):
    scal = _t(SENTINELS, dev)
    partials = _nan(2 * MAXG, dev)
    ops.dot(_t(case.r, dev), _t(case.w, dev), partials, scal, slot,
            accumulate=accumulate)
    return _scal_out(_partials_out({}, partials, elem_blocks(case.n)), scal)


def run_dot2(ops, case, dev, accumulate):
    scal = _t(SENTINELS, dev)
    partials = _nan(2 * MAXG, dev)
    ops.dot2(_t(case.r, dev), _t(case.w, dev), partials, scal, case.n,
             accumulate=accumulate)
    return _scal_out(_partials_out({}, partials, elem_blocks(case.n)), scal)


def check_partials(got, halves):
    """GPU only: slots >= nblocks keep their NaN prefill bits in both halves
    of the scratch; the slots the launch owns hold finite sums."""
    part, nb = got["partials"], got["nblocks"]
    nanbits = np.array([np.nan]).view(np.int64)[0]
    bits = part.view(np.int64)
    assert np.all(bits[nb:MAXG] == nanbits), "partials beyond nblocks written"
    lo = MAXG + (nb if halves == 2 else 0)
    assert np.all(bits[lo:] == nanbits), "second-half partials written"
    assert np.all(np.isfinite(part[:nb]))
    if halves == 2:
        assert np.all(np.isfinite(part[MAXG:MAXG + nb]))


# ---------------------------------------------------------------------------
# the one-launch device CG (k_cg_device): case, step-chained expectations,
# runner and the check procedures the CPU (torch_ref, mutants) and GPU tests
# share

BAR_STATE_WORDS = 400
OUT2_SENTINEL = (-7, -9)
DEVCG_KS = (0, 1, 2, 3)


def device_cg_blocks(nslices):
    """Blocks the launcher asks for before the residency cap."""
    return sell_blocks(nslices)


def device_cg_case(nslices, zero_b=False, zero_x0=False):
    """Symmetric, strictly diagonally dominant system (diagonal >= 2x the
    absolute off-diagonal row sum: Jacobi-scaled spectrum in [1/2, 3/2]) of
    nslices*64 - 13 rows.  The 64-row slices cycle through three classes of
    row length (the diagonal included): at most 3 (only the remainder loop
    of the 4-way unrolled SpMV runs), 5..7 (one unrolled trip and a
    remainder) and up to 13 (several trips).  Couplings stay inside a class:
    neighbours in the same slice, and rows 192 and 384 further on, which
    belong to other 256-thread blocks."""
    rng = np.random.default_rng(8000 + nslices)
    n = nslices * C - 13
    i = np.arange(n, dtype=np.int64)
    lane = i % C
    cls = ((i // C) + nslices) % 3
    ei, ej = [], []

    def link(mask, d):
        m = mask & (i + d < n) & (rng.random(n) < 0.7)
        ei.append(i[m])
        ej.append(i[m] + d)

    link((cls == 0) & (lane % 2 == 0) & (lane < 32), 1)
    link((cls == 0) & (lane >= 32), 3 * C)
    for d in (1, 2):
        link((cls == 1) & (lane + d < C), d)
    link(cls == 1, 3 * C)
    for d in (1, 2, 3, 5):
        link((cls == 2) & (lane + d < C), d)
    for d in (3 * C, 6 * C):
        link(cls == 2, d)
    ei, ej = np.concatenate(ei), np.concatenate(ej)
    w = rng.uniform(0.5, 2.0, size=len(ei)) * rng.choice([-1.0, 1.0], size=len(ei))
    off = (np.bincount(ei, np.abs(w), minlength=n)
           + np.bincount(ej, np.abs(w), minlength=n))
    diag = 2.0 * off * rng.uniform(1.0, 1.25, size=n) + rng.uniform(0.5, 2.0, size=n)
    assert np.all(diag >= 2.0 * off) and np.all(diag > 0)
    rows = np.concatenate([ei, ej, i])
    cols = np.concatenate([ej, ei, i])
    vals = np.concatenate([w, w, diag])
    order = np.lexsort((cols, rows))
    rows, cols, vals = rows[order], cols[order], vals[order]
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=rowptr[1:])
    L = sell_padded_len(rowptr)
    per_slice = L[::C]
    if nslices >= 3:
        assert (per_slice < 4).any() and (per_slice % 4 != 0).any() \
            and (per_slice >= 8).any(), "a row-length class is missing"
    else:
        assert (per_slice > 4).any() and (per_slice % 4 != 0).any()
    rv = lambda: rng.uniform(0.5, 2.0, size=n) * rng.choice([-1.0, 1.0], size=n)
    b, x0 = rv(), rv()
    return SimpleNamespace(nslices=nslices, nrows=n, ncols=n, rowptr=rowptr,
                           cols=cols, vals=vals, L=L,
                           b=np.zeros(n) if zero_b else b,
                           x0=np.zeros(n) if zero_x0 else x0,
                           _hp=None, _packed={}, _dev={}, _expect={})


def _devcg_spmv(case, x, xM):
    """A x and |A| xM by row (sorted CSR without empty rows: one reduceat)."""
    if case._hp is None:
        case._hp = hp(case.vals)
    a, starts = case._hp, case.rowptr[:-1]
    return (np.add.reduceat(a * x[case.cols], starts),
            np.add.reduceat(habs(a) * xM[case.cols], starts))


def device_cg_init_expect(case):
    """The maxits = 0 launch.  t = A x0 carries L products per row; r0 =
    fl(b - t) adds one rounding, relative to |r0| <= |b| + |A||x0|, so it
    stays within (L + 48) u (|b| + |A||x0|) of the exact b - A x0."""
    if "init" in case._expect:
        return case._expect["init"]
    e = Expect("k_cg_device/init")
    xh, bh = hp(case.x0), hp(case.b)
    t, Mt = _devcg_spmv(case, xh, habs(xh))
    r, Mr = bh - t, habs(bh) + Mt
    e.add("t", t, Mt, case.L)
    e.add("r", r, Mr, case.L)
    e.add_same("p", "r")
    e.add_exact("x", case.x0)
    bn, bntol = dot(bh, bh)
    rr, rrtol = dot(r, r, ta=bound(Mr, case.L), tb=bound(Mr, case.L))
    e.add_tol(f"scal{S_BNRM2}", bn, bntol)
    e.add_tol(f"scal{S_RR}", rr, rrtol)
    e.add_same(f"scal{S_RR_PREV}", f"scal{S_RR}")
    e.scalars(SENTINELS, touched=(S_RR, S_PT, S_RR_PREV, S_BNRM2))
    e.add_exact(f"scal{S_PT}", SENTINELS[S_PT])
    case._expect["init"] = e
    return e


_DEVCG_STATE = ("x", "r", "p", f"scal{S_RR}")
_DEVCG_REPORTED = ("t", "r", f"scal{S_PT}", f"scal{S_RR}")


def device_cg_step_expect(case, state, reported, k=None):
    """One CG step from EXACTLY the fp64 state (x_k, r_k, p_k, rr_k) that
    the ``maxits = k`` launch returned, for the ``maxits = k + 1`` launch
    (``reported``), which repeats the first k steps bit for bit.

    No error bound is carried from step to step, and none through the
    coefficients either: the kernel publishes every value that the next
    stage of a step reads back from memory -- t, (p,t), the new r and the
    new (r,r) -- so each stage is compared with the high-precision result
    of ITS inputs as the kernel reports them, and each reported value is
    itself checked against the stage before:

      t      = A p_k                   L products per row
      (p,t)  = (p_k, A p_k)            dot()'s propagated tolerance
      alpha  = rr_k / (p,t)'           1 rounding
      r      = r_k - alpha t'          alpha, product, sum: 3 roundings
      x      = x_k + alpha p_k         3 roundings
      (r,r)  from that r               dot()'s propagated tolerance
      beta   = (r,r)' / rr_k           1 rounding (safe_div: 0 when rr_k = 0)
      p      = beta p_k + r'           3 roundings

    (primes: as reported).  Each rounding is relative to a partial result
    bounded by the magnitude M, so 3 u M (1 + O(u)) is far inside the
    module's 48 u M; no constant is added."""
    bits = [np.asarray(state[k_], np.float64).tobytes() for k_ in _DEVCG_STATE] \
        + [np.asarray(reported[k_], np.float64).tobytes() for k_ in _DEVCG_REPORTED]
    hit = case._expect.get(("step", k))
    if k is not None and hit is not None and hit[0] == bits:
        return hit[1]
    e = Expect("k_cg_device/step")
    xk, rk, pk = hp(state["x"]), hp(state["r"]), hp(state["p"])
    rrk = float(state[f"scal{S_RR}"][0])
    t, Mt = _devcg_spmv(case, pk, habs(pk))
    e.add("t", t, Mt, case.L)
    pt, pttol = dot(pk, t, tb=bound(Mt, case.L))
    e.add_tol(f"scal{S_PT}", pt, pttol)
    alpha = ratio_coeff(rrk, float(reported[f"scal{S_PT}"][0]))
    aa = abs(alpha)
    tr = hp(reported["t"])
    r, Mr = rk - alpha * tr, habs(rk) + aa * habs(tr)
    e.add("r", r, Mr)
    e.add("x", xk + alpha * pk, habs(xk) + aa * habs(pk))
    rr, rrtol = dot(r, r, ta=bound(Mr), tb=bound(Mr))
    e.add_tol(f"scal{S_RR}", rr, rrtol)
    beta = ratio_coeff(float(reported[f"scal{S_RR}"][0]), rrk)
    rn = hp(reported["r"])
    e.add("p", beta * pk + rn, abs(beta) * habs(pk) + habs(rn))
    if k is not None:
        case._expect[("step", k)] = (bits, e)
    return e


def run_device_cg(ops, case, dev, *, maxits, atol=0.0, rtol=0.0, hier=None,
                  col64=False):
    """One launch on poisoned buffers and a freshly zeroed barrier state;
    returns every output plus the grid cg_device reports."""
    import torch

    from acg_amd.ops import torch_ref

    if col64 not in case._packed:
        case._packed[col64] = torch_ref.sell_from_csr(
            case.rowptr, case.cols.astype(np.int64 if col64 else np.int32),
            case.vals)
    key = (str(dev), col64)
    if key not in case._dev:
        case._dev[key] = tuple(_t(a, dev) for a in case._packed[col64])
    sp, sc, sv = case._dev[key]
    n = case.nrows
    x = _t(case.x0, dev)
    r, p, t = _nan(n, dev), _nan(n, dev), _nan(n, dev)
    scal = _t(SENTINELS, dev)
    partials = _nan(2 * MAXG, dev)
    out2 = torch.tensor(OUT2_SENTINEL, dtype=torch.int32, device=dev)
    bar = torch.zeros(BAR_STATE_WORDS, dtype=torch.int32, device=dev)
    grid = ops.cg_device(sp, sc, sv, n, _t(case.b, dev), x, r, p, t, scal,
                         partials, out2, bar, maxits, atol, rtol, hier=hier)
    got = {"x": _np(x), "r": _np(r), "p": _np(p), "t": _np(t),
           "out2": _np(out2), "grid": int(grid)}
    _partials_out(got, partials, int(grid))
    return _scal_out(got, scal)


DEVCG_BITWISE = ("x", "r", "p", "t", "out2") + tuple(f"scal{i}" for i in range(S_NSLOTS))


def device_cg_same_bits(a, b, names=DEVCG_BITWISE):
    """Names whose bits differ between two launches' outputs."""
    return [k for k in names
            if not np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8),
                                  np.ascontiguousarray(b[k]).view(np.uint8))]


def device_cg_check_every_k(got, got0, k, converged=0):
    """What holds after any launch that ran k steps."""
    assert got["out2"].tolist() == [k, converged], (got["out2"], k, converged)
    for slot in (S_BNRM2, S_RR_PREV):
        assert _bits_equal(got[f"scal{slot}"], got0[f"scal{slot}"]), \
            f"slot {slot} differs from the maxits=0 launch at k={k}"
    for slot in (S_GAMMA, S_DELTA, S_GAMMA_PREV, S_ALPHA_PREV):
        assert _bits_equal(got[f"scal{slot}"], SENTINELS[slot]), f"slot {slot} written"
    check_partials(got, halves=1)


def device_cg_check_chain(launch, case, ks=DEVCG_KS, tag=""):
    """Init check, the per-launch invariants and the chained step k -> k+1
    for every k in ``ks``.  ``launch(maxits=...)`` -> got (zero
    tolerances).  Returns {maxits: got}."""
    ms = sorted({0} | set(ks) | {k + 1 for k in ks})
    gots = {m: launch(maxits=m) for m in ms}
    assert_accepts(device_cg_init_expect(case), gots[0], f"{tag} init")
    for m in ms:
        device_cg_check_every_k(gots[m], gots[0], m)
    for k in ks:
        e = device_cg_step_expect(case, gots[k], gots[k + 1], k)
        assert_accepts(e, gots[k + 1], f"{tag} step {k}->{k + 1}")
    return gots


def device_cg_check_tolerances(launch, case, gots):
    """max(atol, rtol*|b|) selection, the (niterations, converged) pair and
    the early exit, against the zero-tolerance launches ``gots`` (0..6).
    ``launch(maxits=, atol=, rtol=)`` -> got."""
    rr = [float(gots[m][f"scal{S_RR}"][0]) for m in range(7)]
    bnrm = float(np.sqrt(gots[0][f"scal{S_BNRM2}"][0]))
    assert bnrm > 0
    for j0 in (2, 4):
        lo, hi = np.sqrt(rr[j0]), np.sqrt(rr[j0 - 1])
        thr = float(np.sqrt(lo * hi))
        if not 0 < lo < thr < hi:  # the case is unfit, not the code wrong
            raise ValueError(f"(r,r) does not fall from step {j0 - 1} to {j0}")
        j = next(m for m in range(7) if rr[m] <= thr * thr)
        if j < 1:
            raise ValueError("threshold already met by x0")
        for atol, rtol in ((thr, 0.0), (0.0, thr / bnrm),
                           (thr, 0.5 * thr / bnrm), (0.5 * thr, thr / bnrm)):
            got = launch(maxits=20, atol=atol, rtol=rtol)
            device_cg_check_every_k(got, gots[0], j, converged=1)
            diff = device_cg_same_bits(got, gots[j], DEVCG_BITWISE[:4] + DEVCG_BITWISE[5:])
            assert not diff, f"atol={atol} rtol={rtol}: {diff} differ from maxits={j}"
        for atol, rtol in ((thr, 0.0), (0.0, thr / bnrm)):
            got = launch(maxits=j, atol=atol, rtol=rtol)
            device_cg_check_every_k(got, gots[0], j, converged=1)
            got = launch(maxits=j - 1, atol=atol, rtol=rtol)
            device_cg_check_every_k(got, gots[0], j - 1, converged=0)
            assert not device_cg_same_bits(got, gots[j - 1], ("x", "r", "p", "t"))
    for atol, rtol in ((2.0 * np.sqrt(rr[0]), 0.0), (0.0, 2.0 * np.sqrt(rr[0]) / bnrm)):
        got = launch(maxits=20, atol=float(atol), rtol=float(rtol))
        device_cg_check_every_k(got, gots[0], 0, converged=1)
        assert _bits_equal(got["x"], case.x0), "x touched although x0 is within tolerance"
        assert not device_cg_same_bits(got, gots[0], ("r", "p", "t"))


def device_cg_check_zero(launch, case):
    """b = 0, x0 = 0: (r,r) = (p,t) = 0 from the start; both coefficient
    divisions are 0/0 and must give 0, freezing x at 0.  ``converged``
    follows the host rule rtol2 > 0 and rr <= rtol2 -- here rtol2 = 0."""
    assert not case.b.any() and not case.x0.any()
    for atol, rtol in ((0.0, 1e-9), (0.0, 0.0)):
        got = launch(maxits=5, atol=atol, rtol=rtol)
        for k in ("x", "r", "p", "t"):
            assert np.all(np.isfinite(got[k])), f"{k} not finite (rtol={rtol})"
        assert not got["x"].any(), "x moved away from 0"
        for slot in (S_RR, S_PT, S_RR_PREV, S_BNRM2):
            assert got[f"scal{slot}"][0] == 0.0, (slot, got[f"scal{slot}"])
        assert got["out2"].tolist() == [5, 0], got["out2"]
