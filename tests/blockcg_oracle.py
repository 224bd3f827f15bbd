"""Oracle helpers for the block-CG kernels.

Plain helper module (not a conftest), built on tests/kernel_oracle.py and
tests/multirhs_oracle.py the way multirhs_oracle.py is built on
kernel_oracle.py.  The same ``run_*`` drivers serve the CPU tests
(torch_ref, mutants) and the GPU tests (gpu_ops).

Acceptance is derived, never tuned.

* Row kernels (``block_update``, ``block_ortho``): every output element is a
  sum of K products plus one more term, evaluated in long double from the
  fp64 inputs, under the project's rule |err| <= (L + 48) * 2^-53 * M with
  L = K + 1 and M the same expression over absolute values.
* Gram entries (``gram_multi``, the W^T W partials of ``block_update``, the
  sums the coefficient kernels form from partials): ``ko.dot`` as it stands.
  The Gram of W is evaluated on the W the kernel stored, which is exactly
  what it accumulated from.
* Dense kernels: backward error, so no condition number enters.  With u =
  2^-53 and gamma_k = k u / (1 - k u) (Higham, Accuracy and Stability of
  Numerical Algorithms, 2nd ed.):
    - Thm 10.3: the computed Cholesky factor satisfies
      |zeta^T zeta - G| <= gamma_{K+1} |zeta^T| |zeta| entrywise.  G is the
      fp64 matrix the kernel published (and factorised); that G itself is
      held to the partial-sum bound of ``ko.dot``.
    - Thm 8.5: a column of zeta^-1 computed by substitution from
      zeta x = e_c satisfies (zeta + dZ) x = e_c, |dZ| <= gamma_K |zeta|, so
      |zeta zeta^-1 - I| <= gamma_K |zeta| |zeta^-1|.
    - Thm 10.4: a column of xi computed by the two triangular solves
      satisfies (M + dM) x = e_c, |dM| <= gamma_{3K+1} |L| |L^T|, so
      |M xi - I| <= gamma_{3K+1} |L| |L^T| |xi|; L is the long-double
      Cholesky factor of M (it differs from the computed one by O(u), which
      moves the bound by O(u^2)).
  xi C and zeta C are K-term products: the rule above with L = K.
* Everything a kernel does not own is compared bitwise: rows >= n and ghost
  rows, partials beyond the block count, state regions of other kernels and
  entries of its own regions outside the leading K x K block, rr_out beyond
  what it publishes; with kg < K the padded columns must be exactly zero and
  the padded parts of the small matrices exactly the identity; with the
  flag set every output keeps its bits.
"""

from __future__ import annotations

from functools import lru_cache
from types import SimpleNamespace

import numpy as np

import kernel_oracle as ko
import multirhs_oracle as mo

KS = mo.KS
KMAX = mo.KMAX
MAXG = ko.MAXG
GHOST_ROWS = mo.GHOST_ROWS
BS_LD = 8
BS_M, BS_XI, BS_XIC, BS_G, BS_ZETA, BS_ZINV, BS_C = 0, 64, 128, 192, 256, 320, 384
BS_FLAG, BS_ITER, BS_SIZE = 448, 449, 456
BLOCK_MAXG = 2048
TAU = 1e-6
REGIONS = {"M": BS_M, "xi": BS_XI, "xic": BS_XIC, "G": BS_G, "zeta": BS_ZETA,
           "zinv": BS_ZINV, "C": BS_C}
ROW_N = (1, 63, 64, 65, 1000)
COEF_NB = (1, 2, 3, 5, BLOCK_MAXG)
ITER_SENTINEL = 977.0


def check_layout(ops):
    """The constants above are the ones of the op layer under test."""
    for nm in ("BS_LD", "BS_M", "BS_XI", "BS_XIC", "BS_G", "BS_ZETA", "BS_ZINV",
               "BS_C", "BS_FLAG", "BS_ITER", "BS_SIZE", "BLOCK_MAXG"):
        assert getattr(ops, nm) == globals()[nm], nm
    assert ops.BLOCK_TAU == TAU


def row_blocks(n):
    """Grid of the row kernels: one row per thread per trip, capped."""
    return max(1, min(BLOCK_MAXG, (n + 255) // 256))


def second_trip_n():
    """Smallest interesting n that sends threads into a second grid-stride
    trip: the block cap times the block size, plus a ragged tail."""
    return BLOCK_MAXG * 256 + 77


def pairs(k):
    return [(a, b) for a in range(k) for b in range(a, k)]


def gamma(k):
    return ko.hps(k * ko.U) / (ko.hps(1.0) - ko.hps(k * ko.U))


def _hmm(A, B):
    """Long-double matrix product (np.matmul has no BLAS path for it)."""
    return np.einsum("ik,kj->ij", A, B) if ko.USE_LONGDOUBLE else A.dot(B)


def hchol(G):
    """Long-double Cholesky factor (lower) of a small SPD matrix."""
    k = G.shape[0]
    L = ko.hp(np.zeros((k, k)))
    for j in range(k):
        d = G[j, j] - (L[j, :j] * L[j, :j]).sum()
        L[j, j] = np.sqrt(d) if ko.USE_LONGDOUBLE else ko.hps(float(d) ** 0.5)
        for i in range(j + 1, k):
            L[i, j] = (G[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
    return L


# ---------------------------------------------------------------------------
# inputs

@lru_cache(maxsize=None)
def row_case(n):
    """x, s, q, t multivectors of n + GHOST_ROWS rows, 8 columns."""
    rows = n + GHOST_ROWS
    return SimpleNamespace(n=n, **{nm: mo.columns(rows, 21000 + 1000 * i + n % 997)
                                   for i, nm in enumerate("xsqt")})


def coeffs(k, seed):
    """Two distinct non-symmetric (k, k) matrices and an upper-triangular
    pair, entries from ko.rand_values scaled to keep sums O(1)."""
    v = ko.rand_values(4 * KMAX * KMAX, np.random.default_rng(seed)) / 4.0
    m = v.reshape(4, KMAX, KMAX)
    return (m[0, :k, :k].copy(), m[1, :k, :k].copy(),
            np.triu(m[2, :k, :k]), np.triu(m[3, :k, :k]))


def sentinel_state():
    """Every slot a distinct finite value; flag 0, iteration a sentinel."""
    s = 3000.0 + 0.125 * np.arange(BS_SIZE)
    s[BS_FLAG] = 0.0
    s[BS_ITER] = ITER_SENTINEL
    return s


def region(state, name, k=BS_LD):
    b = REGIONS[name]
    return state[b:b + 64].reshape(8, 8)[:k, :k]


def put(state, name, mat):
    k = mat.shape[0]
    region(state, name, k)[...] = mat
    return state


def pad_identity(mat, kg):
    out = np.eye(mat.shape[0])
    out[:kg, :kg] = mat[:kg, :kg]
    return out


def pad_cols(X, k, kg):
    Y = np.zeros((X.shape[0], k))
    Y[:, :kg] = X[:, :kg]
    return Y


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits(a, b):
    a, b = _bits(a), _bits(b)
    return a.shape == b.shape and bool(np.array_equal(a, b))


def state_untouched(before, after, owned=(), k=BS_LD):
    """All slots outside the leading k x k block of the ``owned`` regions
    (and outside ``owned`` scalar slots) keep their bits."""
    mask = np.ones(BS_SIZE, dtype=bool)
    for nm in owned:
        if nm in REGIONS:
            m = np.zeros((8, 8), dtype=bool)
            m[:k, :k] = True
            mask[REGIONS[nm]:REGIONS[nm] + 64] &= ~m.reshape(-1)
        else:
            mask[{"flag": BS_FLAG, "iter": BS_ITER}[nm]] = False
    return same_bits(before[mask], after[mask])


# ---------------------------------------------------------------------------
# Gram

def gram_sums(partials, nb, k):
    """Long-double sum of the first nb partials of every pair."""
    flat = np.asarray(partials).reshape(-1)
    return [ko.hsum(ko.hp(flat[p * BLOCK_MAXG:p * BLOCK_MAXG + nb]))
            for p in range(len(pairs(k)))]


def check_partials_untouched(partials, nb, k):
    flat = np.asarray(partials).reshape(-1)
    npair = len(pairs(k))
    for p in range(npair):
        seg = flat[p * BLOCK_MAXG:(p + 1) * BLOCK_MAXG]
        assert np.all(np.isfinite(seg[:nb])), f"pair {p}: owned partials not finite"
        assert mo.all_nan_bits(seg[nb:]), f"pair {p}: partials beyond {nb} written"
    assert mo.all_nan_bits(flat[npair * BLOCK_MAXG:]), "partials of no pair written"


def gram_expect(X, Y, k, kernel):
    """Expectation for the summed upper triangle of X^T Y.  The sum of the
    block partials was formed in long double by the test, so ko.dot's
    (n + 8) u sum|ab| covers the kernel's own additions."""
    e = ko.Expect(kernel)
    for a, b in pairs(k):
        v, tol = ko.dot(ko.hp(X[:, a]), ko.hp(Y[:, b]))
        e.add_tol(f"g{a}{b}", v, tol)
    return e


@lru_cache(maxsize=None)
def _gram_expect_cached(n, k):
    rc = row_case(n)
    return gram_expect(rc.s[:n, :k], rc.t[:n, :k], k, "k_gram_multi")


def run_gram(ops, n, k, dev):
    rc = row_case(n)
    partials = mo._nan2(KMAX, MAXG, dev)
    nb = ops.gram_multi(ko._t(rc.s[:, :k], dev), ko._t(rc.t[:, :k], dev),
                        partials, n=n)
    pp = ko._np(partials)
    sums = gram_sums(pp, nb, k)
    got = {f"g{a}{b}": np.array([ko.to_f64(np.array([sums[p]]))[0]])
           for p, (a, b) in enumerate(pairs(k))}
    return got, {"partials": pp, "nblocks": nb}


def gram_expectation(n, k):
    return _gram_expect_cached(n, k)


# ---------------------------------------------------------------------------
# block_update

def _row_expect(base, left, coef, L):
    """base + left @ coef in long double with magnitude."""
    hl, hc = ko.hp(left), ko.hp(coef)
    v = ko.hp(base) + _hmm(hl, hc)
    M = ko.habs(ko.hp(base)) + _hmm(ko.habs(hl), ko.habs(hc))
    return v, M, L


@lru_cache(maxsize=None)
def _update_expect_cached(n, k, kg):
    rc = row_case(n)
    xi, xic, _, _ = coeffs(k, 500 + k)
    xi, xic = pad_identity(xi, kg), pad_identity(xic, kg)
    X, Sm, Q, T = (pad_cols(a[:n], k, kg) for a in (rc.x, rc.s, rc.q, rc.t))
    e = ko.Expect("k_block_update")
    e.add("x", *_row_expect(X, Sm, xic, k + 1))
    e.add("w", *_row_expect(Q, T, -xi, k + 1))
    return e


def run_update(ops, n, k, kg, dev, flag=False):
    rc = row_case(n)
    xi, xic, _, _ = coeffs(k, 500 + k)
    s0 = sentinel_state()
    put(s0, "xi", pad_identity(xi, kg))
    put(s0, "xic", pad_identity(xic, kg))
    if flag:
        s0[BS_FLAG] = 1.0
    ins = {nm: pad_cols(getattr(rc, nm), k, kg) for nm in "xsqt"}
    X, Sm, Q, T = (ko._t(ins[nm], dev) for nm in "xsqt")
    state = ko._t(s0, dev)
    partials = mo._nan2(KMAX, MAXG, dev)
    nb = ops.block_update(X, Sm, Q, T, state, partials, n)
    out = {nm: ko._np(t) for nm, t in zip("xsqt", (X, Sm, Q, T))}
    got = {"x": out["x"][:n], "w": out["q"][:n]}
    return got, {"in": ins, "out": out, "state0": s0, "state": ko._np(state),
                 "partials": ko._np(partials), "nblocks": nb}


def check_update(n, k, kg, got, ex, tag, on_gpu=False):
    ko.assert_accepts(_update_expect_cached(n, k, kg), got, tag)
    assert ex["nblocks"] == (row_blocks(n) if on_gpu else 1)
    # Gram of the W the kernel stored
    W = ex["out"]["q"][:n]
    sums = gram_sums(ex["partials"], ex["nblocks"], k)
    gg = {f"g{a}{b}": np.array([ko.to_f64(np.array([sums[p]]))[0]])
          for p, (a, b) in enumerate(pairs(k))}
    ko.assert_accepts(gram_expect(W, W, k, "k_block_update(gram)"), gg, tag)
    check_partials_untouched(ex["partials"], ex["nblocks"], k)
    for nm in "xq":  # rows >= n unwritten
        assert same_bits(ex["out"][nm][n:], ex["in"][nm][n:]), f"{nm}: rows >= n written"
    for nm in "st":  # pure inputs
        assert same_bits(ex["out"][nm], ex["in"][nm]), f"{nm} modified"
    assert same_bits(ex["state"], ex["state0"]), "block_update wrote the state"
    if kg < k:
        assert not ex["out"]["x"][:, kg:].any() and not ex["out"]["q"][:, kg:].any(), \
            "padded columns not exactly zero"


def check_frozen_rows(ex, names="xsqt"):
    for nm in names:
        assert same_bits(ex["out"][nm], ex["in"][nm]), f"{nm} written with the flag set"
    assert same_bits(ex["state"], ex["state0"])
    if "partials" in ex:
        assert mo.all_nan_bits(ex["partials"]), "partials written with the flag set"


# ---------------------------------------------------------------------------
# block_ortho

@lru_cache(maxsize=None)
def _ortho_q_expect(n, k, kg):
    rc = row_case(n)
    _, _, zeta, zinv = coeffs(k, 500 + k)
    W = pad_cols(rc.q[:n], k, kg)
    e = ko.Expect("k_block_ortho")
    e.add("q", *_row_expect(np.zeros_like(W), W, pad_identity(zinv, kg), k + 1))
    return e


def run_ortho(ops, n, k, kg, dev, flag=False, s_zero=False):
    rc = row_case(n)
    _, _, zeta, zinv = coeffs(k, 500 + k)
    s0 = sentinel_state()
    put(s0, "zeta", pad_identity(zeta, kg))
    put(s0, "zinv", pad_identity(zinv, kg))
    if flag:
        s0[BS_FLAG] = 1.0
    ins = {"q": pad_cols(rc.q, k, kg), "s": pad_cols(rc.s, k, kg)}
    if s_zero:
        ins["s"][:n] = 0.0
    Q, Sm = ko._t(ins["q"], dev), ko._t(ins["s"], dev)
    state = ko._t(s0, dev)
    ops.block_ortho(Q, Sm, state, n)
    out = {"q": ko._np(Q), "s": ko._np(Sm)}
    return ({"q": out["q"][:n], "s": out["s"][:n]},
            {"in": ins, "out": out, "state0": s0, "state": ko._np(state)})


def check_ortho(n, k, kg, got, ex, tag, s_zero=False):
    ko.assert_accepts(_ortho_q_expect(n, k, kg), {"q": got["q"]}, tag)
    _, _, zeta, _ = coeffs(k, 500 + k)
    e = ko.Expect("k_block_ortho(S)")
    # S <- Q + S zeta^T from the Q the kernel stored
    e.add("s", *_row_expect(got["q"], ex["in"]["s"][:n], pad_identity(zeta, kg).T,
                            k + 1))
    ko.assert_accepts(e, {"s": got["s"]}, tag)
    if s_zero:  # the start-up step: S = Q, bit for bit (up to the sign of 0)
        assert np.array_equal(got["s"], got["q"])
    for nm in "qs":
        assert same_bits(ex["out"][nm][n:], ex["in"][nm][n:]), \
            f"{nm}: rows >= n / ghost rows written"
    assert same_bits(ex["state"], ex["state0"]), "block_ortho wrote the state"
    if kg < k:
        assert not ex["out"]["q"][:n, kg:].any() and not ex["out"]["s"][:n, kg:].any(), \
            "padded columns not exactly zero"


# ---------------------------------------------------------------------------
# coefficient kernels

@lru_cache(maxsize=None)
def gram_partials(kind, nb, scale=1.0):
    """(36, nb) block partials of an 8-column Gram whose leading k x k
    blocks serve every k: chunk sums of V^T V for well-separated columns V
    (``spd``), with column 1 a copy of column 0 (``dup``), column 1 zero
    (``zero``), or one NaN partial in pair (0, 1) (``nan``)."""
    rows = max(64, 2 * nb)
    V = mo.columns(rows, 31000 + nb) * scale
    if kind == "dup":
        V[:, 1] = V[:, 0]
    elif kind == "zero":
        V[:, 1] = 0.0
    bounds = np.linspace(0, rows, nb + 1).astype(int)
    P = np.zeros((len(pairs(KMAX)), nb))
    for i in range(nb):
        Vi = V[bounds[i]:bounds[i + 1]]
        Gi = Vi.T @ Vi
        for p, (a, b) in enumerate(pairs(KMAX)):
            P[p, i] = Gi[a, b]
    if kind == "nan":
        P[1, nb // 2] = np.nan
    return P


def _pair_index(k):
    """Rows of the 8-column pair table that make up the k-column one."""
    p8 = {ab: p for p, ab in enumerate(pairs(KMAX))}
    return [p8[ab] for ab in pairs(k)]


def place_partials(P8, k, dev):
    nb = P8.shape[1]
    flat = np.full(KMAX * MAXG, np.nan)
    for p, src in enumerate(_pair_index(k)):
        flat[p * BLOCK_MAXG:p * BLOCK_MAXG + nb] = P8[src]
    return ko._t(flat.reshape(KMAX, MAXG), dev), flat


def sym_expect(e, name, P8, k, kg):
    """The published symmetric matrix against the partial sums."""
    idx = _pair_index(k)
    v = ko.hp(np.eye(k))
    tol = ko.hp(np.zeros((k, k)))
    for p, (a, b) in enumerate(pairs(k)):
        if b < kg:
            d, t = ko.dot(ko.hp(P8[idx[p]]), ko.hp(np.ones(P8.shape[1])))
            v[a, b] = v[b, a] = d
            tol[a, b] = tol[b, a] = t
    e.add_tol(name, v, tol)


C0_SEED = 733


def c_input(k, kg):
    """The C the coefficient kernels start from: arbitrary in the leading
    kg x kg block, identity beyond it."""
    return pad_identity(coeffs(k, C0_SEED)[0], kg)


def run_coef_alpha(ops, P8, k, kg, dev, it=7, flag=False):
    s0 = sentinel_state()
    put(s0, "C", c_input(k, kg))
    if flag:
        s0[BS_FLAG] = 1.0
    partials, flat = place_partials(P8, k, dev)
    state = ko._t(s0, dev)
    ops.block_coef_alpha(partials, P8.shape[1], state, k, kg, it)
    assert same_bits(ko._np(partials).reshape(-1), flat), "partials modified"
    return {"state0": s0, "state": ko._np(state)}


def check_coef_alpha(P8, k, kg, ex, tag):
    st, s0 = ex["state"], ex["state0"]
    assert state_untouched(s0, st, owned=("M", "xi", "xic"), k=k), \
        "coef_alpha wrote outside M, xi, xi C"
    M, xi, xic = region(st, "M", k), region(st, "xi", k), region(st, "xic", k)
    e = ko.Expect("k_block_coef_alpha")
    sym_expect(e, "M", P8, k, kg)
    hM, hxi = ko.hp(M), ko.hp(xi)
    L = hchol(hM)
    bnd = gamma(3 * k + 1) * _hmm(_hmm(ko.habs(L), ko.habs(L.T)), ko.habs(hxi))
    e.add_tol("Mxi-I", ko.hp(np.zeros((k, k))), bnd)
    C = region(s0, "C", k)
    e.add("xic", _hmm(hxi, ko.hp(C)), _hmm(ko.habs(hxi), ko.habs(ko.hp(C))), k)
    got = {"M": M, "xic": xic,
           "Mxi-I": ko.to_f64(_hmm(hM, hxi) - ko.hp(np.eye(k)))}
    ko.assert_accepts(e, got, tag)
    assert same_bits(M, M.T), "M not mirrored bit for bit"
    assert same_bits(xi[kg:], np.eye(k)[kg:]) and same_bits(xi[:, kg:], np.eye(k)[:, kg:]), \
        "padded part of xi is not the identity"
    assert same_bits(M[kg:], np.eye(k)[kg:]) and same_bits(M[:, kg:], np.eye(k)[:, kg:])


def run_coef_beta(ops, P8, k, kg, dev, it=7, init=False, flag=False):
    s0 = sentinel_state()
    put(s0, "C", c_input(k, kg))
    if flag:
        s0[BS_FLAG] = 1.0
    partials, flat = place_partials(P8, k, dev)
    state = ko._t(s0, dev)
    rr_out = ko._nan(KMAX + 4, dev)
    ops.block_coef_beta(partials, P8.shape[1], state, rr_out, k, kg, it, init=init)
    assert same_bits(ko._np(partials).reshape(-1), flat), "partials modified"
    return {"state0": s0, "state": ko._np(state), "rr_out": ko._np(rr_out)}


def check_coef_beta(P8, k, kg, ex, tag, init=False):
    st, s0, rr = ex["state"], ex["state0"], ex["rr_out"]
    assert state_untouched(s0, st, owned=("G", "zeta", "zinv", "C"), k=k), \
        "coef_beta wrote outside G, zeta, zeta^-1, C"
    G, zeta, zinv, C = (region(st, nm, k) for nm in ("G", "zeta", "zinv", "C"))
    e = ko.Expect("k_block_coef_beta")
    sym_expect(e, "G", P8, k, kg)
    hG, hz, hzi = ko.hp(G), ko.hp(zeta), ko.hp(zinv)
    zero = ko.hp(np.zeros((k, k)))
    e.add_tol("ztz-G", zero, gamma(k + 1) * _hmm(ko.habs(hz.T), ko.habs(hz)))
    e.add_tol("zzi-I", zero, gamma(k) * _hmm(ko.habs(hz), ko.habs(hzi)))
    got = {"G": G, "ztz-G": ko.to_f64(_hmm(hz.T, hz) - hG),
           "zzi-I": ko.to_f64(_hmm(hz, hzi) - ko.hp(np.eye(k)))}
    C0 = region(s0, "C", k)
    if init:
        assert same_bits(C, zeta), "init: C is not zeta"
    else:
        e.add("C", _hmm(hz, ko.hp(C0)), _hmm(ko.habs(hz), ko.habs(ko.hp(C0))), k)
        got["C"] = C
    for c in range(kg):
        v, tol = ko.dot(ko.hp(C[:, c]), ko.hp(C[:, c]))
        e.add_tol(f"rr{c}", v, tol)
        got[f"rr{c}"] = rr[c:c + 1]
    ko.assert_accepts(e, got, tag)
    assert same_bits(G, G.T), "G not mirrored bit for bit"
    assert not np.tril(zeta, -1).any() and not np.tril(zinv, -1).any()
    eye = np.eye(k)
    for m in (G, zeta, zinv):
        assert same_bits(m[kg:], eye[kg:]) and same_bits(m[:, kg:], eye[:, kg:]), \
            "padded part is not the identity"
    assert mo.all_nan_bits(rr[kg:k]) and mo.all_nan_bits(rr[k + 2:]), \
        "rr_out written outside [0, kg) and [K, K+2)"
    assert rr[k] == 0.0 and rr[k + 1] == -1.0


def check_breakdown(ex, k, it, owned_sym, beta):
    """A failed pivot: flag and iteration set, the symmetric matrix may be
    published, everything else keeps its bits."""
    st, s0 = ex["state"], ex["state0"]
    assert st[BS_FLAG] == 1.0 and st[BS_ITER] == float(it), (st[BS_FLAG], st[BS_ITER])
    assert state_untouched(s0, st, owned=(owned_sym, "flag", "iter"), k=k)
    if beta:
        rr = ex["rr_out"]
        assert mo.all_nan_bits(rr[:k]) and mo.all_nan_bits(rr[k + 2:])
        assert rr[k] == 1.0 and rr[k + 1] == float(it)


def check_flag_on_entry(ex, k, beta):
    assert same_bits(ex["state"], ex["state0"]), "state written with the flag set"
    if beta:
        rr = ex["rr_out"]
        assert mo.all_nan_bits(rr[:k]) and mo.all_nan_bits(rr[k + 2:])
        # the flag and its iteration are mirrored for the host copy
        assert rr[k] == 1.0 and rr[k + 1] == ITER_SENTINEL


# ---------------------------------------------------------------------------
# solver level: the two 1728-row systems of test_gpu_multirhs.py

MAXITS, RTOL = 600, 1e-10


def csr_apply(S, X, absval=False):
    vals = np.abs(S.A_vals) if absval else S.A_vals
    rows = ko.csr_rows(S.A_rowptr)
    Y = np.zeros((S.nowned, X.shape[1]))
    np.add.at(Y, rows, vals[:, None] * X[np.asarray(S.A_colidx, np.int64)])
    return Y


@lru_cache(maxsize=None)
def solver_system(name):
    """(S, B): B is A.1 plus seven default_rng(77) normal columns."""
    from acg_amd.gen import STENCIL_7PT_3D, queen_like_spec, stencil_local_slab

    if name == "sell7":
        S = stencil_local_slab(12, 12, 12, dict(STENCIL_7PT_3D), 0, 1)
    else:
        S = stencil_local_slab(8, 8, 9, queen_like_spec(3), 0, 1)
    assert S.nowned == 1728 and S.nghost == 0
    rand = np.random.default_rng(77).standard_normal((S.nowned, 7))
    a1 = csr_apply(S, np.ones((S.nowned, 1)))[:, 0]
    B = np.column_stack([a1] + [rand[:, i] for i in range(7)])
    B.setflags(write=False)
    return S, B


def special_rhs(name, kind, eps=None):
    """Right-hand sides that exercise the breakdown rule."""
    S, B = solver_system(name)
    v, w, z = B[:, 1], B[:, 2], B[:, 3]
    if kind == "dependent":      # hand-over at initialisation
        return np.column_stack([B[:, 0], v, 4.0 * v, w])
    if kind == "near":           # squared sine of the angle ~ eps^2
        return np.column_stack([v, v + eps * w])
    if kind == "exact":          # column 1 is solved exactly by the first step
        return np.column_stack([v, csr_apply(S, v[:, None])[:, 0], w, z])
    raise KeyError(kind)


@lru_cache(maxsize=None)
def cpu_single_solves(name):
    """CGSolverCPU.solve per column of B: (X, iteration counts)."""
    import torch

    from acg_amd.solvers.cpu import CGSolverCPU

    S, B = solver_system(name)
    solver = CGSolverCPU(S)
    X = np.zeros_like(B)
    its = []
    for c in range(B.shape[1]):
        x = torch.zeros(S.nowned, dtype=torch.float64)
        r = solver.solve(torch.from_numpy(B[:, c].copy()), x, maxits=MAXITS,
                         res_rtol=RTOL)
        assert r.converged
        X[:, c] = x.numpy()
        its.append(r.niterations)
    return X, its


@lru_cache(maxsize=None)
def cpu_block_solves(name, k):
    """CGSolverCPU.solve_block of the first k columns: (X, results)."""
    import torch

    from acg_amd.solvers.cpu import CGSolverCPU

    S, B = solver_system(name)
    X = torch.zeros(S.nowned, k, dtype=torch.float64)
    res = CGSolverCPU(S).solve_block(torch.from_numpy(B[:, :k].copy()), X,
                                     maxits=MAXITS, res_rtol=RTOL)
    return X.numpy(), res


def check_true_residual(S, B, X, tag="", AX=None):
    """True residual from the CSR on the host: the target plus what the
    agreement criterion assert_close(rtol=1e-6, atol=1e-8) allows x to be off
    by (the reach term of test_solve_multi).  Returns the relative residuals."""
    AX = csr_apply(S, X) if AX is None else AX
    reach = csr_apply(S, 1e-8 + 1e-6 * np.abs(X), absval=True)
    rel = []
    for c in range(B.shape[1]):
        bn = np.linalg.norm(B[:, c])
        rn = np.linalg.norm(B[:, c] - AX[:, c])
        rel.append(rn / bn if bn else rn)
        print(f"BLOCK_CG {tag} col{c}: true_rel_res={rel[-1]:.3e}")
        assert rn <= RTOL * bn + np.linalg.norm(reach[:, c]), (tag, c, rn, bn)
    return rel
