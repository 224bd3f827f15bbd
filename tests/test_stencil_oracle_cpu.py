"""CPU side of the oracle tests for the matrix-free stencil kernels and the
slab generators (tests/kernel_oracle.py; GPU side: test_gpu_stencil_oracle).

* torch_ref.stencil_spmv / stencil_pipe against the global-coordinate
  oracle on every rank of every shape the GPU tests use;
* the host generator stencil_local_slab against the per-row structure
  oracle, bit for bit, at dof 1-4 -- it is what maps local to global in the
  cases, and what the device generator has been compared with so far;
* discrimination: fp64 emulations of the kernels with one defect each; on
  the very inputs the GPU sees every one must be REJECTED, the unmutated
  emulation accepted;
* the slab table builder refuses |dz| = 2 and keeps the mf dict's keys.
"""

from functools import lru_cache

import numpy as np
import pytest
import torch

import kernel_oracle as ko
from acg_amd.ops import torch_ref

CPU = torch.device("cpu")
CASE_IDS = ko.stencil_case_ids()
DOFS = (1, 2, 3, 4)


@lru_cache(maxsize=None)
def _case(*cid):
    return ko.stencil_case(*cid)


def _tag(cid):
    return "{}-{}x{}x{}-r{}of{}".format(*cid)


# ---------------------------------------------------------------------------
# oracle self-checks

def test_stencil_oracle_parts_and_dense_matrix():
    """matA part + matO part = the whole operator, which in turn equals a
    dense matrix written down entry by entry."""
    gx, gy, gz = 4, 3, 5
    spec = ko.stencil_spec("27pt")
    rng = np.random.default_rng(1)
    xg = ko.rand_values(gx * gy * gz, rng)
    args = (gx, gy, gz, spec["offsets"], spec["diag"], xg)
    v, M, L = ko.stencil_apply(*args)
    n = gx * gy * gz
    dense = np.zeros((n, n))
    for i in range(n):
        x, y, z = i % gx, (i // gx) % gy, i // (gx * gy)
        dense[i, i] = spec["diag"]
        for dx, dy, dz, w in spec["offsets"]:
            if 0 <= x + dx < gx and 0 <= y + dy < gy and 0 <= z + dz < gz:
                dense[i, x + dx + gx * (y + dy + gy * (z + dz))] = w
    assert np.array_equal(L, (dense != 0).sum(axis=1))
    want = (ko.hp(dense) * ko.hp(xg)[None, :]).sum(axis=1)
    assert float(np.max(np.abs(v - want) / M)) < 2.0 ** -58
    z0, z1 = 1, 3
    A = ko.stencil_apply(*args, part=("owned", z0, z1))
    O = ko.stencil_apply(*args, part=("ghost", z0, z1))
    own = slice(z0 * gx * gy, z1 * gx * gy)
    assert np.array_equal((A[2] + O[2])[own], L[own])
    assert float(np.max(np.abs((A[0] + O[0] - v)[own]) / M[own])) < 2.0 ** -58
    assert not A[2][:own.start].any() and not O[2][own.stop:].any()
    # the Fraction fallback gives the same numbers
    ld = ko.to_f64(A[0])
    old, ko.USE_LONGDOUBLE = ko.USE_LONGDOUBLE, False
    try:
        Af = ko.stencil_apply(*args, part=("owned", z0, z1))
    finally:
        ko.USE_LONGDOUBLE = old
    assert Af[0].dtype == object and np.array_equal(ko.to_f64(Af[0]), ld)


def test_stencil_weights_are_discriminating():
    for kind, (offs, diag) in ko.STENCIL_KINDS.items():
        spec = ko.stencil_spec(kind)
        ws = [abs(o[3]) for o in spec["offsets"]]
        assert len(set(ws)) == len(ws) == len(offs)
        assert all(0.25 <= w <= 2.0 for w in ws) and diag != int(diag)
        assert {np.sign(o[3]) for o in spec["offsets"]} == {-1.0, 1.0}
    for dof in (2, 3, 4):
        spec = ko.stencil_spec("27pt", dof)
        for B in (spec["offblock"], spec["diagblock"]):
            assert np.array_equal(B, B.T)
            assert len(np.unique(np.abs(B))) == dof * (dof + 1) // 2


# ---------------------------------------------------------------------------
# references vs oracle

@pytest.mark.parametrize("cid", CASE_IDS, ids=_tag)
def test_ref_stencil_spmv(cid):
    case = _case(*cid)
    mf = ko.stencil_mf(case, CPU)
    assert (mf["w7"] is not None) == (cid[0] == "7pt")
    for fused in (True, False):
        got = ko.run_stencil_spmv(torch_ref, case, CPU, mf, fused)
        ko.assert_accepts(ko.stencil_spmv_expect(case, fused), got,
                          f"{_tag(cid)} fused{fused}")


@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("cid", CASE_IDS, ids=_tag)
def test_ref_stencil_pipe(cid, first):
    case = _case(*cid)
    got = ko.run_stencil_pipe(torch_ref, case, CPU, ko.stencil_mf(case, CPU), first)
    assert (got["nbA"], got["nbO"]) == (1, 1 if case.nborder else 0)
    ko.assert_accepts(ko.stencil_pipe_expect(case, first), got,
                      f"{_tag(cid)} first{first}")


def test_case_shapes_cover_the_edges():
    c = _case("7pt", 5, 3, 7, 1, 3)
    assert (c.z1 - c.z0, c.ninterior, c.nborder, c.nghost) == (2, 0, 30, 30)
    c = _case("7pt", 9, 7, 3, 1, 3)
    assert (c.z1 - c.z0, c.ninterior, c.nborder, c.nghost) == (1, 0, 63, 126)
    assert {(_case("7pt", 5, 3, 7, r, 3).z1 - _case("7pt", 5, 3, 7, r, 3).z0)
            for r in range(3)} == {2, 3}
    c = _case("7pt", 17, 16, 6, 0, 1)
    assert (c.ninterior, c.nborder, c.nghost, c.border_base) == (1632, 0, 0, 1632)


# ---------------------------------------------------------------------------
# host generator vs structure oracle

@pytest.mark.parametrize("dof", DOFS)
@pytest.mark.parametrize("cid", CASE_IDS, ids=_tag)
def test_host_generator_matches_structure_oracle(cid, dof):
    from acg_amd.gen.stencil import stencil_local_slab

    kind, gx, gy, gz, rank, nranks = cid
    spec = ko.stencil_spec(kind, dof)
    S = ko.stencil_structure(gx, gy, gz, spec, rank, nranks)
    H = stencil_local_slab(gx, gy, gz, spec, rank, nranks)
    assert (H.nowned, H.ninterior, H.nborder, H.nghost) == \
        (S.nowned, S.ninterior, S.nborder, S.nghost)
    assert ko.rows_bits_equal(ko.csr_to_rows(H.A_rowptr, H.A_colidx, H.A_vals), S.rowsA)
    assert ko.rows_bits_equal(ko.csr_to_rows(H.O_rowptr, H.O_colidx, H.O_vals), S.rowsO)
    assert (len(H.A_vals), len(H.O_vals)) == (S.nnzA, S.nnzO)
    assert all(c < S.nowned for d in S.rowsA for c in d)
    assert all(S.nowned <= c < S.nlocal for d in S.rowsO for c in d)
    # round trip of the helpers the GPU test decodes with
    sp, sc, sv = torch_ref.sell_from_csr(*ko.rows_to_csr(S.rowsA))
    rows, lens, padcols = ko.sell_to_rows(sp, sc, sv, S.nowned)
    assert ko.rows_bits_equal(rows, S.rowsA)
    assert np.array_equal(lens, ko.sell_padded_len(ko.rows_to_csr(S.rowsA)[0]))


# ---------------------------------------------------------------------------
# discrimination

Q_MUTANTS = ("swap_x", "swap_yz", "nowrap", "drop_hi_ghost", "stale_zcarry",
             "hm_false", "next_weight")
PIPE_MUTANTS = ("qpart", "border", "first", "partials0")


def _applicable(case, m):
    nz = case.z1 - case.z0
    return {
        "swap_x": case.gx > 1,
        "swap_yz": case.kind != "5pt2d",
        "nowrap": True,
        "drop_hi_ghost": case.rank < case.nranks - 1,
        "stale_zcarry": nz >= 2 and case.kind != "5pt2d",
        "hm_false": nz >= 2 and case.kind != "5pt2d",
        "next_weight": True,
        "qpart": case.nborder > 0,
        "border": case.nborder > 0,
        "first": True,
        "partials0": case.nborder > 0 and case.ninterior > 0,
    }[m]


def _emulate_q(case, mutant=None):
    """fp64 matA and matO products on the owned rows from global
    coordinates, with one defect of the column-walk / generic kernels
    switched on.  Memory a defect reads outside the local vector holds
    zeros -- the most forgiving garbage there is."""
    gx, gy, gz, z0, z1 = case.gx, case.gy, case.gz, case.z0, case.z1
    X = case.wg.reshape(gz, gy, gx)
    w = {(dx, dy, dz): wt for dx, dy, dz, wt in case.spec["offsets"]}

    def swap(a, b):
        if a in w and b in w:
            w[a], w[b] = w[b], w[a]

    if mutant == "swap_x":
        swap((-1, 0, 0), (1, 0, 0))
    if mutant == "swap_yz":
        swap((0, -1, 0), (0, 0, -1))
        swap((0, 1, 0), (0, 0, 1))
    if mutant == "next_weight":  # offs[(o + 1) * 4 + 3] for offset o
        ks = list(w)
        w = dict(zip(ks, [w[k] for k in ks[1:] + ks[:1]]))
    qA, qO = np.zeros_like(X), np.zeros_like(X)
    qA[z0:z1] = case.spec["diag"] * X[z0:z1]
    for (dx, dy, dz), wt in w.items():
        ys, xs = slice(max(0, -dy), min(gy, gy - dy)), slice(max(0, -dx), min(gx, gx - dx))
        yt, xt = slice(ys.start + dy, ys.stop + dy), slice(xs.start + dx, xs.stop + dx)
        if ys.start >= ys.stop or xs.start >= xs.stop:
            continue
        for z in range(z0, z1):
            tz = z + dz
            if not 0 <= tz < gz:
                continue
            owned = z0 <= tz < z1
            if mutant == "drop_hi_ghost" and tz == z1:
                continue
            if owned and dz == -1 and mutant == "hm_false":
                continue
            src = X[tz, yt, xt]
            if owned and dz == -1 and mutant == "stale_zcarry":
                # the carried z-1 value still is the one of the plane before
                src = X[tz - 1, yt, xt] if tz - 1 >= z0 else 0.0 * src
            (qA if owned else qO)[z, ys, xs] += wt * src
    o = case.owned_global
    qA, qO = qA.reshape(-1)[o], qO.reshape(-1)[o]
    if mutant == "nowrap":  # x[node + 1] read without the xi < gx - 1 test
        rows = np.nonzero(o % gx == gx - 1)[0]
        wl = np.concatenate([case.w_old, [0.0]])
        qA[rows] += w[(1, 0, 0)] * wl[rows + 1]
    return qA, qO


def _emulate_spmv(case, fused, mutant=None):
    n, ni = case.nowned, case.ninterior
    qA, qO = _emulate_q(case, mutant)
    tail = np.full(case.nghost, np.nan)
    xo = case.w_old[:n]
    y = qA + qO
    got = {"matA/y": qA, "matA/y_tail": tail, "matA/y_interior": qA[:ni],
           "y": y, "y_tail": tail, "y_interior": y[:ni]}
    sA, s = ko.SENTINELS.copy(), ko.SENTINELS.copy()
    if fused:
        sA[ko.S_PT] = xo @ qA
        s[ko.S_PT] = sA[ko.S_PT] + xo[ni:] @ qO[ni:]
    for i in range(ko.S_NSLOTS):
        got[f"matA/scal{i}"], got[f"scal{i}"] = sA[i:i + 1], s[i:i + 1]
    return got


def _emulate_pipe(case, first, mutant=None):
    n, ni, nb = case.nowned, case.ninterior, case.nborder
    qA, qO = _emulate_q(case, mutant)
    scal = case.scal.copy()
    st = {k: getattr(case, k).copy() for k in "ztpxr"}
    w_old, w_new = case.w_old, np.full(case.nlocal, np.nan)
    qpart = np.full(max(nb, 1), np.nan)
    beta, alpha = torch_ref._pipelined_coeffs(
        torch.from_numpy(scal), (not first) if mutant == "first" else first)
    sums = np.zeros((2, 2))  # [pass, (gamma, delta)]

    def update(rows, q, ps):
        zi = q + beta * st["z"][rows]
        ti = w_old[rows] + beta * st["t"][rows]
        pi = st["r"][rows] + beta * st["p"][rows]
        st["z"][rows], st["t"][rows], st["p"][rows] = zi, ti, pi
        st["x"][rows] += alpha * pi
        rn = st["r"][rows] - alpha * ti
        wn = w_old[rows] - alpha * zi
        st["r"][rows], w_new[rows] = rn, wn
        sums[ps] += rn @ rn, wn @ rn

    bb = case.border_base + (1 if mutant == "border" else 0)
    update(np.arange(0, bb), qA[:bb], 0)
    rows = np.arange(bb, n)
    qpart[rows - case.border_base] = qA[rows]
    got = {}
    if nb:
        for k in "ztpxr":
            got[f"matA/{k}_border"] = st[k][ni:].copy()
        got["matA/w_new_border"] = w_new[ni:].copy()
        got["matA/qpart"] = np.where(np.isnan(qpart), 0.0, qpart)
        rows = np.arange(ni, n)
        update(rows, qO[ni:] + (0.0 if mutant == "qpart" else got["matA/qpart"]), 1)
        got["qpart"] = got["matA/qpart"].copy()
    else:
        got["qpart"] = qpart
    tot = sums[1] if mutant == "partials0" else sums[0] + sums[1]
    scal[ko.S_GAMMA_PREV], scal[ko.S_ALPHA_PREV] = scal[ko.S_GAMMA], alpha
    scal[ko.S_GAMMA], scal[ko.S_DELTA] = tot
    got.update(st)
    got["w_new"], got["w_new_tail"] = w_new[:n].copy(), w_new[n:].copy()
    for i in range(ko.S_NSLOTS):
        got[f"scal{i}"] = scal[i:i + 1]
    return got


@pytest.mark.parametrize("cid", CASE_IDS, ids=_tag)
def test_mutants_stencil(cid):
    """Every defect is rejected on every case it can show on, by the SpMV
    expectation (operator defects) and by the megafused one (all)."""
    case = _case(*cid)
    e_spmv = {f: ko.stencil_spmv_expect(case, f) for f in (True, False)}
    e_pipe = {f: ko.stencil_pipe_expect(case, f) for f in (True, False)}
    for f in (True, False):
        assert ko.accepts(e_spmv[f], _emulate_spmv(case, f)), "emulator is off"
        assert ko.accepts(e_pipe[f], _emulate_pipe(case, f)), "emulator is off"
    seen = set()
    for m in Q_MUTANTS + PIPE_MUTANTS:
        if not _applicable(case, m):
            continue
        seen.add(m)
        for f in (True, False):
            if m in Q_MUTANTS:
                assert not ko.accepts(e_spmv[f], _emulate_spmv(case, f, m)), m
            assert not ko.accepts(e_pipe[f], _emulate_pipe(case, f, m)), m
    assert {"nowrap", "first"} <= seen


def test_every_mutant_is_exercised():
    seen = {m for cid in CASE_IDS for m in Q_MUTANTS + PIPE_MUTANTS
            if cid[0] == "7pt" and _applicable(_case(*cid), m)}
    assert seen == set(Q_MUTANTS + PIPE_MUTANTS)


# ---------------------------------------------------------------------------
# slab tables

def test_slab_tables_reject_dz2():
    from acg_amd.gen.device_slab import device_stencil_slab, stencil_slab_tables

    spec = ko.stencil_spec("7pt")
    for dz in (2, -2):
        bad = dict(spec, offsets=spec["offsets"] + [(0, 0, dz, 0.57)])
        with pytest.raises(ValueError, match=r"\|dz\| <= 1"):
            stencil_slab_tables(6, 5, 8, bad, 1, 2)
        with pytest.raises(ValueError, match=r"\|dz\| <= 1"):  # before any allocation
            device_stencil_slab(6, 5, 8, bad, 1, 2, "cpu")


def test_mf_tables_keys_and_values():
    case = _case("7pt", 5, 3, 7, 1, 3)
    mf = ko.stencil_mf(case, CPU)
    assert set(mf) == {"zs", "pb", "offs", "ksten", "diag", "gx", "gy", "gz",
                       "nown_nodes", "z0", "z1", "w7"}
    assert (mf["gx"], mf["gy"], mf["gz"], mf["z0"], mf["z1"]) == (5, 3, 7, 2, 4)
    assert mf["nown_nodes"] == 30 and mf["ksten"] == 6 and mf["diag"] == 5.3
    w = {o[:3]: o[3] for o in case.spec["offsets"]}
    assert mf["w7"] == tuple(w[k] for k in [(-1, 0, 0), (1, 0, 0), (0, -1, 0),
                                            (0, 1, 0), (0, 0, -1), (0, 0, 1)])
    # planes 2, 3 are both border (local 0, 1); ghosts 1 and 4 follow
    assert mf["zs"].tolist() == [2, 3] and mf["zs"].dtype == torch.int32
    assert mf["pb"].tolist() == [-1, -1, 30, 0, 15, 45, -1, -1, -1]
    assert mf["pb"].dtype == torch.int64 and mf["offs"].dtype == torch.float64
    assert mf["offs"].tolist() == [float(v) for o in case.spec["offsets"] for v in o]
    from acg_amd.gen.device_slab import mf_tables_from, stencil_slab_tables

    tab = stencil_slab_tables(5, 3, 7, ko.stencil_spec("27pt", 3), 1, 3)
    assert mf_tables_from(tab, tab["zs_own"], tab["pb"], tab["offs"]) is None
    assert tab["blocks"].numel() == 18
