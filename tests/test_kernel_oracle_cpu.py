"""CPU side of the kernel-level exactness tests (tests/kernel_oracle.py).

* the Block-SELL packer against an independent decoder of the documented
  layout;
* every torch_ref counterpart of a hot-path kernel against the
  high-precision oracle, within the derived bounds, at the GPU tests' shapes;
* a discrimination self-check: for the exact inputs of the GPU tests,
  deliberately wrong results are built in fp64 and every one of them must
  be REJECTED by the acceptance helper -- the inputs, not the bounds, are
  what separates a right kernel from a subtly wrong one.
"""

import sys
from functools import lru_cache

import numpy as np
import pytest
import torch

import kernel_oracle as ko
from acg_amd.ops import torch_ref

CPU = torch.device("cpu")
DOFS = (2, 3, 4)
BSELL_NODES = (1, 63, 65, 130)
PIPE_CASES = [(65, False, False), (200, False, False), (65, True, False),
              (200, True, False), (65, True, True)]
VEC_N = (1, 257, 300_001)
DOT_N = (1, 255, 257, 1025, 300_001)
SELL_SLICES = (3, 37, 100)


@lru_cache(maxsize=None)
def _bsell(dof, nnodes, ghost):
    return ko.bsell_case(dof, nnodes, ghost)


@lru_cache(maxsize=None)
def _pipe(nowned, split, nborder0):
    return ko.pipe_case(nowned, split, nborder0)


@lru_cache(maxsize=None)
def _sell(nslices):
    return ko.sell_case(nslices)


@lru_cache(maxsize=None)
def _vec(n, pt_zero=False):
    return ko.vec_case(n, pt_zero)


# ---------------------------------------------------------------------------
# oracle self-consistency

def test_oracle_arithmetic_is_wider_than_fp64():
    assert ko.USE_LONGDOUBLE == (np.finfo(np.longdouble).eps <= 2.0 ** -63)
    # 1 + 2^-60 is not an fp64 number; the oracle must resolve it
    one, tiny = ko.hps(1.0), ko.hps(2.0 ** -60)
    assert (one + tiny) - one == tiny


def test_oracle_fraction_fallback_agrees(monkeypatch):
    """The exact-rational path (taken where long double is plain fp64) gives
    the same verdicts as the long-double path."""
    case = _bsell(3, 1, True)
    want = ko.to_f64(ko.spmv(case.rowptr, case.cols, case.vals, ko.hp(case.x))[0])
    monkeypatch.setattr(ko, "USE_LONGDOUBLE", False)
    v, M = ko.spmv(case.rowptr, case.cols, case.vals, ko.hp(case.x))
    assert v.dtype == object
    np.testing.assert_array_equal(ko.to_f64(v), want)
    e = ko.bsell_spmv_expect(case, dotslot=ko.S_PT, dot_accum=True)
    got = ko.run_bsell_spmv(torch_ref, case, CPU, dotslot=ko.S_PT, dot_accum=True)
    assert ko.accepts(e, got)
    got["y"][-1] *= 1.0 + 1e-12
    assert not ko.accepts(e, got)


# ---------------------------------------------------------------------------
# layout: packer vs independent decoder

def _force_numpy_fallback(monkeypatch):
    import acg_amd.host as host

    monkeypatch.delattr(host, "_acg_host", raising=False)
    monkeypatch.setitem(sys.modules, "acg_amd.host._acg_host", None)


def _native_built():
    try:
        from acg_amd.host import _acg_host  # noqa: F401
    except ImportError:
        return False
    return True


@pytest.mark.parametrize("path", ["native", "numpy"])
@pytest.mark.parametrize("nnodes", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("dof", DOFS)
def test_bsell_layout_roundtrip(monkeypatch, dof, nnodes, path):
    if path == "numpy":
        _force_numpy_fallback(monkeypatch)
    elif not _native_built():
        pytest.skip("native host extension not built")
    variants = [(False, None), (True, None)]
    if nnodes > 64:
        variants.append((True, 1))  # slice 1 entirely empty
    for ghost, empty in variants:
        case = ko.bsell_case(dof, nnodes, ghost, empty_slice=empty)
        counts = np.diff(case.rowptr).reshape(nnodes, dof).sum(axis=1)
        if nnodes > 8:
            assert (counts == 0).any(), "no empty block-row in the fixture"
        bptr, bcol, bvals, density = torch_ref.bsell_from_csr(
            case.rowptr, case.cols, case.vals, dof)
        assert bcol.dtype == np.int32 and bptr.dtype == np.int64
        if empty is not None:
            assert bptr[empty + 1] == bptr[empty]
        assert len(bvals) == bptr[-1] * dof * dof
        assert 0.0 < density <= 1.0
        dense = ko.unpack_bsell(bptr, bcol, bvals, nnodes, dof, case.ncols)
        want = ko.csr_dense(case.rowptr, case.cols, case.vals, case.ncols)
        assert np.array_equal(dense, want), (dof, nnodes, ghost, empty)
        # the stored values are the CSR values and zeros, nothing else
        assert np.count_nonzero(bvals) == len(case.vals)


# ---------------------------------------------------------------------------
# torch_ref vs oracle

@pytest.mark.parametrize("ghost", [False, True])
@pytest.mark.parametrize("nnodes", BSELL_NODES)
@pytest.mark.parametrize("dof", DOFS)
def test_ref_spmv_bsell(dof, nnodes, ghost):
    case = _bsell(dof, nnodes, ghost)
    for dotslot, acc in ((-1, False), (ko.S_PT, False), (ko.S_PT, True)):
        e = ko.bsell_spmv_expect(case, dotslot, acc)
        got = ko.run_bsell_spmv(torch_ref, case, CPU, dotslot=dotslot, dot_accum=acc)
        ko.assert_accepts(e, got, f"dof{dof} n{nnodes} ghost{ghost} slot{dotslot} acc{acc}")


@pytest.mark.parametrize("beta_zero", [True, False])
@pytest.mark.parametrize("nnodes", BSELL_NODES)
@pytest.mark.parametrize("dof", DOFS)
def test_ref_spmv_bsell_daypx(dof, nnodes, beta_zero):
    case = _bsell(dof, nnodes, False)
    e = ko.bsell_daypx_expect(case, beta_zero)
    got = ko.run_bsell_daypx(torch_ref, case, CPU, beta_zero)
    ko.assert_accepts(e, got, f"dof{dof} n{nnodes} beta0={beta_zero}")


@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("nowned,split,nborder0", PIPE_CASES)
def test_ref_sell_pipe(nowned, split, nborder0, first):
    case = _pipe(nowned, split, nborder0)
    e = ko.pipe_expect(case, first)
    got = ko.run_pipe(torch_ref, case, CPU, first)
    ko.assert_accepts(e, got, f"n{nowned} split{split} nb0{nborder0} first{first}")


@pytest.mark.parametrize("pt_zero", [False, True])
@pytest.mark.parametrize("n", VEC_N)
def test_ref_pcg_fused_update(n, pt_zero):
    case = _vec(n, pt_zero)
    got = ko.run_pcg(torch_ref, case, CPU)
    ko.assert_accepts(ko.pcg_expect(case), got, f"n{n} pt0={pt_zero}")


@pytest.mark.parametrize("n", DOT_N)
def test_ref_dot_dot2_cg_update(n):
    case = _vec(n)
    for acc in (False, True):
        ko.assert_accepts(ko.dot_expect(case, ko.S_PT, acc),
                          ko.run_dot(torch_ref, case, CPU, ko.S_PT, acc), f"n{n} acc{acc}")
        ko.assert_accepts(ko.dot2_expect(case, acc),
                          ko.run_dot2(torch_ref, case, CPU, acc), f"n{n} acc{acc}")
    ko.assert_accepts(ko.cg_update_expect(case),
                      ko.run_cg_update(torch_ref, case, CPU), f"n{n}")


@pytest.mark.parametrize("nslices", SELL_SLICES)
def test_ref_spmv_sell(nslices):
    case = _sell(nslices)
    for col64 in (False, True):
        for acc in (False, True):
            got = ko.run_sell_spmv(torch_ref, case, CPU, col64=col64, dot_accum=acc)
            ko.assert_accepts(ko.sell_spmv_expect(case, dot_accum=acc), got,
                              f"ns{nslices} col64={col64} acc{acc}")
    packed = torch_ref.sell_from_csr(case.rowptr, case.cols.astype(np.int32),
                                     case.vals, sigma=4)
    got = ko.run_sell_spmv(torch_ref, case, CPU, packed=packed)
    ko.assert_accepts(ko.sell_spmv_expect(case, perm=packed[3]), got,
                      f"ns{nslices} sigma4")


def test_ref_csr_spmv_and_binned():
    case = _sell(3)
    for binned in (False, True):
        for rowbase, accum, dacc in ((0, False, False), (5, True, True)):
            got = ko.run_csr_spmv(torch_ref, case, CPU, rowbase=rowbase,
                                  accum=accum, dot_accum=dacc, binned=binned)
            ko.assert_accepts(ko.csr_spmv_expect(case, rowbase, accum, dacc), got,
                              f"binned{binned} rowbase{rowbase}")


@pytest.mark.parametrize("n", [1, 257, 4099])
def test_ref_vector_ops(n):
    case = _vec(n)
    for op in ("axpy_ratio", "daypx_ratio"):
        for n_act in {n, max(n - 3, 0)}:
            ko.assert_accepts(ko.ratio_update_expect(case, op, n_act),
                              ko.run_ratio_update(torch_ref, case, CPU, op, n_act),
                              f"{op} n{n} act{n_act}")
    fc = ko.fused_case(n)
    for first in (True, False):
        ko.assert_accepts(ko.fused_expect(fc, first),
                          ko.run_fused(torch_ref, fc, CPU, first), f"n{n} first{first}")
    for idx64 in (False, True):
        e, got = ko.run_exact_ops(torch_ref, CPU, idx64)
        ko.assert_accepts(e, got, f"idx64={idx64}")


def test_every_gpu_op_has_a_reference():
    """gpu_ops and torch_ref expose the same operations (host-side prep
    aside)."""
    import ast
    from pathlib import Path

    src = Path(torch_ref.__file__).with_name("gpu_ops.py").read_text()
    ops = {n.name for n in ast.parse(src).body
           if isinstance(n, ast.FunctionDef) and not n.name.startswith("_")}
    ops -= {"pick_lanes", "build_row_bins", "build_sellcsr_hybrid"}
    missing = sorted(o for o in ops if not hasattr(torch_ref, o))
    assert not missing, missing
    try:
        from acg_amd.ops import gpu_ops
    except ImportError:  # extension not built on this machine
        return
    # torch_ref keeps its own copy so that it imports without the extension
    assert torch_ref.BAR_STATE_WORDS == gpu_ops.BAR_STATE_WORDS


@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("nowned", [65, 200])
def test_ref_sell_pipe_equals_spmv_plus_fused(nowned, first):
    """On a serial system the megafused reference is the unfused one."""
    case = _pipe(nowned, False, False)
    got = ko.run_pipe(torch_ref, case, CPU, first)
    sp, sc, sv = (torch.from_numpy(a) for a in torch_ref.sell_from_csr(
        case.A[0], case.A[1].astype(np.int32), case.A[2]))
    v = {k: torch.from_numpy(getattr(case, k).copy()) for k in "ztpxr"}
    w = torch.from_numpy(case.w_old.copy())
    q = torch.zeros(nowned, dtype=torch.float64)
    scal = torch.from_numpy(case.scal.copy())
    torch_ref.spmv_sell(sp, sc, sv, nowned, w, q)
    torch_ref.pipelined_fused(v["z"], v["t"], v["p"], v["x"], v["r"], w, q,
                              scal, torch_ref.alloc_partials(), nowned, first)
    for k in "ztpxr":
        assert np.array_equal(got[k], v[k].numpy()), k
    assert np.array_equal(got["w_new"], w.numpy())
    for i in range(ko.S_NSLOTS):
        assert got[f"scal{i}"][0] == float(scal[i]), i


# ---------------------------------------------------------------------------
# discrimination: wrong results the acceptance helper must reject

def _transpose_blocks(dense, dof):
    nn, ncn = dense.shape[0] // dof, dense.shape[1] // dof
    return (dense.reshape(nn, dof, ncn, dof).transpose(0, 3, 2, 1)
            .reshape(nn * dof, ncn * dof))


@pytest.mark.parametrize("ghost", [False, True])
@pytest.mark.parametrize("nnodes", BSELL_NODES)
@pytest.mark.parametrize("dof", DOFS)
def test_mutant_block_transposed(dof, nnodes, ghost):
    """Mutant 1: acc[k % DOF] += a * xv[k / DOF]."""
    case = _bsell(dof, nnodes, ghost)
    dense_t = _transpose_blocks(
        ko.csr_dense(case.rowptr, case.cols, case.vals, case.ncols), dof)
    e = ko.bsell_spmv_expect(case)
    got = ko.run_bsell_spmv(torch_ref, case, CPU)
    assert ko.accepts(e, got)
    got["y"] = dense_t @ case.x
    assert not ko.accepts(e, got)
    if not ghost:
        for beta_zero in (True, False):
            e = ko.bsell_daypx_expect(case, beta_zero)
            got = ko.run_bsell_daypx(torch_ref, case, CPU, beta_zero)
            assert ko.accepts(e, got)
            got["y"] = dense_t @ got["pnew"]
            assert not ko.accepts(e, got)


@pytest.mark.parametrize("ghost", [False, True])
@pytest.mark.parametrize("nnodes", BSELL_NODES)
def test_mutant_odd_tail_from_neighbour_lane(nnodes, ghost):
    """Mutant 2 (dof^2 odd, so dof = 3): element k = 8 read at lane + 1."""
    dof, D2 = 3, 9
    case = _bsell(dof, nnodes, ghost)
    bptr, bcol, bvals, _ = torch_ref.bsell_from_csr(case.rowptr, case.cols,
                                                    case.vals, dof)
    bad = bvals.copy()
    for s in range(len(bptr) - 1):
        for j in range((bptr[s + 1] - bptr[s]) // 64):
            t0 = bptr[s] * D2 + j * D2 * 64 + (D2 - 1) * 64
            bad[t0:t0 + 64] = np.roll(bvals[t0:t0 + 64], -1)
    packed = tuple(torch.from_numpy(a) for a in (bptr, bcol, bad))
    e = ko.bsell_spmv_expect(case)
    assert not ko.accepts(e, ko.run_bsell_spmv(torch_ref, case, CPU, packed=packed))
    if not ghost:
        e = ko.bsell_daypx_expect(case, False)
        assert not ko.accepts(e, ko.run_bsell_daypx(torch_ref, case, CPU, False,
                                                   packed=packed))


def _csr_mv(csr, w, drop_tail=False):
    rowptr, cols, vals = csr
    prod = vals * w[cols]
    if drop_tail:
        lens = np.diff(rowptr)
        prod[rowptr[1:][lens % 8 != 0] - 1] = 0.0
    q = np.zeros(len(rowptr) - 1)
    np.add.at(q, ko.csr_rows(rowptr), prod)
    return q


@pytest.mark.parametrize("nslices", SELL_SLICES)
def test_mutant_sell_tail_entry_dropped(nslices):
    """Mutant 3 on k_spmv_sell: last entry of rows with len % 8 != 0 lost."""
    case = _sell(nslices)
    e = ko.sell_spmv_expect(case)
    got = ko.run_sell_spmv(torch_ref, case, CPU)
    assert ko.accepts(e, got)
    got["y"] = _csr_mv((case.rowptr, case.cols, case.vals), case.x, drop_tail=True)
    assert not ko.accepts(e, got)


def test_short_slices_ref_and_tail_mutant():
    """Slices shorter than the unroll width (and empty ones): reference
    accepted, dropped-tail mutant rejected, for k_spmv_sell and k_sell_pipe."""
    case = ko.sell_case(8, short=True)
    assert set(ko.sell_padded_len(case.rowptr)) == {0, 1, 7, 9}
    e = ko.sell_spmv_expect(case)
    got = ko.run_sell_spmv(torch_ref, case, CPU)
    ko.assert_accepts(e, got, "short")
    got["y"] = _csr_mv((case.rowptr, case.cols, case.vals), case.x, drop_tail=True)
    assert not ko.accepts(e, got)
    for nowned, split in ((250, False), (400, True)):
        pc = ko.pipe_case(nowned, split, short=True)
        for first in (True, False):
            e = ko.pipe_expect(pc, first)
            ko.assert_accepts(e, ko.run_pipe(torch_ref, pc, CPU, first),
                              f"short n{nowned} first{first}")
            assert ko.accepts(e, _emulate_pipe(pc, first))
            for m in ["tail", "swap", "first", "finalize"] + (
                    ["border", "qpart"] if split else []):
                assert not ko.accepts(e, _emulate_pipe(pc, first, m)), m


def _emulate_pipe(case, first, mutant=None):
    """fp64 emulation of matA pass, matO pass and finalize with one defect
    switched on.  Memory a defect reads without having written it holds
    zeros -- the most forgiving garbage there is."""
    n, ni, nb = case.nowned, case.ninterior, case.nborder
    scal = case.scal.copy()
    st = {k: getattr(case, k).copy() for k in "ztpxr"}
    w_old, w_new = case.w_old, np.full(case.nlocal, np.nan)
    qpart = np.zeros(n + 1)
    use_first = (not first) if mutant == "first" else first
    beta, alpha = torch_ref._pipelined_coeffs(torch.from_numpy(scal), use_first)
    if mutant == "swap":
        alpha, beta = beta, alpha
    sums = [0.0, 0.0]

    def update(rows, q):
        zi = q + beta * st["z"][rows]
        ti = w_old[rows] + beta * st["t"][rows]
        pi = st["r"][rows] + beta * st["p"][rows]
        st["z"][rows], st["t"][rows], st["p"][rows] = zi, ti, pi
        st["x"][rows] += alpha * pi
        rn = st["r"][rows] - alpha * ti
        wn = w_old[rows] - alpha * zi
        st["r"][rows], w_new[rows] = rn, wn
        sums[0] += float(rn @ rn)
        sums[1] += float(wn @ rn)

    qA = _csr_mv(case.A, w_old, drop_tail=mutant == "tail")
    bb = case.border_base + (1 if mutant == "border" and nb else 0)
    rows = np.arange(0, bb)
    update(rows, qA[rows])
    rows = np.arange(bb, n)
    qpart[rows - case.border_base] = qA[rows]
    got = {}
    if nb:
        for k in "ztpxr":
            got[f"matA/{k}_border"] = st[k][ni:].copy()
        got["matA/w_new_border"] = w_new[ni:].copy()
        qO = _csr_mv(case.O, w_old, drop_tail=mutant == "tail")
        rows = np.arange(ni, n)
        update(rows, qO + (qpart[rows] if mutant == "qpart" else qpart[rows - ni]))
    if mutant == "finalize":
        scal[ko.S_GAMMA_PREV] = alpha
    else:
        scal[ko.S_GAMMA_PREV] = scal[ko.S_GAMMA]
        scal[ko.S_ALPHA_PREV] = alpha
    scal[ko.S_GAMMA], scal[ko.S_DELTA] = sums
    got.update(st)
    got["w_new"], got["w_new_tail"] = w_new[:n].copy(), w_new[n:].copy()
    for i in range(ko.S_NSLOTS):
        got[f"scal{i}"] = scal[i:i + 1]
    return got


@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("nowned,split,nborder0", PIPE_CASES)
def test_mutants_sell_pipe(nowned, split, nborder0, first):
    """Mutants 3-8 on k_sell_pipe / k_pipelined_finalize."""
    case = _pipe(nowned, split, nborder0)
    e = ko.pipe_expect(case, first)
    assert ko.accepts(e, _emulate_pipe(case, first)), "emulator itself is off"
    mutants = ["tail", "swap", "first", "finalize"]
    if case.nborder:
        mutants += ["border", "qpart"]
    for m in mutants:
        assert not ko.accepts(e, _emulate_pipe(case, first, m)), m


@pytest.mark.parametrize("pt_zero", [False, True])
@pytest.mark.parametrize("n", VEC_N)
def test_mutant_pcg_finalize_slots_swapped(n, pt_zero):
    """Mutant 9: rr published in S_RR and rz in S_GAMMA."""
    case = _vec(n, pt_zero)
    e = ko.pcg_expect(case)
    got = ko.run_pcg(torch_ref, case, CPU)
    assert ko.accepts(e, got)
    k_rz, k_rr = f"scal{ko.S_RR}", f"scal{ko.S_GAMMA}"
    got[k_rz], got[k_rr] = got[k_rr], got[k_rz]
    assert not ko.accepts(e, got)


def test_bound_rejects_one_dropped_entry():
    """The flat atol=1e-10 this replaces would pass a lost entry of size
    1e-11; the derived bound must not, and a one-ulp change of a long
    row's result must still pass."""
    case = _sell(3)
    e = ko.sell_spmv_expect(case)
    got = ko.run_sell_spmv(torch_ref, case, CPU)
    y = got["y"].copy()
    i = int(np.argmax(np.diff(case.rowptr)))
    got["y"] = y.copy()
    got["y"][i] = np.nextafter(y[i], np.inf)
    got[f"scal{ko.S_PT}"] = got[f"scal{ko.S_PT}"].copy()
    assert ko.accepts(e, got)
    got["y"][i] = y[i] + 1e-11
    assert not ko.accepts(e, got)


# ---------------------------------------------------------------------------
# the one-launch device CG: reference vs the step-chained oracle, and mutants

DEVCG_SLICES = (1, 5, 28, 33)
DEVCG_MUTANTS = ("stale_p", "drop_pt", "drop_rr", "alpha_rr", "beta_inv",
                 "p_old_r", "x_from_t", "rotate_prev", "touch_x", "conv_rt")


@lru_cache(maxsize=None)
def _devcg(nslices):
    return ko.device_cg_case(nslices)


def _ref_launch(case):
    return lambda **kw: ko.run_device_cg(torch_ref, case, CPU, **kw)


def _devcg_check_all(launch, case):
    gots = ko.device_cg_check_chain(launch, case, ks=(0, 1, 2, 3, 4, 5))
    ko.device_cg_check_tolerances(launch, case, gots)


@pytest.mark.parametrize("nslices", DEVCG_SLICES)
def test_ref_cg_device(nslices):
    """torch_ref.cg_device passes the init check, the chained steps k = 0..4
    (and 5, which the tolerance checks need) and the tolerance checks."""
    case = _devcg(nslices)
    _devcg_check_all(_ref_launch(case), case)
    got = _ref_launch(case)(maxits=3)
    assert got["grid"] == ko.device_cg_blocks(nslices)
    assert got["grid"] == {1: 1, 5: 2, 28: 7, 33: 9}[nslices]


def test_ref_cg_device_col64_zero_rhs_and_fp32_refusal():
    case = _devcg(5)
    a = ko.run_device_cg(torch_ref, case, CPU, maxits=4)
    b = ko.run_device_cg(torch_ref, case, CPU, maxits=4, col64=True)
    assert not ko.device_cg_same_bits(a, b)
    zero = ko.device_cg_case(5, zero_b=True, zero_x0=True)
    ko.device_cg_check_zero(_ref_launch(zero), zero)
    sp, sc, sv = (torch.from_numpy(a) for a in case._packed[False])
    v = torch.zeros(case.nrows, dtype=torch.float64)
    with pytest.raises(ValueError, match="float64"):
        torch_ref.cg_device(sp, sc, sv.float(), case.nrows, v, v, v, v, v,
                            torch_ref.alloc_scalars(), torch_ref.alloc_partials(),
                            torch.zeros(2, dtype=torch.int32), None, 1, 0.0, 0.0)


def _emulate_device_cg(case, mutant=None, *, maxits, atol=0.0, rtol=0.0):
    """fp64 emulation of k_cg_device on a grid of ceil(nslices/4) blocks of
    256 rows, with one defect switched on.  Memory a defect reads without
    having written it holds zeros."""
    n = case.nrows
    grid = ko.device_cg_blocks(case.nslices)
    last = slice((grid - 1) * 256, n)
    A = (case.rowptr, case.cols, case.vals)
    scal = ko.SENTINELS.copy()
    partials = np.full(2 * ko.MAXG, np.nan)

    def gsum(v, slot, drop=False):
        part = np.add.reduceat(v, np.arange(0, n, 256))
        assert len(part) == grid
        partials[:grid] = part
        scal[slot] = part[:-1].sum() if drop else part.sum()

    b, x = case.b, case.x0.copy()
    gsum(b * b, ko.S_BNRM2)
    t = _csr_mv(A, x)
    r = b - t
    p = r.copy()
    if mutant == "touch_x":
        x[-1] = np.nextafter(x[-1], np.inf)
    gsum(r * r, ko.S_RR)
    scal[ko.S_RR_PREV] = scal[ko.S_RR]
    rr = scal[ko.S_RR]
    rr_stale = scal[ko.S_BNRM2]
    rt = max(rtol * np.sqrt(scal[ko.S_BNRM2]), atol)
    rtol2 = rt if mutant == "conv_rt" else rt * rt
    p_prev = np.zeros(n)
    sdiv = lambda a, d: a / d if d != 0.0 else 0.0
    k, converged = 0, bool(rtol2 > 0.0 and rr <= rtol2)
    while not converged and k < maxits:
        t = _csr_mv(A, p)
        if mutant == "stale_p":  # the last block gathered last iteration's p
            t[last] = _csr_mv(A, p_prev)[last]
        gsum(p * t, ko.S_PT, drop=mutant == "drop_pt")
        alpha = sdiv(rr_stale if mutant == "alpha_rr" else rr, scal[ko.S_PT])
        r_old = r
        r = r - alpha * t
        x = x + alpha * (t if mutant == "x_from_t" else p)
        gsum(r * r, ko.S_RR, drop=mutant == "drop_rr")
        rr_new = scal[ko.S_RR]
        beta = sdiv(rr, rr_new) if mutant == "beta_inv" else sdiv(rr_new, rr)
        p_prev = p
        p = beta * p + (r_old if mutant == "p_old_r" else r)
        if mutant == "rotate_prev":
            scal[ko.S_RR_PREV] = rr
        rr_stale, rr = rr, rr_new
        k += 1
        converged = bool(rtol2 > 0.0 and rr <= rtol2)
    got = {"x": x, "r": r, "p": p, "t": t, "grid": grid, "partials": partials,
           "nblocks": grid, "out2": np.array([k, int(converged)], dtype=np.int32)}
    for i in range(ko.S_NSLOTS):
        got[f"scal{i}"] = scal[i:i + 1].copy()
    return got


@pytest.mark.parametrize("nslices", DEVCG_SLICES)
def test_mutants_cg_device(nslices):
    """Every defect must be rejected by the checks the GPU tests run, at
    every case.  ``alpha_rr``: alpha takes the (r,r) of the wrong iteration
    (the one before; (b,b) in the first step) -- inside one iteration
    rr_new does not exist yet when alpha is formed."""
    case = _devcg(nslices)
    from functools import partial

    _devcg_check_all(partial(_emulate_device_cg, case, None), case)
    for m in DEVCG_MUTANTS:
        with pytest.raises(AssertionError):
            _devcg_check_all(partial(_emulate_device_cg, case, m), case)
        print(f"mutant {m}: rejected")
