"""Kernel-level exactness of the matrix-free stencil kernels (k_stencil_spmv,
k_stencil_spmv7, k_stencil_pipe, k_stencil_pipe7) and the slab generators
(k_stencil_rowlen, k_stencil_fill, k_stencil_blocklen, k_stencil_bfill)
against the global-coordinate oracles of tests/kernel_oracle.py.

Every stencil has pairwise distinct per-offset weights, so an exchanged
weight, a wrong offset index or a wrong plane shows; the inputs are the
ones tests/test_stencil_oracle_cpu.py proves discriminating.  The operator
tables come from device_stencil_slab, i.e. through the dispatch the solver
uses.  Each check prints an ``ORACLE_RATIO`` line."""

import time
from functools import lru_cache

import numpy as np
import pytest
import torch

import kernel_oracle as ko

pytestmark = pytest.mark.gpu

CASE_IDS = ko.stencil_case_ids()
Expect = ko.Expect
DOFS = (1, 2, 3, 4)


def _tag(cid):
    return "{}-{}x{}x{}-r{}of{}".format(*cid)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gpu_ops():
    from acg_amd.ops import gpu_ops

    assert gpu_ops.MAXG == ko.MAXG and gpu_ops.S_NSLOTS == ko.S_NSLOTS
    return gpu_ops


@lru_cache(maxsize=None)
def _case(*cid):
    return ko.stencil_case(*cid)


@lru_cache(maxsize=None)
def _structure(cid, dof):
    kind, gx, gy, gz, rank, nranks = cid
    return ko.stencil_structure(gx, gy, gz, ko.stencil_spec(kind, dof), rank, nranks)


def _variants(case, dev):
    """(matA kernel name, mf) pairs: the dispatch of device_stencil_slab
    and, for 7-point stencils, the generic kernel forced on top."""
    from acg_amd.gen.device_slab import device_stencil_slab

    S = device_stencil_slab(case.gx, case.gy, case.gz, case.spec, case.rank,
                            case.nranks, dev, operator=False)
    assert (S.nowned, S.ninterior, S.nborder, S.nghost) == \
        (case.nowned, case.ninterior, case.nborder, case.nghost)
    mf = S.mf_tables
    assert (mf["w7"] is not None) == (case.kind == "7pt")
    if mf["w7"] is None:
        return [("", mf)]
    return [("7", mf), ("", {**mf, "w7": None})]


@pytest.mark.parametrize("cid", CASE_IDS, ids=_tag)
def test_stencil_spmv(dev, gpu_ops, cid):
    case = _case(*cid)
    for sfx, mf in _variants(case, dev):
        for fused in (True, False):
            got = ko.run_stencil_spmv(gpu_ops, case, dev, mf, fused)
            ko.assert_accepts(
                ko.stencil_spmv_expect(case, fused, f"k_stencil_spmv{sfx}"), got,
                f"{_tag(cid)} fused{fused}")
            ko.check_partials(got, halves=1)


@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("cid", CASE_IDS, ids=_tag)
def test_stencil_pipe(dev, gpu_ops, cid, first):
    case = _case(*cid)
    for sfx, mf in _variants(case, dev):
        got = ko.run_stencil_pipe(gpu_ops, case, dev, mf, first)
        nbA = ko.stencil_blocks(case, sfx == "7", case.nowned)
        nbO = ko.stencil_blocks(case, False, case.nborder) if case.nborder else 0
        assert (got["nbA"], got["nbO"]) == (nbA, nbO)
        ko.assert_accepts(
            ko.stencil_pipe_expect(case, first, f"k_stencil_pipe{sfx}"), got,
            f"{_tag(cid)} first{first}")
        ko.check_partials(got, halves=2)


def test_large_plane_grid_stride(dev, gpu_ops):
    """A 2049 x 2048 plane has more (x, y) columns than either walk kernel
    may start threads for: both run their grid-stride loop."""
    t0 = time.perf_counter()
    case = ko.stencil_case(*ko.STENCIL_LARGE, host_map=False)
    ko.stencil_products(case)
    e_spmv = ko.stencil_spmv_expect(case, True, "k_stencil_spmv7")
    e_pipe = ko.stencil_pipe_expect(case, True, "k_stencil_pipe7")
    print(f"LARGE_PLANE_ORACLE_SECONDS {time.perf_counter() - t0:.1f}")
    (sfx, mf), _ = _variants(case, dev)
    assert sfx == "7"
    got = ko.run_stencil_spmv(gpu_ops, case, dev, mf, True)
    assert case.plane > ko.MAXG * 256 and got["nblocks"] == ko.MAXG
    ko.assert_accepts(e_spmv, got, "large")
    ko.check_partials(got, halves=1)
    got = ko.run_stencil_pipe(gpu_ops, case, dev, mf, True)
    assert (got["nbA"], got["nbO"]) == (ko.MAXG - 1024, 0)
    ko.assert_accepts(e_pipe, got, "large")
    ko.check_partials(got, halves=2)


# ---------------------------------------------------------------------------
# generators

def _check_sell(e, got, name, sell, rows, nrows, nlocal):
    sellptr, cols, vals = (a.cpu().numpy() for a in sell)
    assert cols.dtype == np.int32 and vals.dtype == np.float64
    if nrows == 0:
        assert sellptr.tolist() == [0] and len(cols) == len(vals) == 0
        return
    assert not np.signbit(vals[vals == 0.0]).any()
    drows, lens, padcols = ko.sell_to_rows(sellptr, cols, vals, nrows)
    rowptr, wcols, wvals = ko.rows_to_csr(rows)
    grp, gcols, gvals = ko.rows_to_csr(drows)
    e.add_exact(f"{name}/rowptr", rowptr)
    e.add_exact(f"{name}/cols", wcols)
    e.add_exact(f"{name}/vals", wvals)
    e.add_exact(f"{name}/slice_len", ko.sell_padded_len(rowptr))
    got.update({f"{name}/rowptr": grp, f"{name}/cols": gcols,
                f"{name}/vals": gvals, f"{name}/slice_len": lens})
    # padding: value exactly 0 (by construction of padcols), column in range
    assert len(padcols) == len(vals) - len(wvals)
    assert np.all((padcols >= 0) & (padcols < nlocal)), name


@pytest.mark.parametrize("dof", DOFS)
@pytest.mark.parametrize("cid", CASE_IDS, ids=_tag)
def test_generators(dev, cid, dof):
    from acg_amd.gen.device_slab import device_stencil_slab

    kind, gx, gy, gz, rank, nranks = cid
    spec = ko.stencil_spec(kind, dof)
    W = _structure(cid, dof)
    S = device_stencil_slab(gx, gy, gz, spec, rank, nranks, dev)
    assert (S.nowned, S.ninterior, S.nborder, S.nghost) == \
        (W.nowned, W.ninterior, W.nborder, W.nghost)
    assert (S.nnzA, S.nnzO) == (W.nnzA, W.nnzO)
    S0 = device_stencil_slab(gx, gy, gz, spec, rank, nranks, dev, operator=False)
    assert (S0.nnzA, S0.nnzO) == (W.nnzA, W.nnzO)
    assert S0.A_sell is None and S0.O_sell is None and S0.A_bsell is None
    e, got = Expect("k_stencil_rowlen/k_stencil_fill"), {}
    _check_sell(e, got, "A", S.A_sell, W.rowsA, W.nowned, W.nlocal)
    _check_sell(e, got, "O", S.O_sell, W.rowsO, W.nborder, W.nlocal)
    ko.assert_accepts(e, got, f"{_tag(cid)} dof{dof}")
    if dof == 1:
        assert S.A_bsell is None
        return
    bptr, bcol, bvals, bdof = S.A_bsell
    assert bdof == dof and bcol.dtype == torch.int32
    bptr, bcol, bvals = (a.cpu().numpy() for a in (bptr, bcol, bvals))
    nnodes = W.nowned // dof
    rowptr, wcols, wvals = ko.rows_to_csr(W.rowsA)
    e, got = Expect("k_stencil_blocklen/k_stencil_bfill"), {}
    # unpack_bsell asserts every block column (padding included) in bounds
    e.add_exact("dense", ko.csr_dense(rowptr, wcols, wvals, W.nowned))
    got["dense"] = ko.unpack_bsell(bptr, bcol, bvals, nnodes, dof, W.nowned)
    e.add_exact("slice_len", ko.bsell_padded_len(rowptr, wcols, dof))
    assert np.all(np.diff(bptr) % 64 == 0) and len(bptr) == (nnodes + 63) // 64 + 1
    got["slice_len"] = np.repeat(np.repeat(np.diff(bptr) // 64, 64)[:nnodes], dof) * dof
    ko.assert_accepts(e, got, f"{_tag(cid)} dof{dof}")
    # every stored value is an operator entry or an exact zero
    assert np.count_nonzero(bvals) == W.nnzA and len(bvals) == bptr[-1] * dof * dof

