"""Kernel-level exactness on the GPU: the block-SELL, megafused pipelined,
Jacobi-PCG, SELL-variant and reduction kernels against the high-precision
oracle (tests/kernel_oracle.py), through gpu_ops, on NaN-poisoned buffers.

The acceptance bounds are derived (kernel_oracle docstring), the inputs are
the ones tests/test_kernel_oracle_cpu.py proves discriminating.  Each check
prints an ``ORACLE_RATIO`` line with the worst observed error/bound."""

from functools import lru_cache

import numpy as np
import pytest
import torch

import kernel_oracle as ko

pytestmark = pytest.mark.gpu

DOFS = (2, 3, 4)
BSELL_NODES = (1, 63, 65, 130)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gpu_ops():
    from acg_amd.ops import gpu_ops

    assert gpu_ops.MAXG == ko.MAXG and gpu_ops.S_NSLOTS == ko.S_NSLOTS
    for name in ("S_RR", "S_PT", "S_RR_PREV", "S_BNRM2", "S_GAMMA", "S_DELTA",
                 "S_GAMMA_PREV", "S_ALPHA_PREV"):
        assert getattr(gpu_ops, name) == getattr(ko, name)
    return gpu_ops


@lru_cache(maxsize=None)
def _bsell(dof, nnodes, ghost):
    return ko.bsell_case(dof, nnodes, ghost)


@lru_cache(maxsize=None)
def _pipe(nowned, split, nborder0):
    return ko.pipe_case(nowned, split, nborder0)


@lru_cache(maxsize=None)
def _sell(nslices):
    case = ko.sell_case(nslices)
    return case, ko.sell_spmv_expect(case), ko.sell_spmv_expect(case, dot_accum=True)


@lru_cache(maxsize=None)
def _vec(n, pt_zero=False):
    return ko.vec_case(n, pt_zero)


# ---------------------------------------------------------------------------
# Block-SELL

@pytest.mark.parametrize("ghost", [False, True])
@pytest.mark.parametrize("nnodes", BSELL_NODES)
@pytest.mark.parametrize("dof", DOFS)
def test_spmv_bsell(dev, gpu_ops, dof, nnodes, ghost):
    case = _bsell(dof, nnodes, ghost)
    packed = ko.pack_bsell(case, dev)
    for dotslot, acc in ((-1, False), (ko.S_PT, False), (ko.S_PT, True)):
        got = ko.run_bsell_spmv(gpu_ops, case, dev, dotslot=dotslot,
                                dot_accum=acc, packed=packed)
        ko.assert_accepts(ko.bsell_spmv_expect(case, dotslot, acc), got,
                          f"dof{dof} n{nnodes} ghost{ghost} slot{dotslot} acc{acc}")
        ko.check_partials(got, halves=1)


@pytest.mark.parametrize("beta_zero", [True, False])
@pytest.mark.parametrize("nnodes", BSELL_NODES)
@pytest.mark.parametrize("dof", DOFS)
def test_spmv_bsell_daypx(dev, gpu_ops, dof, nnodes, beta_zero):
    case = _bsell(dof, nnodes, False)
    got = ko.run_bsell_daypx(gpu_ops, case, dev, beta_zero)
    ko.assert_accepts(ko.bsell_daypx_expect(case, beta_zero), got,
                      f"dof{dof} n{nnodes} beta0={beta_zero}")
    ko.check_partials(got, halves=1)


# ---------------------------------------------------------------------------
# megafused pipelined iteration

@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("nowned,split,nborder0", [
    (65, False, False), (200, False, False),   # serial
    (65, True, False), (200, True, False),     # interior | border | ghost
    (65, True, True),                          # ghosts but nborder = 0
])
def test_sell_pipe_and_finalize(dev, gpu_ops, nowned, split, nborder0, first):
    case = _pipe(nowned, split, nborder0)
    got = ko.run_pipe(gpu_ops, case, dev, first)
    nslA = (nowned + 63) // 64
    nslO = (case.nborder + 63) // 64
    assert got["nblocks"] == ko.sell_blocks(nslA) + (ko.sell_blocks(nslO) if nslO else 0)
    ko.assert_accepts(ko.pipe_expect(case, first), got,
                      f"n{nowned} split{split} nb0{nborder0} first{first}")
    ko.check_partials(got, halves=2)


# ---------------------------------------------------------------------------
# Jacobi-PCG epilogue

@pytest.mark.parametrize("pt_zero", [False, True])
@pytest.mark.parametrize("n", [1, 257, 300_001])
def test_pcg_fused_update(dev, gpu_ops, n, pt_zero):
    case = _vec(n, pt_zero)
    got = ko.run_pcg(gpu_ops, case, dev)
    assert (got["nblocks"] > 256) == (n == 300_001)
    ko.assert_accepts(ko.pcg_expect(case), got, f"n{n} pt0={pt_zero}")
    ko.check_partials(got, halves=2)


# ---------------------------------------------------------------------------
# SELL kernel variants

@pytest.mark.parametrize("col64", [False, True])
@pytest.mark.parametrize("nslices", [3, 37, 100])
@pytest.mark.parametrize("variant", range(8))
def test_spmv_sell_variants(dev, gpu_ops, variant, nslices, col64):
    case, e_set, e_acc = _sell(nslices)
    assert ko.sell_blocks(nslices) == {3: 1, 37: 10, 100: 25}[nslices]
    for acc, e in ((False, e_set), (True, e_acc)):
        got = ko.run_sell_spmv(gpu_ops, case, dev, col64=col64, variant=variant,
                               dot_accum=acc)
        ko.assert_accepts(e, got, f"v{variant} ns{nslices} col64={col64} acc{acc}")
        ko.check_partials(got, halves=1)


@pytest.mark.parametrize("u8", [False, True])
def test_spmv_sell_sigma_perm(dev, gpu_ops, u8):
    from acg_amd.ops import torch_ref

    case, _, _ = _sell(37)
    packed = torch_ref.sell_from_csr(case.rowptr, case.cols.astype(np.int32),
                                     case.vals, sigma=4)
    variant = gpu_ops.SELL_NT | (gpu_ops.SELL_U8 if u8 else 0)
    got = ko.run_sell_spmv(gpu_ops, case, dev, variant=variant, packed=packed)
    ko.assert_accepts(ko.sell_spmv_expect(case, perm=packed[3]), got, f"u8={u8}")
    ko.check_partials(got, halves=1)


@pytest.mark.parametrize("variant", [0, 1, 4, 5])
def test_spmv_sell_short_slices(dev, gpu_ops, variant):
    """Slice lengths 0, 1, 7, 9: below the unroll width of either flavour,
    empty, and one full unrolled step plus a one-entry tail."""
    case = ko.sell_case(8, short=True)
    got = ko.run_sell_spmv(gpu_ops, case, dev, variant=variant)
    ko.assert_accepts(ko.sell_spmv_expect(case), got, f"short v{variant}")
    ko.check_partials(got, halves=1)


@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("nowned,split", [(250, False), (400, True)])
def test_sell_pipe_short_slices(dev, gpu_ops, nowned, split, first):
    case = ko.pipe_case(nowned, split, short=True)
    got = ko.run_pipe(gpu_ops, case, dev, first)
    ko.assert_accepts(ko.pipe_expect(case, first), got,
                      f"short n{nowned} split{split} first{first}")
    ko.check_partials(got, halves=2)


# ---------------------------------------------------------------------------
# reductions and the classic fused update

@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("n", [1, 255, 257, 1025, 300_001])
def test_dot_and_dot2(dev, gpu_ops, n, accumulate):
    case = _vec(n)
    got = ko.run_dot(gpu_ops, case, dev, ko.S_PT, accumulate)
    ko.assert_accepts(ko.dot_expect(case, ko.S_PT, accumulate), got,
                      f"n{n} acc{accumulate}")
    ko.check_partials(got, halves=1)
    got = ko.run_dot2(gpu_ops, case, dev, accumulate)
    ko.assert_accepts(ko.dot2_expect(case, accumulate), got, f"n{n} acc{accumulate}")
    ko.check_partials(got, halves=2)


@pytest.mark.parametrize("col64", [False, True])
@pytest.mark.parametrize("lanes", [4, 8, 16, 32, 64])
def test_spmv_csr_vector(dev, gpu_ops, lanes, col64):
    case = _sell(3)[0]
    for rowbase, accum, dacc in ((0, False, False), (5, True, True)):
        got = ko.run_csr_spmv(gpu_ops, case, dev, rowbase=rowbase, accum=accum,
                              dot_accum=dacc, col64=col64, lanes=lanes)
        ko.assert_accepts(ko.csr_spmv_expect(case, rowbase, accum, dacc), got,
                          f"lanes{lanes} col64={col64} rowbase{rowbase}")
        ko.check_partials(got, halves=1)


@pytest.mark.parametrize("col64", [False, True])
def test_spmv_binned(dev, gpu_ops, col64):
    case = _sell(37)[0]
    for rowbase, accum, dacc in ((0, False, False), (5, True, True)):
        got = ko.run_csr_spmv(gpu_ops, case, dev, rowbase=rowbase, accum=accum,
                              dot_accum=dacc, col64=col64, binned=True)
        ko.assert_accepts(
            ko.csr_spmv_expect(case, rowbase, accum, dacc, kernel="spmv_binned"),
            got, f"col64={col64} rowbase{rowbase}")
        ko.check_partials(got, halves=1)


@pytest.mark.parametrize("n", [1, 257, 300_001])
def test_vector_ops(dev, gpu_ops, n):
    case = _vec(n)
    for op in ("axpy_ratio", "daypx_ratio"):
        for n_act in sorted({n, max(n - 3, 0)}):
            ko.assert_accepts(ko.ratio_update_expect(case, op, n_act),
                              ko.run_ratio_update(gpu_ops, case, dev, op, n_act),
                              f"{op} n{n} act{n_act}")
    fc = ko.fused_case(n)
    for first in (True, False):
        for nt in (True, False):
            got = ko.run_fused(gpu_ops, fc, dev, first, nt_update=nt)
            ko.assert_accepts(ko.fused_expect(fc, first), got,
                              f"n{n} first{first} nt{nt}")
            ko.check_partials(got, halves=2)


@pytest.mark.parametrize("idx64", [False, True])
def test_data_movement_ops(dev, gpu_ops, idx64):
    e, got = ko.run_exact_ops(gpu_ops, dev, idx64)
    ko.assert_accepts(e, got, f"idx64={idx64}")


@pytest.mark.parametrize("n", [1, 255, 257, 1025, 300_001])
def test_cg_fused_update(dev, gpu_ops, n):
    case = _vec(n)
    got = ko.run_cg_update(gpu_ops, case, dev)
    ko.assert_accepts(ko.cg_update_expect(case), got, f"n{n}")
    ko.check_partials(got, halves=1)
