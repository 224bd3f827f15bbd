"""Block-Jacobi PCG on the GPU: the three HIP kernels against the oracles
of tests/bjacobi_systems.py, the solver against the CPU solver and a direct
solve, a device-generated system, error paths and the CLI."""

from functools import lru_cache

import numpy as np
import pytest
import torch

import bjacobi_systems as bs
import kernel_oracle as ko
from acg_amd.ops import torch_ref
from acg_amd.utils.errors import AcgError, ErrCode

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# (G, dof): 27 nodes = one partial slice; 125 = two slices, 61 live lanes
# in the last; 1728 = 27 full slices and 4 blocks of the update kernels.
# Stencil boundary nodes have 8-18 blocks against 27 inside, so padding
# blocks occur in every slice.
KERNEL_CASES = [(G, dof) for G in (3, 5, 12) for dof in (2, 3, 4)]
SOLVE_CASES = [(5, 2), (5, 3), (5, 4), (7, 3)]  # n = 250, 375, 500, 1029


def _ops():
    from acg_amd.ops import gpu_ops

    return gpu_ops


def _dev_bsell(S, dof):
    return tuple(torch.from_numpy(a).to(DEV) for a in bs.bsell_arrays(S, dof))


@lru_cache(maxsize=None)
def _dev_minv(G, dof):
    s = bs.rotated_system(G, dof)
    return _ops().bsell_diag_inv(*_dev_bsell(s.S, dof), s.nnodes, dof)


@lru_cache(maxsize=None)
def _solver(G, dof):
    from acg_amd.solvers.hip import CGSolverHIP

    return CGSolverHIP(bs.rotated_system(G, dof).S, device=DEV)


def _solve(G, dof, method="solve_bjacobi", maxits=5000, rtol=bs.RTOL):
    s = bs.rotated_system(G, dof)
    gpu = _solver(G, dof)
    b = torch.from_numpy(s.b).to(DEV)
    x = torch.zeros(s.n, dtype=torch.float64, device=DEV)
    res = getattr(gpu, method)(b, x, maxits=maxits, res_rtol=rtol)
    return res, x


# ---- bsell_diag_inv ----

@pytest.mark.parametrize("G,dof", KERNEL_CASES)
def test_diag_inv(G, dof):
    s = bs.rotated_system(G, dof)
    minv, nbad = _dev_minv(G, dof)
    assert nbad == 0
    assert minv.numel() == torch_ref.block_inv_len(s.nnodes, dof)
    inv = torch_ref.unpack_block_inv(minv, s.nnodes, dof).cpu().numpy()
    ratio = bs.diag_inv_ratio(s.blocks, inv)
    print(f"DIAG_INV G={G} dof={dof} worst error/bound = {ratio:.3g}")
    assert ratio <= 1.0
    # lanes past nnodes in the last slice stay untouched (zero)
    comp = minv.view(-1, dof * (dof + 1) // 2, 64)
    live = s.nnodes - 64 * (comp.shape[0] - 1)
    assert not comp[-1, :, live:].any()
    # a second run is bitwise equal
    again, nbad2 = _ops().bsell_diag_inv(*_dev_bsell(s.S, dof), s.nnodes, dof)
    assert nbad2 == 0 and torch.equal(again, minv)


def test_diag_inv_device_generated_slab():
    from acg_amd.gen.device_slab import device_stencil_slab
    from acg_amd.gen.stencil import queen_like_spec

    spec = queen_like_spec(3)
    L = device_stencil_slab(9, 9, 9, spec, 0, 1, DEV)
    bptr, bcol, bvals, dof = L.A_bsell
    assert dof == 3
    minv, nbad = _ops().bsell_diag_inv(bptr, bcol, bvals, 729, 3)
    assert nbad == 0
    inv = torch_ref.unpack_block_inv(minv, 729, 3).cpu().numpy()
    D = np.broadcast_to(np.asarray(spec["diagblock"]), (729, 3, 3))
    assert bs.diag_inv_ratio(D, inv) <= 1.0
    assert (inv == inv[0]).all()  # one block, one inverse


@pytest.mark.parametrize("kind", ["indefinite", "zeroed", "missing"])
def test_diag_inv_counts_bad_nodes(kind):
    nodes = (0, 31, 93, 124)  # boundary and interior nodes of both slices
    _, S = bs.modified_system(5, 3, kind, nodes)
    minv, nbad = _ops().bsell_diag_inv(*_dev_bsell(S, 3), 125, 3)
    assert nbad == len(nodes)
    inv = torch_ref.unpack_block_inv(minv, 125, 3).cpu().numpy()
    assert not inv[list(nodes)].any()
    good = np.setdiff1d(np.arange(125), nodes)
    assert bs.diag_inv_ratio(bs.rotated_system(5, 3).blocks[good],
                             inv[good]) <= 1.0


def test_wrappers_validate():
    ops = _ops()
    minv, _ = _dev_minv(5, 3)
    n = 375
    v = torch.zeros(n, dtype=torch.float64, device=DEV)
    scal, partials = ops.alloc_scalars(DEV), ops.alloc_partials(DEV)
    with pytest.raises(ValueError):  # n != nnodes * dof
        ops.bjacobi_apply(minv, v, v.clone(), partials, scal, n - 1, 3)
    with pytest.raises(ValueError):  # inverse buffer of another dof
        ops.bjacobi_apply(minv, v, v.clone(), partials, scal, 250, 2)
    with pytest.raises(TypeError):
        ops.bpcg_fused_update(v.float(), v, v, v, v, minv, scal, partials, n, 3)
    with pytest.raises(ValueError):  # short vector
        ops.bpcg_fused_update(v[:-1], v, v, v, v, minv, scal, partials, n, 3)
    with pytest.raises(ValueError):  # not contiguous
        ops.bpcg_fused_update(v, v, torch.zeros(2 * n, dtype=torch.float64,
                                                device=DEV)[::2],
                              v, v, minv, scal, partials, n, 3)
    with pytest.raises(ValueError):  # host tensor
        ops.bjacobi_apply(minv, v.cpu(), v.clone(), partials, scal, n, 3)
    s = bs.rotated_system(5, 3)
    bptr, bcol, bvals = _dev_bsell(s.S, 3)
    with pytest.raises(TypeError):  # never the fp32 copy
        ops.bsell_diag_inv(bptr, bcol, bvals.float(), 125, 3)
    with pytest.raises(ValueError):
        ops.bsell_diag_inv(bptr, bcol, bvals, 125, 5)
    with pytest.raises(ValueError):  # slices do not hold that many nodes
        ops.bsell_diag_inv(bptr, bcol, bvals, 129, 3)


# ---- bjacobi_apply / bpcg_fused_update ----

@pytest.mark.parametrize("G,dof", KERNEL_CASES)
def test_bjacobi_apply_oracle(G, dof):
    s = bs.rotated_system(G, dof)
    minv, _ = _dev_minv(G, dof)
    Mi = torch_ref.unpack_block_inv(minv, s.nnodes, dof).cpu().numpy()
    case = bs.bj_case(s.nnodes, dof)
    got = bs.run_bj_apply(_ops(), case, minv, DEV)
    assert (got["nblocks"] > 1) == (G == 12)
    ko.assert_accepts(bs.bj_apply_expect(case, Mi), got, f"G{G} dof{dof}")
    ko.check_partials(got, halves=2)
    again = bs.run_bj_apply(_ops(), case, minv, DEV)
    for k in got:
        assert ko._bits_equal(got[k], again[k]), k


@pytest.mark.parametrize("pt_zero", [False, True])
@pytest.mark.parametrize("G,dof", KERNEL_CASES)
def test_bpcg_fused_update_oracle(G, dof, pt_zero):
    s = bs.rotated_system(G, dof)
    minv, _ = _dev_minv(G, dof)
    Mi = torch_ref.unpack_block_inv(minv, s.nnodes, dof).cpu().numpy()
    case = bs.bj_case(s.nnodes, dof, pt_zero)
    got = bs.run_bj_update(_ops(), case, minv, DEV)
    assert (got["nblocks"] > 1) == (G == 12)
    ko.assert_accepts(bs.bj_update_expect(case, Mi), got,
                      f"G{G} dof{dof} pt0={pt_zero}")
    ko.check_partials(got, halves=2)
    again = bs.run_bj_update(_ops(), case, minv, DEV)
    for k in got:
        assert ko._bits_equal(got[k], again[k]), k


# ---- solve_bjacobi ----

@pytest.mark.parametrize("G,dof", SOLVE_CASES)
def test_solve_bjacobi_matches_cpu_and_direct(G, dof):
    from acg_amd.solvers.cpu import CGSolverCPU

    s = bs.rotated_system(G, dof)
    rg, xg = _solve(G, dof)
    assert rg.converged and rg.solver == "cg-hip-bjacobi"
    assert _solver(G, dof).bsell[3] == dof
    xc = torch.zeros(s.n, dtype=torch.float64)
    rc = CGSolverCPU(s.S).solve_bjacobi(torch.from_numpy(s.b), xc,
                                        maxits=5000, res_rtol=bs.RTOL)
    rj, _ = _solve(G, dof, "solve_jacobi")
    print(f"BJ_GPU G={G} dof={dof} its={rg.niterations} cpu={rc.niterations} "
          f"point-jacobi={rj.niterations}")
    assert abs(rg.niterations - rc.niterations) <= 2
    np.testing.assert_allclose(xg.cpu().numpy(), bs.direct_solution(G, dof),
                               rtol=1e-6, atol=1e-8)
    assert rj.converged
    assert rg.niterations * 10 < rj.niterations


@pytest.mark.parametrize("maxits", [1, 2, 3])
def test_solve_bjacobi_tiny_maxits(maxits):
    res, x = _solve(5, 3, maxits=maxits, rtol=0.0)
    assert res.niterations == maxits
    assert np.isfinite(res.rnrm2) and res.rnrm2 > 0.0
    assert not res.converged
    assert torch.isfinite(x).all()


def test_solve_bjacobi_repeat_is_bitwise_identical():
    r1, x1 = _solve(5, 3)
    r2, x2 = _solve(5, 3)
    assert r1.niterations == r2.niterations and r1.rnrm2 == r2.rnrm2
    assert torch.equal(x1, x2)


def test_solve_bjacobi_device_generated_system():
    from acg_amd.gen.device_slab import device_stencil_slab
    from acg_amd.gen.stencil import queen_like_spec
    from acg_amd.solvers.hip import CGSolverHIP

    ops = _ops()
    L = device_stencil_slab(14, 14, 14, queen_like_spec(3), 0, 1, DEV)
    gpu = CGSolverHIP(L, device=DEV)
    n = L.nowned
    b = torch.from_numpy(np.random.default_rng(5).standard_normal(n)).to(DEV)
    x = torch.zeros(L.nowned + L.nghost, dtype=torch.float64, device=DEV)
    with pytest.raises(AcgError) as ei:
        gpu.solve_jacobi(b, x.clone(), maxits=5)
    assert ei.value.code == ErrCode.NOT_SUPPORTED
    res = gpu.solve_bjacobi(b, x, maxits=500, res_rtol=1e-9)
    assert res.converged
    bptr, bcol, bvals, dof = L.A_bsell
    y = torch.zeros(n, dtype=torch.float64, device=DEV)
    ops.spmv_bsell(bptr, bcol, bvals, n // dof, dof, x, y)
    rtrue = float(torch.linalg.vector_norm(b - y))
    print(f"BJ_GPU device slab its={res.niterations} "
          f"true={rtrue / res.bnrm2:.3e}")
    assert rtrue <= 1.05e-9 * float(torch.linalg.vector_norm(b))


def test_solve_bjacobi_error_paths():
    from acg_amd.solvers.hip import CGSolverHIP

    s = bs.rotated_system(5, 3)
    b = torch.from_numpy(s.b).to(DEV)
    x = torch.zeros(s.n, dtype=torch.float64, device=DEV)
    with pytest.raises(AcgError, match="Block-SELL") as ei:
        CGSolverHIP(s.S, device=DEV, force_format="sell").solve_bjacobi(
            b, x, maxits=5)
    assert ei.value.code == ErrCode.NOT_SUPPORTED
    _, S = bs.modified_system(5, 3, "indefinite", (17,))
    with pytest.raises(AcgError) as ei:
        CGSolverHIP(S, device=DEV).solve_bjacobi(b, x, maxits=5)
    assert ei.value.code == ErrCode.INVALID_VALUE


def test_cli_gpu_bjacobi(tmp_path, monkeypatch, capsys):
    from acg_amd import cli

    p = tmp_path / "A.mtx"
    bs.write_mtx_file(p, bs.rotated_system(5, 3).A)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("RANK", raising=False)
    rc = cli.main([str(p), "--solver", "acg-bjacobi",
                   "--manufactured-solution", "--max-iterations", "200",
                   "--residual-rtol", "1e-9", "-q"])
    out = capsys.readouterr()
    assert rc == 0, out.err
    assert "manufactured solution" in out.err
