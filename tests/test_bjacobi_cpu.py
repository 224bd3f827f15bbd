"""Block-Jacobi PCG, host side: the inverse helper, the CPU solver on the
rotated-anisotropy systems (tests/bjacobi_systems.py), the torch_ref forms
of the three HIP kernels against the long-double oracle, error paths and
the CLI."""

import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import bjacobi_systems as bs
import kernel_oracle as ko
from acg_amd.ops import torch_ref
from acg_amd.solvers.cpu import CGSolverCPU
from acg_amd.solvers.precond import block_jacobi_inverse, detect_block_dof
from acg_amd.utils.errors import AcgError, ErrCode

REPO = Path(__file__).resolve().parent.parent
SOLVE_CASES = [(5, 2), (5, 3), (5, 4)]  # n = 250, 375, 500
# (G, dof): 27 nodes = one partial slice; 125 = two slices, 61 live lanes
# in the last; 1728 = 27 full slices and 4 blocks of the update kernels
KERNEL_CASES = [(G, dof) for G in (3, 5, 12) for dof in (2, 3, 4)]


@pytest.mark.parametrize("G,dof", SOLVE_CASES)
def test_block_jacobi_inverse_matches_numpy(G, dof):
    s = bs.rotated_system(G, dof)
    inv = block_jacobi_inverse(s.S, dof)
    assert inv.shape == (s.nnodes, dof, dof)
    np.testing.assert_allclose(inv, np.linalg.inv(s.blocks), rtol=1e-12,
                               atol=0.0)
    assert bs.diag_inv_ratio(s.blocks, inv) <= 1.0


@pytest.mark.parametrize("G,dof", SOLVE_CASES)
def test_detect_block_dof(G, dof):
    assert detect_block_dof(bs.rotated_system(G, dof).S) == dof


@pytest.mark.parametrize("G,dof", SOLVE_CASES)
def test_cpu_bjacobi_solves_and_beats_point_jacobi(G, dof):
    s = bs.rotated_system(G, dof)
    solver = CGSolverCPU(s.S)
    b = torch.from_numpy(s.b)
    x = torch.zeros(s.n, dtype=torch.float64)
    rb = solver.solve_bjacobi(b, x, maxits=2000, res_rtol=bs.RTOL)
    assert rb.converged and rb.solver == "cg-bjacobi-cpu"
    np.testing.assert_allclose(x.numpy(), bs.direct_solution(G, dof),
                               rtol=1e-6, atol=1e-8)
    rtrue = np.linalg.norm(s.b - s.Af @ x.numpy())
    print(f"BJ_CPU G={G} dof={dof} its={rb.niterations} "
          f"true={rtrue / rb.bnrm2:.3e}")
    assert rtrue <= 1.05 * bs.RTOL * rb.bnrm2
    # explicit dof = detected dof: same iteration
    x2 = torch.zeros(s.n, dtype=torch.float64)
    r2 = solver.solve_bjacobi(b, x2, maxits=2000, res_rtol=bs.RTOL, dof=dof)
    assert r2.niterations == rb.niterations and torch.equal(x, x2)
    xj = torch.zeros(s.n, dtype=torch.float64)
    rj = solver.solve_jacobi(b, xj, maxits=5000, res_rtol=bs.RTOL)
    print(f"BJ_CPU point jacobi its={rj.niterations}")
    assert rj.converged
    assert rb.niterations * 10 < rj.niterations, \
        (rb.niterations, rj.niterations)


# ---- torch_ref forms of the three kernels vs the long-double oracle ----

def _ref_minv(G, dof):
    s = bs.rotated_system(G, dof)
    bptr, bcol, bvals = (torch.from_numpy(a) for a in bs.bsell_arrays(s.S, dof))
    return s, torch_ref.bsell_diag_inv(bptr, bcol, bvals, s.nnodes, dof)


@pytest.mark.parametrize("G,dof", KERNEL_CASES)
def test_torch_ref_diag_inv(G, dof):
    s, (minv, nbad) = _ref_minv(G, dof)
    assert nbad == 0
    assert minv.numel() == torch_ref.block_inv_len(s.nnodes, dof)
    inv = torch_ref.unpack_block_inv(minv, s.nnodes, dof).numpy()
    assert bs.diag_inv_ratio(s.blocks, inv) <= 1.0
    # the pack is the inverse of the unpack; dead lanes hold zeros
    assert torch.equal(torch_ref.pack_block_inv(torch.from_numpy(inv)), minv)


@pytest.mark.parametrize("kind", ["indefinite", "zeroed", "missing"])
def test_torch_ref_diag_inv_counts_bad_nodes(kind):
    nodes = (0, 31, 93, 124)  # boundary and interior nodes of both slices
    _, S = bs.modified_system(5, 3, kind, nodes)
    bptr, bcol, bvals = (torch.from_numpy(a) for a in bs.bsell_arrays(S, 3))
    minv, nbad = torch_ref.bsell_diag_inv(bptr, bcol, bvals, 125, 3)
    assert nbad == len(nodes)
    inv = torch_ref.unpack_block_inv(minv, 125, 3).numpy()
    assert not inv[list(nodes)].any()
    good = np.setdiff1d(np.arange(125), nodes)
    assert bs.diag_inv_ratio(bs.rotated_system(5, 3).blocks[good],
                             inv[good]) <= 1.0


@pytest.mark.parametrize("pt_zero", [False, True])
@pytest.mark.parametrize("G,dof", KERNEL_CASES)
def test_torch_ref_apply_and_update_vs_oracle(G, dof, pt_zero):
    s, (minv, _) = _ref_minv(G, dof)
    Mi = torch_ref.unpack_block_inv(minv, s.nnodes, dof).numpy()
    case = bs.bj_case(s.nnodes, dof, pt_zero)
    if not pt_zero:
        got = bs.run_bj_apply(torch_ref, case, minv, "cpu")
        ko.assert_accepts(bs.bj_apply_expect(case, Mi), got, f"G{G} dof{dof}")
    got = bs.run_bj_update(torch_ref, case, minv, "cpu")
    ko.assert_accepts(bs.bj_update_expect(case, Mi), got,
                      f"G{G} dof{dof} pt0={pt_zero}")


def test_oracle_rejects_a_wrong_block_product():
    """The z bound discriminates: two swapped components, one dropped term
    and one element off by 1e-12 relative all fail."""
    s, (minv, _) = _ref_minv(5, 3)
    Mi = torch_ref.unpack_block_inv(minv, s.nnodes, 3).numpy()
    case = bs.bj_case(s.nnodes, 3)
    expect = bs.bj_update_expect(case, Mi)
    good = bs.run_bj_update(torch_ref, case, minv, "cpu")
    assert ko.accepts(expect, good)
    for mutate in ("swap", "drop", "scale"):
        bad = dict(good)
        z = good["z"].copy().reshape(-1, 3)
        if mutate == "swap":
            z[:, [0, 1]] = z[:, [1, 0]]
        elif mutate == "drop":
            z[7, 2] -= Mi[7, 2, 1] * good["r"][7 * 3 + 1]
        else:
            z[100, 0] *= 1.0 + 1e-12
        bad["z"] = z.reshape(-1)
        assert not ko.accepts(expect, bad), mutate


# ---- error paths ----

def test_block_jacobi_error_paths():
    s = bs.rotated_system(5, 3)
    with pytest.raises(AcgError) as ei:
        block_jacobi_inverse(s.S, 2)  # 375 % 2 != 0
    assert ei.value.code == ErrCode.INVALID_VALUE
    for kind in ("indefinite", "zeroed", "missing"):
        _, S = bs.modified_system(5, 3, kind, (17,))
        with pytest.raises(AcgError) as ei:
            block_jacobi_inverse(S, 3)
        assert ei.value.code == ErrCode.INVALID_VALUE
        with pytest.raises(AcgError) as ei:
            CGSolverCPU(S).solve_bjacobi(torch.from_numpy(s.b),
                                         torch.zeros(s.n, dtype=torch.float64),
                                         maxits=5, dof=3)
        assert ei.value.code == ErrCode.INVALID_VALUE


def _powerlaw():
    from acg_amd.gen.irregular import powerlaw_spd

    return powerlaw_spd(600, mean_nnz=10, seed=1)


def test_no_block_structure_is_not_supported():
    A = _powerlaw()
    S = bs._local(A)
    assert detect_block_dof(S) is None
    with pytest.raises(AcgError, match="Block-SELL") as ei:
        CGSolverCPU(S).solve_bjacobi(torch.ones(A.n, dtype=torch.float64),
                                     torch.zeros(A.n, dtype=torch.float64),
                                     maxits=5)
    assert ei.value.code == ErrCode.NOT_SUPPORTED


# ---- CLI ----

def test_cli_cpu_bjacobi(tmp_path, monkeypatch, capsys):
    from acg_amd import cli

    p = tmp_path / "A.mtx"
    bs.write_mtx_file(p, bs.rotated_system(5, 3).A)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("RANK", raising=False)
    rc = cli.main([str(p), "--solver", "cpu-bjacobi",
                   "--manufactured-solution", "--max-iterations", "200",
                   "--residual-rtol", "1e-9", "-q"])
    out = capsys.readouterr()
    assert rc == 0, out.err
    assert "manufactured solution" in out.err


def test_cli_cpu_bjacobi_without_block_structure(tmp_path):
    """The process exits non-zero and says why on stderr."""
    p = tmp_path / "P.mtx"
    bs.write_mtx_file(p, _powerlaw())
    r = subprocess.run([sys.executable, "-m", "acg_amd", str(p), "--solver",
                        "cpu-bjacobi", "--max-iterations", "5", "-q"],
                       cwd=REPO, capture_output=True, text=True)
    assert r.returncode != 0
    assert "block Jacobi needs a Block-SELL operator" in r.stderr
    assert "NOT_SUPPORTED" in r.stderr
