"""Shared inputs of the mixed-precision solver tests (plain helper module,
not a conftest): the two symmetrically scaled systems, their right-hand
sides and an independent fp64 residual.

Scaling ``s_i * a_ij * s_j`` with ``s in [0.5, 2)`` from ``default_rng(0)``
leaves no matrix value fp32-representable, so a solve that only ever sees
the fp32-rounded operator stalls near ``kappa * 2^-24`` while the refined
solve reaches the fp64 tolerance."""

from __future__ import annotations

import numpy as np

from acg_amd.gen import STENCIL_5PT_2D, queen_like_spec, stencil_global
from acg_amd.part import extract_subdomains, partition_rows

RES_RTOL = 1e-11
# pinned: the solvers' default is tuned by measurement and may move
INNER_RTOL = 1e-4
MAXITS = 2000
MIXED_KW = dict(maxits=MAXITS, res_rtol=RES_RTOL, inner_rtol=INNER_RTOL)


def scaled(A):
    """Scale the packed SymCSRMatrix values in place; returns A."""
    s = np.random.default_rng(0).uniform(0.5, 2.0, size=A.n)
    rows = np.repeat(np.arange(A.n, dtype=np.int64), np.diff(A.rowptr))
    A.vals *= s[rows] * s[A.colidx]
    assert not np.array_equal(A.vals.astype(np.float32).astype(np.float64),
                              A.vals)
    return A


def poisson32():
    return scaled(stencil_global(32, 32, 1, dict(STENCIL_5PT_2D)))


def queen6():
    return scaled(stencil_global(6, 6, 6, queen_like_spec(3)))


SYSTEMS = {"poisson32": poisson32, "queen6": queen6}


def rhs(A):
    return np.random.default_rng(1).standard_normal(A.n)


def local(A, nparts=1, rank=0):
    part = partition_rows(A, nparts, method="block")
    return extract_subdomains(A, part, nparts)[rank]


_SOLVES = {}


def cpu_solves(name):
    """Serial CGSolverCPU fp64 solve and mixed solve of one system, computed
    once and shared (the GPU tests use them as their oracle)."""
    if name not in _SOLVES:
        import torch

        from acg_amd.solvers.cpu import CGSolverCPU

        A = SYSTEMS[name]()
        b = rhs(A)
        S = local(A)
        assert np.array_equal(S.owned_global, np.arange(A.n))
        solver = CGSolverCPU(S)
        bt = torch.from_numpy(b)
        out = {"A": A, "b": b, "S": S, "solver": solver, "bt": bt,
               "tol": RES_RTOL * float(np.linalg.norm(b))}
        x = torch.zeros(S.nowned + S.nghost, dtype=torch.float64)
        out["plain"] = solver.solve(bt, x, maxits=MAXITS, res_rtol=RES_RTOL)
        x = torch.zeros(S.nowned + S.nghost, dtype=torch.float64)
        out["mixed"] = solver.solve_mixed(bt, x, **MIXED_KW)
        out["x"] = x[:S.nowned].numpy().copy()
        _SOLVES[name] = out
    return _SOLVES[name]


def true_residual(A, b, x):
    """||b - A x|| recomputed in fp64 from the global matrix (scipy), i.e.
    by code the solvers do not share."""
    return float(np.linalg.norm(b - A.to_scipy_full() @ x))
