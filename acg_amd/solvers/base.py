"""Solver result / statistics structures.

Reference: struct acgsolverhip counters (cghip.h:109-118) and the
statistics block printed by acgsolverhip_fwritempi (cghip.c:2003-2270):
iterations, b/r0/r 2-norms, per-op seconds/flops/bytes, halo traffic.
"""

from __future__ import annotations

import math
from dataclasses import dataclass, field


@dataclass
class OpStats:
    seconds: float = 0.0
    count: int = 0
    flops: float = 0.0
    bytes: float = 0.0

    @property
    def gflops_rate(self) -> float:
        return self.flops / self.seconds / 1e9 if self.seconds > 0 else 0.0

    @property
    def gbytes_rate(self) -> float:
        return self.bytes / self.seconds / 1e9 if self.seconds > 0 else 0.0


@dataclass
class SolveResult:
    converged: bool = False
    niterations: int = 0
    bnrm2: float = 0.0
    r0nrm2: float = 0.0
    rnrm2: float = 0.0
    tsolve: float = 0.0
    maxits: int = 0
    res_atol: float = 0.0
    res_rtol: float = 0.0
    solver: str = ""
    nflops: float = 0.0
    nbytes: float = 0.0
    ops: dict = field(default_factory=dict)  # name -> OpStats
    halo_bytes_sent: int = 0
    halo_msgs_sent: int = 0
    nranks: int = 1
    nouter: int = 0  # mixed-precision refinement sweeps (0 = not refined)
    # solve_block: block iteration at which the block broke down and the
    # columns were handed to solve_multi (0 = at initialisation, -1 = never)
    block_breakdown: int = -1
    # pipelined CG: residual replacements performed (rr_period > 0)
    nreplacements: int = 0

    @property
    def iters_per_s(self) -> float:
        return self.niterations / self.tsolve if self.tsolve > 0 else 0.0

    @property
    def gflops(self) -> float:
        return self.nflops / self.tsolve / 1e9 if self.tsolve > 0 else 0.0

    def summary(self) -> str:
        lines = [
            f"solver: {self.solver}",
            f"ranks: {self.nranks}",
            f"iterations: {self.niterations} (max {self.maxits})",
            f"converged: {self.converged}",
            f"b 2-norm: {self.bnrm2:.6e}",
            f"initial residual 2-norm: {self.r0nrm2:.6e}",
            f"final residual 2-norm: {self.rnrm2:.6e}",
            f"solve time: {self.tsolve:.6f} s"
            f" ({self.iters_per_s:.2f} it/s, {self.gflops:.1f} Gflop/s)",
        ]
        if self.nouter:
            lines.insert(3, f"outer refinement sweeps: {self.nouter} "
                            f"({self.niterations} inner iterations)")
        if self.nreplacements:
            lines.insert(3, f"residual replacements: {self.nreplacements}")
        if self.halo_bytes_sent:
            per_it = self.halo_bytes_sent / max(self.niterations, 1)
            lines.append(
                f"halo: {self.halo_bytes_sent} B sent total, {per_it:.0f} B/it, "
                f"{self.halo_msgs_sent / max(self.niterations, 1):.1f} msg/it")
        for name, op in self.ops.items():
            if op.count:
                lines.append(
                    f"  {name}: {op.seconds:.4f} s / {op.count} calls"
                    f" ({op.gbytes_rate:.1f} GB/s, {op.gflops_rate:.1f} Gflop/s)")
        return "\n".join(lines)


def refine(res: SolveResult, tol: float, maxits: int, inner_rtol: float,
           max_outer: int, residual_norm, inner_solve) -> int:
    """Outer loop of mixed-precision iterative refinement, shared by the
    CPU and GPU solvers so both take the same decisions.

    ``residual_norm()`` returns the all-reduced true ``||b - A x||`` of the
    current x with the fp64 operator; ``inner_solve(target, budget)`` solves
    ``A_lo d = r`` from d = 0 to the absolute residual ``target`` in at most
    ``budget`` iterations, applies ``x += d`` and returns the iterations it
    used.  Every decision uses all-reduced scalars only, so all ranks take
    the same branch.  Fills niterations / nouter / r0nrm2 / rnrm2 /
    converged of ``res`` and returns the number of residual evaluations.

    The sweep target ``max(inner_rtol*||r||, 0.5*tol)`` keeps the last sweep
    from over-solving; a residual that does not halve between sweeps means
    the low-precision operator is too far from A (kappa * 2^-24 not small)
    and the loop stops unconverged instead of spinning."""
    nrm = residual_norm()
    nres = 1
    res.r0nrm2 = nrm
    prev = None
    while True:
        if not math.isfinite(nrm):
            raise FloatingPointError(f"refinement diverged: ||r||={nrm}")
        if nrm <= tol:
            res.converged = True
            break
        if res.nouter >= max_outer or res.niterations >= maxits:
            break
        if prev is not None and nrm > 0.5 * prev:
            break  # stagnated
        target = max(inner_rtol * nrm, 0.5 * tol)
        res.niterations += inner_solve(target, maxits - res.niterations)
        res.nouter += 1
        prev = nrm
        nrm = residual_norm()
        nres += 1
    res.rnrm2 = nrm
    return nres


def check_multi_shapes(B, X, nowned: int, nlocal: int) -> int:
    """Shape contract of ``solve_multi``: B (nowned, k), X (nlocal, k), fp64.
    Returns k."""
    import torch

    if B.dim() != 2 or X.dim() != 2 or B.shape[1] < 1:
        raise ValueError("solve_multi: B must have shape (nowned, k) and X "
                         f"(nlocal, k); got {tuple(B.shape)} and {tuple(X.shape)}")
    k = B.shape[1]
    if B.shape[0] != nowned or tuple(X.shape) != (nlocal, k):
        raise ValueError(f"solve_multi: expected B ({nowned}, k) and X "
                         f"({nlocal}, k); got {tuple(B.shape)} and {tuple(X.shape)}")
    if B.dtype != torch.float64 or X.dtype != torch.float64:
        raise TypeError("solve_multi: B and X must be float64")
    return k


def solve_multi_by_column(solve, B, X, maxits, res_atol, res_rtol) -> list:
    """Multiple right-hand sides as k independent ``solve`` calls on
    contiguous copies of the columns; X is overwritten column by column."""
    out = []
    for c in range(B.shape[1]):
        xc = X[:, c].contiguous()
        out.append(solve(B[:, c].contiguous(), xc, maxits=maxits,
                         res_atol=res_atol, res_rtol=res_rtol))
        X[:, c] = xc
    return out


def next_multi_k(kg: int, widths=(2, 4, 8)) -> int:
    """Smallest kernel width that holds kg columns."""
    return next(kk for kk in widths if kk >= kg)


class ColumnTolerances:
    """Per-column stopping test of one multi-RHS group, the same on the CPU
    and the GPU: column c has met its tolerance when ``rr`` (a residual
    norm SQUARED) is at most ``max(res_atol, res_rtol*bnrm[c])**2``; with a
    zero tolerance only an exactly zero residual counts.  ``conv_it[c]`` is
    the first iteration at which column c met it (None: not yet; 0: the
    initial residual ``rr0[c]`` already did)."""

    def __init__(self, bnrm: list, rr0: list, res_atol: float,
                 res_rtol: float):
        self.rtol2 = [max(res_atol, res_rtol * bn) ** 2 for bn in bnrm]
        self.conv_it: list = [0 if self.met(c, rr) else None
                              for c, rr in enumerate(rr0)]

    def met(self, c: int, rr: float) -> bool:
        return rr <= self.rtol2[c] if self.rtol2[c] > 0 else rr == 0.0

    def record(self, c: int, rr: float, it: int) -> None:
        if self.conv_it[c] is None and self.met(c, rr):
            self.conv_it[c] = it

    def all_met(self) -> bool:
        return all(ci is not None for ci in self.conv_it)


def block_results(solver: str, ncols: int, active: list,
                  tol: ColumnTolerances, nit: int, breakdown: int,
                  finish: list | None, bnrm: list, rr0: list, rr: list,
                  maxits: int, res_atol: float, res_rtol: float,
                  tsolve: float, flops_per_it: float) -> list:
    """SolveResults of one ``solve_block`` group, the same bookkeeping on
    the CPU and the GPU.  ``active`` lists the group columns that formed
    the block (the others had a zero initial residual), ``tol.conv_it[c]``
    the block iteration at which column c first met its tolerance (None:
    not yet), ``nit`` the block iterations run, ``rr[c]`` the last
    recurrence residual norm squared.  After a breakdown at block iteration
    ``breakdown`` >= 0, ``finish[i]`` is the solve_multi result of
    ``active[i]``: its iterations are added to the block's."""
    conv_it, met = tol.conv_it, tol.met
    out = []
    for c in range(ncols):
        res = SolveResult(solver=solver, maxits=maxits, res_atol=res_atol,
                          res_rtol=res_rtol, nranks=1)
        res.bnrm2 = bnrm[c]
        res.r0nrm2 = math.sqrt(max(rr0[c], 0.0))
        res.tsolve = tsolve
        fin = finish[active.index(c)] if finish is not None and c in active else None
        if fin is not None:
            res.block_breakdown = breakdown
            res.converged = fin.converged
            res.rnrm2 = fin.rnrm2
            if conv_it[c] is not None and fin.niterations == 0:
                res.niterations = conv_it[c]
            else:
                res.niterations = breakdown + fin.niterations
        else:
            res.rnrm2 = math.sqrt(max(rr[c], 0.0))
            res.converged = conv_it[c] is not None or met(c, rr[c])
            res.niterations = conv_it[c] if conv_it[c] is not None else nit
        res.nflops = res.niterations * flops_per_it
        out.append(res)
    return out


def cg_flops_per_iter(nnz_full: int, n: int) -> float:
    """Flops per classic-CG iteration: SpMV 2*nnz + 2 dots + 3 axpy-likes."""
    return 2.0 * nnz_full + 10.0 * n


def replacement_flops(nnz_full: int, n: int) -> float:
    """Flops of one residual replacement of the pipelined CG: four SpMVs,
    the subtraction from b and the two dots."""
    return 8.0 * nnz_full + 5.0 * n


def cg_bytes_per_iter(nnz_full: int, n: int, colbytes: int = 4) -> float:
    """Approximate HBM traffic per iteration (fp64 vals + colidx + vectors)."""
    spmv = nnz_full * (8 + colbytes) + 8.0 * n * 3
    vecs = 8.0 * n * 9
    return spmv + vecs
