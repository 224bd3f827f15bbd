"""Host (CPU) CG solvers — the reference oracle path.

Reference: acg/cg.c — acgsolver_solve / acgsolver_solvempi: textbook CG
with a halo exchange before each SpMV and an all-reduce per dot
(cg.c:408-649).  Unlike the GPU solvers it also supports the
diff_atol/diff_rtol stopping criteria.  solve_pipelined mirrors the
Ghysels–Vanroose recurrences used by the GPU pipelined solver so the
algorithm is testable without a GPU.

Runs on torch CPU tensors (gloo for multi-rank tests); the same code
drives the ops in acg_amd.ops.torch_ref that the HIP kernels are tested
against.
"""

from __future__ import annotations

import math
import time

import numpy as np
import torch

from ..dist.halo import HaloExchange
from ..ops import torch_ref as ops
from ..part.subdomain import LocalSystem
from .base import (ColumnTolerances, SolveResult, block_results,
                   cg_flops_per_iter, check_multi_shapes, next_multi_k,
                   refine, replacement_flops, solve_multi_by_column)


class CGSolverCPU:
    """Distributed classic / pipelined CG on host tensors."""

    def __init__(self, local: LocalSystem, comm=None, device="cpu"):
        self.local = local
        self.comm = comm
        self.device = torch.device(device)
        L = local
        self.A_rowptr = torch.from_numpy(np.ascontiguousarray(L.A_rowptr)).to(self.device)
        self.A_colidx = torch.from_numpy(np.ascontiguousarray(L.A_colidx)).to(self.device)
        self.A_vals = torch.from_numpy(np.ascontiguousarray(L.A_vals)).to(self.device)
        self.O_rowptr = torch.from_numpy(np.ascontiguousarray(L.O_rowptr)).to(self.device)
        self.O_colidx = torch.from_numpy(np.ascontiguousarray(L.O_colidx)).to(self.device)
        self.O_vals = torch.from_numpy(np.ascontiguousarray(L.O_vals)).to(self.device)
        self.halo = HaloExchange(L.halo, L.nowned, self.device, comm)
        self.n = L.nowned
        self.nlocal = L.nowned + L.nghost
        self._A_vals32 = None  # fp32 copy of the matA values (solve_mixed)
        self.multi_group = 8  # solve_block: columns per block, 2, 4 or 8

    # -- helpers ----------------------------------------------------------

    def _allreduce(self, t: torch.Tensor) -> torch.Tensor:
        if self.comm is not None:
            self.comm.allreduce_(t)
        return t

    def _dot(self, a: torch.Tensor, b: torch.Tensor) -> float:
        v = torch.dot(a[: self.n], b[: self.n]).reshape(1)
        return float(self._allreduce(v)[0])

    def _spmv(self, xfull: torch.Tensor, y: torch.Tensor,
              lowprec: bool = False) -> None:
        """y = A_local x (halo exchange + split matA/matO SpMV).
        ``lowprec``: matA values rounded to fp32 storage (widened back
        exactly, fp64 arithmetic); matO stays fp64 as on the GPU."""
        self.halo.exchange(xfull)
        avals = self.A_vals
        if lowprec:
            if self._A_vals32 is None:
                self._A_vals32 = self.A_vals.to(torch.float32)
            avals = self._A_vals32.to(torch.float64)
        ops.spmv(self.A_rowptr, self.A_colidx, avals, xfull, y)
        ops.spmv(self.O_rowptr, self.O_colidx, self.O_vals, xfull, y,
                 rowbase=self.local.ninterior, accum=True)

    def _vec(self, nghost: bool = False) -> torch.Tensor:
        return torch.zeros(self.nlocal if nghost else self.n,
                           dtype=torch.float64, device=self.device)

    # -- classic CG (reference acgsolver_solvempi, cg.c:408-649) ----------

    def solve(self, b: torch.Tensor, x: torch.Tensor, maxits: int = 100,
              res_atol: float = 0.0, res_rtol: float = 1e-9,
              diff_atol: float = 0.0, diff_rtol: float = 0.0) -> SolveResult:
        return self._solve_classic(b, x, maxits, res_atol, res_rtol,
                                   diff_atol, diff_rtol, lowprec=False)

    def _solve_classic(self, b, x, maxits, res_atol, res_rtol,
                       diff_atol=0.0, diff_rtol=0.0, *,
                       lowprec: bool) -> SolveResult:
        res = SolveResult(solver="cg-cpu", maxits=maxits, res_atol=res_atol,
                          res_rtol=res_rtol,
                          nranks=self.comm.size if self.comm else 1)
        n = self.n
        t0 = time.perf_counter()
        bnrm2 = math.sqrt(self._dot(b, b))
        res.bnrm2 = bnrm2
        r = self._vec()
        t = self._vec()
        p = self._vec(nghost=True)
        # r0 = b - A x0
        self._spmv(x, t, lowprec)
        r[:] = b[:n] - t
        p[:n] = r
        rr = self._dot(r, r)
        res.r0nrm2 = math.sqrt(rr)
        rtol2 = max(res_atol, res_rtol * bnrm2) ** 2
        dtol = max(diff_atol, diff_rtol * bnrm2)
        if rr <= rtol2 and (dtol == 0.0):
            res.converged = True
            res.rnrm2 = math.sqrt(rr)
            res.tsolve = time.perf_counter() - t0
            return res
        for k in range(maxits):
            self._spmv(p, t, lowprec)
            pt = self._dot(p, t)
            alpha = rr / pt if pt != 0.0 else 0.0  # 0/0 at underflow: freeze
            r -= alpha * t
            x[:n] += alpha * p[:n]
            rr_new = self._dot(r, r)
            res.niterations = k + 1
            converged = False
            if rtol2 > 0 and rr_new <= rtol2:
                converged = True
            if dtol > 0:
                dx = abs(alpha) * math.sqrt(self._dot(p, p))
                if dx <= dtol:
                    converged = True
            if converged:
                res.converged = True
                res.rnrm2 = math.sqrt(rr_new)
                break
            beta = rr_new / rr if rr != 0.0 else 0.0
            p[:n] = r + beta * p[:n]
            rr = rr_new
            res.rnrm2 = math.sqrt(rr_new)
        res.tsolve = time.perf_counter() - t0
        nnz_full = self.local.nnzA + self.local.nnzO
        res.nflops = res.niterations * cg_flops_per_iter(nnz_full, n)
        res.halo_bytes_sent = self.halo.bytes_sent
        res.halo_msgs_sent = self.halo.nmsgs_sent
        return res

    def solve_multi(self, B: torch.Tensor, X: torch.Tensor, maxits: int = 100,
                    res_atol: float = 0.0, res_rtol: float = 1e-9) -> list:
        """k right-hand sides: ``B`` (nowned, k), ``X`` (nlocal, k), both
        fp64; X is overwritten.  The plain loop over :meth:`solve`, one
        SolveResult per column (the oracle of CGSolverHIP.solve_multi)."""
        check_multi_shapes(B, X, self.n, self.nlocal)
        return solve_multi_by_column(self.solve, B, X, maxits, res_atol,
                                     res_rtol)

    # -- block CG (beyond reference; the oracle of CGSolverHIP.solve_block)

    def solve_block(self, B: torch.Tensor, X: torch.Tensor, maxits: int = 100,
                    res_atol: float = 0.0, res_rtol: float = 1e-9) -> list:
        """Block CG with orthonormalised residuals for k right-hand sides,
        serial: the algorithm, grouping (``self.multi_group``), padding,
        removal of zero-residual columns, pivot threshold and hand-over to
        :meth:`solve_multi` of CGSolverHIP.solve_block, driven through the
        torch_ref ops without the host-test lag.  Several ranks and k = 1
        fall back to :meth:`solve_multi`."""
        k = check_multi_shapes(B, X, self.n, self.nlocal)
        if self.multi_group not in ops.MULTI_K:
            raise ValueError(f"multi_group must be one of {ops.MULTI_K}, "
                             f"got {self.multi_group}")
        serial = self.comm is None or self.comm.size == 1
        if k == 1 or not serial or self.n == 0:
            return self.solve_multi(B, X, maxits, res_atol, res_rtol)
        out = []
        for g0 in range(0, k, self.multi_group):
            kg = min(self.multi_group, k - g0)
            out += self._solve_block_group(B[:, g0:g0 + kg], X[:, g0:g0 + kg],
                                           maxits, res_atol, res_rtol)
        return out

    def _spmm(self, Xm: torch.Tensor, Y: torch.Tensor) -> None:
        for c in range(Xm.shape[1]):
            y = self._vec()
            self._spmv(Xm[:, c].contiguous(), y)
            Y[:, c] = y

    def _solve_block_group(self, B, X, maxits, res_atol, res_rtol) -> list:
        n, kg0 = self.n, B.shape[1]
        t0 = time.perf_counter()
        T0 = torch.zeros(n, kg0, dtype=torch.float64)
        self._spmm(X, T0)
        R0 = B - T0
        bnrm = [math.sqrt(float(torch.dot(B[:, c], B[:, c]))) for c in range(kg0)]
        rr0 = [float(torch.dot(R0[:, c], R0[:, c])) for c in range(kg0)]
        for c in range(kg0):
            if not math.isfinite(rr0[c]):
                raise FloatingPointError(
                    f"block CG: initial rr={rr0[c]} in column {c}")
        tol = ColumnTolerances(bnrm, rr0, res_atol, res_rtol)
        active = [c for c in range(kg0) if rr0[c] != 0.0]
        rr = list(rr0)
        nit, bd, finish = 0, -1, None
        if not tol.all_met():
            kg = len(active)
            K = next_multi_k(kg, ops.MULTI_K)

            def mv(rows):
                return torch.zeros(rows, K, dtype=torch.float64)

            Xi, Q, T, Sm = mv(self.nlocal), mv(n), mv(n), mv(self.nlocal)
            Xi[:, :kg] = X[:, active]
            Q[:, :kg] = R0[:, active]
            partials = ops.alloc_partials_multi("cpu", K)
            state = ops.alloc_block_state("cpu")
            rr_out = torch.zeros(K + 2, dtype=torch.float64)
            nb = ops.gram_multi(Q, Q, partials, n=n)
            ops.block_coef_beta(partials, nb, state, rr_out, K, kg, 0, init=True)
            ops.block_ortho(Q, Sm, state, n)
            if float(rr_out[K]) != 0.0:
                bd = 0
            while bd < 0 and nit < maxits:
                self._spmm(Sm, T)
                nb = ops.gram_multi(Sm, T, partials, n=n)
                ops.block_coef_alpha(partials, nb, state, K, kg, nit + 1)
                nb = ops.block_update(Xi, Sm, Q, T, state, partials, n)
                ops.block_coef_beta(partials, nb, state, rr_out, K, kg, nit + 1)
                ops.block_ortho(Q, Sm, state, n)
                nit += 1
                if float(rr_out[K]) != 0.0:
                    bd = int(rr_out[K + 1])
                    break
                for i, c in enumerate(active):
                    v = float(rr_out[i])
                    if not math.isfinite(v):
                        raise FloatingPointError(
                            f"block CG diverged: rr={v} in column {c} at it {nit}")
                    rr[c] = v
                    tol.record(c, v, nit)
                if tol.all_met():
                    break
            if bd >= 0:
                Xf = Xi[:, :kg].contiguous()
                finish = self.solve_multi(B[:, active].contiguous(), Xf,
                                          max(maxits - bd, 0), res_atol,
                                          res_rtol)
                Xi[:, :kg] = Xf
            for i, c in enumerate(active):
                X[:, c] = Xi[:, i]
        return block_results(
            "cg-block", kg0, active, tol, nit, bd, finish, bnrm, rr0, rr,
            maxits, res_atol, res_rtol, time.perf_counter() - t0,
            cg_flops_per_iter(self.local.nnzA + self.local.nnzO, n))

    # -- mixed precision: fp32-stored operator + fp64 refinement (beyond
    # reference; the oracle of CGSolverHIP.solve_mixed) -------------------

    def solve_mixed(self, b: torch.Tensor, x: torch.Tensor, maxits: int = 100,
                    res_atol: float = 0.0, res_rtol: float = 1e-9,
                    inner_rtol: float = 1e-6,
                    max_outer: int = 20) -> SolveResult:
        """CG on the fp32-rounded matA values wrapped in fp64 iterative
        refinement (see base.refine): r = b - A x with the fp64 operator,
        classic CG on ``A_lo d = r`` from d = 0 down to
        ``max(inner_rtol*||r||, 0.5*tol)``, x += d; at most ``max_outer``
        sweeps and ``maxits`` inner iterations in total.  ``niterations``
        counts inner iterations, ``nouter`` sweeps, ``rnrm2`` is the true
        fp64 residual norm of the returned x."""
        res = SolveResult(solver="cg-cpu-mixed", maxits=maxits,
                          res_atol=res_atol, res_rtol=res_rtol,
                          nranks=self.comm.size if self.comm else 1)
        n = self.n
        t0 = time.perf_counter()
        res.bnrm2 = math.sqrt(self._dot(b, b))
        tol = max(res_atol, res_rtol * res.bnrm2)
        r = self._vec()
        t = self._vec()
        d = self._vec(nghost=True)

        def residual_norm() -> float:
            self._spmv(x, t)
            torch.sub(b[:n], t, out=r)
            return math.sqrt(self._dot(r, r))

        def inner_solve(target: float, budget: int) -> int:
            d.zero_()
            inner = self._solve_classic(r, d, budget, target, 0.0,
                                        lowprec=True)
            x[:n] += d[:n]
            return inner.niterations

        nres = refine(res, tol, maxits, inner_rtol, max_outer,
                      residual_norm, inner_solve)
        res.tsolve = time.perf_counter() - t0
        nnz_full = self.local.nnzA + self.local.nnzO
        # every sweep adds the fp64 residual SpMV and the inner solve's
        # initial SpMV; one more residual closes the loop
        res.nflops = (res.niterations * cg_flops_per_iter(nnz_full, n)
                      + (nres + res.nouter) * (2.0 * nnz_full + 3.0 * n))
        res.halo_bytes_sent = self.halo.bytes_sent
        res.halo_msgs_sent = self.halo.nmsgs_sent
        return res

    # -- Jacobi-preconditioned CG (beyond reference: aCG runs
    # unpreconditioned CG only, PCNONE even in its PETSc oracle,
    # cgpetsc.c:181-193.  Diagonal preconditioning is the standard
    # production lever for time-to-solution on ill-conditioned SPD
    # systems; opt-in so every parity bench stays unpreconditioned) -----

    def _diag_inv(self) -> torch.Tensor:
        d = torch.zeros(self.n, dtype=torch.float64, device=self.device)
        rowptr = self.A_rowptr
        rows = torch.repeat_interleave(
            torch.arange(self.n, dtype=torch.int64, device=self.device),
            rowptr[1:] - rowptr[:-1])
        mask = rows == self.A_colidx.long()
        d[rows[mask]] = self.A_vals[mask]
        if (d == 0).any():
            from ..utils.errors import AcgError, ErrCode

            raise AcgError(ErrCode.INVALID_VALUE,
                           "jacobi preconditioner needs a full diagonal")
        return 1.0 / d

    def solve_jacobi(self, b: torch.Tensor, x: torch.Tensor,
                     maxits: int = 100, res_atol: float = 0.0,
                     res_rtol: float = 1e-9) -> SolveResult:
        """Jacobi-PCG: z = D^-1 r, alpha = (r,z)/(p,t), beta = rz'/rz.
        Convergence is tested on the TRUE residual 2-norm (same semantics
        as the unpreconditioned solvers)."""
        res = SolveResult(solver="cg-jacobi-cpu", maxits=maxits,
                          res_atol=res_atol, res_rtol=res_rtol,
                          nranks=self.comm.size if self.comm else 1)
        n = self.n
        t0 = time.perf_counter()
        dinv = self._diag_inv()
        bnrm2 = math.sqrt(self._dot(b, b))
        res.bnrm2 = bnrm2
        r = self._vec()
        t = self._vec()
        p = self._vec(nghost=True)
        self._spmv(x, t)
        r[:] = b[:n] - t
        z = dinv * r
        p[:n] = z
        rz = self._dot(r, z)
        rr = self._dot(r, r)
        res.r0nrm2 = math.sqrt(rr)
        rtol2 = max(res_atol, res_rtol * bnrm2) ** 2
        if rtol2 > 0 and rr <= rtol2:
            res.converged = True
            res.rnrm2 = math.sqrt(rr)
            res.tsolve = time.perf_counter() - t0
            return res
        for k in range(maxits):
            self._spmv(p, t)
            pt = self._dot(p, t)
            alpha = rz / pt if pt != 0.0 else 0.0
            r -= alpha * t
            x[:n] += alpha * p[:n]
            z = dinv * r
            rz_new = self._dot(r, z)
            rr = self._dot(r, r)
            res.niterations = k + 1
            res.rnrm2 = math.sqrt(max(rr, 0.0))
            if rtol2 > 0 and rr <= rtol2:
                res.converged = True
                break
            beta = rz_new / rz if rz != 0.0 else 0.0
            p[:n] = z + beta * p[:n]
            rz = rz_new
        res.tsolve = time.perf_counter() - t0
        nnz_full = self.local.nnzA + self.local.nnzO
        res.nflops = res.niterations * (cg_flops_per_iter(nnz_full, n) + 3.0 * n)
        res.halo_bytes_sent = self.halo.bytes_sent
        res.halo_msgs_sent = self.halo.nmsgs_sent
        return res

    # -- block-Jacobi PCG (beyond reference; the host oracle of
    # CGSolverHIP.solve_bjacobi): M = blockdiag of the dof x dof node blocks

    def solve_bjacobi(self, b: torch.Tensor, x: torch.Tensor,
                      maxits: int = 100, res_atol: float = 0.0,
                      res_rtol: float = 1e-9,
                      dof: int | None = None) -> SolveResult:
        """Block-Jacobi PCG: z_node = (A_node,node)^-1 r_node, otherwise
        the algebra of :meth:`solve_jacobi` (true-residual convergence
        test).  ``dof`` None: detected with the GPU solver's Block-SELL
        ladder (4, 3, 2 at density >= 0.75)."""
        from ..utils.errors import AcgError, ErrCode
        from .precond import block_jacobi_inverse, detect_block_dof

        if dof is None:
            dof = detect_block_dof(self.local)
            if dof is None:
                raise AcgError(ErrCode.NOT_SUPPORTED,
                               "block Jacobi needs a Block-SELL operator: no "
                               "dense dof x dof block structure (dof 4/3/2, "
                               "density >= 0.75) in this matrix")
        res = SolveResult(solver="cg-bjacobi-cpu", maxits=maxits,
                          res_atol=res_atol, res_rtol=res_rtol,
                          nranks=self.comm.size if self.comm else 1)
        n = self.n
        t0 = time.perf_counter()
        minv = torch.from_numpy(block_jacobi_inverse(self.local, dof)).to(
            self.device)

        def apply(r):
            return torch.einsum("nab,nb->na", minv,
                                r.view(n // dof, dof)).reshape(n)

        bnrm2 = math.sqrt(self._dot(b, b))
        res.bnrm2 = bnrm2
        r = self._vec()
        t = self._vec()
        p = self._vec(nghost=True)
        self._spmv(x, t)
        r[:] = b[:n] - t
        z = apply(r)
        p[:n] = z
        rz = self._dot(r, z)
        rr = self._dot(r, r)
        res.r0nrm2 = math.sqrt(rr)
        rtol2 = max(res_atol, res_rtol * bnrm2) ** 2
        if rtol2 > 0 and rr <= rtol2:
            res.converged = True
            res.rnrm2 = math.sqrt(rr)
            res.tsolve = time.perf_counter() - t0
            return res
        for k in range(maxits):
            self._spmv(p, t)
            pt = self._dot(p, t)
            alpha = rz / pt if pt != 0.0 else 0.0
            r -= alpha * t
            x[:n] += alpha * p[:n]
            z = apply(r)
            rz_new = self._dot(r, z)
            rr = self._dot(r, r)
            res.niterations = k + 1
            res.rnrm2 = math.sqrt(max(rr, 0.0))
            if rtol2 > 0 and rr <= rtol2:
                res.converged = True
                break
            beta = rz_new / rz if rz != 0.0 else 0.0
            p[:n] = z + beta * p[:n]
            rz = rz_new
        res.tsolve = time.perf_counter() - t0
        nnz_full = self.local.nnzA + self.local.nnzO
        res.nflops = res.niterations * (cg_flops_per_iter(nnz_full, n)
                                        + (2.0 * dof + 2.0) * n)
        res.halo_bytes_sent = self.halo.bytes_sent
        res.halo_msgs_sent = self.halo.nmsgs_sent
        return res

    # -- pipelined CG (reference acgsolverhip_solve_pipelined, §3.3) ------

    def solve_pipelined(self, b: torch.Tensor, x: torch.Tensor, maxits: int = 100,
                        res_atol: float = 0.0, res_rtol: float = 1e-9,
                        rr_period: int = 0) -> SolveResult:
        """``rr_period`` > 0: residual replacement.  After the update of
        every iteration k with (k + 1) % rr_period == 0 the four recurrence
        vectors are recomputed from x and p: r = b - A x, t = A p, w = A r,
        z = A t.  gamma_prev / alpha_prev stay; the next iteration's
        gamma = (r,r) and delta = (w,r) come from the replaced vectors.
        0 (the default) is the plain Ghysels-Vanroose recurrence."""
        if rr_period < 0:
            raise ValueError(f"rr_period must not be negative, got {rr_period}")
        res = SolveResult(solver="cg-pipelined-cpu", maxits=maxits,
                          res_atol=res_atol, res_rtol=res_rtol,
                          nranks=self.comm.size if self.comm else 1)
        n = self.n
        t0 = time.perf_counter()
        bnrm2 = math.sqrt(self._dot(b, b))
        res.bnrm2 = bnrm2
        tmp = self._vec()
        r = self._vec(nghost=True)
        w = self._vec(nghost=True)
        q = self._vec()
        z = self._vec()
        t = self._vec()
        p = self._vec()
        if rr_period:
            # t and p become SpMV inputs: they need ghost tails
            tfull = self._vec(nghost=True)
            pfull = self._vec(nghost=True)
            t, p = tfull[:n], pfull[:n]
        self._spmv(x, tmp)
        r[:n] = b[:n] - tmp
        self._spmv(r, w)  # w = A r  (writes w[:n])
        rtol2 = max(res_atol, res_rtol * bnrm2) ** 2
        gamma_prev = alpha_prev = None
        for k in range(maxits):
            gd = torch.stack([torch.dot(r[:n], r[:n]), torch.dot(w[:n], r[:n])])
            self._allreduce(gd)
            gamma, delta = float(gd[0]), float(gd[1])
            if k == 0:
                res.r0nrm2 = math.sqrt(gamma)
            res.rnrm2 = math.sqrt(gamma)
            if rtol2 > 0 and gamma <= rtol2:
                res.converged = True
                res.niterations = k
                break
            self._spmv(w, q)  # q = A w (halo on w inside)
            if k == 0:
                beta = 0.0
                alpha = gamma / delta if delta != 0.0 else 0.0
            else:
                beta = gamma / gamma_prev if gamma_prev != 0.0 else 0.0
                den = delta - beta * (gamma / alpha_prev if alpha_prev != 0.0 else 0.0)
                alpha = gamma / den if den != 0.0 else 0.0
            z[:] = q + beta * z
            t[:] = w[:n] + beta * t
            p[:] = r[:n] + beta * p
            x[:n] += alpha * p
            r[:n] -= alpha * t
            w[:n] -= alpha * z
            gamma_prev, alpha_prev = gamma, alpha
            res.niterations = k + 1
            if rr_period and (k + 1) % rr_period == 0:
                self._spmv(x, tmp)
                r[:n] = b[:n] - tmp
                self._spmv(pfull, t)
                self._spmv(r, w)
                self._spmv(tfull, z)
                res.nreplacements += 1
        res.tsolve = time.perf_counter() - t0
        nnz_full = self.local.nnzA + self.local.nnzO
        res.nflops = (res.niterations * (cg_flops_per_iter(nnz_full, n) + 8.0 * n)
                      + res.nreplacements * replacement_flops(nnz_full, n))
        res.halo_bytes_sent = self.halo.bytes_sent
        res.halo_msgs_sent = self.halo.nmsgs_sent
        return res
