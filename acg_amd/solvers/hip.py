"""MI355X HIP CG solvers: classic and pipelined, with stream overlap.

Reference: acg/cghip.c (acgsolverhip_init :140-330, _solvempi :402-1159,
_solve_pipelined :1187-1933).  The structure here is the MI355X-native
re-design:

- All matrix/vector state is torch tensors on the GPU; the hot ops are the
  hand-written gfx950 kernels in ops/kernels.hip (no hipBLAS/hipSPARSE).
- Scalars (alpha/beta numerators/denominators) live in an 8-slot fp64
  device slab; every coefficient is computed *on device* inside the fused
  kernels.  The only D2H per iteration is the 8-byte residual norm for the
  host convergence test (reference cghip.c:996-1001).
- (p,t) is fused into the SpMV kernels (dot accumulated while t is
  produced), and the r/x updates + the new (r,r) are one fused kernel --
  the classic iteration runs 2 SpMV + 2 tiny prep kernels + 1 fused
  update + 1 daypx + 2 one-double RCCL allreduces.
- Streams: compute work on the caller's current stream; the halo
  (pack + grouped RCCL send/recv into the ghost tail) on a side
  ``comm_stream`` ordered by events exactly like the reference's
  preadytosend/preceived discipline (cghip.c:887-931): SpMV(matA) overlaps
  the exchange, SpMV(matO) waits for it.
"""

from __future__ import annotations

import math
import os
import sys
import time

import numpy as np
import torch

from ..dist.halo import HaloExchange
from ..ops import gpu_ops as ops
from ..part.subdomain import LocalSystem
from .base import (ColumnTolerances, SolveResult, block_results,
                   cg_flops_per_iter, check_multi_shapes, next_multi_k,
                   refine, replacement_flops, solve_multi_by_column)
from .operator import build_operators


class LaggedReadback:
    """Ring of ``lag + 1`` pinned host buffers (``width`` doubles each) and
    events for the lagged host convergence test: iteration k pushes its
    value into slot ``k % (lag + 1)`` and the host reads iteration
    ``k - lag``, so the test runs for every iteration while the host stays
    ``lag`` iterations ahead of the GPU instead of blocking on each
    iteration's tail.  What index j means (residual after j or after j + 1
    iterations) is the caller's business."""

    def __init__(self, width: int, lag: int):
        self.lag = lag
        self._buf = [torch.zeros(width, dtype=torch.float64, pin_memory=True)
                     for _ in range(lag + 1)]
        self._ev = [torch.cuda.Event() for _ in range(lag + 1)]

    def push(self, k: int, src: torch.Tensor, stream) -> None:
        """Enqueue on ``stream`` the D2H copy of ``src`` into slot k and
        record the slot's event behind it."""
        j = k % (self.lag + 1)
        if stream == torch.cuda.current_stream(stream.device):
            # the usual case; skips the stream context's two set_stream
            # calls in the host-bound small-system loop
            self._buf[j].copy_(src, non_blocking=True)
        else:
            with torch.cuda.stream(stream):
                self._buf[j].copy_(src, non_blocking=True)
        self._ev[j].record(stream)

    def event(self, k: int):
        return self._ev[k % (self.lag + 1)]

    def get(self, j: int) -> torch.Tensor:
        """Wait for slot j's copy; returns the pinned buffer (valid until
        iteration ``j + lag + 1`` is pushed)."""
        self._ev[j % (self.lag + 1)].synchronize()
        return self._buf[j % (self.lag + 1)]

    def tail(self, nit: int) -> range:
        """The iterations still unread after ``nit`` pushes."""
        return range(max(nit - self.lag, 0), nit)


class CGSolverHIP:
    """Distributed CG on one MI355X per rank (classic + pipelined)."""

    def __init__(self, local: LocalSystem, comm=None, device=None,
                 lanes: int | None = None, use_sell: bool = True,
                 profile: bool = False, matfree: bool = False,
                 force_format: str | None = None):
        self.local = local
        self.comm = comm
        if device is None:
            device = comm.device if comm is not None and comm.device is not None \
                else torch.device("cuda", 0)
        self.device = torch.device(device)
        L = local
        self.n = L.nowned
        self.nlocal = L.nowned + L.nghost
        # every format-specific tensor and kernel call lives in the operator
        # module; the solver holds the operators by role (see OperatorSet):
        # opA / opO are what _spmv_overlapped applies, ``operators.pipe`` and
        # ``operators.device_cg`` the SELL or stencil operators of the
        # megafused pass and the one-launch CG (SELL copies where opA is
        # BSELL)
        self.operators = build_operators(
            L, force_format, use_sell, lanes, matfree, self.device,
            serial=comm is None or comm.size == 1, ops=ops)
        self.opA, self.opO = self.operators.A, self.operators.O
        self._opA32 = None  # fp32-stored twin of opA, built by _lowprec_op
        self.can_megafuse = self.operators.pipe is not None
        self.megafuse_auto = self.operators.pipe_auto
        self.halo = HaloExchange(L.halo, L.nowned, self.device, comm)
        self.scal = ops.alloc_scalars(self.device)
        self.partials = ops.alloc_partials(self.device)
        from .profiling import EventProfiler

        self.prof = EventProfiler(profile)
        self.comm_stream = torch.cuda.Stream(self.device)
        self.allred_stream = torch.cuda.Stream(self.device)
        self.copy_stream = torch.cuda.Stream(self.device)
        self._rr_host = torch.zeros(1, dtype=torch.float64, pin_memory=True)
        self._ev_p = torch.cuda.Event()
        self._ev_recv = torch.cuda.Event()
        self._ev_rr = torch.cuda.Event()
        # always-on counters (reference cghip.h:109-118)
        self.niterations_total = 0
        # persistent per-method workspace vectors + captured iteration
        # graphs: repeated solves on one solver instance replay the graphs
        # captured on the FIRST solve (capture costs ~5-10 ms; re-capturing
        # inside every solve costs 2-10% at typical step counts).  Solution
        # state lives in the internal "xi" buffer so graph-referenced
        # addresses never change; the caller's x is copied in/out.
        self._ws: dict = {}
        self._graphs: dict = {}
        self._nstag = 0
        # solve_multi: columns per SpMM group, 2, 4 or 8.  A group of 8
        # reads the matrix least often; on the 4.1 M-row Queen-shaped
        # system two groups of 4 were nevertheless measured faster than
        # one of 8 (profiles/multi_rhs.md, NOTES.md).
        self.multi_group = 8
        # solve_pipelined(rr_period > 0): False forces the four-SpMV
        # replacement where the dual-SpMV fast path would apply (A/B, tests)
        self._rr_fast = True

    # -- the benchmark's interface: bench.py reads these five (and tests and
    # tools a few more below); everything in this file asks the operators --

    @property
    def matfree(self):
        return getattr(self.opA, "mf", None)

    @property
    def bsell(self):
        b = self.operators.bsell
        return b.arrays if b is not None else None

    @property
    def sell(self):
        s = self.operators.sell
        return s.arrays if s is not None else None

    @property
    def sell_perm(self):
        s = self.operators.sell
        return s.perm if s is not None else None

    @property
    def hybrid(self):
        """The hybrid or binned operator as the dict this attribute used to
        be (None without one): the SELL part's ``sellptr``/``cols``/
        ``svals``/``perm`` and the binned part's ``rowlist``, each None for
        an empty part, ``bins``, and ``rowlistO``/``binsO`` where the matO
        rows were binned too."""
        h = self.operators.hybrid
        if h is None:
            return None
        sell, binned = getattr(h, "sell", None), getattr(h, "binned", h)
        sp, sc, sv = sell.arrays if sell is not None else (None,) * 3
        d = {"sellptr": sp, "cols": sc, "svals": sv,
             "perm": sell.perm if sell is not None else None,
             "rowlist": binned.rowlist if binned is not None else None,
             "bins": binned.bins if binned is not None else []}
        if self.opO is not None and self.opO.fmt == "binned":
            d["rowlistO"], d["binsO"] = self.opO.rowlist, self.opO.bins
        return d

    @property
    def sellO(self):
        s = self.operators.sellO
        return s.arrays if s is not None else None

    @property
    def bsell_st(self):
        """Tile-symmetric BSELL (ops/symtile.py) of the same operator; only
        the serial classic solve runs on it, everything else on bsell."""
        return self.opA.st

    @property
    def _vals32(self):
        return self._opA32.vals if self._opA32 is not None else None

    @property
    def lanesO(self):
        return self.operators.lanesO

    def _csr_view(self, which: str, i: int):
        """Array i of the CSR triple ``csrA`` / ``csrO`` still on the
        device, or None."""
        csr = getattr(self.operators, which)
        return csr[i] if csr is not None else None

    A_rowptr = property(lambda self: self._csr_view("csrA", 0))
    O_rowptr = property(lambda self: self._csr_view("csrO", 0))
    O_colidx = property(lambda self: self._csr_view("csrO", 1))
    O_vals = property(lambda self: self._csr_view("csrO", 2))

    def _workspace(self, key: str, names) -> dict:
        """Per-method persistent vectors, base-address STAGGERED: equal-size
        allocations come back congruent mod large powers of two, so the
        fused update's 6+ streams hit the same L2 set / HBM channel at every
        index -- measured as a ~10% per-instance placement lottery
        (535-589 us/it on identical Queen solvers).  A 4160 B (64 B-odd)
        offset per vector de-correlates the streams deterministically."""
        ws = self._ws.setdefault(key, {})
        for nm, nghost in names:
            if nm not in ws:
                n = self.nlocal if nghost else self.n
                off = 520 * self._nstag  # 520 doubles = 4096 + 64 bytes
                self._nstag += 1
                buf = torch.zeros(n + off, dtype=torch.float64,
                                  device=self.device)
                ws[nm] = buf[off:] if off else buf
        return ws

    # -- pieces -----------------------------------------------------------

    def _allreduce_slot(self, slot: int, count: int = 1):
        if self.comm is not None and self.comm.size > 1:
            self.comm.allreduce_(self.scal[slot:slot + count])

    def _halo_fork(self, x: torch.Tensor, span=None) -> None:
        """Start the halo exchange of ``x`` on comm_stream, ordered after
        what the current stream has queued (the reference's preadytosend).
        A profiler ``span`` is opened between the wait and the exchange, so
        it times the exchange and not the wait for x."""
        self._ev_p.record(torch.cuda.current_stream(self.device))
        self.comm_stream.wait_event(self._ev_p)
        if span is not None:
            span.__enter__()
        with torch.cuda.stream(self.comm_stream):
            self.halo.begin(x)

    def _halo_join(self) -> None:
        """Finish the exchange; the current stream waits for the ghost tail
        (the reference's preceived)."""
        with torch.cuda.stream(self.comm_stream):
            self.halo.end()
            self._ev_recv.record(self.comm_stream)
        torch.cuda.current_stream(self.device).wait_event(self._ev_recv)

    def _dist_capture_ok(self, use_graph: bool, failed_key: str) -> bool:
        """Whether the whole distributed iteration may be captured into a
        graph: asked for, several ranks, profiler off, a backend that can
        capture, no earlier failure on this solver.  ACG_DIST_GRAPH=0 is
        the operational kill switch (eager iterations everywhere)."""
        serial = self.comm is None or self.comm.size == 1
        return bool(use_graph and not serial and not self.prof.enabled
                    and getattr(self.comm, "can_capture", False)
                    and os.environ.get("ACG_DIST_GRAPH", "1") != "0"
                    and not self._graphs.get(failed_key, False))

    def _capture_dist(self, body, failed_key: str, what: str = ""):
        """Record ``body()`` into a new graph and return it.  Capture is
        rank-local and records without executing, so no rank-sync is
        involved; ANY failure (e.g. the gloo test backend cannot capture)
        sets ``failed_key`` -- a permanent fall-back to eager iterations
        for this solver -- and returns None.  Mixed replay/eager ranks
        remain correct because replay issues the identical collective
        sequence."""
        try:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                body()
            return graph
        except Exception as e:
            self._graphs[failed_key] = True
            torch.cuda.synchronize(self.device)
            if self.comm is None or self.comm.rank == 0:
                print(f"[acg_amd] {what}distributed graph capture unavailable "
                      f"({type(e).__name__}); eager iterations",
                      file=sys.stderr)
            return None

    def _count_work(self, res: SolveResult, flops_per_it: float,
                    extra_flops: float = 0.0) -> None:
        """Always-on counters of a finished solve (reference
        cghip.h:109-118)."""
        res.nflops = res.niterations * flops_per_it + extra_flops
        res.halo_bytes_sent = self.halo.bytes_sent
        res.halo_msgs_sent = self.halo.nmsgs_sent
        self.niterations_total += res.niterations

    def _annotate_profile(self, res: SolveResult) -> None:
        if not self.prof.enabled:
            return
        from .profiling import annotate_op_stats

        annotate_op_stats(res, self.local, self.prof.collect(),
                          idx_bytes_per_nnz=self.opA.idx_bytes_per_nnz)
        self.prof.reset()

    def _format_name(self) -> str:
        return self.opA.name

    @property
    def classic_format(self) -> str:
        """Operator format of the plain classic solve: "bsell-st" when the
        tile-symmetric operator was built, else :meth:`_format_name`."""
        return "bsell-st" if self.opA.st is not None else self.opA.name

    def _lowprec_op(self):
        """opA on fp32-stored values (plain SELL, sigma-SELL or BSELL;
        ValueError names any other format), built on first use.  The solver
        then holds 1.5x the value memory.  matO stays fp64."""
        if self._opA32 is None:
            self._opA32 = self.opA.fp32()
        return self._opA32

    def _spmv_overlapped(self, xfull: torch.Tensor, y: torch.Tensor,
                         fuse_dotslot: int = -1, lowprec: bool = False):
        """halo(x) on comm stream overlapped with SpMV(matA); SpMV(matO)
        after the ghost tail arrives.  Mirrors reference cghip.c:887-931.
        ``lowprec`` selects the fp32-stored matA values (see
        _lowprec_op); the default is the fp64 operator."""
        opA = self._lowprec_op() if lowprec else self.opA
        have_halo = self.comm is not None and self.comm.size > 1
        if have_halo:
            halo_span = self.prof.span("halo", self.comm_stream)
            self._halo_fork(xfull, halo_span)  # closed after the join below
        scal = self.scal if fuse_dotslot >= 0 else None
        with self.prof.span("spmvA"):
            # the matA pass OVERWRITES the dot slot (dot_accum=False), so
            # no zeroing prep kernel is needed; matO accumulates on top
            opA.apply(xfull, y, accum=False, dot_accum=False,
                      partials=self.partials, scal=scal, dotslot=fuse_dotslot)
        if have_halo:
            self._halo_join()
            halo_span.__exit__(None, None, None)
        if self.opO is not None:
            with self.prof.span("spmvO"):
                self.opO.apply(xfull, y, accum=True, dot_accum=True,
                               partials=self.partials, scal=scal,
                               dotslot=fuse_dotslot)

    def _host_scalar(self, slot: int) -> float:
        cur = torch.cuda.current_stream(self.device)
        self._ev_rr.record(cur)
        self.copy_stream.wait_event(self._ev_rr)
        with torch.cuda.stream(self.copy_stream):
            self._rr_host.copy_(self.scal[slot:slot + 1], non_blocking=True)
        self.copy_stream.synchronize()
        return float(self._rr_host[0])

    def _vec(self, nghost: bool = False) -> torch.Tensor:
        return torch.zeros(self.nlocal if nghost else self.n,
                           dtype=torch.float64, device=self.device)

    # -- classic CG -------------------------------------------------------

    def solve(self, b: torch.Tensor, x: torch.Tensor, maxits: int = 100,
              res_atol: float = 0.0, res_rtol: float = 1e-9,
              use_graph: bool | None = None,
              fold_daypx: bool | None = None,
              diff_atol: float = 0.0, diff_rtol: float = 0.0) -> SolveResult:
        """Classic CG (reference acgsolverhip_solvempi, cghip.c:402-1159).

        ``x`` must be an nlocal vector (ghost tail included); ``b`` nowned.
        The host convergence test runs every iteration on the lag-1
        pipeline (see solve_pipelined).

        ``use_graph`` default None = measured policy (same as pipelined):
        OFF serial (eager wins by ~8 us/it), ON multi-GPU -- the WHOLE
        distributed iteration (halo fork, split SpMV, both allreduces,
        fused update, daypx) is captured once and replayed so the
        ~100 us/it of host-side c10d/launch work leaves the critical
        path.  Unlike pipelined no in-graph scalar snapshot is needed:
        the body ENDS with scal[S_RR] holding the allreduced new (r,r)
        (daypx reads but never writes it), so the post-replay lagged D2H
        reads a rank-consistent value by stream order.  Any capture
        failure (e.g. gloo) permanently falls back to eager;
        ACG_DIST_GRAPH=0 is the kill switch.

        ``diff_atol``/``diff_rtol`` stop on the solution change
        ``|alpha|*||p|| <= max(diff_atol, diff_rtol*||b||)`` -- a
        beyond-reference capability (the reference GPU solvers REJECT diff
        tolerances, cghip.c:427); engaging it switches to a blocking
        per-iteration host test (no lag pipeline, no graph replay).
        """
        return self._solve_classic(b, x, maxits, res_atol, res_rtol,
                                   use_graph, fold_daypx, diff_atol,
                                   diff_rtol, lowprec=False)

    def _solve_classic(self, b, x, maxits, res_atol, res_rtol,
                       use_graph=None, fold_daypx=None, diff_atol=0.0,
                       diff_rtol=0.0, *, lowprec: bool) -> SolveResult:
        """The classic iteration behind :meth:`solve`.  ``lowprec`` runs
        every SpMV on the fp32-stored matA values (the inner solver of
        :meth:`solve_mixed`); captured graphs are keyed per value set, so
        a graph recorded with one operator is never replayed for the
        other."""
        gkey = "classic:f32" if lowprec else "classic"
        res = SolveResult(solver="cg-hip", maxits=maxits, res_atol=res_atol,
                          res_rtol=res_rtol,
                          nranks=self.comm.size if self.comm else 1)
        n = self.n
        S = ops
        scal = self.scal
        ws = self._workspace("classic", [("r", False), ("t", False),
                                         ("p", True), ("xi", True)])
        r, t, p, xi = ws["r"], ws["t"], ws["p"], ws["xi"]
        # BSELL-ST: the whole solve runs in the operator's permuted node
        # order (b and x gathered once here, x scattered back in
        # _finish_classic); the vector kernels do not care about the order
        st = self.opA.st
        if lowprec or fold_daypx is True or diff_atol > 0 or diff_rtol > 0:
            st = None

        def spmv(xv, yv, fuse_dotslot=-1):
            if st is None:
                self._spmv_overlapped(xv, yv, fuse_dotslot=fuse_dotslot,
                                      lowprec=lowprec)
                return
            with self.prof.span("spmvA"):
                self.opA.apply_st(xv, yv, partials=self.partials,
                                  scal=scal if fuse_dotslot >= 0 else None,
                                  dotslot=fuse_dotslot, dot_accum=False)

        if st is None:
            xi.copy_(x)
        else:
            torch.index_select(x[:n], 0, st.vperm, out=xi[:n])
        torch.cuda.synchronize(self.device)
        t0 = time.perf_counter()
        # bnrm2
        S.dot(b, b, self.partials, scal, S.S_BNRM2, n=n)
        self._allreduce_slot(S.S_BNRM2)
        # r0 = b - A x0;  p = r0
        spmv(xi, t)
        if st is None:
            torch.sub(b[:n], t, out=r)
        else:
            torch.index_select(b[:n], 0, st.vperm, out=r)
            r.sub_(t)
        p[:n] = r
        S.dot(r, r, self.partials, scal, S.S_RR, n=n)
        self._allreduce_slot(S.S_RR)
        bnrm2sqr = self._host_scalar(S.S_BNRM2)
        rr = self._host_scalar(S.S_RR)
        res.bnrm2 = math.sqrt(max(bnrm2sqr, 0.0))
        res.r0nrm2 = math.sqrt(max(rr, 0.0))
        rtol2 = max(res_atol, res_rtol * res.bnrm2) ** 2
        dtol = max(diff_atol, diff_rtol * res.bnrm2)
        if rtol2 > 0 and rr <= rtol2 and dtol == 0.0:
            res.converged = True
            res.rnrm2 = math.sqrt(rr)
            res.tsolve = time.perf_counter() - t0
            return res
        converged = False
        serial = self.comm is None or self.comm.size == 1
        if dtol > 0:
            converged = self._solve_diffmode(res, r, t, p, xi, rtol2, dtol,
                                             maxits)
            return self._finish_classic(res, x, xi, converged, rtol2, t0)
        # daypx folded into the BSELL SpMV (serial matA-only): the gather
        # computes beta*p_old + r on the fly and the row side materialises
        # p_new into a ping-pong buffer, eliminating the 3n-stream daypx
        # kernel.  MEASURED NEGATIVE and therefore opt-in: doubling the
        # gather footprint (p_old AND r) costs +60 us/it on Queen vs the
        # ~15 us the daypx saves (553.6 vs 493.8 us/it interleaved) --
        # the SpMV gather is the roofline resource, not kernel count.
        fold = (serial and self.opA.has_daypx and self.local.nnzO == 0
                and fold_daypx is True)
        if fold:
            p2 = self._workspace("classic", [("p2", True)])["p2"]
            scal[S.S_RR_PREV] = math.inf
        if use_graph is None:
            use_graph = not serial  # measured policy (see docstring)
        graph_ok = use_graph and serial and not self.prof.enabled and not fold
        graph = self._graphs.get(gkey) if graph_ok else None
        # multi-GPU: capture the whole distributed iteration (see docstring)
        dist_key = gkey + ":dist"
        dist_failed_key = "classic:capture_failed"
        dist_graph_ok = (not fold
                         and self._dist_capture_ok(use_graph, dist_failed_key))
        dgraph = self._graphs.get(dist_key) if dist_graph_ok else None
        # lag-2 convergence pipeline (+ optional hipGraph replay), mirroring
        # solve_pipelined (the host test runs for every iteration; the host
        # reads the value two iterations late).  Classic's rr copy lands at
        # the END of its iteration, so lag 1 would make the host wake
        # exactly when the GPU drains -- lag 2 keeps one full iteration
        # queued and the GPU never idles (measured 582 -> ~545 us/it).
        ring = LaggedReadback(1, lag=2)

        def body(k: int = 0):
            if fold:
                pold, pnew = (p, p2) if k % 2 == 0 else (p2, p)
                with self.prof.span("spmvA"):
                    self.opA.spmv_daypx(pold, r, pnew, t, scal,
                                        self.partials, S.S_PT)
                with self.prof.span("update_classic"):
                    S.cg_fused_update(r, xi, pnew, t, scal, self.partials, n)
                return
            # halo+split SpMV with the (p,t) reduction fused into both
            # passes (matA overwrites the slot, matO accumulates)
            spmv(p, t, fuse_dotslot=S.S_PT)
            with self.prof.span("allreduce"):
                self._allreduce_slot(S.S_PT)
            # fused r/x update (alpha = rr/pt on device) + combined
            # finalize (rr -> rr_prev rotation + new (r,r))
            with self.prof.span("update_classic"):
                S.cg_fused_update(r, xi, p, t, scal, self.partials, n)
            with self.prof.span("allreduce"):
                self._allreduce_slot(S.S_RR)
            # p = (rr/rr_prev) p + r
            with self.prof.span("daypx"):
                S.daypx_ratio(p, r, scal, S.S_RR, S.S_RR_PREV, n=n)

        def check(j):
            """Host test of rr after iteration j."""
            nonlocal rr, converged
            rr = float(ring.get(j)[0])
            if not math.isfinite(rr):
                raise FloatingPointError(f"CG diverged: rr={rr} at it {j + 1}")
            if rtol2 > 0 and rr <= rtol2:
                converged = True
                res.niterations = j + 1
                return True
            return False

        k = 0
        cur = torch.cuda.current_stream(self.device)
        rr_slot = scal[S.S_RR:S.S_RR + 1]
        while k < maxits:
            if k >= ring.lag and check(k - ring.lag):
                break
            if graph is not None:
                graph.replay()
            elif dgraph is not None and k > 0:
                dgraph.replay()
            else:
                body(k)
                if graph_ok and k == 1:
                    graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graph):
                        body()
                    self._graphs[gkey] = graph
                elif dist_graph_ok and k == 2 and dgraph is None:
                    # RCCL channels are warm after 2 eager iterations
                    dgraph = self._capture_dist(body, dist_failed_key,
                                                "classic ")
                    if dgraph is not None:
                        self._graphs[dist_key] = dgraph
            # lagged rr D2H on the SAME stream: cross-stream event chains
            # measured ~20 us each in fire->launch latency (45 us/iter of
            # the iteration period); the in-order 8-byte copy costs ~3 us
            # on the critical path and makes the overwrite race impossible
            # by stream ordering.
            ring.push(k, rr_slot, cur)
            k += 1
            res.niterations = k
        if not converged:
            for j in ring.tail(maxits):
                if check(j):
                    break
        return self._finish_classic(res, x, xi, converged, rtol2, t0, st)

    def _solve_diffmode(self, res, r, t, p, xi, rtol2: float, dtol: float,
                        maxits: int) -> bool:
        """Classic iterations with the solution-change stopping criterion
        ``|alpha|*||p|| <= dtol`` (CPU-solver semantics, cg.c:1059-1068).
        Blocking host test each iteration: alpha = rr_prev/pt comes from
        the device scalar slab AFTER the fused update rotated rr ->
        rr_prev; ||p||^2 is one extra fused-dot + allreduce per iteration
        (S_GAMMA used as scratch -- classic never touches it)."""
        S = ops
        n = self.n
        scal = self.scal
        converged = False
        for k in range(maxits):
            self._spmv_overlapped(p, t, fuse_dotslot=S.S_PT)
            self._allreduce_slot(S.S_PT)
            S.dot(p, p, self.partials, scal, S.S_GAMMA, n=n)
            self._allreduce_slot(S.S_GAMMA)
            S.cg_fused_update(r, xi, p, t, scal, self.partials, n)
            self._allreduce_slot(S.S_RR)
            res.niterations = k + 1
            rr_old = self._host_scalar(S.S_RR_PREV)
            pt = self._host_scalar(S.S_PT)
            pp = self._host_scalar(S.S_GAMMA)
            rr = self._host_scalar(S.S_RR)
            if not math.isfinite(rr):
                raise FloatingPointError(f"CG diverged: rr={rr} at it {k + 1}")
            alpha = rr_old / pt if pt != 0.0 else 0.0
            dx = abs(alpha) * math.sqrt(max(pp, 0.0))
            if (rtol2 > 0 and rr <= rtol2) or dx <= dtol:
                converged = True
                break
            S.daypx_ratio(p, r, scal, S.S_RR, S.S_RR_PREV, n=n)
        return converged

    def _finish_classic(self, res, x, xi, converged: bool, rtol2: float,
                        t0: float, st=None):
        """``st``: the BSELL-ST operator the solve ran on; xi is then in
        its node order and goes back to the caller's."""
        S = ops
        torch.cuda.synchronize(self.device)
        res.tsolve = time.perf_counter() - t0
        if st is None:
            x.copy_(xi)
        else:
            x[:self.n].index_copy_(0, st.vperm, xi[:self.n])
        rr = self._host_scalar(S.S_RR)
        res.rnrm2 = math.sqrt(max(rr, 0.0))
        res.converged = converged or (rtol2 > 0 and rr <= rtol2)
        nnz_full = self.local.nnzA + self.local.nnzO
        self._count_work(res, cg_flops_per_iter(nnz_full, self.n))
        self._annotate_profile(res)
        return res

    # -- multiple right-hand sides (beyond reference) ----------------------

    def _multi_fast_path(self) -> bool:
        """The SpMM iteration exists for one rank with a SELL, sigma-SELL
        or BSELL matA and no matO; everything else loops over solve()."""
        serial = self.comm is None or self.comm.size == 1
        return (serial and self.opA.has_spmm and self.local.nnzO == 0
                and self.n > 0)

    def _multi_kmax(self) -> int:
        """Largest kernel-level K the operator format offers (a BSELL
        (dof, K) pair may be refused by the op layer)."""
        if self.multi_group not in ops.MULTI_K:
            raise ValueError(f"multi_group must be one of {ops.MULTI_K}, "
                             f"got {self.multi_group}")
        return self.opA.spmm_kmax(self.multi_group)

    def solve_multi(self, B: torch.Tensor, X: torch.Tensor, maxits: int = 100,
                    res_atol: float = 0.0, res_rtol: float = 1e-9) -> list:
        """Classic CG for k right-hand sides of one matrix: ``B`` is
        (nowned, k), ``X`` (nlocal, k), both fp64; X is overwritten and a
        list of k SolveResult returned.

        Fast path (one rank, SELL / sigma-SELL / BSELL matA, no matO): the
        columns are processed in groups of up to 8 (``self.multi_group``),
        a remainder padded with zero columns to the next size in
        {2, 4, 8}; every iteration applies the operator to the whole group
        with one SpMM, so each matrix entry and column index is read once
        per group instead of once per column.
        Each column has its own tolerance max(res_atol, res_rtol*||b_c||);
        a group iterates until all its real columns have met theirs (a
        column that converged early keeps iterating, which only improves
        it).  A column's ``niterations`` is the first iteration at which it
        met its tolerance; a column with b_c = 0 and x0_c = 0 is converged
        at iteration 0 and stays exactly zero.  ``tsolve`` of every column
        is its group's wall time.

        Every other configuration (several ranks, CSR / hybrid formats, a
        matO part, matrix-free) loops over :meth:`solve` column by column.
        """
        k = check_multi_shapes(B, X, self.n, self.nlocal)
        kmax = self._multi_kmax() if self._multi_fast_path() else 0
        if k == 1 or kmax == 0:
            return solve_multi_by_column(self.solve, B, X, maxits, res_atol,
                                         res_rtol)
        out = []
        for g0 in range(0, k, kmax):
            kg = min(kmax, k - g0)
            K = next(kk for kk in ops.MULTI_K if kk >= kg)
            out += self._solve_multi_group(B[:, g0:g0 + kg], X[:, g0:g0 + kg],
                                           K, maxits, res_atol, res_rtol)
        return out

    def _spmm(self, Xm: torch.Tensor, Y: torch.Tensor, scal, partials,
              dotslot: int = -1) -> None:
        fuse = dict(partials=partials, scal=scal, dotslot=dotslot) \
            if dotslot >= 0 else {}
        self.opA.spmm(Xm, Y, **fuse)

    def _multi_ws(self, kind: str, K: int) -> dict:
        """Persistent (rows, K) buffers of one group width, kept as
        ``_ws["multi{K}"]`` (residual R, direction P) or ``_ws["block{K}"]``
        (Q, S, the coefficient state and two more rr_out slots for the
        breakdown flag and its iteration)."""
        key = f"{kind}{K}"
        ws = self._ws.get(key)
        if ws is None:
            block = kind == "block"
            resid, dirn = ("Q", "S") if block else ("R", "P")

            def mv(rows):
                return torch.zeros(rows, K, dtype=torch.float64,
                                   device=self.device)
            ws = self._ws[key] = {
                resid: mv(self.n), "T": mv(self.n), "Bp": mv(self.n),
                dirn: mv(self.nlocal), "Xi": mv(self.nlocal),
                "scal": ops.alloc_scalars_multi(self.device, K),
                "partials": ops.alloc_partials_multi(self.device, K),
            }
            if block:
                ws["state"] = ops.alloc_block_state(self.device)
            ws["rr_out"] = torch.zeros(K + 2 if block else K,
                                       dtype=torch.float64, device=self.device)
        return ws

    def _multi_prologue(self, ws: dict, B, X, R, time_padding: bool):
        """Start of a multi-RHS group: B and X zero-padded to the workspace
        width, ``R = Bp - A Xi`` and the norms of the real columns.
        Returns (t0, bnrm, rr0), rr0 squared.  The timing window opens
        before the padding copies or after them, as the caller has always
        reported its ``tsolve``."""
        S = ops
        n, kg = self.n, B.shape[1]
        Bp, Xi, T = ws["Bp"], ws["Xi"], ws["T"]
        scal, partials = ws["scal"], ws["partials"]

        def start() -> float:
            torch.cuda.synchronize(self.device)
            return time.perf_counter()

        if time_padding:
            t0 = start()
        scal.zero_()
        Bp.zero_()
        Bp[:, :kg] = B
        Xi.zero_()
        Xi[:, :kg] = X
        if not time_padding:
            t0 = start()
        S.dot_multi(Bp, Bp, partials, scal, S.S_BNRM2, n=n)
        self._spmm(Xi, T, scal, partials)
        torch.sub(Bp, T, out=R)
        S.dot_multi(R, R, partials, scal, S.S_RR, n=n)
        slab = scal.cpu()
        bnrm = [math.sqrt(max(float(slab[c, S.S_BNRM2]), 0.0)) for c in range(kg)]
        rr0 = [float(slab[c, S.S_RR]) for c in range(kg)]
        return t0, bnrm, rr0

    def _solve_multi_group(self, B, X, K: int, maxits: int, res_atol: float,
                           res_rtol: float) -> list:
        """One group of kg <= K columns on the SpMM iteration (eager, same
        lag-2 host test as _solve_classic, reading the contiguous rr_out)."""
        S = ops
        n, kg = self.n, B.shape[1]
        ws = self._multi_ws("multi", K)
        R, T, P, Xi = ws["R"], ws["T"], ws["P"], ws["Xi"]
        scal, partials, rr_out = ws["scal"], ws["partials"], ws["rr_out"]
        P.zero_()
        t0, bnrm, rr0 = self._multi_prologue(ws, B, X, R, time_padding=False)
        P[:n] = R
        tol = ColumnTolerances(bnrm, rr0, res_atol, res_rtol)
        ring = LaggedReadback(K, lag=2)

        def check(j: int) -> bool:
            """Host test of rr_out after iteration j."""
            rrs = ring.get(j)
            for c in range(kg):
                rr = float(rrs[c])
                if not math.isfinite(rr):
                    raise FloatingPointError(
                        f"CG diverged: rr={rr} in column {c} at it {j + 1}")
                tol.record(c, rr, j + 1)
            return tol.all_met()

        nit = 0
        done = tol.all_met()
        cur = torch.cuda.current_stream(self.device)
        while not done and nit < maxits:
            if nit >= ring.lag and check(nit - ring.lag):
                done = True
                break
            with self.prof.span("spmvA"):
                self._spmm(P, T, scal, partials, dotslot=S.S_PT)
            with self.prof.span("update_classic"):
                nb = S.cg_fused_update_multi(R, Xi, P, T, scal, partials, n)
                S.cg_finalize_multi(partials, nb, scal, rr_out)
            with self.prof.span("daypx"):
                S.daypx_ratio_multi(P, R, scal, n=n)
            ring.push(nit, rr_out, cur)
            nit += 1
        if not done:
            for j in ring.tail(nit):
                if check(j):
                    break
        torch.cuda.synchronize(self.device)
        tsolve = time.perf_counter() - t0
        X.copy_(Xi[:, :kg])
        slab = scal.cpu()
        if self.prof.enabled:
            self.prof.reset()
        nnz_full = self.local.nnzA + self.local.nnzO
        out = []
        for c in range(kg):
            rr = float(slab[c, S.S_RR])
            res = SolveResult(solver="cg-hip-multi", maxits=maxits,
                              res_atol=res_atol, res_rtol=res_rtol, nranks=1)
            res.bnrm2 = bnrm[c]
            res.r0nrm2 = math.sqrt(max(rr0[c], 0.0))
            res.rnrm2 = math.sqrt(max(rr, 0.0))
            res.converged = tol.conv_it[c] is not None or tol.met(c, rr)
            res.niterations = tol.conv_it[c] if tol.conv_it[c] is not None else nit
            res.tsolve = tsolve
            res.nflops = res.niterations * cg_flops_per_iter(nnz_full, n)
            out.append(res)
        self.niterations_total += nit
        return out

    # -- block CG for several right-hand sides (beyond reference; opt-in,
    # never auto-selected) -------------------------------------------------

    def solve_block(self, B: torch.Tensor, X: torch.Tensor, maxits: int = 100,
                    res_atol: float = 0.0, res_rtol: float = 1e-9) -> list:
        """Block CG (Dubrulle's form with orthonormalised residuals, QR by
        Cholesky-QR) for k right-hand sides: same shapes, grouping and
        per-column tolerances as :meth:`solve_multi`, the same one SpMM per
        iteration, but every column searches the sum of the group's Krylov
        spaces, so ill-conditioned systems need fewer iterations.

        A column whose initial residual is exactly zero is left out of the
        block (converged at iteration 0, X column untouched).  When a
        Cholesky pivot fails the relative test (dependent right-hand sides,
        a column that converged exactly) the block stops where it is and
        :meth:`solve_multi` finishes from the current X: ``block_breakdown``
        of the results holds the block iteration of the hand-over and
        ``niterations`` counts both parts.  Outside the fast path of
        solve_multi, and for k = 1, this IS solve_multi."""
        k = check_multi_shapes(B, X, self.n, self.nlocal)
        kmax = self._multi_kmax() if self._multi_fast_path() else 0
        if k == 1 or kmax == 0:
            return self.solve_multi(B, X, maxits, res_atol, res_rtol)
        out = []
        for g0 in range(0, k, kmax):
            kg = min(kmax, k - g0)
            out += self._solve_block_group(B[:, g0:g0 + kg], X[:, g0:g0 + kg],
                                           maxits, res_atol, res_rtol)
        return out

    def _solve_block_group(self, B, X, maxits: int, res_atol: float,
                           res_rtol: float) -> list:
        """One group of up to multi_group columns (eager; the lag-2 host
        test of _solve_multi_group reads residual norms, breakdown flag and
        iteration from one (K + 2)-double copy)."""
        S = ops
        n, kg0 = self.n, B.shape[1]
        ws = self._multi_ws("block", next_multi_k(kg0, S.MULTI_K))
        Xi, Q = ws["Xi"], ws["Q"]
        # R0 = B - A X0 and the norms of the whole group
        t0, bnrm, rr0 = self._multi_prologue(ws, B, X, Q, time_padding=True)
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
            K = next_multi_k(kg, S.MULTI_K)
            Ract, Xact = Q[:, active], Xi[:, active]  # copies
            ws = self._multi_ws("block", K)
            Xi, Q = ws["Xi"], ws["Q"]
            for buf in (Xi, Q, ws["S"], ws["state"], ws["rr_out"]):
                buf.zero_()
            Xi[:, :kg] = Xact
            Q[:, :kg] = Ract
            nit, bd = self._block_iterate(ws, K, kg, active, tol, rr, maxits)
            if bd >= 0:
                Xf = Xi[:, :kg].contiguous()
                finish = self.solve_multi(B[:, active].contiguous(), Xf,
                                          max(maxits - bd, 0), res_atol,
                                          res_rtol)
                Xi[:, :kg] = Xf
            for i, c in enumerate(active):
                X[:, c] = Xi[:, i]
        torch.cuda.synchronize(self.device)
        tsolve = time.perf_counter() - t0
        if self.prof.enabled:
            self.prof.reset()
        self.niterations_total += nit
        return block_results(
            "cg-hip-block", kg0, active, tol, nit, bd, finish, bnrm, rr0, rr,
            maxits, res_atol, res_rtol, tsolve,
            cg_flops_per_iter(self.local.nnzA + self.local.nnzO, n))

    def _block_iterate(self, ws: dict, K: int, kg: int, active: list,
                       tol: ColumnTolerances, rr: list, maxits: int):
        """The block iteration on a prepared workspace (Q = R0, S = 0,
        state = 0).  Updates tol / rr of the active columns; returns
        (block iterations run, breakdown iteration or -1)."""
        S = ops
        n = self.n
        Xi, Q, T, Sm = ws["Xi"], ws["Q"], ws["T"], ws["S"]
        partials, state, rr_out = ws["partials"], ws["state"], ws["rr_out"]
        ring = LaggedReadback(K + 2, lag=2)
        cur = torch.cuda.current_stream(self.device)
        bd = -1

        def check(j: int) -> bool:
            """Host test of the state after block iteration ``j + 1``; True
            when the group is finished (all met, or breakdown)."""
            nonlocal bd
            buf, it = ring.get(j), j + 1
            if float(buf[K]) != 0.0:
                bd = int(buf[K + 1])
                return True
            for i, c in enumerate(active):
                v = float(buf[i])
                if not math.isfinite(v):
                    raise FloatingPointError(
                        f"block CG diverged: rr={v} in column {c} at it {it}")
                rr[c] = v
                tol.record(c, v, it)
            return tol.all_met()

        # start-up: Q <- R0 zeta^-1, C = zeta, S = Q
        with self.prof.span("block_init"):
            nb = S.gram_multi(Q, Q, partials, n=n)
            S.block_coef_beta(partials, nb, state, rr_out, K, kg, 0, init=True)
            S.block_ortho(Q, Sm, state, n)
        if float(rr_out.cpu()[K]) != 0.0:
            return 0, 0

        nit = 0
        done = False
        while not done and nit < maxits:
            if nit >= ring.lag and check(nit - ring.lag):
                done = True
                break
            with self.prof.span("spmvA"):
                self._spmm(Sm, T, None, None)
            with self.prof.span("block_gram"):
                nb = S.gram_multi(Sm, T, partials, n=n)
                S.block_coef_alpha(partials, nb, state, K, kg, nit + 1)
            with self.prof.span("block_update"):
                nb = S.block_update(Xi, Sm, Q, T, state, partials, n)
                S.block_coef_beta(partials, nb, state, rr_out, K, kg, nit + 1)
            with self.prof.span("block_ortho"):
                S.block_ortho(Q, Sm, state, n)
            ring.push(nit, rr_out, cur)
            nit += 1
        if not done:
            for j in ring.tail(nit):
                if check(j):
                    break
        torch.cuda.synchronize(self.device)
        return nit, bd

    # -- mixed precision: fp32-stored operator + fp64 refinement (beyond
    # reference; opt-in, no auto-selection) -------------------------------

    def solve_mixed(self, b: torch.Tensor, x: torch.Tensor, maxits: int = 100,
                    res_atol: float = 0.0, res_rtol: float = 1e-9,
                    inner_rtol: float = 1e-6,
                    max_outer: int = 20) -> SolveResult:
        """Classic CG on the fp32-STORED matA values wrapped in fp64
        iterative refinement (oracle: CGSolverCPU.solve_mixed; loop:
        base.refine).  The SpMV is at the HBM roofline and the values are
        its largest stream: fp32 storage cuts a dof-3 BSELL block from 76
        to 40 B and a SELL entry from 12 to 8 B, while every vector, product
        and sum stays fp64.  Each sweep computes r = b - A x with the fp64
        operator, solves ``A_lo d = r`` from d = 0 with the classic
        iteration to ``max(inner_rtol*||r||, 0.5*tol)`` and adds d to x.

        Needs the plain SELL, sigma-SELL or BSELL format (ValueError names
        any other) and keeps BOTH value sets: 1.5x the value memory.
        ``niterations`` counts inner iterations (at most ``maxits`` in
        total), ``nouter`` the sweeps; ``rnrm2`` is the TRUE fp64 residual
        norm of the returned x.  ``fold_daypx`` and the diff tolerances are
        not offered here.

        ``inner_rtol`` default 1e-6 is MEASURED (profiles/mixed_precision.md,
        scaled Queen-shaped system: -15% / -19% time-to-solution at rtol
        1e-9 / 1e-12 against 1e-4's -10% / -13%): a sweep costs 3-4
        iteration equivalents, so few deep sweeps beat many shallow ones."""
        self._lowprec_op()  # unsupported format: fail before any work
        res = SolveResult(solver="cg-hip-mixed", maxits=maxits,
                          res_atol=res_atol, res_rtol=res_rtol,
                          nranks=self.comm.size if self.comm else 1)
        n = self.n
        S = ops
        scal = self.scal
        ws = self._workspace("mixed", [("ro", False), ("to", False),
                                       ("d", True)])
        ro, to, d = ws["ro"], ws["to"], ws["d"]
        torch.cuda.synchronize(self.device)
        t0 = time.perf_counter()
        S.dot(b, b, self.partials, scal, S.S_BNRM2, n=n)
        self._allreduce_slot(S.S_BNRM2)
        res.bnrm2 = math.sqrt(max(self._host_scalar(S.S_BNRM2), 0.0))
        tol = max(res_atol, res_rtol * res.bnrm2)

        def residual_norm() -> float:
            self._spmv_overlapped(x, to)
            torch.sub(b[:n], to, out=ro)
            S.dot(ro, ro, self.partials, scal, S.S_RR, n=n)
            self._allreduce_slot(S.S_RR)
            return math.sqrt(max(self._host_scalar(S.S_RR), 0.0))

        def inner_solve(target: float, budget: int) -> int:
            d.zero_()
            inner = self._solve_classic(ro, d, budget, target, 0.0,
                                        lowprec=True)
            x[:n] += d[:n]
            return inner.niterations

        nres = refine(res, tol, maxits, inner_rtol, max_outer,
                      residual_norm, inner_solve)
        torch.cuda.synchronize(self.device)
        res.tsolve = time.perf_counter() - t0
        nnz_full = self.local.nnzA + self.local.nnzO
        # every sweep adds the fp64 residual SpMV and the inner solve's
        # initial SpMV; one more residual closes the loop
        res.nflops = (res.niterations * cg_flops_per_iter(nnz_full, n)
                      + (nres + res.nouter) * (2.0 * nnz_full + 3.0 * n))
        res.halo_bytes_sent = self.halo.bytes_sent
        res.halo_msgs_sent = self.halo.nmsgs_sent
        return res

    # -- monolithic device-side CG ---------------------------------------

    def solve_device(self, b: torch.Tensor, x: torch.Tensor, maxits: int = 100,
                     res_atol: float = 0.0, res_rtol: float = 1e-9) -> SolveResult:
        """Whole CG solve in ONE cooperative kernel launch (reference
        acgsolverhip_solve_device, §3.4; single-GPU only, as in the
        reference's HIP build -- cg-kernels-hip.hip:1832).  Zero
        per-iteration launch overhead: wins in the launch-bound regime
        (small/medium systems)."""
        if self.comm is not None and self.comm.size > 1:
            from ..utils.errors import AcgError, ErrCode

            raise AcgError(ErrCode.NOT_SUPPORTED,
                           "device-side CG is single-GPU (reference parity)")
        sell = self.operators.device_cg
        if sell is None:
            from ..utils.errors import AcgError, ErrCode

            raise AcgError(ErrCode.NOT_SUPPORTED,
                           "device-side CG requires the unpermuted SELL format")
        res = SolveResult(solver="cg-hip-device", maxits=maxits,
                          res_atol=res_atol, res_rtol=res_rtol, nranks=1)
        n = self.n
        r = self._vec()
        t = self._vec()
        p = self._vec(nghost=True)
        out2 = torch.zeros(2, dtype=torch.int32, device=self.device)
        barrier_state = torch.zeros(ops.BAR_STATE_WORDS, dtype=torch.int32,
                                    device=self.device)
        torch.cuda.synchronize(self.device)
        t0 = time.perf_counter()
        sell.cg_device(b, x, r, p, t, self.scal, self.partials, out2,
                       barrier_state, maxits, res_atol, res_rtol)
        torch.cuda.synchronize(self.device)
        res.tsolve = time.perf_counter() - t0
        S = ops
        res.bnrm2 = math.sqrt(max(float(self.scal[S.S_BNRM2]), 0.0))
        res.r0nrm2 = math.sqrt(max(float(self.scal[S.S_RR_PREV]), 0.0))
        rr = float(self.scal[S.S_RR])
        res.rnrm2 = math.sqrt(max(rr, 0.0))
        res.niterations = int(out2[0])
        conv = int(out2[1])
        if conv < 0:
            raise RuntimeError("device CG grid barrier timed out (residency?)")
        if not math.isfinite(rr):
            raise FloatingPointError(
                f"CG diverged: rr={rr} at it {res.niterations}")
        res.converged = bool(conv)
        nnz_full = self.local.nnzA + self.local.nnzO
        # (one rank never exchanges a halo: its counters stay zero)
        self._count_work(res, cg_flops_per_iter(nnz_full, n))
        return res

    # -- Jacobi-preconditioned CG (beyond reference: aCG is strictly
    # unpreconditioned, PCNONE even in its PETSc oracle cgpetsc.c:181-193;
    # opt-in so every parity bench stays unpreconditioned) ----------------

    def solve_jacobi(self, b: torch.Tensor, x: torch.Tensor,
                     maxits: int = 100, res_atol: float = 0.0,
                     res_rtol: float = 1e-9) -> SolveResult:
        """Jacobi-PCG composed from the existing device-scalar kernels:
        alpha = (r,z)/(p,t) via axpy_ratio, beta = rz'/rz via the
        RR/RR_PREV rotation, z = D^-1 r as one elementwise multiply.
        Convergence is tested on the TRUE residual 2-norm every iteration
        (blocking host read -- PCG trades per-iteration polish for a
        several-fold iteration-count cut on ill-conditioned systems)."""
        L = self.local
        if getattr(L, "A_rowptr", None) is None or not hasattr(L, "owned_global"):
            from ..utils.errors import AcgError, ErrCode

            raise AcgError(ErrCode.NOT_SUPPORTED,
                           "jacobi PCG needs the host CSR arrays "
                           "(file/extracted systems; not device-generated "
                           "slabs)")
        res = SolveResult(solver="cg-hip-jacobi", maxits=maxits,
                          res_atol=res_atol, res_rtol=res_rtol,
                          nranks=self.comm.size if self.comm else 1)
        n = self.n
        S = ops
        scal = self.scal
        if "jacobi_dinv" not in self._ws:
            rows = np.repeat(np.arange(n, dtype=np.int64),
                             np.diff(L.A_rowptr))
            dmask = rows == L.A_colidx
            d = np.zeros(n, dtype=np.float64)
            d[rows[dmask]] = L.A_vals[dmask]
            if (d == 0).any():
                from ..utils.errors import AcgError, ErrCode

                raise AcgError(ErrCode.INVALID_VALUE,
                               "jacobi preconditioner needs a full diagonal")
            self._ws["jacobi_dinv"] = torch.from_numpy(1.0 / d).to(self.device)
        dinv = self._ws["jacobi_dinv"]
        ws = self._workspace("jacobi", [("r", False), ("t", False),
                                        ("z", False), ("p", True),
                                        ("xi", True)])
        r, t, z, p, xi = ws["r"], ws["t"], ws["z"], ws["p"], ws["xi"]
        xi.copy_(x)
        torch.cuda.synchronize(self.device)
        t0 = time.perf_counter()
        S.dot(b, b, self.partials, scal, S.S_BNRM2, n=n)
        self._allreduce_slot(S.S_BNRM2)
        self._spmv_overlapped(xi, t)
        torch.sub(b[:n], t, out=r)
        torch.mul(r, dinv, out=z)
        p[:n] = z
        S.dot(r, z, self.partials, scal, S.S_RR, n=n)
        self._allreduce_slot(S.S_RR)
        S.dot(r, r, self.partials, scal, S.S_GAMMA, n=n)
        self._allreduce_slot(S.S_GAMMA)
        res.bnrm2 = math.sqrt(max(self._host_scalar(S.S_BNRM2), 0.0))
        rr = self._host_scalar(S.S_GAMMA)
        res.r0nrm2 = math.sqrt(max(rr, 0.0))
        rtol2 = max(res_atol, res_rtol * res.bnrm2) ** 2
        converged = rtol2 > 0 and rr <= rtol2
        k = 0
        while not converged and k < maxits:
            self._spmv_overlapped(p, t, fuse_dotslot=S.S_PT)
            self._allreduce_slot(S.S_PT)
            # ONE fused kernel: alpha = rz/pt (device), r/x updates,
            # z = dinv*r, next rz (-> S_RR, rotated) and true rr
            # (-> S_GAMMA) -- replaces 6 launches and ~2x the traffic
            S.pcg_fused_update(r, xi, p, t, z, dinv, scal, self.partials, n)
            self._allreduce_slot(S.S_RR)
            self._allreduce_slot(S.S_GAMMA)
            rr = self._host_scalar(S.S_GAMMA)
            k += 1
            res.niterations = k
            if not math.isfinite(rr):
                raise FloatingPointError(f"jacobi PCG diverged at it {k}")
            if rtol2 > 0 and rr <= rtol2:
                converged = True
                break
            # p = (rz/rz_prev) p + z
            S.daypx_ratio(p, z, scal, S.S_RR, S.S_RR_PREV, n=n)
        torch.cuda.synchronize(self.device)
        res.tsolve = time.perf_counter() - t0
        x.copy_(xi)
        res.rnrm2 = math.sqrt(max(rr, 0.0))
        res.converged = converged
        nnz_full = L.nnzA + L.nnzO
        self._count_work(res, cg_flops_per_iter(nnz_full, n) + 3.0 * n)
        return res

    # -- block-Jacobi PCG on Block-SELL operators (beyond reference,
    # opt-in, never auto-selected) ----------------------------------------

    def _block_inverse(self) -> torch.Tensor:
        """Packed inverse diagonal blocks of the Block-SELL matA, built on
        the GPU once per solver instance (one launch + one status read)."""
        if "bjacobi_minv" not in self._ws:
            self._ws["bjacobi_minv"] = self.opA.diag_inv()
        return self._ws["bjacobi_minv"]

    def solve_bjacobi(self, b: torch.Tensor, x: torch.Tensor,
                      maxits: int = 100, res_atol: float = 0.0,
                      res_rtol: float = 1e-9) -> SolveResult:
        """Block-Jacobi PCG: M = blockdiag of the dof x dof node blocks of
        the Block-SELL operator, inverted on the GPU at the first solve
        (file-extracted and device-generated systems alike).  The algebra
        of :meth:`solve_jacobi` with z_node = M_node^-1 r_node inside the
        fused update; the SpMV with its fused (p,t) and every reduced slot
        take the paths of the other solvers.  Convergence is tested on the
        TRUE (r,r) (S_GAMMA) through the lag-2 ring of :meth:`solve`: the
        host never blocks on an iteration's tail, and ``niterations`` is
        the first iteration whose rr met the tolerance.  Eager (no graph
        capture)."""
        minv = self._block_inverse()
        dof = self.opA.dof
        res = SolveResult(solver="cg-hip-bjacobi", maxits=maxits,
                          res_atol=res_atol, res_rtol=res_rtol,
                          nranks=self.comm.size if self.comm else 1)
        n = self.n
        S = ops
        scal = self.scal
        ws = self._workspace("bjacobi", [("r", False), ("t", False),
                                         ("z", False), ("p", True),
                                         ("xi", True)])
        r, t, z, p, xi = ws["r"], ws["t"], ws["z"], ws["p"], ws["xi"]
        xi.copy_(x)
        torch.cuda.synchronize(self.device)
        t0 = time.perf_counter()
        S.dot(b, b, self.partials, scal, S.S_BNRM2, n=n)
        self._allreduce_slot(S.S_BNRM2)
        self._spmv_overlapped(xi, t)
        torch.sub(b[:n], t, out=r)
        # z0 = M^-1 r0, rz -> S_RR, true rr -> S_GAMMA;  p0 = z0
        S.bjacobi_apply(minv, r, z, self.partials, scal, n, dof)
        self._allreduce_slot(S.S_RR)
        self._allreduce_slot(S.S_GAMMA)
        p[:n] = z
        res.bnrm2 = math.sqrt(max(self._host_scalar(S.S_BNRM2), 0.0))
        rr = self._host_scalar(S.S_GAMMA)
        res.r0nrm2 = math.sqrt(max(rr, 0.0))
        rtol2 = max(res_atol, res_rtol * res.bnrm2) ** 2
        converged = rtol2 > 0 and rr <= rtol2
        ring = LaggedReadback(1, lag=2)

        def check(j):
            """Host test of the true rr after iteration j."""
            nonlocal rr, converged
            rr = float(ring.get(j)[0])
            if not math.isfinite(rr):
                raise FloatingPointError(
                    f"block-jacobi PCG diverged: rr={rr} at it {j + 1}")
            if rtol2 > 0 and rr <= rtol2:
                converged = True
                res.niterations = j + 1
                return True
            return False

        k = 0
        cur = torch.cuda.current_stream(self.device)
        rr_slot = scal[S.S_GAMMA:S.S_GAMMA + 1]
        while not converged and k < maxits:
            if k >= ring.lag and check(k - ring.lag):
                break
            self._spmv_overlapped(p, t, fuse_dotslot=S.S_PT)
            with self.prof.span("allreduce"):
                self._allreduce_slot(S.S_PT)
            # ONE fused kernel: alpha = rz/pt (device), r/x updates,
            # z = M^-1 r, next rz (-> S_RR, rotated) and true rr (-> S_GAMMA)
            with self.prof.span("update_bjacobi"):
                S.bpcg_fused_update(r, xi, p, t, z, minv, scal,
                                    self.partials, n, dof)
            with self.prof.span("allreduce"):
                self._allreduce_slot(S.S_RR)
                self._allreduce_slot(S.S_GAMMA)
            # p = (rz/rz_prev) p + z
            with self.prof.span("daypx"):
                S.daypx_ratio(p, z, scal, S.S_RR, S.S_RR_PREV, n=n)
            ring.push(k, rr_slot, cur)
            k += 1
            res.niterations = k
        if not converged:
            for j in ring.tail(k):
                if check(j):
                    break
        torch.cuda.synchronize(self.device)
        res.tsolve = time.perf_counter() - t0
        x.copy_(xi)
        rr = self._host_scalar(S.S_GAMMA)
        res.rnrm2 = math.sqrt(max(rr, 0.0))
        res.converged = converged or (rtol2 > 0 and rr <= rtol2)
        nnz_full = self.local.nnzA + self.local.nnzO
        self._count_work(res, cg_flops_per_iter(nnz_full, n)
                         + (2.0 * dof + 2.0) * n)
        self._annotate_profile(res)
        return res

    # -- pipelined CG -----------------------------------------------------

    def solve_pipelined(self, b: torch.Tensor, x: torch.Tensor, maxits: int = 100,
                        res_atol: float = 0.0, res_rtol: float = 1e-9,
                        use_graph: bool | None = None,
                        megafuse: bool | None = None,
                        rr_period: int = 0) -> SolveResult:
        """Pipelined (Ghysels-Vanroose) CG: ONE 2-double allreduce per
        iteration, overlapped with the halo + SpMV of q = A w
        (reference acgsolverhip_solve_pipelined, cghip.c:1187-1933).

        ``use_graph``: capture the steady-state iteration into a hipGraph
        and replay it (captured once per solver, cached).  Default None =
        measured policy: OFF on one GPU (the eager 1-3 launch body is ~8
        us/it cheaper than hipGraphLaunch, profiles/RESULTS.md), ON for
        multi-GPU where the eager iteration's ~100 us of host-side c10d /
        launch work rivals the per-rank GPU time -- there the WHOLE
        iteration (side-stream allreduce fork, RCCL halo, split SpMV,
        fused update) is captured, with automatic permanent fallback to
        eager if the backend cannot capture (e.g. gloo).  Replay
        semantics: the update is enqueued before the host reads the
        previous gamma, so on the converging iteration 1-2 extra (valid)
        updates have already been applied to x; reported
        niterations/rnrm2 match the eager path.

        ``rr_period`` > 0: residual replacement (beyond reference; PETSc's
        KSPPIPECGRR idea with a fixed period).  After the update of every
        iteration k with (k + 1) % rr_period == 0 the recurrence vectors
        are recomputed from xi and p, eagerly on the solve's stream and
        outside any graph: (r, t) = (b - A xi, A p), then (w, z) =
        (A r, A t) with gamma = (r,r), delta = (w,r); gamma_prev and
        alpha_prev keep the rotation of the iteration just finished.  One
        rank without matO on SELL, sigma-SELL or BSELL takes two dual-SpMV
        launches plus a finalize; every other configuration runs the same
        algebra as four ``_spmv_overlapped`` calls and ``dot2`` (or, with
        the fast path only switched off by ``_rr_fast``, ``dot2_slices``:
        the dual kernels' summation order, same bits).  The next
        iteration's allreduce picks up the replaced local gamma/delta.
        ``nreplacements`` counts the replacements inside the reported
        iterations.  0 (default) issues exactly the launches of the plain
        solve on the plain workspaces.
        """
        if rr_period < 0:
            raise ValueError(f"rr_period must not be negative, got {rr_period}")
        rr_period = int(rr_period)
        res = SolveResult(solver="cg-hip-pipelined", maxits=maxits,
                          res_atol=res_atol, res_rtol=res_rtol,
                          nranks=self.comm.size if self.comm else 1)
        n = self.n
        S = ops
        L = self.local
        scal = self.scal
        mega = self.megafuse_auto if megafuse is None else (megafuse and self.can_megafuse)
        wskey = f"pipelined{'_mega' if mega else ''}"
        if rr_period:
            # a workspace (and graphs) of its own: t and p are SpMV inputs
            # of the replacement and carry ghost tails here
            wskey += "_rr"
        names = [("r", True), ("w", True), ("z", False),
                 ("t", bool(rr_period)), ("p", bool(rr_period)),
                 ("tmp", False), ("xi", True)]
        names += [("w2", True)] if mega else [("q", False)]
        ws = self._workspace(wskey, names)
        r, w, z, t, p, tmp, xi = (ws["r"], ws["w"], ws["z"], ws["t"],
                                  ws["p"], ws["tmp"], ws["xi"])
        # megafused path double-buffers w (SpMV gathers w_old while the
        # fused epilogue writes w_new) and stages border q in qpart;
        # the separate q vector exists only on the fallback path.
        w2 = ws.get("w2")
        q = ws.get("q")
        if mega and "qpart" not in ws:
            ws["qpart"] = torch.zeros(max(L.nborder, 1), dtype=torch.float64,
                                      device=self.device)
        qpart = ws.get("qpart")
        xi.copy_(x)
        # first=True multiplies z/t/p by beta=0: stale non-finite values
        # from an aborted earlier solve must not poison 0*x
        for v in (z, t, p):
            v.zero_()
        torch.cuda.synchronize(self.device)
        t0 = time.perf_counter()
        S.dot(b, b, self.partials, scal, S.S_BNRM2, n=n)
        self._allreduce_slot(S.S_BNRM2)
        self._spmv_overlapped(xi, tmp)
        torch.sub(b[:n], tmp, out=r[:n])
        self._spmv_overlapped(r, w)  # w = A r
        res.bnrm2 = math.sqrt(max(self._host_scalar(S.S_BNRM2), 0.0))
        rtol2 = max(res_atol, res_rtol * res.bnrm2) ** 2
        # initial local gamma/delta; per-iteration dots are fused into the
        # 6-vector update kernel, so no standalone dot pass ever runs again
        S.dot2(r, w, self.partials, scal, n)
        converged = False
        gamma_host = None
        serial = self.comm is None or self.comm.size == 1
        if use_graph is None:
            # measured policy: eager wins on one GPU (~8 us/it cheaper than
            # hipGraphLaunch); captured iterations win the host-bound
            # distributed loop (capture failure falls back to eager)
            use_graph = not serial
        graph_ok = use_graph and serial and not self.prof.enabled
        graph = self._graphs.get(wskey) if graph_ok and not mega else None
        # megafused: even/odd w ping-pong graphs
        graphs = (self._graphs.get(wskey, [None, None])
                  if graph_ok and mega else [None, None])

        pipeA, pipeO = self.operators.pipe if mega else (None, None)

        def mega_body(wa, wb, first):
            """One megafused iteration: halo(wa) || matA pass (SpMV + update
            of interior rows), then matO pass finishing border rows."""
            have_halo = not serial
            if have_halo:
                self._halo_fork(wa)
            border_base = L.ninterior if pipeO is not None else n
            nb = pipeA.pipe(border_base, wa, qpart, z, t, p, xi, r, wb, scal,
                            first, self.partials, 0, mato=False)
            if have_halo:
                self._halo_join()
            if pipeO is not None:
                nb += pipeO.pipe(L.ninterior, wa, qpart, z, t, p, xi, r, wb,
                                 scal, first, self.partials, nb, mato=True)
            S.pipelined_finalize(self.partials, nb, scal, first)

        opA = self.opA
        rr_dual_ok = (rr_period > 0 and serial and L.nnzO == 0
                      and opA.has_dual)
        rr_fast = rr_dual_ok and self._rr_fast

        def replace(wdst):
            """Residual replacement; ``wdst`` is the w buffer the next
            iteration gathers from."""
            with self.prof.span("replace"):
                if rr_fast:
                    opA.spmv2(xi, p, r, t, b=b, ncols=self.nlocal)
                    nb = opA.spmv2(r, t, wdst, z, partials=self.partials,
                                   ncols=self.nlocal)
                    S.pipelined_replace_finalize(self.partials, nb, scal)
                else:
                    self._spmv_overlapped(xi, tmp)
                    torch.sub(b[:n], tmp, out=r[:n])
                    self._spmv_overlapped(p, t)
                    self._spmv_overlapped(r, wdst)
                    self._spmv_overlapped(t, z)
                    if not rr_dual_ok:
                        S.dot2(r, wdst, self.partials, scal, n)
                    else:
                        # fast path switched off (_rr_fast): the dots in
                        # the dual kernels' summation order, so the two
                        # paths give the same gamma / delta bit for bit
                        nb = opA.dot2_slices(r, wdst, self.partials)
                        S.pipelined_replace_finalize(self.partials, nb, scal)
        # lag-1 convergence pipeline: gamma_k is copied to the host as soon
        # as its allreduce lands, but the host *reads* it one iteration
        # later -- the test still runs for every iteration, the host just
        # stays an iteration ahead of the GPU instead of blocking on each
        # iteration's tail (measured: the blocking check serializes
        # host<->GPU and costs ~8% at Queen scale).  On the detecting
        # iteration 1-2 extra (valid) updates have been applied to x;
        # reported niterations/rnrm2 correspond to the detected gamma.
        ring = LaggedReadback(1, lag=1)

        def check(j):
            """Host convergence test on gamma_j; True => converged at j."""
            nonlocal gamma_host, converged
            gamma_host = float(ring.get(j)[0])
            if j == 0:
                res.r0nrm2 = math.sqrt(max(gamma_host, 0.0))
            if not math.isfinite(gamma_host):
                raise FloatingPointError(f"pipelined CG diverged at it {j}")
            if rtol2 > 0 and gamma_host <= rtol2:
                converged = True
                res.rnrm2 = math.sqrt(max(gamma_host, 0.0))
                res.niterations = j
                return True
            return False

        ev_gd = torch.cuda.Event()
        ev_ar = torch.cuda.Event()
        # Multi-GPU graph capture: the eager distributed iteration costs
        # ~100 us of host work (c10d op lists for the halo, allreduce
        # setup, kernel launches) which rivals the GPU time per iteration
        # at 8-GPU Queen scale.  The ENTIRE steady-state iteration --
        # side-stream allreduce fork, halo send/recv, split SpMV, fused
        # update + finalize -- is captured once and replayed (RCCL
        # collectives and event forks are capturable; the 8-byte gamma
        # D2H stays outside, same-stream after the replay).  A capture
        # failure falls back to the eager path for good (_capture_dist).
        dist_key = wskey + ":dist"  # dist bodies INCLUDE the allreduce --
        dist_failed_key = wskey + ":capture_failed"  # never mix with serial
        dist_graph_ok = self._dist_capture_ok(use_graph, dist_failed_key)
        dgraph = self._graphs.get(dist_key) if dist_graph_ok and not mega else None
        dgraphs = (self._graphs.get(dist_key, [None, None])
                   if dist_graph_ok and mega else [None, None])

        # in-graph snapshot of the ALLREDUCED gamma: the replayed body both
        # allreduces gamma_{k-1} and overwrites it (finalize), so the host
        # copy after replay must read this intermediate, not scal itself --
        # otherwise each rank would test its LOCAL gamma and ranks could
        # break at different iterations (collective deadlock).
        if "gsnap" not in ws:
            ws["gsnap"] = torch.zeros(1, dtype=torch.float64,
                                      device=self.device)
        gsnap = ws["gsnap"]
        gamma = scal[S.S_GAMMA:S.S_GAMMA + 1]

        def fork_allreduce():
            """The 2-double (gamma, delta) allreduce on allred_stream,
            ordered after what the current stream has queued; ev_ar marks
            its end."""
            ev_gd.record(torch.cuda.current_stream(self.device))
            self.allred_stream.wait_event(ev_gd)
            with torch.cuda.stream(self.allred_stream):
                with self.prof.span("allreduce", self.allred_stream):
                    self._allreduce_slot(S.S_GAMMA, 2)
                ev_ar.record(self.allred_stream)

        def body_dist(wa=None, wb=None):
            """One steady-state (first=False) distributed iteration in the
            shape the capture needs (allreduce included)."""
            if mega:
                self._allreduce_slot(S.S_GAMMA, 2)
                gsnap.copy_(gamma)
                mega_body(wa, wb, False)
            else:
                fork_allreduce()
                self._spmv_overlapped(w, q)
                torch.cuda.current_stream(self.device).wait_event(ev_ar)
                gsnap.copy_(gamma)
                S.pipelined_fused(z, t, p, xi, r, w, q, scal, self.partials,
                                  n, False)

        k = 0
        cur = torch.cuda.current_stream(self.device)
        while k < maxits:
            first = (k == 0)
            g = dgraphs[k % 2] if mega else dgraph
            if g is not None and k > 0:
                # whole iteration (incl. allreduce) is in the graph
                if k >= ring.lag and check(k - ring.lag):
                    break
                g.replay()
                # same slot/value as the eager path: the ALLREDUCED
                # previous gamma, snapshotted inside the replay
                ring.push(k, gsnap, cur)
                if rr_period and (k + 1) % rr_period == 0:
                    replace((w2 if k % 2 == 0 else w) if mega else w)
                k += 1
                res.niterations = k
                continue
            # ONE 2-double allreduce per iteration (gamma,delta adjacent).
            # Multi-GPU non-megafused: the allreduce rides a dedicated side
            # stream so SpMV(q = A w) -- which does not read the scalars --
            # overlaps it; only the fused update waits (this is the point
            # of Ghysels-Vanroose pipelining: reference cghip.c:1750-1811).
            overlap_ar = (not serial) and not mega
            if overlap_ar:
                fork_allreduce()
            else:
                with self.prof.span("allreduce"):
                    self._allreduce_slot(S.S_GAMMA, 2)
            # lagged host test of the previous iteration's gamma (read
            # BEFORE issuing this iteration's copy: lag+1 buffers rotate)
            if k >= ring.lag and check(k - ring.lag):
                break
            if overlap_ar:
                # D2H of gamma chains off the allreduce, not the main stream
                # (the SpMV below must NOT wait for it -- that is the
                # overlap; only the fused update is ordered after it)
                self.copy_stream.wait_event(ev_ar)
                ring.push(k, gamma, self.copy_stream)
            else:
                # same-stream D2H (cross-stream event chains cost ~20 us
                # each in fire->launch latency; the in-order 8-byte copy
                # ~3 us) -- also makes the gamma-overwrite race impossible
                # by ordering
                ring.push(k, gamma, cur)
            if mega:
                wa, wb = (w, w2) if k % 2 == 0 else (w2, w)
                g = graphs[k % 2]
                if g is not None and k > 0:  # graphs are first=False bodies
                    g.replay()
                else:
                    mega_body(wa, wb, first)
                    if graph_ok and graphs[k % 2] is None and k in (2, 3):
                        gg = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(gg):
                            mega_body(wa, wb, False)
                        graphs[k % 2] = gg
                        self._graphs[wskey] = graphs
            elif graph is not None and k > 0:
                graph.replay()
            else:
                self._spmv_overlapped(w, q)
                if overlap_ar:
                    # the fused update reads gamma/delta (allreduce) and its
                    # finalize overwrites them (in-flight D2H copy): order
                    # after both
                    cur.wait_event(ev_ar)
                    cur.wait_event(ring.event(k))
                with self.prof.span("update"):
                    S.pipelined_fused(z, t, p, xi, r, w, q, scal, self.partials,
                                      n, first)
                if graph_ok and graph is None and k == 2:
                    # steady state (first=False): capture SpMV + fused update
                    graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graph):
                        self._spmv_overlapped(w, q)
                        S.pipelined_fused(z, t, p, xi, r, w, q, scal,
                                          self.partials, n, False)
                    self._graphs[wskey] = graph
            if dist_graph_ok and not self._graphs.get(dist_failed_key):
                if mega and k in (2, 3) and dgraphs[k % 2] is None:
                    dgraphs[k % 2] = self._capture_dist(
                        lambda: body_dist(wa, wb), dist_failed_key)
                    if dgraphs[k % 2] is not None:
                        self._graphs[dist_key] = dgraphs
                elif not mega and k == 2 and dgraph is None:
                    dgraph = self._capture_dist(body_dist, dist_failed_key)
                    if dgraph is not None:
                        self._graphs[dist_key] = dgraph
            if rr_period and (k + 1) % rr_period == 0:
                replace((w2 if k % 2 == 0 else w) if mega else w)
            k += 1
            res.niterations = k
        if not converged:
            # drain the lagged checks for the tail iterations
            for j in ring.tail(maxits):
                if check(j):
                    break
        torch.cuda.synchronize(self.device)
        res.tsolve = time.perf_counter() - t0
        x.copy_(xi)
        if not converged and gamma_host is not None:
            res.rnrm2 = math.sqrt(max(gamma_host, 0.0))
        res.converged = converged
        nnz_full = self.local.nnzA + self.local.nnzO
        if rr_period:
            res.nreplacements = res.niterations // rr_period
        self._count_work(res, cg_flops_per_iter(nnz_full, n) + 8.0 * n,
                         res.nreplacements * replacement_flops(nnz_full, n))
        self._annotate_profile(res)
        return res
