"""The operator formats of the HIP solver: which format a system gets, its
upload, and every call into the SpMV family of the ops layer.

One small class per kernel family.  Each holds its device tensors and
applies itself with ``apply(x, y, accum=, dot_accum=, partials=, scal=,
dotslot=)``; the same classes serve matO through ``rowbase`` and
``accum=True``.  What only some formats can do (SpMM, the dual SpMV, the
megafused pass, fp32-stored values, the Block-SELL extras, the one-launch
device CG) is a capability: :class:`Operator` says "not offered" and a
format overrides what it has, so the solver asks the operator and never
asks which format it is.

:func:`choose_formats` runs the format ladder on host arrays only;
:func:`build_operators` uploads its result and fills the solver's three
roles (:class:`OperatorSet`).  The ops backend is a parameter: ``gpu_ops``
in the solver, ``torch_ref`` (same names and signatures) to drive this
dispatch code on the CPU.
"""

from __future__ import annotations

import copy
import inspect
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

from ..ops.gpu_ops import build_row_bins, build_sellcsr_hybrid, pick_lanes
from ..ops.symtile import bsell_st_build
from ..ops.torch_ref import bsell_from_csr, sell_from_csr
from ..utils.errors import AcgError, ErrCode

# Whether a solver builds BSELL-ST without being asked (force_format or
# ACG_BSELL_ST=1); set from the interleaved measurement in
# profiles/symtile.md.
BSELL_ST_DEFAULT = True

# formats whose values may be stored in fp32 (same element order, so the
# cast is the whole pack step)
FP32_FORMATS = ("sell", "sigma", "bsell")


class Operator:
    """What every format answers.  The defaults mean "not offered"."""

    fmt = "csr"                # the format; see name
    generated = False          # built on the device by gen.device_slab
    idx_bytes_per_nnz = None   # profile annotation; None = 4 B columns
    st = None                  # BSELL-ST twin of the serial classic solve
    has_spmm = False           # spmm() and spmm_kmax()
    has_dual = False           # spmv2() and dot2_slices()
    has_daypx = False          # spmv_daypx()
    can_pipe = False           # pipe(): the megafused pipelined pass
    can_cg_device = False      # cg_device()

    def __init__(self, ops, device, nrows: int, rowbase: int = 0):
        self.ops, self.device = ops, device
        self.nrows, self.rowbase = nrows, rowbase
        self._fp32 = None

    @property
    def name(self) -> str:
        """CGSolverHIP._format_name(): the format, except that a
        device-generated operator says only that (and is thereby refused
        where a format is asked for by name, e.g. fp32 storage)."""
        return "device-generated" if self.generated else self.fmt

    def spmm_kmax(self, group: int) -> int:
        return 0

    def fp32(self):
        """This operator on fp32-stored values, built on first use: same
        index tensors, ``vals.to(float32)``.  The fp64 operator is KEPT --
        refinement needs the exact residual -- so both value sets are held
        (1.5x the value memory)."""
        if self._fp32 is None:
            if self.nrows == 0:  # rank without rows
                vals32 = torch.empty(0, dtype=torch.float32, device=self.device)
            elif self.name not in FP32_FORMATS:
                raise ValueError(
                    f"the fp32-stored operator needs the SELL, sigma-SELL or "
                    f"BSELL format; this system uses {self.name}")
            else:
                vals32 = self.vals.to(torch.float32)
            self._fp32 = copy.copy(self)
            self._fp32.vals = vals32
        return self._fp32

    def diag_inv(self):
        raise AcgError(ErrCode.NOT_SUPPORTED,
                       "block Jacobi needs a Block-SELL operator (dense "
                       "dof x dof node blocks, dof 2/3/4); this system "
                       f"uses {self.name}")


class Stencil(Operator):
    """Matrix-free dof=1 stencil (ops/kernels.hip k_stencil_spmv): reads no
    matrix data.  ``accum=True`` is the matO pass (the ghost couplings of
    rows ``rowbase``..), which is what accumulating means here."""

    fmt = "matrix-free"
    idx_bytes_per_nnz = -8.0  # no vals (8 B) and no cols read
    can_pipe = True

    def __init__(self, ops, device, mf, nrows: int, rowbase: int = 0):
        super().__init__(ops, device, nrows, rowbase)
        self.mf = mf

    def apply(self, x, y, *, accum=False, dot_accum=True, partials=None,
              scal=None, dotslot=-1):
        self.ops.stencil_spmv(self.mf, self.nrows, self.rowbase, x, y,
                              mato=accum, partials=partials, scal=scal,
                              dotslot=dotslot, dot_accum=dot_accum)

    def pipe(self, border_base, wa, qpart, z, t, p, x, r, wb, scal, first,
             partials, partials_off, mato):
        return self.ops.stencil_pipe(self.mf, self.nrows, self.rowbase,
                                     border_base, wa, qpart, z, t, p, x, r,
                                     wb, scal, first, partials, partials_off,
                                     mato=mato)


class Bsell(Operator):
    """Block-SELL: dense dof x dof node blocks, dof 2/3/4."""

    fmt = "bsell"  # classic_format says whether solve() takes bsell-st
    has_spmm = has_dual = has_daypx = True

    def __init__(self, ops, device, bptr, bcol, vals, dof: int, nrows: int):
        super().__init__(ops, device, nrows)
        self.bptr, self.bcol, self.vals, self.dof = bptr, bcol, vals, dof
        self.nnodes = nrows // dof
        self.idx_bytes_per_nnz = 4.0 / dof ** 2

    @property
    def arrays(self):
        return self.bptr, self.bcol, self.vals, self.dof

    def apply(self, x, y, *, accum=False, dot_accum=True, partials=None,
              scal=None, dotslot=-1):
        self.ops.spmv_bsell(self.bptr, self.bcol, self.vals, self.nnodes,
                            self.dof, x, y, partials=partials, scal=scal,
                            dotslot=dotslot, dot_accum=dot_accum)

    def apply_st(self, x, y, *, dot_accum=True, partials=None, scal=None,
                 dotslot=-1):
        """The same product on the BSELL-ST twin, x and y in its order."""
        self.ops.spmv_bsell_st(self.st, x, y, partials=partials, scal=scal,
                               dotslot=dotslot, dot_accum=dot_accum)

    def spmv_daypx(self, pold, r, pnew, y, scal, partials, dotslot):
        self.ops.spmv_bsell_daypx(self.bptr, self.bcol, self.vals,
                                  self.nnodes, self.dof, pold, r, pnew, y,
                                  scal, partials, dotslot)

    def spmm_kmax(self, group: int) -> int:
        """Largest kernel-level K <= group (a (dof, K) pair may be refused
        by the op layer); 0 when there is none."""
        return max((k for k in self.ops.MULTI_K if k <= group
                    and self.ops.spmm_bsell_supported(self.dof, k)), default=0)

    def spmm(self, X, Y, **fuse):
        self.ops.spmm_bsell(self.bptr, self.bcol, self.vals, self.nnodes,
                            self.dof, X, Y, **fuse)

    def spmv2(self, x1, x2, y1, y2, **kw):
        return self.ops.spmv2_bsell(self.bptr, self.bcol, self.vals,
                                    self.nnodes, self.dof, x1, x2, y1, y2, **kw)

    def dot2_slices(self, r, w, partials):
        return self.ops.dot2_slices(r, w, self.nnodes, self.dof, partials)

    def diag_inv(self):
        """Packed inverse diagonal blocks, built on the GPU (one launch +
        one status read)."""
        minv, nbad = self.ops.bsell_diag_inv(self.bptr, self.bcol, self.vals,
                                             self.nnodes, self.dof)
        if nbad > 0:
            raise AcgError(ErrCode.INVALID_VALUE,
                           f"block Jacobi: {nbad} nodes have a missing "
                           f"or not positive definite diagonal block")
        return minv


class Sell(Operator):
    """SELL-C-64; ``perm`` (SELL row -> matrix row) makes it sigma-SELL."""

    has_spmm = has_dual = True

    def __init__(self, ops, device, sellptr, cols, vals, nrows: int,
                 perm=None, rowbase: int = 0):
        super().__init__(ops, device, nrows, rowbase)
        self.sellptr, self.cols, self.vals, self.perm = sellptr, cols, vals, perm
        self.fmt = "sell" if perm is None else "sigma"
        # the megafused pass and the device CG take int32 columns in
        # matrix row order
        self.can_pipe = perm is None and cols.dtype == torch.int32
        self.can_cg_device = perm is None

    @property
    def arrays(self):
        return self.sellptr, self.cols, self.vals

    def apply(self, x, y, *, accum=False, dot_accum=True, partials=None,
              scal=None, dotslot=-1):
        self.ops.spmv_sell(self.sellptr, self.cols, self.vals, self.nrows,
                           x, y, rowbase=self.rowbase, accum=accum,
                           perm=self.perm, partials=partials, scal=scal,
                           dotslot=dotslot, dot_accum=dot_accum)

    def pipe(self, border_base, wa, qpart, z, t, p, x, r, wb, scal, first,
             partials, partials_off, mato):
        return self.ops.sell_pipe(self.sellptr, self.cols, self.vals,
                                  self.nrows, self.rowbase, border_base, wa,
                                  qpart, z, t, p, x, r, wb, scal, first,
                                  partials, partials_off, mato=mato)

    def spmm_kmax(self, group: int) -> int:
        return max((k for k in self.ops.MULTI_K if k <= group), default=0)

    def spmm(self, X, Y, **fuse):
        self.ops.spmm_sell(self.sellptr, self.cols, self.vals, self.nrows,
                           X, Y, perm=self.perm, **fuse)

    def spmv2(self, x1, x2, y1, y2, **kw):
        return self.ops.spmv2_sell(self.sellptr, self.cols, self.vals,
                                   self.nrows, x1, x2, y1, y2,
                                   perm=self.perm, **kw)

    def dot2_slices(self, r, w, partials):
        return self.ops.dot2_slices(r, w, self.nrows, 1, partials,
                                    perm=self.perm)

    def cg_device(self, b, x, r, p, t, scal, partials, out2, barrier_state,
                  maxits, res_atol, res_rtol):
        self.ops.cg_device(self.sellptr, self.cols, self.vals, self.nrows, b,
                           x, r, p, t, scal, partials, out2, barrier_state,
                           maxits, res_atol, res_rtol)


class Csr(Operator):
    """Plain CSR-vector, ``lanes`` lanes per row."""

    def __init__(self, ops, device, rowptr, colidx, vals, lanes: int,
                 rowbase: int = 0):
        super().__init__(ops, device, rowptr.numel() - 1, rowbase)
        self.rowptr, self.colidx, self.vals = rowptr, colidx, vals
        # lanes only schedule rows on the GPU; torch_ref.spmv has no such
        # parameter (the one SpMV-family signature that differs)
        takes = "lanes" in inspect.signature(ops.spmv).parameters
        self.lanes = {"lanes": lanes} if takes else {}

    def apply(self, x, y, *, accum=False, dot_accum=True, partials=None,
              scal=None, dotslot=-1):
        self.ops.spmv(self.rowptr, self.colidx, self.vals, x, y,
                      rowbase=self.rowbase, accum=accum, partials=partials,
                      scal=scal, dotslot=dotslot, dot_accum=dot_accum,
                      **self.lanes)


class Binned(Operator):
    """Row-binned CSR: ``rowlist`` (longest first) and ``bins`` schedule the
    rows of a CSR that stays on the device."""

    fmt = "binned"

    def __init__(self, ops, device, csr, rowlist, bins, rowbase: int = 0):
        super().__init__(ops, device, csr[0].numel() - 1, rowbase)
        self.rowptr, self.colidx, self.vals = csr
        self.rowlist, self.bins = rowlist, bins

    def apply(self, x, y, *, accum=False, dot_accum=True, partials=None,
              scal=None, dotslot=-1):
        self.ops.spmv_binned(self.rowptr, self.colidx, self.vals,
                             self.rowlist, self.bins, x, y,
                             rowbase=self.rowbase, accum=accum,
                             partials=partials, scal=scal, dotslot=dotslot,
                             dot_accum=dot_accum)


class Hybrid(Operator):
    """SELL+CSR split: short rows as sigma-SELL, the long tail row-binned.
    Either part may be empty (``None``).  The row sets are disjoint, so
    both parts write y in the caller's mode; the fused dot of the binned
    part ACCUMULATES on top of the SELL part's."""

    def __init__(self, sell: Sell | None, binned: Binned | None, nrows: int):
        part = sell or binned
        super().__init__(part.ops if part else None,
                         part.device if part else None, nrows)
        self.sell, self.binned = sell, binned
        self.fmt = "binned" if sell is None else "hybrid"

    def apply(self, x, y, *, accum=False, dot_accum=True, partials=None,
              scal=None, dotslot=-1):
        if self.sell is not None:
            self.sell.apply(x, y, accum=accum, dot_accum=dot_accum,
                            partials=partials, scal=scal, dotslot=dotslot)
        if self.binned is not None:
            self.binned.apply(x, y, accum=accum,
                              dot_accum=dot_accum or self.sell is not None,
                              partials=partials, scal=scal, dotslot=dotslot)


# -- construction -----------------------------------------------------------

def choose_formats(L, force: str | None, use_sell: bool) -> SimpleNamespace:
    """Choose the matA operator format of a host-CSR system and build it on
    host arrays; no device is touched, though the numpy builders it calls
    live in gpu_ops, which imports the compiled extension (reference
    analog: the choice between hipsparse ALG_DEFAULT and the hand
    merge-path kernel, cghip.c:533-585 / cg-kernels-hip.hip:348).

    Auto ladder by measured fit:
      1. plain SELL-C-64 when padding waste <= 0.3 (stencil/FEM rows),
      2. sigma-SELL (window 16) when waste <= 0.5 (mildly irregular),
      3. row-binned hybrid CSR otherwise (power-law rows; MEASURED on
         MI355X 1M-row power-law: hybrid 665 us/it vs single-lane CSR
         855 vs wide-sigma SELL 2627 -- slice-length imbalance makes
         wide sigma lose badly, so it is force-only),
    plus Block-SELL whenever dense dof x dof block structure is found
    (density >= 0.75) -- it wins on index bytes.
    ``force`` in {csr, sell, sigma, bsell, hybrid, binned} overrides for A/B
    measurement (bench --format).

    Returns host arrays or None per field: ``sell`` (sellptr, cols, vals,
    perm), ``sellO`` (sellptr, cols, vals), ``bsell`` (bptr, bcol, bvals,
    dof), ``hybrid`` (sellptr, cols, svals, perm, rowlist, bins; sellptr
    None without short rows), ``binned`` (rowlist, bins) and ``binnedO``."""
    h = SimpleNamespace(sell=None, sellO=None, bsell=None, hybrid=None,
                        binned=None, binnedO=None)
    if L.nowned == 0:
        return h

    def mk_hybrid():
        """SELL+CSR split (short rows SELL, long tail binned CSR).
        MEASURED (MI355X 1M-row power-law): the pure binned hybrid's
        4/8-lane short-row bins cost 400 us/it of its 587 us SpMV --
        SELL's lockstep 512 B line loads serve those rows instead.
        Costs ~1.75x operator memory (CSR kept for the long rows).
        ACG_HYBRID_CUT overrides the split length (tuning sweeps)."""
        cut = int(os.environ.get("ACG_HYBRID_CUT", "192"))
        window = int(os.environ.get("ACG_HYBRID_WINDOW", "0"))
        bucket = int(os.environ.get("ACG_HYBRID_BUCKET", "8"))
        h.hybrid = build_sellcsr_hybrid(L.A_rowptr, L.A_colidx, L.A_vals,
                                        cut=cut, window=window, bucket=bucket)
        if L.nnzO > 0:
            # matO rows inherit the same power-law tail: bin them too
            h.binnedO = build_row_bins(L.O_rowptr)

    def mk_sell(sigma):
        out = sell_from_csr(L.A_rowptr, L.A_colidx, L.A_vals, sigma=sigma)
        h.sell = tuple(out) if sigma > 1 else (*out, None)
        if L.nnzO > 0:
            h.sellO = sell_from_csr(L.O_rowptr, L.O_colidx, L.O_vals)
        return (int(h.sell[0][-1]) - L.nnzA) / max(L.nnzA, 1)

    def mk_bsell():
        for dof_try in (4, 3, 2):  # kernel dispatch covers 2/3/4
            out = bsell_from_csr(L.A_rowptr, L.A_colidx, L.A_vals, dof_try)
            if out is not None and out[3] >= 0.75:
                h.bsell = (*out[:3], dof_try)
                return True
        return False

    if force == "csr":
        pass
    elif force == "hybrid":
        mk_hybrid()
    elif force == "binned":
        h.binned = build_row_bins(L.A_rowptr)
    elif force == "sell":
        mk_sell(1)
    elif force == "sigma":
        mk_sell(4096)
    elif force in ("bsell", "bsell-st"):
        if not mk_bsell():
            raise ValueError(f"force_format={force}: no dense dof x dof "
                             "block structure (density < 0.75)")
    elif use_sell:  # auto ladder
        if mk_sell(1) > 0.3:
            h.sell = h.sellO = None
            if mk_sell(16) > 0.5:
                h.sell = h.sellO = None
                mk_hybrid()
        mk_bsell()
    return h


class OperatorSet:
    """The operators of one solver, by role:

    ``A``     what ``_spmv_overlapped`` applies to the owned columns, by
              priority matrix-free, BSELL, SELL, hybrid / binned, CSR;
    ``O``     the ghost-column pass (stencil, SELL-O, binned-O or CSR-O), or
              None without matO entries;
    ``sell``, ``sellO``  the SELL operators, or None.  Where ``A`` is BSELL
              (auto ladder, device-generated slabs) or matrix-free these are
              COPIES kept next to it, and the paths that exist only for SELL
              run on them: ``pipe`` and ``device_cg``;
    ``pipe``  (matA, matO or None) operators of the megafused pipelined
              pass, or None where it is not offered: the stencils, else
              unpermuted int32-column SELL on both sides;
    ``pipe_auto``  whether that pass is the default (see build_operators);
    ``device_cg``  the unpermuted SELL of the one-launch CG, or None;
    ``bsell``, ``hybrid``  A's candidates of those families, or None;
    ``csrA``, ``csrO``  the CSR triples still on the device, or None."""

    A = O = sell = sellO = bsell = hybrid = pipe = device_cg = None
    csrA = csrO = None
    pipe_auto = False
    lanesA = lanesO = 16


def build_operators(L, force: str | None, use_sell: bool, lanes: int | None,
                    matfree: bool, device, serial: bool = True,
                    ops=None) -> OperatorSet:
    """(LocalSystem, options) -> the solver's operators on ``device``,
    calling into the ``ops`` backend (default gpu_ops)."""
    if ops is None:
        from ..ops import gpu_ops as ops
    device = torch.device(device)
    s = OperatorSet()
    n = L.nowned
    s.lanesA = s.lanesO = lanes or 16

    def up(a):
        t = torch.from_numpy(np.ascontiguousarray(a))
        return t.to(device, non_blocking=True)

    def ups(arrs):
        return [up(a) for a in arrs]

    mf = None
    if matfree:
        mf = getattr(L, "mf_tables", None)
        if mf is None:
            raise ValueError(
                "matfree=True needs a device-generated dof=1 stencil "
                "system (gen.device_slab with spec dof==1)")
    generated = hasattr(L, "A_sell")
    if generated:
        # device-generated system (gen.device_slab): SELL already in HBM
        if L.A_sell is not None:
            s.sell = Sell(ops, device, *L.A_sell, n)
            s.sell.generated = True
        if L.O_sell is not None:
            s.sellO = Sell(ops, device, *L.O_sell, L.nborder,
                           rowbase=L.ninterior)
        if getattr(L, "A_bsell", None) is not None:
            s.bsell = Bsell(ops, device, *L.A_bsell, n)
            s.bsell.generated = True
        if s.sell is None and mf is None:
            raise ValueError("system generated with operator=False "
                             "requires matfree=True")
    else:
        s.csrA = ups((L.A_rowptr, L.A_colidx, L.A_vals))
        s.csrO = ups((L.O_rowptr, L.O_colidx, L.O_vals))
        s.lanesA = lanes or pick_lanes(L.nnzA / max(L.nowned, 1))
        s.lanesO = lanes or pick_lanes(L.nnzO / max(L.nborder, 1))
        h = choose_formats(L, force, use_sell)
        if h.sell is not None:
            perm = up(h.sell[3]) if h.sell[3] is not None else None
            s.sell = Sell(ops, device, *ups(h.sell[:3]), n, perm)
        if h.sellO is not None:
            s.sellO = Sell(ops, device, *ups(h.sellO), L.nborder,
                           rowbase=L.ninterior)
        if h.hybrid is not None:
            sellptr, cols, svals, perm, rowlist, bins = h.hybrid
            s.hybrid = Hybrid(
                Sell(ops, device, *ups((sellptr, cols, svals)), n, up(perm))
                if sellptr is not None else None,
                Binned(ops, device, s.csrA, up(rowlist), bins)
                if len(rowlist) else None, n)
        if h.binned is not None:
            s.hybrid = Binned(ops, device, s.csrA, up(h.binned[0]),
                              h.binned[1])
        if h.bsell is not None:
            s.bsell = Bsell(ops, device, *ups(h.bsell[:3]), h.bsell[3], n)
        if s.sell is not None or s.bsell is not None:
            s.csrA = None  # free CSR
    # role A, by priority
    if mf is not None:
        s.A = Stencil(ops, device, mf, n)
    else:
        s.A = s.bsell or s.sell or s.hybrid \
            or Csr(ops, device, *s.csrA, s.lanesA)
    # role O
    if L.nborder > 0 and L.nnzO > 0:
        if mf is not None:
            s.O = Stencil(ops, device, mf, L.nborder, L.ninterior)
        elif s.sellO is not None:
            s.O = s.sellO
        elif not generated and h.binnedO is not None:
            s.O = Binned(ops, device, s.csrO, up(h.binnedO[0]), h.binnedO[1],
                         rowbase=L.ninterior)
        else:
            s.O = Csr(ops, device, *s.csrO, s.lanesO, rowbase=L.ninterior)
    # the megafused pipelined iteration needs its pass on both sides.
    # Measured on MI355X: for wide rows (~80 nnz, Queen-shaped) the fused
    # epilogue's 6 vector streams cost the SpMV more x-gather locality
    # than the saved q round-trip is worth (815us fused vs 805us split);
    # for narrow rows (7-pt Poisson) the q elimination is ~8% of the
    # iteration's traffic.  Auto-enable below ~16 nnz/row.  Matrix-free:
    # megafusion always pays (the SpMV reads no matrix, so the
    # vector-traffic saving has no x-gather-locality cost to trade)
    if mf is not None:
        s.pipe, s.pipe_auto = (s.A, s.O), True
    elif (s.sell is not None and s.sell.can_pipe
          and (L.nnzO == 0 or (s.sellO is not None and s.sellO.can_pipe))):
        s.pipe = (s.sell, s.sellO if L.nnzO > 0 else None)
        s.pipe_auto = L.nnzA / max(L.nowned, 1) <= 16.0
    if s.sell is not None and s.sell.can_cg_device:
        s.device_cg = s.sell
    _build_symtile(s, L, force, serial, mf is not None)
    return s


def _build_symtile(s: OperatorSet, L, force: str | None, serial: bool,
                   matfree: bool) -> None:
    """Build BSELL-ST next to BSELL where the classic solve can use it:
    one rank, no matO, a bsell operator, no other format forced.  The
    builder's own gate (exact transposes inside a tile, padded bytes
    <= 0.9 of BSELL's) decides; a refusal keeps BSELL, except under
    ``force_format="bsell-st"``, which raises.  Without the force the
    format is built when BSELL_ST_DEFAULT or ACG_BSELL_ST=1 says so;
    ACG_BSELL_ST=0 is the kill switch."""
    env = os.environ.get("ACG_BSELL_ST", "")
    wanted = force == "bsell-st" or (
        force is None and (env == "1" or (BSELL_ST_DEFAULT and env != "0")))
    st = None
    if (wanted and env != "0" and serial and L.nnzO == 0
            and s.bsell is not None and not matfree):
        b = s.bsell
        st = b.st = bsell_st_build(b.bptr, b.bcol, b.vals, b.nnodes, b.dof,
                                   getattr(L, "node_order", None))
        if st is not None:
            print(f"# classic CG operator format: bsell-st "
                  f"({st.ratio:.3f} of the bsell bytes)",
                  file=sys.stderr, flush=True)
    if force == "bsell-st" and st is None:
        raise ValueError(
            "force_format=bsell-st: not built (needs one rank, no matO, "
            "ACG_BSELL_ST != 0, exact transposes inside every tile and "
            "stored bytes <= 0.9 of BSELL's)")
