"""The solver's operator module driven on the CPU with the torch_ref
kernels: format choice, the matA + matO dispatch with its fused dot,
capabilities and refusals.

Reference: kernel_oracle's high-precision SpMV of the ORIGINAL CSR (matA
plus matO rows), bound ``(L_i + 48) * 2^-53 * M_i`` with L_i the row's
nonzero count in matA and matO -- SELL / BSELL padding only adds exact
zeros, so the row's own products are all that round.  The fused dot is
checked against ``ko.dot`` with the tolerance it propagates from that bound.
"""

from types import SimpleNamespace

import numpy as np
import pytest
import torch

import kernel_oracle as ko
from acg_amd.gen import STENCIL_7PT_3D, queen_like_spec, stencil_local_slab
from acg_amd.gen.irregular import powerlaw_spd
from acg_amd.ops import torch_ref
from acg_amd.part import extract_subdomains, partition_rows
from acg_amd.solvers import operator as opm

SLOT = torch_ref.S_PT


def _powerlaw(nparts):
    A = powerlaw_spd(600, mean_nnz=12, clip=48, seed=4)
    part = partition_rows(A, nparts, method="ml", seed=1) if nparts > 1 \
        else partition_rows(A, 1)
    return extract_subdomains(A, part, nparts, only_parts=[0])[0]


SYSTEMS = {
    "stencil": lambda: stencil_local_slab(6, 5, 4, dict(STENCIL_7PT_3D), 0, 1),
    "slab3": lambda: stencil_local_slab(5, 4, 3, queen_like_spec(3), 0, 1),
    "powerlaw": lambda: _powerlaw(1),
    "stencil/2": lambda: stencil_local_slab(6, 5, 4, dict(STENCIL_7PT_3D), 0, 2),
    "powerlaw/2": lambda: _powerlaw(2),
}
EXTRA = {"slab3-8x8x4": lambda: stencil_local_slab(8, 8, 4, queen_like_spec(3), 0, 1)}
_cache = {}


def system(name):
    """(LocalSystem, x with a hand-filled ghost tail, oracle), built once
    and shared."""
    if name not in _cache:
        L = {**SYSTEMS, **EXTRA}[name]()
        rng = np.random.default_rng(7)
        x = rng.standard_normal(L.nowned + L.nghost)
        xh = ko.hp(x)
        y, M = ko.spmv(L.A_rowptr, L.A_colidx, L.A_vals, xh)
        Ln = np.diff(L.A_rowptr).astype(np.float64)
        dot, tol = ko.dot(xh[:L.nowned], y, tb=ko.bound(M, Ln))
        if L.nnzO > 0:
            b = slice(L.ninterior, L.ninterior + L.nborder)
            yO, MO = ko.spmv(L.O_rowptr, L.O_colidx, L.O_vals, xh)
            LO = np.diff(L.O_rowptr).astype(np.float64)
            dO, tO = ko.dot(xh[b], yO, tb=ko.bound(MO, LO))
            y[b] += yO
            M[b] += MO
            Ln[b] += LO
            dot, tol = dot + dO, tol + tO
        e = ko.Expect("operator")
        e.add("y", y, M, Ln)
        e.add_tol("dot", dot, tol)
        _cache[name] = (L, x, e)
    return _cache[name]


def build(name, force, **kw):
    L, _, _ = system(name)
    return opm.build_operators(L, force, True, None, False, "cpu",
                               ops=torch_ref, **kw)


def run(name, s):
    """The solver's two passes (matA overwrites y and the dot slot, matO
    accumulates into both) on a NaN-poisoned y and slot."""
    L, x, _ = system(name)
    xt = torch.from_numpy(x)
    y = torch.full((L.nowned,), float("nan"), dtype=torch.float64)
    scal = torch.full((torch_ref.S_NSLOTS,), float("nan"), dtype=torch.float64)
    partials = torch.zeros(2 * torch_ref.MAXG, dtype=torch.float64)
    fuse = dict(partials=partials, scal=scal, dotslot=SLOT)
    s.A.apply(xt, y, accum=False, dot_accum=False, **fuse)
    if s.O is not None:
        s.O.apply(xt, y, accum=True, dot_accum=True, **fuse)
    return {"y": y.numpy(), "dot": scal[SLOT].item()}


# format -> the systems it can be forced on (None = the auto ladder)
CASES = [(f, n) for f, names in {
    "sell": SYSTEMS, "sigma": SYSTEMS, "hybrid": SYSTEMS, "binned": SYSTEMS,
    "csr": SYSTEMS, None: SYSTEMS, "bsell": ("slab3",)}.items() for n in names]
AUTO_NAME = {"stencil": ("sell",), "stencil/2": ("sell",), "slab3": ("bsell",),
             "powerlaw": ("sigma", "hybrid"), "powerlaw/2": ("sigma", "hybrid")}


@pytest.mark.parametrize("force,name", CASES)
def test_formats_apply_and_name(force, name, monkeypatch):
    monkeypatch.setenv("ACG_HYBRID_CUT", "16")
    s = build(name, force)
    L, _, expect = system(name)
    want = AUTO_NAME[name] if force is None else (force,)
    if force == "hybrid" and np.diff(L.A_rowptr).min() > 16:
        want = ("binned",)  # no row short enough for the SELL part
    assert s.A.name in want
    assert (s.O is not None) == (L.nnzO > 0)
    if s.A.name == "hybrid" and name.startswith("powerlaw"):
        assert s.A.sell is not None and s.A.binned is not None
        assert 0 < s.A.binned.rowlist.numel() < L.nowned
    if force in ("hybrid", "binned") and L.nnzO > 0:
        assert s.O.name == ("binned" if force == "hybrid" else "csr")
    ko.assert_accepts(expect, run(name, s), f"{force}/{name}")


def test_mutants_are_rejected(monkeypatch):
    """The checks above see a hybrid whose binned part overwrites the dot
    and a matO pass that overwrites y."""
    monkeypatch.setenv("ACG_HYBRID_CUT", "16")
    s = build("powerlaw/2", "hybrid")
    _, _, expect = system("powerlaw/2")
    assert ko.accepts(expect, run("powerlaw/2", s))
    binned_apply = opm.Binned.apply
    with monkeypatch.context() as m:
        m.setattr(opm.Binned, "apply", lambda self, x, y, **kw: binned_apply(
            self, x, y, **{**kw, "dot_accum": kw["accum"]}))
        rs = ko.ratios(expect, run("powerlaw/2", s))
        assert rs["dot"] > 1.0 and rs["y"] <= 1.0
    s = build("stencil/2", None)
    _, _, expect = system("stencil/2")
    sell_apply = opm.Sell.apply
    with monkeypatch.context() as m:
        m.setattr(opm.Sell, "apply", lambda self, x, y, **kw: sell_apply(
            self, x, y, **{**kw, "accum": False}))
        rs = ko.ratios(expect, run("stencil/2", s))
        assert rs["y"] > 1.0


def test_solver_hybrid_view(monkeypatch):
    """``solver.hybrid`` stays the dict it was: the property is evaluated on
    a stand-in that has the two attributes it reads."""
    from acg_amd.solvers.hip import CGSolverHIP

    def view(s):
        return CGSolverHIP.hybrid.fget(SimpleNamespace(operators=s, opO=s.O))
    monkeypatch.setenv("ACG_HYBRID_CUT", "16")
    h = view(build("powerlaw/2", "hybrid"))
    assert all(h[k] is not None for k in ("sellptr", "cols", "svals", "perm",
                                          "rowlist", "rowlistO"))
    assert h["bins"] and h["binsO"]
    h = view(build("powerlaw/2", "binned"))
    assert h["sellptr"] is None and h["perm"] is None
    assert h["rowlist"] is not None and "rowlistO" not in h
    assert view(build("powerlaw/2", "sigma")) is None


def test_ladder_on_host_arrays():
    """choose_formats touches no device."""
    L = system("stencil")[0]
    h = opm.choose_formats(L, None, True)
    assert h.sell is not None and h.sell[3] is None  # plain SELL
    assert h.bsell is None and h.hybrid is None
    h = opm.choose_formats(system("powerlaw")[0], None, True)
    assert h.hybrid is not None or (h.sell is not None and h.sell[3] is not None)
    h = opm.choose_formats(system("slab3")[0], None, True)
    assert h.sell is not None and h.bsell is not None and h.bsell[3] == 3
    assert opm.choose_formats(L, None, False).sell is None  # use_sell=False
    with pytest.raises(ValueError, match=r"force_format=bsell: no dense dof x "
                       r"dof block structure \(density < 0.75\)"):
        opm.choose_formats(L, "bsell", True)
    empty = SimpleNamespace(nowned=0)
    assert all(v is None for v in vars(
        opm.choose_formats(empty, None, True)).values())


def test_roles_and_sell_twin():
    """The dof-3 slab runs on BSELL and keeps a SELL copy for the megafused
    pass and the one-launch CG; megafusion is the default only for narrow
    rows."""
    s = build("slab3", None)  # so small that its SELL copy is sigma-sorted
    assert s.A is s.bsell and s.sell.perm is not None and s.csrA is None
    assert s.pipe is None and s.device_cg is None
    assert s.A.st is not None  # one rank, no matO: BSELL-ST next to it
    assert build("slab3", None, serial=False).A.st is None
    s = build("slab3-8x8x4", None)  # the flagship's shape: plain SELL copy
    assert s.A is s.bsell and s.A.name == "bsell"
    assert s.pipe == (s.sell, None) and not s.pipe_auto
    assert s.device_cg is s.sell
    s = build("stencil", None)
    assert s.A is s.sell and s.pipe == (s.sell, None) and s.pipe_auto
    s = build("stencil/2", None)
    assert s.pipe == (s.sell, s.sellO) and s.O is s.sellO
    assert s.sellO.rowbase == system("stencil/2")[0].ninterior
    for force in ("sigma", "bsell", "hybrid", "csr"):
        s = build("slab3", force)
        assert s.pipe is None and s.device_cg is None and not s.pipe_auto, force
    assert build("slab3", "csr").csrA is not None
    assert build("powerlaw/2", "sell").csrO is not None  # matO CSR stays


@pytest.mark.parametrize("force,spmm,kmax4", [
    ("sell", True, 4), ("sigma", True, 4), ("bsell", True, 4),
    ("hybrid", False, 0), ("binned", False, 0), ("csr", False, 0)])
def test_capabilities(force, spmm, kmax4):
    A = build("slab3", force).A
    assert A.has_spmm == A.has_dual == spmm
    assert A.spmm_kmax(4) == kmax4 and A.spmm_kmax(8) == 2 * kmax4
    assert A.has_daypx == (force == "bsell")
    assert (A.idx_bytes_per_nnz is not None) == (force == "bsell")
    if force != "bsell":
        from acg_amd.utils.errors import AcgError

        with pytest.raises(AcgError, match=f"this system uses {force}"):
            A.diag_inv()
    if spmm:
        lo = A.fp32()
        assert lo is A.fp32() and lo.name == A.name
        assert lo.vals.dtype == torch.float32 and A.vals.dtype == torch.float64
        assert torch.equal(lo.vals, A.vals.to(torch.float32))
        for idx in ("bptr", "bcol") if force == "bsell" else ("sellptr", "cols"):
            assert getattr(lo, idx).data_ptr() == getattr(A, idx).data_ptr()
    else:
        with pytest.raises(ValueError, match="the fp32-stored operator needs "
                           "the SELL, sigma-SELL or BSELL format; this system "
                           f"uses {force}"):
            A.fp32()
