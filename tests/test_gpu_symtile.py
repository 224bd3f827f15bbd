"""BSELL-ST on the GPU: k_spmv_bsell_st against the long-double oracle of
tests/symtile_systems.py on NaN-poisoned outputs, the device-side builder
against the host one, and the classic solve with and without the format."""

from functools import lru_cache

import numpy as np
import pytest
import torch

import kernel_oracle as ko
import symtile_systems as ss

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# 27 nodes: one tile, one partial slice.  125: one tile, 61 live lanes in
# its second slice.  381 (strip): two tiles, 61 live lanes in the last
# slice.  1728: seven tiles, the last of three slices; 8 x 8 x 4 bricks do
# not divide 12^3, so tile boundaries cut bricks.
KERNEL_CASES = [(g, dof, o) for g in ss.CUBES for dof in ss.DOFS
                for o in ss.ORDERS] + [(ss.STRIP, dof, "brick") for dof in ss.DOFS]


def _ops():
    from acg_amd.ops import gpu_ops

    return gpu_ops


@lru_cache(maxsize=None)
def _st(shape, dof, order, **kw):
    return ss.build(shape, dof, order, DEV, **kw)


def _check(st, shape, dof, tag, **kw):
    ops = _ops()
    for dotslot in (-1, ko.S_PT):
        got = ss.run_spmv(ops, st, shape, dof, DEV, dotslot=dotslot, **kw)
        ko.assert_accepts(ss.expect(shape, dof, dotslot), got, f"{tag} dot{dotslot}")
        ss.check_untouched(got)
        again = ss.run_spmv(ops, st, shape, dof, DEV, dotslot=dotslot, **kw)
        for k in ("yperm", "partials", f"scal{ko.S_PT}"):
            assert ko._bits_equal(got[k], again[k]), k
    return got


@pytest.mark.parametrize("shape,dof,order", KERNEL_CASES)
def test_spmv_bsell_st(shape, dof, order):
    st = _st(shape, dof, order)
    assert st is not None and st.svals.device.type == "cuda"
    _check(st, shape, dof, f"{shape} dof{dof} {order}")


@pytest.mark.parametrize("dof", ss.DOFS)
def test_grid_stride_second_trip(dof):
    """Seven tiles on two blocks: every block walks 3-4 tiles and reuses
    its slots; exactly two partials are written."""
    st = _st(12, dof, "brick")
    assert st.ntiles == 7
    got = _check(st, 12, dof, f"two blocks dof{dof}", max_blocks=2)
    assert got["nblocks"] == 2
    full = ss.run_spmv(_ops(), st, 12, dof, DEV)
    assert ko._bits_equal(full["yperm"], got["yperm"])


@pytest.mark.parametrize("dof", ss.DOFS)
def test_cap_and_no_receives(dof):
    # qmax 2: nodes with exactly 2 receives, pairs over the cap stored twice
    st = _st(5, dof, "brick", qmax=2)
    assert int(st.nrecv.max()) == 2 and ss.overcap_pairs(st)
    _check(st, 5, dof, f"qmax2 dof{dof}")
    # qmax 0: no LDS at all, nrecv = 0 everywhere
    st0 = _st(5, dof, "brick", qmax=0)
    assert not st0.nrecv.any()
    _check(st0, 5, dof, f"qmax0 dof{dof}")


@pytest.mark.parametrize("shape,dof,order", [(5, 3, "brick"), (12, 2, "natural"),
                                             (ss.STRIP, 4, "brick")])
def test_device_build_equals_host_build(shape, dof, order):
    host = ss.build(shape, dof, order)
    dev = _st(shape, dof, order)
    for k, v in vars(host).items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(v, getattr(dev, k).cpu()), k
        else:
            assert v == getattr(dev, k), k


def test_wrapper_refuses_bad_arguments():
    ops = _ops()
    st = _st(5, 3, "brick")
    x = torch.zeros(375, dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError):
        ops.spmv_bsell_st(st, x[:100], x.clone())
    with pytest.raises(TypeError):
        ops.spmv_bsell_st(st, x.float(), x.clone())
    with pytest.raises(ValueError):
        ops.spmv_bsell_st(ss.build(5, 3, "brick", DEV, tile=64), x, x.clone())


# ---- solver ----

RTOL = 1e-6


def _solve(monkeypatch, env, force=None):
    from acg_amd.solvers.hip import CGSolverHIP

    s = ss.system(12, 3)
    if env is None:
        monkeypatch.delenv("ACG_BSELL_ST", raising=False)
    else:
        monkeypatch.setenv("ACG_BSELL_ST", env)
    solver = CGSolverHIP(s.S, device=DEV, force_format=force)
    b = torch.from_numpy(s.b).to(DEV)
    x = torch.zeros(s.n, dtype=torch.float64, device=DEV)
    res = solver.solve(b, x, maxits=20000, res_rtol=RTOL)
    # true residual from the caller-order CSR, in the caller's order
    xt = x.cpu().numpy()
    true = np.linalg.norm(s.b - s.Af @ xt) / np.linalg.norm(s.b)
    return solver, res, xt, true


def test_solve_with_and_without_bsell_st(monkeypatch):
    """The 1728-node dof-3 rotated system, hint-less LocalSystem order.
    Both arms stop on the recursion residual <= RTOL; the gap to the true
    residual is O(u kappa) ~ 1e-9 here, hence the 5 % allowance the other
    solver tests use."""
    on, ron, xon, ton = _solve(monkeypatch, "1", force="bsell-st")
    off, roff, xoff, toff = _solve(monkeypatch, "0")
    assert on.bsell_st is not None and on.classic_format == "bsell-st"
    assert off.bsell_st is None and off.classic_format == "bsell"
    assert on.bsell is not None and on._format_name() == "bsell"
    print(f"SYMTILE_SOLVE its st={ron.niterations} bsell={roff.niterations} "
          f"true st={ton:.3e} bsell={toff:.3e} ratio={on.bsell_st.ratio:.3f}")
    assert ron.converged and roff.converged
    assert abs(ron.niterations - roff.niterations) <= 1
    assert ton <= 1.05 * RTOL and toff <= 1.05 * RTOL
    # (the true residuals above use the caller-order matrix: an x left in
    # the operator's node order would miss them by orders of magnitude)
    # kill switch against the force: refused loudly
    with pytest.raises(ValueError):
        _solve(monkeypatch, "0", force="bsell-st")


def test_solve_with_brick_hint_and_other_solvers_keep_bsell(monkeypatch):
    from acg_amd.gen import queen_like_spec, stencil_local_slab
    from acg_amd.solvers.hip import CGSolverHIP

    monkeypatch.setenv("ACG_BSELL_ST", "1")
    S = stencil_local_slab(12, 12, 12, queen_like_spec(3), 0, 1)
    assert S.node_order is not None
    solver = CGSolverHIP(S, device=DEV)
    assert solver.bsell_st is not None
    b = torch.from_numpy(np.random.default_rng(3).standard_normal(S.nowned)).to(DEV)
    x = torch.zeros(S.nowned, dtype=torch.float64, device=DEV)
    res = solver.solve(b, x, maxits=500, res_rtol=1e-9)
    x2 = torch.zeros_like(x)
    res2 = solver.solve_pipelined(b, x2, maxits=500, res_rtol=1e-9)
    assert res.converged and res2.converged
    assert (x - x2).abs().max().item() <= 1e-7 * x2.abs().max().item()
    y = torch.zeros_like(x)
    solver._spmv_overlapped(x, y)
    assert float(torch.linalg.vector_norm(b - y)) <= 1.05e-9 * res.bnrm2
    # a second solve on the same solver is bitwise the first
    x3 = torch.zeros_like(x)
    res3 = solver.solve(b, x3, maxits=500, res_rtol=1e-9)
    assert res3.niterations == res.niterations and torch.equal(x, x3)
    # diff mode and the fp32 operator stay on BSELL and still work
    x4 = torch.zeros_like(x)
    assert solver.solve(b, x4, maxits=500, res_rtol=1e-9, diff_rtol=1e-30).converged
