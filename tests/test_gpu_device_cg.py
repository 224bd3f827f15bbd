"""The one-launch device CG (k_cg_device, both grid barriers) on the GPU
against the step-chained high-precision oracle of tests/kernel_oracle.py.

The kernel is deterministic (fixed-order reductions, no atomics in the
arithmetic), so a launch with maxits = k + 1 and zero tolerances repeats the
maxits = k launch bit for bit and then does one more step: every step is
checked on its own, from exactly the fp64 state the previous launch
returned, within the bounds of a single step.  CG's self-correction cannot
hide a stale gather, a dropped partial or an early barrier release that way.
tests/test_kernel_oracle_cpu.py proves the same checks reject ten defects.

The grid is chosen through nslices (the launcher clamps it to
ceil(nslices*64/256) blocks): 1, 2, 7, 8, 9 around the hierarchical
barrier's group size of 8, 64 and 65 around the automatic flat ->
hierarchical switch, and 8200 slices (2050 blocks wanted) for the capped
grid whose waves take further grid-stride trips.  Each test prints the grid
it got (``DEVCG_GRID``)."""

from functools import lru_cache

import numpy as np
import pytest
import torch

import kernel_oracle as ko

pytestmark = pytest.mark.gpu

BLOCKS = {1: 1, 5: 2, 28: 7, 32: 8, 33: 9, 256: 64, 257: 65}
CAPPED = 8200
SLICES = tuple(BLOCKS) + (CAPPED,)
COL64_SLICES = (1, 33, 257)
DEEP = {33: (12,)}  # one link far down the chain


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gpu_ops():
    from acg_amd.ops import gpu_ops

    assert gpu_ops.MAXG == ko.MAXG and gpu_ops.S_NSLOTS == ko.S_NSLOTS
    assert gpu_ops.BAR_STATE_WORDS == ko.BAR_STATE_WORDS
    for name in ("S_RR", "S_PT", "S_RR_PREV", "S_BNRM2", "S_GAMMA", "S_DELTA",
                 "S_GAMMA_PREV", "S_ALPHA_PREV"):
        assert getattr(gpu_ops, name) == getattr(ko, name)
    return gpu_ops


@lru_cache(maxsize=None)
def _case(nslices, zero=False):
    return ko.device_cg_case(nslices, zero_b=zero, zero_x0=zero)


def _check_grid(nslices, got, dev):
    grid, need = got["grid"], ko.device_cg_blocks(nslices)
    print(f"DEVCG_GRID nslices={nslices} need={need} grid={grid}")
    if nslices == CAPPED:
        cus = torch.cuda.get_device_properties(dev).multi_processor_count
        assert need == 2050 and cus <= grid < need and grid % cus == 0, (grid, cus)
    else:
        assert grid == need == BLOCKS[nslices]


def _launcher(gpu_ops, case, dev, **fixed):
    return lambda **kw: ko.run_device_cg(gpu_ops, case, dev, **fixed, **kw)


@pytest.mark.parametrize("nslices,hier,col64",
                         [(ns, h, False) for ns in SLICES for h in (False, True)]
                         + [(ns, None, True) for ns in COL64_SLICES])
def test_init_and_chained_steps(dev, gpu_ops, nslices, hier, col64):
    """maxits = 0 against the init expectation, then every link k -> k + 1
    for k = 0..3 (and 12 -> 13 on the 9-block grid).  ``hier=None`` lets the
    launcher choose (flat below 64 blocks), with 64-bit column indices."""
    case = _case(nslices)
    ks = ko.DEVCG_KS + DEEP.get(nslices, ())
    gots = ko.device_cg_check_chain(
        _launcher(gpu_ops, case, dev, hier=hier, col64=col64), case, ks=ks,
        tag=f"ns{nslices} hier={hier} col64={col64}")
    for got in gots.values():
        assert got["grid"] == gots[0]["grid"]
    _check_grid(nslices, gots[0], dev)


@pytest.mark.parametrize("nslices", SLICES)
def test_barriers_and_index_width_are_bitwise_neutral(dev, gpu_ops, nslices):
    case = _case(nslices)
    base = ko.run_device_cg(gpu_ops, case, dev, maxits=6, hier=False)
    _check_grid(nslices, base, dev)
    ko.device_cg_check_every_k(base, base, 6)
    for hier, col64 in ((True, False), (False, True), (True, True)):
        got = ko.run_device_cg(gpu_ops, case, dev, maxits=6, hier=hier, col64=col64)
        assert got["grid"] == base["grid"]
        diff = ko.device_cg_same_bits(base, got)
        assert not diff, f"hier={hier} col64={col64}: {diff} differ"
        ko.check_partials(got, halves=1)


@pytest.mark.parametrize("hier", [False, True])
@pytest.mark.parametrize("nslices", SLICES)
def test_repeat_is_bitwise(dev, gpu_ops, nslices, hier):
    """The premise of the chaining: the same launch, each time on a freshly
    zeroed barrier state, gives the same bits."""
    case = _case(nslices)
    a = ko.run_device_cg(gpu_ops, case, dev, maxits=6, hier=hier)
    b = ko.run_device_cg(gpu_ops, case, dev, maxits=6, hier=hier)
    diff = ko.device_cg_same_bits(a, b)
    assert not diff and a["grid"] == b["grid"], diff
    assert np.array_equal(a["partials"][:a["grid"]], b["partials"][:a["grid"]])


@pytest.mark.parametrize("hier", [False, True])
def test_tolerances(dev, gpu_ops, hier):
    case = _case(33)
    launch = _launcher(gpu_ops, case, dev, hier=hier)
    gots = ko.device_cg_check_chain(launch, case, ks=tuple(range(6)),
                                    tag=f"tol hier={hier}")
    print("DEVCG_RR " + " ".join(f"{float(gots[m]['scal0'][0]):.6g}" for m in range(7)))
    ko.device_cg_check_tolerances(launch, case, gots)


@pytest.mark.parametrize("nslices,hier", [(1, None), (33, False), (33, True),
                                          (257, None)])
def test_zero_rhs_and_exact_zero_residual(dev, gpu_ops, nslices, hier):
    """b = 0, x0 = 0: (r,r) is exactly 0, so beta = rr_new/rr is 0/0.  An
    unguarded division stores NaN into p and the next step poisons x."""
    case = _case(nslices, zero=True)
    ko.device_cg_check_zero(_launcher(gpu_ops, case, dev, hier=hier), case)


def test_wrapper_refuses_bad_arguments(dev, gpu_ops):
    """Every refusal is a ValueError raised before the launch: all outputs
    keep their prefill.  One valid launch at the end shows that nothing but
    the named argument was wrong."""
    case = _case(5)
    n = case.nrows
    ko.run_device_cg(gpu_ops, case, dev, maxits=0)  # packs and uploads the operator
    sp, sc, sv = case._dev[(str(dev), False)]

    def fresh():
        return dict(sellptr=sp, cols=sc, vals=sv, nrows=n, b=ko._t(case.b, dev),
                    x=ko._t(case.x0, dev), r=ko._nan(n, dev), p=ko._nan(n, dev),
                    t=ko._nan(n, dev), scal=ko._t(ko.SENTINELS, dev),
                    partials=ko._nan(2 * ko.MAXG, dev),
                    out2=torch.tensor(ko.OUT2_SENTINEL, dtype=torch.int32, device=dev),
                    barrier_state=torch.zeros(ko.BAR_STATE_WORDS, dtype=torch.int32,
                                              device=dev),
                    maxits=3, res_atol=0.0, res_rtol=0.0)

    def untouched(a):
        for k in "rpt":
            assert torch.isnan(a[k]).all(), k
        assert torch.isnan(a["partials"]).all()
        assert np.array_equal(ko._np(a["x"]), case.x0)
        assert np.array_equal(ko._np(a["scal"]), ko.SENTINELS)
        assert ko._np(a["out2"]).tolist() == list(ko.OUT2_SENTINEL)
        assert not a["barrier_state"].any()

    bad = {
        "sellptr int32": lambda a: {"sellptr": sp.to(torch.int32)},
        "sellptr one entry": lambda a: {"sellptr": sp[:1]},
        "cols int16": lambda a: {"cols": sc.to(torch.int16)},
        "vals float32": lambda a: {"vals": sv.float()},
        "cols shorter than vals": lambda a: {"cols": sc[:-64]},
        "nrows beyond the slices": lambda a: {"nrows": case.nslices * 64 + 1},
        "scal short": lambda a: {"scal": a["scal"][:ko.S_NSLOTS - 1]},
        "scal float32": lambda a: {"scal": a["scal"].float()},
        "partials short": lambda a: {"partials": a["partials"][:ko.MAXG - 1]},
        "out2 int64": lambda a: {"out2": a["out2"].long()},
        "out2 one element": lambda a: {"out2": a["out2"][:1]},
        "barrier int64": lambda a: {"barrier_state": a["barrier_state"].long()},
        "barrier short": lambda a: {"barrier_state":
                                    a["barrier_state"][:ko.BAR_STATE_WORDS - 1]},
        "maxits negative": lambda a: {"maxits": -1},
        "r on the host": lambda a: {"r": a["r"].cpu()},
    }
    for v in "bxrpt":
        bad[f"{v} float32"] = lambda a, v=v: {v: a[v].float()}
        bad[f"{v} short"] = lambda a, v=v: {v: a[v][:n - 1]}
        bad[f"{v} strided"] = lambda a, v=v: {
            v: torch.zeros(2 * n, dtype=torch.float64, device=dev)[::2]}
    for name, change in bad.items():
        a = fresh()
        call = dict(a, **change(a))
        with pytest.raises(ValueError, match="cg_device"):
            gpu_ops.cg_device(**call)
        torch.cuda.synchronize(dev)
        untouched(a)
    a = fresh()
    assert gpu_ops.cg_device(**a) == BLOCKS[5]
    assert ko._np(a["out2"]).tolist() == [3, 0]
    assert torch.isfinite(a["x"]).all() and torch.isfinite(a["p"]).all()
