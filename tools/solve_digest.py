#!/usr/bin/env python3
"""Behaviour digest of CGSolverHIP: every solve method on every operator
format, one JSON line per case with the format names, iteration counts, the
norms in hex and a sha256 of the bytes of x.  Seeded and bitwise
deterministic across processes, so two trees compute the same thing exactly
when their outputs are identical line for line (run each tree in a fresh
process).  Needs a GPU; uses the solver's public surface only.

Usage: python tools/solve_digest.py > digest.jsonl
"""

from __future__ import annotations

import hashlib
import json
import os
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from acg_amd.gen import STENCIL_7PT_3D, queen_like_spec, stencil_local_slab  # noqa: E402
from acg_amd.gen.device_slab import device_stencil_slab  # noqa: E402
from acg_amd.gen.irregular import powerlaw_spd  # noqa: E402
from acg_amd.part import extract_subdomains, partition_rows  # noqa: E402
from acg_amd.solvers.hip import CGSolverHIP  # noqa: E402
from acg_amd.utils.errors import AcgError  # noqa: E402

DEV = "cuda:0"
FIXED = dict(maxits=30, res_rtol=0.0)  # nothing depends on convergence


def case(system, solver, name, method, k=0, **kw):
    """Run ``solver.<method>`` from x = 0 on a seeded right-hand side (k
    columns for the multi-RHS methods) and print the digest line."""
    S = solver.local
    rng = np.random.default_rng(0)
    shape = (S.nowned, k) if k else (S.nowned,)
    b = torch.from_numpy(rng.standard_normal(shape)).to(DEV)
    x = torch.zeros((S.nowned + S.nghost,) + shape[1:], dtype=torch.float64,
                    device=DEV)
    head = {"case": f"{system}/{name}", "format": solver._format_name()}
    try:
        out = getattr(solver, method)(b, x, **{**FIXED, **kw})
    except (ValueError, AcgError) as e:  # a refusal is behaviour too
        print(json.dumps({**head, "refused": str(e)}), flush=True)
        return
    rs = out if isinstance(out, list) else [out]
    print(json.dumps({
        **head,
        "classic_format": solver.classic_format,
        "niterations": [r.niterations for r in rs],
        "converged": [bool(r.converged) for r in rs],
        "rnrm2": [float(r.rnrm2).hex() for r in rs],
        "bnrm2": [float(r.bnrm2).hex() for r in rs],
        "nreplacements": [getattr(r, "nreplacements", 0) for r in rs],
        "x": hashlib.sha256(x.cpu().numpy().tobytes()).hexdigest()}), flush=True)


def pair(system, solver):
    case(system, solver, "solve", "solve")
    case(system, solver, "pipelined", "solve_pipelined")


def main() -> None:
    spec7, spec3 = dict(STENCIL_7PT_3D), queen_like_spec(3)
    # 1: host dof-3 slab (BSELL with BSELL-ST)
    S = stencil_local_slab(12, 12, 12, spec3, 0, 1)
    s = CGSolverHIP(S, device=DEV)
    case("slab3", s, "solve", "solve")
    case("slab3", s, "fold_daypx", "solve", fold_daypx=True)
    case("slab3", s, "diff", "solve", diff_rtol=1e-6)
    case("slab3", s, "pipelined", "solve_pipelined", megafuse=False)
    case("slab3", s, "pipelined_mega", "solve_pipelined", megafuse=True)
    for fast in (True, False):
        s._rr_fast = fast
        case("slab3", s, f"rr5_fast{int(fast)}", "solve_pipelined", rr_period=5)
    s._rr_fast = True
    case("slab3", s, "multi3", "solve_multi", k=3)
    case("slab3", s, "block3", "solve_block", k=3)
    for m in ("solve_mixed", "solve_jacobi", "solve_bjacobi", "solve_device"):
        case("slab3", s, m, m)
    os.environ["ACG_BSELL_ST"] = "0"
    case("slab3", CGSolverHIP(S, device=DEV), "solve_st0", "solve")
    del os.environ["ACG_BSELL_ST"]
    # 2: host 7-pt dof 1 (SELL, auto-megafused)
    S = stencil_local_slab(16, 16, 16, spec7, 0, 1)
    s = CGSolverHIP(S, device=DEV)
    case("poisson7", s, "solve", "solve")
    case("poisson7", s, "solve_graph", "solve", use_graph=True)
    case("poisson7", s, "pipelined", "solve_pipelined")
    case("poisson7", s, "pipelined_graph", "solve_pipelined", use_graph=True)
    case("poisson7", s, "rr5", "solve_pipelined", rr_period=5)
    case("poisson7", s, "multi5", "solve_multi", k=5)
    case("poisson7", s, "block2", "solve_block", k=2)
    case("poisson7", s, "solve_mixed", "solve_mixed")
    case("poisson7", s, "solve_device", "solve_device")
    # 3: power-law rows, every format of the ladder
    A = powerlaw_spd(3000, mean_nnz=24, clip=48, seed=4)
    S = extract_subdomains(A, partition_rows(A, 1), 1)[0]
    os.environ["ACG_HYBRID_CUT"] = "24"
    for fmt in ("sigma", "hybrid", "binned", "csr", None):
        s = CGSolverHIP(S, device=DEV, force_format=fmt)
        pair(f"powerlaw-{fmt}", s)
        case(f"powerlaw-{fmt}", s, "solve_jacobi", "solve_jacobi")
        case(f"powerlaw-{fmt}", s, "multi2", "solve_multi", k=2)
        if fmt == "sigma":
            case("powerlaw-sigma", s, "solve_mixed", "solve_mixed")
            case("powerlaw-sigma", s, "rr5", "solve_pipelined", rr_period=5)
    # 4: part 0 of 2 with comm=None (ghosts stay zero; still SPD)
    S = extract_subdomains(A, partition_rows(A, 2, method="ml", seed=1), 2,
                           only_parts=[0])[0]
    pair("powerlaw/2-hybrid", CGSolverHIP(S, device=DEV, force_format="hybrid"))
    del os.environ["ACG_HYBRID_CUT"]
    pair("poisson7/2", CGSolverHIP(stencil_local_slab(16, 16, 16, spec7, 0, 2),
                                   device=DEV))
    pair("slab3/2-bsell", CGSolverHIP(stencil_local_slab(12, 12, 12, spec3, 0, 2),
                                      device=DEV, force_format="bsell"))
    pair("poisson7/2-csr", CGSolverHIP(stencil_local_slab(16, 16, 16, spec7, 0, 2),
                                       device=DEV, force_format="csr"))
    # 5: device-generated slabs
    for nranks in (1, 2):
        for tag, spec, G, mf in (("dev7-mf", spec7, 16, True),
                                 ("dev7", spec7, 16, False),
                                 ("dev3", spec3, 12, False)):
            S = device_stencil_slab(G, G, G, spec, 0, nranks, DEV)
            pair(f"{tag}/{nranks}", CGSolverHIP(S, device=DEV, matfree=mf))


if __name__ == "__main__":
    main()
