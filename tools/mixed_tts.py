#!/usr/bin/env python3
"""fp32-stored operator: SpMV bandwidth and time-to-solution A/B on an MI355X.

    python tools/mixed_tts.py [--grid 111] [--poisson 256] [--tts-grid 80]
                              [--reps 5] [--out FILE.json]

Everything is interleaved A/B in ONE process and reported as medians
(NOTES.md: run-to-run placement noise is larger than most effects).

(a) SpMV alone, fp64 against fp32 values: BSELL dof 3 at the bench's
    Queen-shaped size (device-generated, G=111) and SELL 7-pt Poisson 256^3,
    in us and achieved GB/s (bytes = matrix stream + x + y once each).
    Yardstick: the matrix stream shrinks 76 -> 40 B per dof-3 block and
    12 -> 8 B per SELL entry.
(b) Time-to-solution, ``solve`` against ``solve_mixed`` at res_rtol 1e-9 and
    1e-12 for inner_rtol in {1e-2, 1e-4, 1e-6} on a Queen-shaped system
    whose values a symmetric scaling s_i a_ij s_j, s in [0.5, 2), has made
    non-representable in fp32.  Host-assembled (solve_mixed keeps both value
    sets and refuses device-generated systems), hence the smaller default
    grid; both operators still exceed the 256 MiB Infinity Cache.
(c) The true relative residual ||b - A x|| / ||b|| each arm reached,
    recomputed with the fp64 operator.
"""

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def bench_pair(fns, iters, reps):
    """Interleaved timing of several closures: ``reps`` rounds, each timing
    ``iters`` calls of every closure in turn; returns median seconds/call."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / iters)
    return {k: statistics.median(v) for k, v in times.items()}


def spmv_bsell_ab(G, dof, dev, iters, reps):
    from acg_amd.gen import queen_like_spec
    from acg_amd.gen.device_slab import device_stencil_slab
    from acg_amd.ops import gpu_ops

    S = device_stencil_slab(G, G, G, queen_like_spec(dof), 0, 1, dev)
    bptr, bcol, bvals, dof = S.A_bsell
    bvals32 = bvals.to(torch.float32)
    n = S.nowned
    nblocks = bcol.numel()
    x = torch.randn(n + S.nghost, dtype=torch.float64, device=dev)
    y = torch.zeros(n, dtype=torch.float64, device=dev)
    t = bench_pair({
        "fp64": lambda: gpu_ops.spmv_bsell(bptr, bcol, bvals, n // dof, dof, x, y),
        "fp32": lambda: gpu_ops.spmv_bsell(bptr, bcol, bvals32, n // dof, dof, x, y),
    }, iters, reps)
    out = {"system": f"queen-like 27pt dof{dof} G{G}", "rows": n,
           "blocks": nblocks}
    for k, vb in (("fp64", 8), ("fp32", 4)):
        nbytes = nblocks * (4 + vb * dof * dof) + 16 * n
        out[k] = {"us": t[k] * 1e6, "GBps": nbytes / t[k] / 1e9,
                  "bytes": nbytes}
    out["speedup"] = t["fp64"] / t["fp32"]
    out["byte_ratio"] = out["fp32"]["bytes"] / out["fp64"]["bytes"]
    return out


def spmv_sell_ab(G, dev, iters, reps):
    from acg_amd.gen import STENCIL_7PT_3D
    from acg_amd.gen.device_slab import device_stencil_slab
    from acg_amd.ops import gpu_ops

    S = device_stencil_slab(G, G, G, dict(STENCIL_7PT_3D), 0, 1, dev)
    sellptr, cols, vals = S.A_sell
    vals32 = vals.to(torch.float32)
    n = S.nowned
    nent = cols.numel()
    x = torch.randn(n + S.nghost, dtype=torch.float64, device=dev)
    y = torch.zeros(n, dtype=torch.float64, device=dev)
    t = bench_pair({
        "fp64": lambda: gpu_ops.spmv_sell(sellptr, cols, vals, n, x, y),
        "fp32": lambda: gpu_ops.spmv_sell(sellptr, cols, vals32, n, x, y),
    }, iters, reps)
    out = {"system": f"poisson 7pt G{G}", "rows": n, "entries": nent}
    for k, vb in (("fp64", 8), ("fp32", 4)):
        nbytes = nent * (cols.element_size() + vb) + 16 * n
        out[k] = {"us": t[k] * 1e6, "GBps": nbytes / t[k] / 1e9,
                  "bytes": nbytes}
    out["speedup"] = t["fp64"] / t["fp32"]
    out["byte_ratio"] = out["fp32"]["bytes"] / out["fp64"]["bytes"]
    return out


def tts_ab(G, dof, dev, reps, maxits):
    from acg_amd.gen import queen_like_spec, stencil_global
    from acg_amd.part import extract_subdomains, partition_rows
    from acg_amd.solvers.hip import CGSolverHIP

    A = stencil_global(G, G, G, queen_like_spec(dof))
    s = np.random.default_rng(0).uniform(0.5, 2.0, size=A.n)
    rows = np.repeat(np.arange(A.n, dtype=np.int64), np.diff(A.rowptr))
    A.vals *= s[rows] * s[A.colidx]
    S = extract_subdomains(A, partition_rows(A, 1), 1)[0]
    del A, rows
    solver = CGSolverHIP(S, device=dev)
    fmt = solver._format_name()
    b = torch.from_numpy(
        np.random.default_rng(1).standard_normal(S.nowned)).to(dev)
    bn = float(torch.linalg.norm(b))
    chk = torch.zeros(S.nowned, dtype=torch.float64, device=dev)

    def true_rel(x):
        solver._spmv_overlapped(x, chk)
        return float(torch.linalg.norm(b - chk)) / bn

    out = {"system": f"queen-like 27pt dof{dof} G{G}, scaled", "format": fmt,
           "rows": S.nowned, "nnz": int(S.nnzA), "arms": []}
    for rtol in (1e-9, 1e-12):
        arms = {"fp64": lambda x, r=rtol: solver.solve(
            b, x, maxits=maxits, res_rtol=r)}
        for ir in (1e-2, 1e-4, 1e-6):
            arms[f"mixed {ir:g}"] = lambda x, r=rtol, i=ir: solver.solve_mixed(
                b, x, maxits=maxits, res_rtol=r, inner_rtol=i)
        rec = {k: {"t": []} for k in arms}
        for rep in range(reps + 1):  # round 0 warms every arm
            for k, fn in arms.items():
                x = torch.zeros(S.nowned + S.nghost, dtype=torch.float64,
                                device=dev)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = fn(x)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if rep:
                    rec[k]["t"].append(dt)
                rec[k].update(its=res.niterations, nouter=res.nouter,
                              converged=res.converged, true_rel=true_rel(x))
        base = statistics.median(rec["fp64"]["t"])
        for k, r in rec.items():
            med = statistics.median(r["t"])
            out["arms"].append({
                "res_rtol": rtol, "arm": k, "ms": med * 1e3,
                "min_ms": min(r["t"]) * 1e3, "max_ms": max(r["t"]) * 1e3,
                "vs_fp64": med / base, "its": r["its"], "nouter": r["nouter"],
                "converged": r["converged"], "true_rel": r["true_rel"],
                "us_per_it": med / max(r["its"], 1) * 1e6})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=111,
                    help="Queen-shaped grid edge of the SpMV part")
    ap.add_argument("--poisson", type=int, default=256)
    ap.add_argument("--tts-grid", type=int, default=80,
                    help="Queen-shaped grid edge of the time-to-solution part")
    ap.add_argument("--dof", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--maxits", type=int, default=5000)
    ap.add_argument("--skip", default="", help="comma list of spmv,tts")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "mixed_tts measures on the GPU only"
    dev = torch.device("cuda:0")
    skip = set(args.skip.split(","))
    result = {}
    if "spmv" not in skip:
        result["spmv"] = [spmv_bsell_ab(args.grid, args.dof, dev, args.iters,
                                        args.reps)]
        torch.cuda.empty_cache()
        result["spmv"].append(spmv_sell_ab(args.poisson, dev, args.iters,
                                           args.reps))
        torch.cuda.empty_cache()
        for r in result["spmv"]:
            print(f"SPMV {r['system']}: fp64 {r['fp64']['us']:.1f} us "
                  f"({r['fp64']['GBps']:.0f} GB/s)  fp32 {r['fp32']['us']:.1f} us "
                  f"({r['fp32']['GBps']:.0f} GB/s)  speedup {r['speedup']:.3f} "
                  f"(byte ratio {r['byte_ratio']:.3f})", flush=True)
    if "tts" not in skip:
        result["tts"] = tts_ab(args.tts_grid, args.dof, dev, args.reps,
                               args.maxits)
        t = result["tts"]
        print(f"TTS {t['system']} [{t['format']}] rows={t['rows']} nnz={t['nnz']}")
        for a in t["arms"]:
            print(f"TTS rtol={a['res_rtol']:g} {a['arm']:12s} {a['ms']:9.2f} ms "
                  f"[{a['min_ms']:.2f}..{a['max_ms']:.2f}] x{a['vs_fp64']:.3f} "
                  f"its={a['its']} outer={a['nouter']} conv={a['converged']} "
                  f"true_rel={a['true_rel']:.2e} {a['us_per_it']:.1f} us/it",
                  flush=True)
    print(json.dumps(result))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
