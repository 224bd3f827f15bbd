#!/usr/bin/env python3
"""BSELL-ST against BSELL: SpMV and classic-CG iteration A/B on an MI355X.

    python tools/symtile_tts.py [--grids 111,80] [--reps 7] [--its 200]
                                [--qmax 8] [--out FILE.json]

Everything is interleaved in ONE process and reported as medians
(NOTES.md: run-to-run placement noise is larger than most effects).  Three
arms: ``bsell``, ``bsell-st`` and a second, separately constructed
``bsell2`` arm; bsell2 / bsell is the spread two identical arms show, the
yardstick for the bsell-st / bsell ratio.

(a) SpMV alone, with the fused (x, y) dot the classic iteration uses, in
    us and in GB/s of each format's own bytes (operator + x + y once).
(b) the classic iteration: ``solve(maxits=its, res_rtol=0)`` per arm,
    us per iteration from the solver's own timer.
Systems are device-generated Queen-shaped (G=111) and Flan-shaped (G=80)
27-point dof-3 stencils, as in bench.py.
"""

import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def interleaved(fns, reps):
    """``reps`` rounds over the closures in turn (one untimed round first);
    each returns seconds.  Median, min and max per arm."""
    for fn in fns.values():
        fn()
    rec = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            rec[k].append(fn())
    return {k: {"med": statistics.median(v), "min": min(v), "max": max(v)}
            for k, v in rec.items()}


def one_grid(G, dof, dev, reps, its, iters, qmax):
    from acg_amd.gen import queen_like_spec
    from acg_amd.gen.device_slab import device_stencil_slab
    from acg_amd.ops import gpu_ops
    from acg_amd.ops.symtile import bsell_st_build
    from acg_amd.solvers.hip import CGSolverHIP

    S = device_stencil_slab(G, G, G, queen_like_spec(dof), 0, 1, dev)
    n = S.nowned
    out = {"system": f"27pt dof{dof} G{G}", "rows": n}

    os.environ["ACG_BSELL_ST"] = "0"
    plain, plain2 = CGSolverHIP(S, device=dev), CGSolverHIP(S, device=dev)
    os.environ["ACG_BSELL_ST"] = "1"
    sym = CGSolverHIP(S, device=dev, force_format="bsell-st")
    if qmax != sym.bsell_st.qmax:
        bptr, bcol, bvals, _ = S.A_bsell
        sym.opA.st = bsell_st_build(bptr, bcol, bvals, n // dof, dof,
                                    S.node_order, qmax=qmax)
        assert sym.bsell_st is not None, "gate refused this qmax"
    st = sym.bsell_st
    out.update(qmax=st.qmax, byte_ratio=st.ratio, stored_bytes=st.stored_bytes,
               bsell_bytes=st.bsell_bytes, pairs=st.npairs, paired=st.npaired,
               mean_nrecv=float(st.nrecv.float().sum()) / st.nnodes)

    # (a) SpMV with the fused dot
    bptr, bcol, bvals, _ = S.A_bsell
    x = torch.randn(n, dtype=torch.float64, device=dev)
    xs = x[st.vperm]
    y, ys = torch.zeros_like(x), torch.zeros_like(x)
    scal, part = plain.scal, plain.partials
    fuse = dict(partials=part, scal=scal, dotslot=gpu_ops.S_PT, dot_accum=False)
    calls = {
        "bsell": lambda: gpu_ops.spmv_bsell(bptr, bcol, bvals, n // dof, dof,
                                            x, y, **fuse),
        "bsell-st": lambda: gpu_ops.spmv_bsell_st(st, xs, ys, **fuse),
        "bsell2": lambda: gpu_ops.spmv_bsell(bptr, bcol, bvals, n // dof, dof,
                                             x, y, **fuse),
    }

    def timed(fn):
        def run():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / iters
        return run

    t = interleaved({k: timed(f) for k, f in calls.items()}, reps)
    yback = torch.empty_like(y)
    yback[st.vperm] = ys
    out["spmv_max_rel_diff"] = float((yback - y).abs().max() / y.abs().max())
    byt = {"bsell": st.bsell_bytes + 16 * n, "bsell2": st.bsell_bytes + 16 * n,
           "bsell-st": st.stored_bytes + 16 * n}
    out["spmv"] = {k: {"us": v["med"] * 1e6, "min_us": v["min"] * 1e6,
                       "max_us": v["max"] * 1e6,
                       "GBps": byt[k] / v["med"] / 1e9} for k, v in t.items()}

    # (b) classic iteration
    b = torch.from_numpy(np.random.default_rng(10_000).standard_normal(n)).to(dev)
    xsol = {}

    def solve(name, solver):
        def run():
            xv = torch.zeros(n + S.nghost, dtype=torch.float64, device=dev)
            res = solver.solve(b, xv, maxits=its, res_rtol=0.0)
            xsol[name] = xv
            return res.tsolve / res.niterations
        return run

    t = interleaved({"bsell": solve("bsell", plain),
                     "bsell-st": solve("bsell-st", sym),
                     "bsell2": solve("bsell2", plain2)}, reps)
    out["classic"] = {k: {"us_per_it": v["med"] * 1e6, "min": v["min"] * 1e6,
                          "max": v["max"] * 1e6} for k, v in t.items()}
    out["classic_x_max_rel_diff"] = float(
        (xsol["bsell-st"] - xsol["bsell"]).abs().max() / xsol["bsell"].abs().max())
    for part_ in ("spmv", "classic"):
        key = "us" if part_ == "spmv" else "us_per_it"
        a = out[part_]
        a["st_over_bsell"] = a["bsell-st"][key] / a["bsell"][key]
        a["bsell2_over_bsell"] = a["bsell2"][key] / a["bsell"][key]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", default="111,80")
    ap.add_argument("--dof", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--its", type=int, default=200)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--qmax", type=int, default=8)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "symtile_tts measures on the GPU only"
    dev = torch.device("cuda:0")
    result = []
    for G in (int(g) for g in args.grids.split(",")):
        r = one_grid(G, args.dof, dev, args.reps, args.its, args.iters, args.qmax)
        result.append(r)
        torch.cuda.empty_cache()
        print(f"SYMTILE {r['system']} rows={r['rows']} qmax={r['qmax']} "
              f"bytes {r['byte_ratio']:.3f} of bsell, mean nrecv "
              f"{r['mean_nrecv']:.2f}", flush=True)
        for k in ("bsell", "bsell-st", "bsell2"):
            s, c = r["spmv"][k], r["classic"][k]
            print(f"SYMTILE {k:9s} spmv {s['us']:7.1f} us [{s['min_us']:.1f}.."
                  f"{s['max_us']:.1f}] {s['GBps']:6.0f} GB/s | classic "
                  f"{c['us_per_it']:7.1f} us/it [{c['min']:.1f}..{c['max']:.1f}]",
                  flush=True)
        print(f"SYMTILE ratios spmv st/bsell {r['spmv']['st_over_bsell']:.3f} "
              f"(bsell2/bsell {r['spmv']['bsell2_over_bsell']:.3f}) | classic "
              f"st/bsell {r['classic']['st_over_bsell']:.3f} (bsell2/bsell "
              f"{r['classic']['bsell2_over_bsell']:.3f})", flush=True)
    print(json.dumps(result))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
