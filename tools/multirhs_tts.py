#!/usr/bin/env python3
"""Multiple right-hand sides: SpMM bandwidth and time-to-solution A/B on an
MI355X, written up as profiles/multi_rhs.md.

    python tools/multirhs_tts.py --resources-only      # no GPU needed
    python tools/multirhs_tts.py [--grid 111] [--poisson 256] [--tts-grid 111]
                                 [--reps 5] [--parent-json FILE] [--out FILE.json]
    python tools/multirhs_tts.py --single-only --out FILE.json
    python tools/multirhs_tts.py --from-json FILE.json [--parent-json FILE]

Everything is interleaved A/B in ONE process and reported as medians, after
a cold warm-up of every arm (NOTES.md: run-to-run placement noise is larger
than most effects).  Every table carries two IDENTICAL single-vector arms;
their ratio is the run-to-run spread the other ratios have to beat.

(a) SpMM against K x SpMV at K = 2, 4, 8: BSELL dof 3 at the bench's
    Queen-shaped size (device-generated, G=111) and SELL 7-pt Poisson 256^3,
    in us and effective GB/s (bytes = matrix stream once + x and y of K
    columns once each).
(b) Time-to-solution of ``solve_multi`` against k sequential ``solve`` calls
    on the Queen-shaped system, with the true relative residual
    ||b_c - A x_c|| / ||b_c|| every arm reached.
(c) us/iteration of the single-RHS ``solve`` (``--single-only`` runs just
    this; run at the parent commit it gives ``--parent-json``).

``--resources-only`` compiles kernels.hip for the device with the compiler's
kernel resource-usage remarks and stores VGPRs / scratch of the multi-RHS
kernels in profiles/multi_rhs_resources.json, which the measuring run folds
into the note.
"""

import argparse
import json
import re
import statistics
import subprocess
import sys
import sysconfig
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
RES_JSON = ROOT / "profiles" / "multi_rhs_resources.json"
NOTE = ROOT / "profiles" / "multi_rhs.md"
KS = (2, 4, 8)


# ---------------------------------------------------------------------------
# register / scratch table (CPU only)

def resource_table():
    import pybind11

    src = ROOT / "acg_amd" / "ops" / "kernels.hip"
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run(
            ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17",
             "--cuda-device-only", "-c", f"-I{pybind11.get_include()}",
             f"-I{sysconfig.get_paths()['include']}",
             "-Rpass-analysis=kernel-resource-usage", str(src),
             "-o", str(Path(tmp) / "dev.o")], capture_output=True, text=True)
    if r.returncode:
        raise RuntimeError(r.stderr[-2000:])
    rows = {}
    for blk in r.stderr.split("remark: Function Name: ")[1:]:
        mangled = blk.split()[0]
        if "k_spmm" not in mangled and "_multi" not in mangled:
            continue
        name = subprocess.run(["c++filt", mangled], capture_output=True,
                              text=True).stdout.strip()
        name = re.sub(r"^void ", "", name).split("(")[0]

        def g(key):
            return int(re.search(key + r": (\d+)", blk).group(1))

        rows[name] = {"vgprs": g("VGPRs"), "agprs": g("AGPRs"),
                      "scratch": g(r"ScratchSize \[bytes/lane\]"),
                      "occupancy": g(r"Occupancy \[waves/SIMD\]"),
                      "vgpr_spill": g("VGPRs Spill")}
    return dict(sorted(rows.items()))


def resources_md(rows):
    out = ["| kernel | VGPRs | AGPRs | scratch B/lane | VGPR spills | waves/SIMD |",
           "|---|---:|---:|---:|---:|---:|"]
    for name, r in rows.items():
        out.append(f"| `{name}` | {r['vgprs']} | {r['agprs']} | {r['scratch']} "
                   f"| {r['vgpr_spill']} | {r['occupancy']} |")
    return "\n".join(out)


# ---------------------------------------------------------------------------
# measurements (GPU)

def bench_pair(fns, iters, reps):
    """Interleaved timing of several closures: a cold warm-up of every arm,
    then ``reps`` rounds timing ``iters`` calls of every closure in turn;
    returns median seconds/call."""
    import torch

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


def _spmm_table(system, n, matrix_bytes, single, multi, dev, iters, reps):
    import torch

    x = torch.randn(n, dtype=torch.float64, device=dev)
    y = torch.zeros(n, dtype=torch.float64, device=dev)
    arms = {"spmv": lambda: single(x, y), "spmv (repeat)": lambda: single(x, y)}
    keep = []
    for k in KS:
        X = torch.randn(n, k, dtype=torch.float64, device=dev)
        Y = torch.zeros(n, k, dtype=torch.float64, device=dev)
        keep.append((X, Y))
        arms[f"spmm K={k}"] = lambda X=X, Y=Y: multi(X, Y)
    t = bench_pair(arms, iters, reps)
    out = {"system": system, "rows": n, "matrix_bytes": matrix_bytes, "arms": []}
    for name, sec in t.items():
        k = int(name.split("=")[1]) if "=" in name else 1
        nbytes = matrix_bytes + 16 * n * k
        out["arms"].append({"arm": name, "K": k, "us": sec * 1e6,
                            "us_per_rhs": sec * 1e6 / k,
                            "GBps": nbytes / sec / 1e9,
                            "vs_k_spmv": k * t["spmv"] / sec})
    out["spread"] = max(t["spmv"], t["spmv (repeat)"]) / \
        min(t["spmv"], t["spmv (repeat)"])
    return out


def spmm_bsell_ab(G, dof, dev, iters, reps):
    from acg_amd.gen import queen_like_spec
    from acg_amd.gen.device_slab import device_stencil_slab
    from acg_amd.ops import gpu_ops

    S = device_stencil_slab(G, G, G, queen_like_spec(dof), 0, 1, dev)
    bptr, bcol, bvals, dof = S.A_bsell
    n = S.nowned
    return _spmm_table(
        f"queen-like 27pt dof{dof} G{G} (BSELL)", n,
        bcol.numel() * (4 + 8 * dof * dof),
        lambda x, y: gpu_ops.spmv_bsell(bptr, bcol, bvals, n // dof, dof, x, y),
        lambda X, Y: gpu_ops.spmm_bsell(bptr, bcol, bvals, n // dof, dof, X, Y),
        dev, iters, reps)


def spmm_sell_ab(G, dev, iters, reps):
    from acg_amd.gen import STENCIL_7PT_3D
    from acg_amd.gen.device_slab import device_stencil_slab
    from acg_amd.ops import gpu_ops

    S = device_stencil_slab(G, G, G, dict(STENCIL_7PT_3D), 0, 1, dev)
    sellptr, cols, vals = S.A_sell
    n = S.nowned
    return _spmm_table(
        f"poisson 7pt G{G} (SELL)", n, cols.numel() * (cols.element_size() + 8),
        lambda x, y: gpu_ops.spmv_sell(sellptr, cols, vals, n, x, y),
        lambda X, Y: gpu_ops.spmm_sell(sellptr, cols, vals, n, X, Y),
        dev, iters, reps)


def _queen_solver(G, dof, dev):
    from acg_amd.gen import queen_like_spec
    from acg_amd.gen.device_slab import device_stencil_slab
    from acg_amd.solvers.hip import CGSolverHIP

    S = device_stencil_slab(G, G, G, queen_like_spec(dof), 0, 1, dev)
    return S, CGSolverHIP(S, comm=None, device=dev)


def single_ab(G, dof, dev, reps, its):
    """us/iteration of the single-RHS solve at a fixed iteration count, as
    two identical interleaved arms."""
    import numpy as np
    import torch

    S, solver = _queen_solver(G, dof, dev)
    b = torch.from_numpy(np.random.default_rng(1).standard_normal(S.nowned)).to(dev)
    rec = {"solve": [], "solve (repeat)": []}
    for rep in range(reps + 1):  # round 0 warms
        for k in rec:
            x = torch.zeros(S.nowned + S.nghost, dtype=torch.float64, device=dev)
            res = solver.solve(b, x, maxits=its, res_rtol=0.0)
            if rep:
                rec[k].append(res.tsolve / max(res.niterations, 1) * 1e6)
    med = {k: statistics.median(v) for k, v in rec.items()}
    return {"system": f"queen-like 27pt dof{dof} G{G}", "rows": S.nowned,
            "iterations": its, "us_per_it": med,
            "all_us_per_it": rec,
            "spread": max(med.values()) / min(med.values())}


def tts_ab(G, dof, dev, reps, maxits, rtol, ks):
    import numpy as np
    import torch

    S, solver = _queen_solver(G, dof, dev)
    n, nl = S.nowned, S.nowned + S.nghost
    kmax = max(ks)
    B = torch.from_numpy(
        np.random.default_rng(2).standard_normal((n, kmax))).to(dev)
    chk = torch.zeros(n, dtype=torch.float64, device=dev)

    def true_rel(b, x):
        solver._spmv_overlapped(x.contiguous(), chk)
        return float(torch.linalg.norm(b - chk) / torch.linalg.norm(b))

    def sequential(k):
        X = torch.zeros(nl, k, dtype=torch.float64, device=dev)
        its = []
        for c in range(k):
            x = torch.zeros(nl, dtype=torch.float64, device=dev)
            its.append(solver.solve(B[:, c].contiguous(), x, maxits=maxits,
                                    res_rtol=rtol).niterations)
            X[:, c] = x
        return X, its

    def multi(k, group=8):
        X = torch.zeros(nl, k, dtype=torch.float64, device=dev)
        solver.multi_group = group
        res = solver.solve_multi(B[:, :k].contiguous(), X, maxits=maxits,
                                 res_rtol=rtol)
        solver.multi_group = 8
        return X, [r.niterations for r in res]

    out = {"system": f"queen-like 27pt dof{dof} G{G}", "rows": n,
           "format": solver._format_name(), "res_rtol": rtol, "arms": []}
    for k in ks:
        arms = {"sequential": sequential, "sequential (repeat)": sequential,
                "solve_multi": multi}
        if k > 4:
            arms["solve_multi (groups of 4)"] = lambda k: multi(k, 4)
        rec = {a: {"t": []} for a in arms}
        for rep in range(reps + 1):  # round 0 warms every arm
            for a, fn in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                X, its = fn(k)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if rep:
                    rec[a]["t"].append(dt)
                rec[a].update(its=its, true_rel=max(
                    true_rel(B[:, c], X[:, c]) for c in range(k)))
        base = statistics.median(rec["sequential"]["t"])
        for a, r in rec.items():
            med = statistics.median(r["t"])
            out["arms"].append({
                "k": k, "arm": a, "ms": med * 1e3, "min_ms": min(r["t"]) * 1e3,
                "max_ms": max(r["t"]) * 1e3, "speedup": base / med,
                "max_its": max(r["its"]), "sum_its": sum(r["its"]),
                "worst_true_rel": r["true_rel"],
                "us_per_it_per_rhs": med * 1e6 / max(sum(r["its"]), 1)
                if a.startswith("sequential")
                else med * 1e6 / max(max(r["its"]) * k, 1)})
    return out


# ---------------------------------------------------------------------------
# the note

BYTE_ESTIMATE = """\
Byte estimate per row per iteration (the expectation the measurement is
held against): Queen-shaped dof-3 BSELL, ~80 nnz/row, costs ~670 B of
matrix against ~90 B of vector streams, so K = 4 should cut the traffic
per right-hand side roughly 3x; 7-pt Poisson SELL costs ~84 B of matrix
against ~88 B of vectors, so about 1.6x."""


def write_note(result, resources, parent):
    L = ["# Multiple right-hand sides: SpMM kernels and the batched classic CG",
         "",
         "Written by `tools/multirhs_tts.py`.  Layout: multivectors are "
         "contiguous fp64 `(n, K)`, element `(i, c)` at `i*K + c`; the scalar "
         "slab is `(K, 8)`, the partials `(K, MAXG)`.", "", BYTE_ESTIMATE, ""]
    L += ["## Registers and scratch (gfx950, `-Rpass-analysis=kernel-resource-usage`)", ""]
    if resources:
        L += [resources_md(resources), ""]
        spill = [k for k, r in resources.items() if r["scratch"] or r["vgpr_spill"]]
        L += ["No instantiation uses scratch or spills; every (dof, K) pair is "
              "offered by the op layer and the solver never has to split a "
              "group below K = 8 for register reasons."
              if not spill else
              "Instantiations with scratch: " + ", ".join(spill), ""]
    else:
        L += ["(not recorded: run `tools/multirhs_tts.py --resources-only`)", ""]
    measured = bool(result)
    if not measured:
        L += ["## Measurements", "",
              "**No GPU was available when this note was written: every ratio "
              "above is an unmeasured byte estimate.**", ""]
    for tab in result.get("spmm", []):
        L += [f"## SpMM against K x SpMV: {tab['system']}", "",
              f"{tab['rows']} rows, matrix stream {tab['matrix_bytes'] / 1e9:.3f} GB; "
              f"identical-arm spread {100 * (tab['spread'] - 1):.1f} %.", "",
              "| arm | us | us per RHS | effective GB/s | speedup over K x SpMV |",
              "|---|---:|---:|---:|---:|"]
        for a in tab["arms"]:
            L.append(f"| {a['arm']} | {a['us']:.1f} | {a['us_per_rhs']:.1f} | "
                     f"{a['GBps']:.0f} | {a['vs_k_spmv']:.2f} |")
        L.append("")
    t = result.get("tts")
    if t:
        L += [f"## Time to solution: {t['system']} [{t['format']}], "
              f"res_rtol {t['res_rtol']:g}", "",
              "`sequential` = k `solve` calls one after the other; the "
              "repeat arm is identical (run-to-run spread).  `worst true rel` "
              "is the largest ||b_c - A x_c|| / ||b_c|| over the columns, "
              "recomputed with the operator.", "",
              "| k | arm | ms | [min..max] | speedup | max its | worst true rel | us/it per RHS |",
              "|---:|---|---:|---|---:|---:|---:|---:|"]
        for a in t["arms"]:
            L.append(f"| {a['k']} | {a['arm']} | {a['ms']:.1f} | "
                     f"[{a['min_ms']:.1f}..{a['max_ms']:.1f}] | {a['speedup']:.2f} | "
                     f"{a['max_its']} | {a['worst_true_rel']:.2e} | "
                     f"{a['us_per_it_per_rhs']:.1f} |")
        L.append("")
    s = result.get("single")
    if s:
        L += [f"## Single-RHS `solve`, unchanged code: {s['system']}", "",
              f"{s['iterations']} iterations, res_rtol 0, medians of the "
              "interleaved identical arms.", "",
              "| commit | arm | us/it |", "|---|---|---:|"]
        if parent:
            for k, v in parent["us_per_it"].items():
                L.append(f"| parent | {k} | {v:.1f} |")
        for k, v in s["us_per_it"].items():
            L.append(f"| this | {k} | {v:.1f} |")
        L.append("")
        if parent:
            a = statistics.median(parent["us_per_it"].values())
            b = statistics.median(s["us_per_it"].values())
            spread = max(parent["spread"], s["spread"])
            L += [f"Parent {a:.1f} us/it, this commit {b:.1f} us/it: ratio "
                  f"{b / a:.3f}; identical-arm spread within one process "
                  f"{100 * (spread - 1):.1f} % (the two commits ran in "
                  "separate processes, which adds placement noise on top).", ""]
        else:
            L += ["The parent commit was not measured in this run.", ""]
    if measured:
        L += ["## Verdict", ""] + verdict(result) + [""]
    NOTE.write_text("\n".join(L))


def verdict(result):
    out = []
    for tab in result.get("spmm", []):
        best = max((a for a in tab["arms"] if a["K"] > 1),
                   key=lambda a: a["vs_k_spmv"])
        k4 = next(a for a in tab["arms"] if a["K"] == 4)
        single = next(a for a in tab["arms"] if a["K"] == 1)
        # the estimate covers the whole iteration; for the operator alone
        # the bytes say K*(m + v) / (m + K*v), v = 16 B of x and y per row
        m, v = tab["matrix_bytes"], 16 * tab["rows"]
        out.append(f"- {tab['system']}: K = 4 runs {k4['vs_k_spmv']:.2f}x faster "
                   f"than 4 SpMVs where the bytes say {4 * (m + v) / (m + 4 * v):.2f}x; "
                   f"best is {best['arm']} at {best['vs_k_spmv']:.2f}x.  Effective "
                   f"bandwidth falls from {single['GBps']:.0f} GB/s (SpMV) to "
                   f"{k4['GBps']:.0f} (K = 4) and "
                   f"{next(a for a in tab['arms'] if a['K'] == 8)['GBps']:.0f} (K = 8).")
    t = result.get("tts")
    if t:
        for a in t["arms"]:
            if a["arm"].startswith("solve_multi"):
                out.append(f"- {a['arm']}, k = {a['k']}: {a['speedup']:.2f}x "
                           f"the sequential solves at worst true residual "
                           f"{a['worst_true_rel']:.1e}.")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=111)
    ap.add_argument("--poisson", type=int, default=256)
    ap.add_argument("--tts-grid", type=int, default=111)
    ap.add_argument("--dof", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--maxits", type=int, default=5000)
    ap.add_argument("--rtol", type=float, default=1e-9)
    ap.add_argument("--single-its", type=int, default=300)
    ap.add_argument("--skip", default="", help="comma list of spmm,tts,single")
    ap.add_argument("--resources-only", action="store_true")
    ap.add_argument("--single-only", action="store_true")
    ap.add_argument("--parent-json", default=None,
                    help="--single-only --out result of the parent commit")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--no-note", action="store_true")
    ap.add_argument("--from-json", default=None,
                    help="write the note from a saved --out result (no GPU)")
    args = ap.parse_args()
    if args.resources_only:
        rows = resource_table()
        RES_JSON.write_text(json.dumps(rows, indent=1) + "\n")
        print(resources_md(rows))
        return
    resources = json.loads(RES_JSON.read_text()) if RES_JSON.exists() else None
    parent = None
    if args.parent_json and Path(args.parent_json).exists():
        parent = json.loads(Path(args.parent_json).read_text())["single"]
    if args.from_json:
        write_note(json.loads(Path(args.from_json).read_text()), resources, parent)
        return
    import torch

    result = {}
    if not torch.cuda.is_available():
        if not args.no_note:
            write_note(result, resources, None)
        print("no GPU: wrote the note with the byte estimates only")
        return
    dev = torch.device("cuda:0")
    skip = set(args.skip.split(","))
    if args.single_only:
        skip = {"spmm", "tts"}
    if "spmm" not in skip:
        result["spmm"] = [spmm_bsell_ab(args.grid, args.dof, dev, args.iters,
                                        args.reps)]
        torch.cuda.empty_cache()
        result["spmm"].append(spmm_sell_ab(args.poisson, dev, args.iters,
                                           args.reps))
        torch.cuda.empty_cache()
        for tab in result["spmm"]:
            for a in tab["arms"]:
                print(f"SPMM {tab['system']}: {a['arm']:14s} {a['us']:9.1f} us "
                      f"{a['GBps']:7.0f} GB/s  x{a['vs_k_spmv']:.3f} vs K*spmv",
                      flush=True)
    if "single" not in skip:
        result["single"] = single_ab(args.tts_grid, args.dof, dev, args.reps,
                                     args.single_its)
        print("SINGLE", json.dumps(result["single"]["us_per_it"]), flush=True)
        torch.cuda.empty_cache()
    if "tts" not in skip:
        result["tts"] = tts_ab(args.tts_grid, args.dof, dev, args.reps,
                               args.maxits, args.rtol, (4, 8))
        for a in result["tts"]["arms"]:
            print(f"TTS k={a['k']} {a['arm']:20s} {a['ms']:9.2f} ms "
                  f"x{a['speedup']:.3f} its={a['max_its']} "
                  f"true_rel={a['worst_true_rel']:.2e}", flush=True)
    print(json.dumps(result))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(result, indent=1))
    if not args.no_note and not args.single_only:
        write_note(result, resources, parent)


if __name__ == "__main__":
    main()
