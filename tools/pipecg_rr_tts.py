#!/usr/bin/env python3
"""Residual replacement of the pipelined CG: dual-SpMV bandwidth, the cost
of a replacement and time-to-solution on an MI355X, written up as
profiles/pipecg_rr.md.

    python tools/pipecg_rr_tts.py --resources-only          # no GPU needed
    python tools/pipecg_rr_tts.py [--grid 111] [--poisson 256] [--tts-grid 64]
                                  [--steps 400] [--reps 5] [--out FILE.json]
    python tools/pipecg_rr_tts.py --from-json FILE.json [--bench-json FILE]

Everything is interleaved A/B in ONE process and reported as medians, after
a warm-up round of every arm (NOTES.md: run-to-run placement noise is larger
than most effects).  Tables carry two IDENTICAL arms where a ratio is read
off; their ratio is the spread the other ratios have to beat.

(a) One dual pass (``spmv2_*``) against two single SpMVs: BSELL dof 3 at the
    bench's Queen-shaped size (device-generated, G=111) and SELL 7-pt
    Poisson 256^3.  Bytes = matrix stream once (dual) or twice (2 x single)
    + two x and two y.
(b) Cost of one replacement, dual-SpMV fast path against the four-SpMV
    fallback: (time of a fixed-step solve with rr_period=p) - (time of the
    same solve with rr_period=0), divided by the replacements -- and, since
    the plain solve runs on other buffers (placement offset), the slope of
    solve time against the number of replacements over the three periods.
(c) The same solves as per-iteration overhead at rr_period 25 / 50 / 100.
(d) Iterations and time to a TRUE relative residual of 1e-12 on a plain and
    a ``mixed_systems.scaled`` 7-pt system (host-assembled, --tts-grid):
    classic, pipelined, pipelined with replacement, megafused on and off.
    Every arm runs with res_rtol=1e-12; an arm whose returned x misses a
    true residual of 1e-12 ||b|| "did not reach" whatever it reported.

``--bench-json``: lines ``{"arm": "parent"|"this", "solver": ..., "value":
...}`` of bench.py runs that alternate the parent commit and this commit in
one job; folded into the note as the untouched-path comparison.
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
sys.path.insert(0, str(ROOT / "tests"))
RES_JSON = ROOT / "profiles" / "pipecg_rr_resources.json"
NOTE = ROOT / "profiles" / "pipecg_rr.md"
RAW = ROOT / "profiles" / "pipecg_rr.json"
PERIODS = (25, 50, 100)
TRUE_RTOL = 1e-12


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
        if not any(k in mangled for k in ("k_spmv2", "replace_finalize",
                                          "k_dot2_slices")):
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
    """Interleaved timing of several closures: a warm-up of every arm, then
    ``reps`` rounds timing ``iters`` calls of every closure in turn; returns
    median seconds/call."""
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


def _dual_table(system, n, matrix_bytes, single, dual, nlocal, dev, iters, reps):
    import torch

    x1, x2 = (torch.randn(nlocal, dtype=torch.float64, device=dev) for _ in range(2))
    y1, y2 = (torch.zeros(n, dtype=torch.float64, device=dev) for _ in range(2))

    def two():
        single(x1, y1)
        single(x2, y2)

    t = bench_pair({"2 x spmv": two, "2 x spmv (repeat)": two,
                    "spmv2": lambda: dual(x1, x2, y1, y2)}, iters, reps)
    out = {"system": system, "rows": n, "matrix_bytes": matrix_bytes, "arms": []}
    for name, sec in t.items():
        nbytes = (1 if name == "spmv2" else 2) * matrix_bytes + 32 * n
        out["arms"].append({"arm": name, "us": sec * 1e6, "bytes": nbytes,
                            "GBps": nbytes / sec / 1e9,
                            "speedup_vs_2x": t["2 x spmv"] / sec})
    return out


def dual_bsell(G, dof, dev, iters, reps):
    from acg_amd.gen import queen_like_spec
    from acg_amd.gen.device_slab import device_stencil_slab
    from acg_amd.ops import gpu_ops

    S = device_stencil_slab(G, G, G, queen_like_spec(dof), 0, 1, dev)
    bptr, bcol, bvals, dof = S.A_bsell
    n, nl = S.nowned, S.nowned + S.nghost
    mb = bcol.numel() * (4 + 8 * dof * dof)
    return _dual_table(
        f"queen-like 27pt dof{dof} G{G} (BSELL)", n, mb,
        lambda x, y: gpu_ops.spmv_bsell(bptr, bcol, bvals, n // dof, dof, x, y),
        lambda a, b, c, d: gpu_ops.spmv2_bsell(bptr, bcol, bvals, n // dof, dof,
                                               a, b, c, d, ncols=nl),
        nl, dev, iters, reps)


def dual_sell(G, dev, iters, reps):
    from acg_amd.gen import STENCIL_7PT_3D
    from acg_amd.gen.device_slab import device_stencil_slab
    from acg_amd.ops import gpu_ops

    S = device_stencil_slab(G, G, G, dict(STENCIL_7PT_3D), 0, 1, dev)
    sp, sc, sv = S.A_sell
    n, nl = S.nowned, S.nowned + S.nghost
    mb = sc.numel() * (sc.element_size() + 8)
    return _dual_table(
        f"poisson 7pt G{G} (SELL)", n, mb,
        lambda x, y: gpu_ops.spmv_sell(sp, sc, sv, n, x, y),
        lambda a, b, c, d: gpu_ops.spmv2_sell(sp, sc, sv, n, a, b, c, d, ncols=nl),
        nl, dev, iters, reps)


def replacement_cost(system, S, dev, steps, reps, **solver_kw):
    """(b) + (c): fixed-step solves (res_rtol=0), rr_period 0 twice (the
    spread), then every period on the fast path and on the fallback."""
    import torch

    from acg_amd.solvers.hip import CGSolverHIP

    solver = CGSolverHIP(S, device=dev, **solver_kw)
    n = S.nowned
    b = torch.randn(n, dtype=torch.float64, device=dev)
    arms = {"plain": (0, True), "plain (repeat)": (0, True)}
    for p in PERIODS:
        arms[f"rr {p} dual"] = (p, True)
        arms[f"rr {p} 4 x spmv"] = (p, False)
    times = {k: [] for k in arms}
    nrep = {}
    for rep in range(reps + 1):  # round 0 warms every arm
        for k, (p, fast) in arms.items():
            solver._rr_fast = fast
            x = torch.zeros(n + S.nghost, dtype=torch.float64, device=dev)
            res = solver.solve_pipelined(b, x, maxits=steps, res_rtol=0.0,
                                         rr_period=p)
            nrep[k] = res.nreplacements
            if rep:
                times[k].append(res.tsolve)
    solver._rr_fast = True
    base = statistics.median(times["plain"])
    out = {"system": system, "format": solver._format_name(), "rows": n,
           "steps": steps, "megafused": bool(solver.megafuse_auto), "arms": []}
    for k, v in times.items():
        med = statistics.median(v)
        out["arms"].append({
            "arm": k, "ms": med * 1e3, "us_per_it": med / steps * 1e6,
            "vs_plain": med / base, "nreplacements": nrep[k],
            "us_per_replacement": ((med - base) / nrep[k] * 1e6
                                   if nrep[k] else None)})
    del solver
    torch.cuda.empty_cache()
    return out


def tts(G, scaled, dev, reps, maxits):
    """(d): time and iterations to a true relative residual of 1e-12."""
    import numpy as np
    import torch

    import mixed_systems as ms
    from acg_amd.gen import STENCIL_7PT_3D, stencil_global
    from acg_amd.solvers.hip import CGSolverHIP

    A = stencil_global(G, G, G, dict(STENCIL_7PT_3D))
    if scaled:
        A = ms.scaled(A)
    S = ms.local(A)
    del A
    solver = CGSolverHIP(S, device=dev)
    b = torch.from_numpy(np.random.default_rng(1).standard_normal(S.nowned)).to(dev)
    bn = float(torch.linalg.norm(b))
    chk = torch.zeros(S.nowned, dtype=torch.float64, device=dev)

    def true_rel(x):
        solver._spmv_overlapped(x, chk)
        return float(torch.linalg.norm(b - chk)) / bn

    kw = dict(maxits=maxits, res_rtol=TRUE_RTOL)
    arms = {"classic": lambda x: solver.solve(b, x, **kw),
            "classic (repeat)": lambda x: solver.solve(b, x, **kw)}
    for mega in (False, True):
        tag = "megafused" if mega else "split"
        arms[f"pipelined {tag}"] = lambda x, m=mega: solver.solve_pipelined(
            b, x, megafuse=m, **kw)
        for p in PERIODS:
            arms[f"pipelined {tag} rr {p}"] = lambda x, m=mega, p=p: \
                solver.solve_pipelined(b, x, megafuse=m, rr_period=p, **kw)
    rec = {k: {"t": []} for k in arms}
    for rep in range(reps + 1):  # round 0 warms every arm
        for k, fn in arms.items():
            x = torch.zeros(S.nowned + S.nghost, dtype=torch.float64, device=dev)
            res = fn(x)
            if rep:
                rec[k]["t"].append(res.tsolve)
            rec[k].update(its=res.niterations, converged=res.converged,
                          nrepl=res.nreplacements, true_rel=true_rel(x))
    base = statistics.median(rec["classic"]["t"])
    out = {"system": f"poisson 7pt G{G}" + (", scaled" if scaled else ""),
           "format": solver._format_name(), "rows": S.nowned, "arms": []}
    for k, r in rec.items():
        med = statistics.median(r["t"])
        out["arms"].append({
            "arm": k, "ms": med * 1e3, "vs_classic": med / base, "its": r["its"],
            "reported_converged": r["converged"], "true_rel": r["true_rel"],
            "reached": bool(r["true_rel"] <= TRUE_RTOL * 1.0000001),
            "nreplacements": r["nrepl"],
            "us_per_it": med / max(r["its"], 1) * 1e6})
    del solver
    torch.cuda.empty_cache()
    return out


# ---------------------------------------------------------------------------
# the note

def _fit(pts):
    """Least-squares line through (x, y) points: (slope, intercept)."""
    n = len(pts)
    mx = sum(x for x, _ in pts) / n
    my = sum(y for _, y in pts) / n
    sxx = sum((x - mx) ** 2 for x, _ in pts)
    slope = sum((x - mx) * (y - my) for x, y in pts) / sxx
    return slope, my - slope * mx


def write_note(result, resources, bench):
    L = ["# Pipelined CG with residual replacement on a dual SpMV", "",
         "Written by `tools/pipecg_rr_tts.py`; raw numbers in "
         "`pipecg_rr.json`, kernel resources in `pipecg_rr_resources.json`.  "
         "Interleaved same-process medians on one MI355X.", ""]
    L += ["## Kernel resources (gfx950, compiler remarks)", ""]
    if resources:
        L += [resources_md(resources), ""]
        spill = [k for k, r in resources.items() if r["scratch"] or r["vgpr_spill"]]
        L += ["No kernel uses scratch." if not spill
              else f"Kernels with scratch or spills: {spill}.", ""]
    else:
        L += ["(not recorded: run `tools/pipecg_rr_tts.py --resources-only`)", ""]
    if result.get("dual"):
        L += ["## (a) One dual pass against two single SpMVs", "",
              "| system | arm | us | GB/s | speed-up vs 2 x spmv |",
              "|---|---|---:|---:|---:|"]
        for t in result["dual"]:
            for a in t["arms"]:
                L.append(f"| {t['system']} | {a['arm']} | {a['us']:.1f} | "
                         f"{a['GBps']:.0f} | {a['speedup_vs_2x']:.3f} |")
        L.append("")
    if result.get("replace"):
        L += ["## (b), (c) Cost of a replacement and per-iteration overhead", "",
              "Fixed-step pipelined solves, res_rtol 0.  `dual` = two "
              "dual-SpMV launches + finalize, `4 x spmv` = the fallback.", "",
              "| system | arm | us/it | vs plain | replacements | us per replacement |",
              "|---|---|---:|---:|---:|---:|"]
        for t in result["replace"]:
            tag = f"{t['system']} [{t['format']}{', megafused' if t['megafused'] else ''}]"
            for a in t["arms"]:
                upr = ("" if a["us_per_replacement"] is None
                       else f"{a['us_per_replacement']:.0f}")
                L.append(f"| {tag} | {a['arm']} | {a['us_per_it']:.1f} | "
                         f"{a['vs_plain']:.3f} | {a['nreplacements']} | {upr} |")
        L += ["", "The last column subtracts the plain solve, which runs on "
              "OTHER buffers (the replacement workspace is allocated under "
              "its own key), so it carries the per-allocation placement "
              "offset of NOTES.md and can even come out negative.  The fit "
              "below stays inside one workspace: solve time against the "
              "number of replacements over the three periods, slope = one "
              "replacement, intercept = the iteration without any.", "",
              "| system | path | us per replacement (slope) | us/it at 0 "
              "replacements (intercept) | plain us/it | overhead at 25 / 50 / 100 |",
              "|---|---|---:|---:|---:|---|"]
        for t in result["replace"]:
            plain = next(a for a in t["arms"] if a["arm"] == "plain")["us_per_it"]
            for path in ("dual", "4 x spmv"):
                pts = [(a["nreplacements"], a["ms"]) for a in t["arms"]
                       if a["arm"].endswith(path)]
                slope, icpt = _fit(pts)
                it0 = icpt / t["steps"] * 1e3
                ov = " / ".join(f"{slope * 1e3 / p / it0 * 100:.1f} %" for p in PERIODS)
                L.append(f"| {t['system']} | {path} | {slope * 1e3:.0f} | {it0:.1f} | "
                         f"{plain:.1f} | {ov} |")
        L.append("")
    if result.get("tts"):
        L += [f"## (d) To a true relative residual of {TRUE_RTOL:g}", "",
              "Every arm runs with res_rtol 1e-12; `reached` compares the "
              "recomputed ||b - A x|| / ||b|| of the returned x with 1e-12.", "",
              "| system | arm | its | ms | vs classic | reported | true residual | reached |",
              "|---|---|---:|---:|---:|---|---:|---|"]
        for t in result["tts"]:
            for a in t["arms"]:
                L.append(f"| {t['system']} ({t['rows']} rows) | {a['arm']} | "
                         f"{a['its']} | {a['ms']:.2f} | {a['vs_classic']:.3f} | "
                         f"{'converged' if a['reported_converged'] else 'not converged'} | "
                         f"{a['true_rel']:.2e} | {'yes' if a['reached'] else 'NO'} |")
        L.append("")
    if bench:
        L += ["## The untouched path: bench.py, parent commit against this commit", "",
              "Alternating runs in one job, default flags apart from "
              "`--solver`; value = the bench's headline figure (iterations/s).", ""]
        for solver in sorted({r["solver"] for r in bench}):
            L += ["| solver | run | parent | this commit |", "|---|---:|---:|---:|"]
            pa = [r["value"] for r in bench if r["solver"] == solver and r["arm"] == "parent"]
            th = [r["value"] for r in bench if r["solver"] == solver and r["arm"] == "this"]
            for i, (p, t) in enumerate(zip(pa, th)):
                L.append(f"| {solver} | {i + 1} | {p:.4g} | {t:.4g} |")
            if pa and th:
                mp, mt = statistics.median(pa), statistics.median(th)
                spread = max(max(pa) / min(pa), max(th) / min(th)) - 1.0
                L.append(f"| {solver} | median | {mp:.4g} | {mt:.4g} |")
                L += ["", f"{solver}: this / parent = {mt / mp:.4f}; spread of "
                      f"identical runs {spread * 100:.1f} % (box band 8 %).", ""]
    NOTE.write_text("\n".join(L) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=111)
    ap.add_argument("--poisson", type=int, default=256)
    ap.add_argument("--tts-grid", type=int, default=64)
    ap.add_argument("--dof", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--maxits", type=int, default=5000)
    ap.add_argument("--skip", default="", help="comma list of dual,replace,tts")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--from-json", default=None)
    ap.add_argument("--bench-json", default=None)
    ap.add_argument("--resources-only", action="store_true")
    args = ap.parse_args()
    if args.resources_only:
        rows = resource_table()
        RES_JSON.write_text(json.dumps(rows, indent=1) + "\n")
        print(resources_md(rows))
        return
    resources = json.loads(RES_JSON.read_text()) if RES_JSON.exists() else None
    bench = None
    if args.bench_json:
        bench = [json.loads(l) for l in Path(args.bench_json).read_text().splitlines()
                 if l.startswith("{")]
    if args.from_json:
        result = json.loads(Path(args.from_json).read_text())
        if bench:
            result["bench"] = bench
        bench = result.get("bench")
        RAW.write_text(json.dumps(result, indent=1) + "\n")
        write_note(result, resources, bench)
        return
    import torch

    assert torch.cuda.is_available(), "pipecg_rr_tts measures on the GPU only"
    dev = torch.device("cuda:0")
    skip = set(args.skip.split(","))
    result = {}

    def save():
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text(json.dumps(result, indent=1))

    if "dual" not in skip:
        result["dual"] = [dual_bsell(args.grid, args.dof, dev, args.iters, args.reps)]
        torch.cuda.empty_cache()
        result["dual"].append(dual_sell(args.poisson, dev, args.iters, args.reps))
        torch.cuda.empty_cache()
        for t in result["dual"]:
            for a in t["arms"]:
                print(f"DUAL {t['system']}: {a['arm']:18s} {a['us']:.1f} us "
                      f"{a['GBps']:.0f} GB/s x{a['speedup_vs_2x']:.3f}", flush=True)
        save()
    if "replace" not in skip:
        from acg_amd.gen import STENCIL_7PT_3D, queen_like_spec
        from acg_amd.gen.device_slab import device_stencil_slab

        result["replace"] = []
        for system, mk in (
                (f"queen-like 27pt dof{args.dof} G{args.grid}",
                 lambda: device_stencil_slab(args.grid, args.grid, args.grid,
                                             queen_like_spec(args.dof), 0, 1, dev)),
                (f"poisson 7pt G{args.poisson}",
                 lambda: device_stencil_slab(args.poisson, args.poisson,
                                             args.poisson, dict(STENCIL_7PT_3D),
                                             0, 1, dev))):
            t = replacement_cost(system, mk(), dev, args.steps, args.reps)
            result["replace"].append(t)
            for a in t["arms"]:
                print(f"REPLACE {system} [{t['format']}]: {a['arm']:16s} "
                      f"{a['us_per_it']:.1f} us/it x{a['vs_plain']:.3f} "
                      f"nrepl={a['nreplacements']} "
                      f"us/repl={a['us_per_replacement']}", flush=True)
            save()
    if "tts" not in skip:
        result["tts"] = []
        for scaled in (False, True):
            t = tts(args.tts_grid, scaled, dev, args.reps, args.maxits)
            result["tts"].append(t)
            for a in t["arms"]:
                print(f"TTS {t['system']}: {a['arm']:26s} its={a['its']} "
                      f"{a['ms']:.2f} ms x{a['vs_classic']:.3f} "
                      f"conv={a['reported_converged']} true={a['true_rel']:.2e} "
                      f"reached={a['reached']}", flush=True)
            save()
    print(json.dumps(result))
    save()


if __name__ == "__main__":
    main()
