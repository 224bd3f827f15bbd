#!/usr/bin/env python3
"""Block CG for several right-hand sides: kernel bandwidth and
time-to-solution A/B on an MI355X, written up as profiles/block_cg.md.

    python tools/blockcg_tts.py --resources-only       # no GPU needed
    python tools/blockcg_tts.py [--grid 111] [--poisson 256] [--ill 160]
                                [--reps 3] [--parent-json FILE] [--out FILE.json]
    python tools/blockcg_tts.py --unchanged-only [--root DIR] --out FILE.json
    python tools/blockcg_tts.py --from-json FILE.json [--parent-json FILE]

Conventions of tools/multirhs_tts.py: every arm is warmed, arms are
interleaved in ONE process, tables report medians with [min..max], and every
table carries an identical repeat arm whose ratio to its twin is the spread
the other ratios have to beat.

(a) us and effective GB/s of gram_multi, block_update, block_ortho and the
    two coefficient kernels at K = 2, 4, 8, at the row counts of the
    Queen-shaped G111 dof-3 system and of 7-pt Poisson G256.
(b) Time to solution of ``solve_block`` against ``solve_multi`` (twice: the
    baseline and its repeat) against sequential ``solve`` for k = 4, 8 on the
    device-generated Queen-shaped system, 7-pt Poisson, and the same 7-pt
    operator under the row/column scaling s_i a_ij s_j, s in [0.5, 2) from
    default_rng(0), of tests/mixed_systems.scaled (the ill-conditioned one).
(c) us/iteration of the unchanged ``solve`` and ``solve_multi``
    (``--unchanged-only``; with ``--root`` pointing at a checkout of the
    parent commit it gives ``--parent-json``).
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
RES_JSON = ROOT / "profiles" / "block_cg_resources.json"
NOTE = ROOT / "profiles" / "block_cg.md"
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
        if "k_gram_multi" not in mangled and "k_block_" not in mangled:
            continue
        name = subprocess.run(["c++filt", mangled], capture_output=True,
                              text=True).stdout.strip()
        name = re.sub(r"^void ", "", name).split("(")[0]

        def g(key):
            return int(re.search(key + r": (\d+)", blk).group(1))

        rows[name] = {"vgprs": g("VGPRs"), "agprs": g("AGPRs"),
                      "scratch": g(r"ScratchSize \[bytes/lane\]"),
                      "occupancy": g(r"Occupancy \[waves/SIMD\]"),
                      "vgpr_spill": g("VGPRs Spill"),
                      "lds": g(r"LDS Size \[bytes/block\]")}
    return dict(sorted(rows.items()))


def resources_md(rows):
    out = ["| kernel | VGPRs | AGPRs | scratch B/lane | VGPR spills | LDS B/block | waves/SIMD |",
           "|---|---:|---:|---:|---:|---:|---:|"]
    for name, r in rows.items():
        out.append(f"| `{name}` | {r['vgprs']} | {r['agprs']} | {r['scratch']} "
                   f"| {r['vgpr_spill']} | {r['lds']} | {r['occupancy']} |")
    return "\n".join(out)


# ---------------------------------------------------------------------------
# measurements (GPU)

def bench(fns, iters, reps):
    """Interleaved timing: warm every arm, then ``reps`` rounds of ``iters``
    calls of every closure in turn; seconds/call of every round."""
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
    return times


def kernel_table(system, n, dev, iters, reps):
    """The five block kernels at K = 2, 4, 8 on n rows.  The coefficients are
    a well-conditioned state (identity matrices), so the kernels run their
    full path; bytes are the streams each kernel has to move once."""
    import torch

    from acg_amd.ops import gpu_ops as G

    arms, streams = {}, {}
    keep = []
    for k in KS:
        X, Sm, Q, T = (torch.randn(n, k, dtype=torch.float64, device=dev)
                       for _ in range(4))
        partials = G.alloc_partials_multi(dev, k)
        state = G.alloc_block_state(dev)
        rr_out = torch.zeros(k + 2, dtype=torch.float64, device=dev)
        eye = torch.eye(8, dtype=torch.float64, device=dev).reshape(-1)
        for base in (G.BS_XI, G.BS_ZETA, G.BS_ZINV, G.BS_C):
            state[base:base + 64] = eye
        state[G.BS_XIC:G.BS_XIC + 64] = 1e-3 * eye
        nb = G.gram_multi(Q, Q, partials, n=n)
        keep.append((X, Sm, Q, T, partials, state, rr_out))
        arms[f"gram_multi K={k}"] = \
            lambda Sm=Sm, T=T, p=partials: G.gram_multi(Sm, T, p, n=n)
        streams[f"gram_multi K={k}"] = 2
        arms[f"block_update K={k}"] = \
            lambda X=X, Sm=Sm, Q=Q, T=T, s=state, p=partials: \
            G.block_update(X, Sm, Q, T, s, p, n)
        streams[f"block_update K={k}"] = 6
        arms[f"block_ortho K={k}"] = \
            lambda Sm=Sm, Q=Q, s=state: G.block_ortho(Q, Sm, s, n)
        streams[f"block_ortho K={k}"] = 4
        # coefficient kernels on Gram partials of orthonormal-ish columns
        Qn = torch.linalg.qr(torch.randn(4096, k, dtype=torch.float64,
                                         device=dev))[0].contiguous()
        pc = G.alloc_partials_multi(dev, k)
        nbc = G.gram_multi(Qn, Qn, pc)
        pfull = G.alloc_partials_multi(dev, k)
        pfull.view(-1)[:] = 0.0
        for p in range(k * (k + 1) // 2):
            seg = pc.view(-1)[p * G.BLOCK_MAXG:p * G.BLOCK_MAXG + nbc].sum() / nb
            pfull.view(-1)[p * G.BLOCK_MAXG:p * G.BLOCK_MAXG + nb] = seg
        keep.append((Qn, pc, pfull))
        arms[f"block_coef_alpha K={k}"] = \
            lambda p=pfull, s=state, k=k: G.block_coef_alpha(p, nb, s, k, k, 1)
        arms[f"block_coef_beta K={k}"] = \
            lambda p=pfull, s=state, r=rr_out, k=k: \
            G.block_coef_beta(p, nb, s, r, k, k, 1, init=True)
        streams[f"block_coef_alpha K={k}"] = streams[f"block_coef_beta K={k}"] = 0
    arms["gram_multi K=4 (repeat)"] = arms["gram_multi K=4"]
    streams["gram_multi K=4 (repeat)"] = 2
    t = bench(arms, iters, reps)
    flagged = any(float(st[5][G.BS_FLAG]) != 0.0 for st in keep[::2])
    out = {"system": system, "rows": n, "nblocks": nb, "flagged": flagged,
           "arms": []}
    for name, secs in t.items():
        k = int(re.search(r"K=(\d)", name).group(1))
        med = statistics.median(secs)
        nbytes = streams[name] * 8 * n * k
        out["arms"].append({"arm": name, "K": k, "us": med * 1e6,
                            "min_us": min(secs) * 1e6, "max_us": max(secs) * 1e6,
                            "bytes": nbytes,
                            "GBps": nbytes / med / 1e9 if nbytes else None})
    a, b = (statistics.median(t[nm]) for nm in
            ("gram_multi K=4", "gram_multi K=4 (repeat)"))
    out["spread"] = max(a, b) / min(a, b)
    return out


def scale_sell_(S, dev):
    """s_i a_ij s_j on the SELL-C-64 arrays of a device slab, s in [0.5, 2)
    from default_rng(0) (tests/mixed_systems.scaled on the device layout)."""
    import numpy as np
    import torch

    sellptr, cols, vals = S.A_sell
    s = torch.from_numpy(np.random.default_rng(0).uniform(
        0.5, 2.0, size=S.nowned + S.nghost)).to(dev)
    nsl = sellptr.numel() - 1
    sl = torch.repeat_interleave(torch.arange(nsl, device=dev),
                                 sellptr[1:] - sellptr[:-1])
    lane = (torch.arange(vals.numel(), device=dev) - sellptr[sl]) % 64
    row = torch.clamp(sl * 64 + lane, max=S.nowned - 1)
    vals.mul_(s[row] * s[cols.long()])


def make_system(kind, G, dof, dev):
    from acg_amd.gen import STENCIL_7PT_3D, queen_like_spec
    from acg_amd.gen.device_slab import device_stencil_slab
    from acg_amd.solvers.hip import CGSolverHIP

    if kind == "queen":
        S = device_stencil_slab(G, G, G, queen_like_spec(dof), 0, 1, dev)
        name = f"queen-like 27pt dof{dof} G{G}"
    else:
        S = device_stencil_slab(G, G, G, dict(STENCIL_7PT_3D), 0, 1, dev)
        name = f"poisson 7pt G{G}"
        if kind == "scaled":
            scale_sell_(S, dev)
            name += ", scaled s_i a_ij s_j"
    return name, S, CGSolverHIP(S, comm=None, device=dev)


def tts_ab(kind, G, dof, dev, reps, maxits, rtol, ks):
    import numpy as np
    import torch

    name, S, solver = make_system(kind, G, dof, dev)
    n, nl = S.nowned, S.nowned + S.nghost
    B = torch.from_numpy(
        np.random.default_rng(2).standard_normal((n, max(ks)))).to(dev)
    chk = torch.zeros(n, dtype=torch.float64, device=dev)

    def true_rel(b, x):
        solver._spmv_overlapped(x.contiguous(), chk)
        return float(torch.linalg.norm(b - chk) / torch.linalg.norm(b))

    def sequential(k):
        X = torch.zeros(nl, k, dtype=torch.float64, device=dev)
        res = []
        for c in range(k):
            x = torch.zeros(nl, dtype=torch.float64, device=dev)
            res.append(solver.solve(B[:, c].contiguous(), x, maxits=maxits,
                                    res_rtol=rtol))
            X[:, c] = x
        return X, res

    def multi(k):
        X = torch.zeros(nl, k, dtype=torch.float64, device=dev)
        return X, solver.solve_multi(B[:, :k].contiguous(), X, maxits=maxits,
                                     res_rtol=rtol)

    def block(k):
        X = torch.zeros(nl, k, dtype=torch.float64, device=dev)
        return X, solver.solve_block(B[:, :k].contiguous(), X, maxits=maxits,
                                     res_rtol=rtol)

    out = {"system": name, "kind": kind, "rows": n,
           "format": solver._format_name(), "res_rtol": rtol, "arms": []}
    for k in ks:
        arms = {"solve_multi": multi, "solve_multi (repeat)": multi,
                "solve_block": block, "sequential solve": sequential}
        rec = {a: {"t": []} for a in arms}
        for rep in range(reps + 1):  # round 0 warms every arm
            for a, fn in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                X, res = fn(k)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if rep:
                    rec[a]["t"].append(dt)
                rec[a].update(
                    its=[r.niterations for r in res],
                    converged=all(r.converged for r in res),
                    breakdown=max(r.block_breakdown for r in res),
                    true_rel=max(true_rel(B[:, c], X[:, c]) for c in range(k)))
        base = statistics.median(rec["solve_multi"]["t"])
        for a, r in rec.items():
            med = statistics.median(r["t"])
            seq = a.startswith("sequential")
            out["arms"].append({
                "k": k, "arm": a, "ms": med * 1e3, "min_ms": min(r["t"]) * 1e3,
                "max_ms": max(r["t"]) * 1e3, "vs_multi": base / med,
                "max_its": max(r["its"]), "sum_its": sum(r["its"]),
                "converged": r["converged"], "breakdown": r["breakdown"],
                "worst_true_rel": r["true_rel"],
                "us_per_it_per_rhs": med * 1e6 / max(sum(r["its"]), 1) if seq
                else med * 1e6 / max(max(r["its"]) * k, 1)})
            print(f"TTS {name} k={k} {a:22s} {med * 1e3:9.2f} ms "
                  f"x{base / med:.3f} its={max(r['its'])} "
                  f"true_rel={r['true_rel']:.2e}", flush=True)
    del solver, S
    torch.cuda.empty_cache()
    return out


def span_breakdown(kind, G, dof, dev, k, maxits, rtol):
    """One profiled solve of solve_multi and of solve_block (event pairs
    around every span; the second of two runs): where an iteration's time
    goes, and how much of the wall time lies outside the iteration."""
    import numpy as np
    import torch

    from acg_amd.solvers.hip import CGSolverHIP

    name, S, _ = make_system(kind, G, dof, dev)
    solver = CGSolverHIP(S, comm=None, device=dev, profile=True)
    solver.prof.reset = lambda: None  # keep the pairs the solvers would drop
    n, nl = S.nowned, S.nowned + S.nghost
    B = torch.from_numpy(np.random.default_rng(2).standard_normal((n, k))).to(dev)
    out = {"system": name, "k": k, "arms": {}}
    for arm in ("solve_multi", "solve_block"):
        for rep in range(2):
            solver.prof.pairs.clear()
            X = torch.zeros(nl, k, dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = getattr(solver, arm)(B, X, maxits=maxits, res_rtol=rtol)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
        spans = {nm: {"ms": st.seconds * 1e3, "count": st.count}
                 for nm, st in solver.prof.collect().items()}
        out["arms"][arm] = {"wall_ms": wall * 1e3, "spans": spans,
                            "max_its": max(r.niterations for r in res)}
        print(f"SPANS {name} k={k} {arm}: wall {wall * 1e3:.2f} ms "
              + " ".join(f"{nm}={v['ms']:.2f}ms/{v['count']}"
                         for nm, v in spans.items()), flush=True)
    del solver, S
    torch.cuda.empty_cache()
    return out


def unchanged_ab(G, dof, dev, reps, its):
    """us/iteration of solve and of solve_multi (k = 4) at a fixed iteration
    count, each as two identical interleaved arms."""
    import numpy as np
    import torch

    name, S, solver = make_system("queen", G, dof, dev)
    n, nl = S.nowned, S.nowned + S.nghost
    B = torch.from_numpy(np.random.default_rng(1).standard_normal((n, 4))).to(dev)
    b = B[:, 0].contiguous()

    def one():
        x = torch.zeros(nl, dtype=torch.float64, device=dev)
        r = solver.solve(b, x, maxits=its, res_rtol=0.0)
        return r.tsolve / max(r.niterations, 1) * 1e6

    def four():
        X = torch.zeros(nl, 4, dtype=torch.float64, device=dev)
        r = solver.solve_multi(B, X, maxits=its, res_rtol=0.0)
        return r[0].tsolve / its * 1e6

    rec = {"solve": [], "solve (repeat)": [], "solve_multi k=4": [],
           "solve_multi k=4 (repeat)": []}
    for rep in range(reps + 1):  # round 0 warms
        for key in rec:
            v = one() if key.startswith("solve (") or key == "solve" else four()
            if rep:
                rec[key].append(v)
    med = {k: statistics.median(v) for k, v in rec.items()}
    spread = max(max(med["solve"], med["solve (repeat)"])
                 / min(med["solve"], med["solve (repeat)"]),
                 max(med["solve_multi k=4"], med["solve_multi k=4 (repeat)"])
                 / min(med["solve_multi k=4"], med["solve_multi k=4 (repeat)"]))
    return {"system": name, "rows": n, "iterations": its, "us_per_it": med,
            "all_us_per_it": rec, "spread": spread}


# ---------------------------------------------------------------------------
# the note

EXPECTATION = """\
Expectation, stated before measuring.  A block iteration moves, per row
and per column, 2 streams in `gram_multi` (S, T), 6 in `block_update`
(X read + write, S, Q read + write, T) and 4 in `block_ortho` (Q and S read
+ write): 12 x 8 B = 96 B against the 9 x 8 = 72 B of the batched classic
iteration (`cg_fused_update_multi`: R and X read + write, P, T;
`daypx_ratio_multi`: P read + write, R), on top of the same SpMM without
its fused dot.  The vector part of a block iteration should therefore
cost about 1.33x that of `solve_multi`, plus two one-workgroup
coefficient kernels whose cost does not depend on n; per iteration block
CG can only lose.  It wins where the iteration count falls by more than that: the
triage prototype saw up to 2.3x fewer iterations on ill-conditioned
systems and 1.1-1.4x on the Queen-shaped one.  The n-sized kernels map one
row per thread, so at K = 8 every 16-byte access of a wave strides 64 B;
`multi_rhs.md` measured that shape at 2.6 TB/s for the fused update, and
the same ceiling is expected here.  Fusing the M = S^T T Gram into the SpMM
kernels (out of scope here) would save the 2 `gram_multi` streams, 16 B of
the 96."""


NOT_KEPT = """\
Nontemporal loads and stores for Q in `k_block_ortho`.  In the span table
the SpMM costs about 1.5x more inside the block iteration than inside
`solve_multi` on the Queen-shaped system at K = 4, which is its
stand-alone time in `multi_rhs.md`; the supposed cause is that `daypx`
leaves the direction multivector in the Infinity Cache while `block_ortho`
moves four multivectors.  Sending Q through NT accesses was meant to keep S
resident; measured on the same system it changed nothing for the SpMM
(1007 us per call) and slowed `block_ortho` (110 against 91 us), so it was
reverted.  The cause stays a supposition: no cache counters were
collected."""


def _kernel_md(tab):
    L = [f"## Kernels: {tab['system']}", "",
         f"{tab['rows']} rows, {tab['nblocks']} blocks; identical-arm spread "
         f"{100 * (tab['spread'] - 1):.1f} %.", "",
         "| kernel | us | [min..max] | stream bytes | effective GB/s |",
         "|---|---:|---|---:|---:|"]
    for a in tab["arms"]:
        gb = f"{a['GBps']:.0f}" if a["GBps"] else "-"
        by = f"{a['bytes'] / 1e9:.3f} GB" if a["bytes"] else "-"
        L.append(f"| {a['arm']} | {a['us']:.1f} | [{a['min_us']:.1f}..{a['max_us']:.1f}] "
                 f"| {by} | {gb} |")
    if tab.get("flagged"):
        L += ["", "**The benchmark state broke down: the row kernels ran their "
                  "early-exit path, the numbers above are not kernel times.**"]
    return L + [""]


def _tts_md(t):
    L = [f"## Time to solution: {t['system']} [{t['format']}], "
         f"res_rtol {t['res_rtol']:g}", "",
         f"{t['rows']} rows.  `vs multi` is the median of the `solve_multi` "
         "baseline arm over the arm's median; its repeat arm is identical "
         "code.  `worst true rel` is the largest ||b_c - A x_c|| / ||b_c||, "
         "recomputed with the operator.", "",
         "| k | arm | ms | [min..max] | vs multi | max its | hand-over | worst true rel | us/it per RHS |",
         "|---:|---|---:|---|---:|---:|---:|---:|---:|"]
    for a in t["arms"]:
        L.append(f"| {a['k']} | {a['arm']} | {a['ms']:.1f} | "
                 f"[{a['min_ms']:.1f}..{a['max_ms']:.1f}] | {a['vs_multi']:.2f} | "
                 f"{a['max_its']}{'' if a['converged'] else ' (not converged)'} | "
                 f"{a['breakdown'] if a['breakdown'] >= 0 else '-'} | "
                 f"{a['worst_true_rel']:.2e} | {a['us_per_it_per_rhs']:.1f} |")
    return L + [""]


def _spans_md(sp):
    L = [f"## Where the time goes: {sp['system']}, k = {sp['k']}", "",
         "One profiled solve per arm (event pairs around every span, which "
         "adds a few us per span); `outside` is the wall time not covered by "
         "a span: residual set-up, host tests, copies, and for block CG the "
         "start-up orthonormalisation.", "",
         "| arm | span | calls | ms | us per call |", "|---|---|---:|---:|---:|"]
    for arm, a in sp["arms"].items():
        tot = 0.0
        for nm, v in a["spans"].items():
            tot += v["ms"]
            L.append(f"| {arm} | {nm} | {v['count']} | {v['ms']:.2f} | "
                     f"{1e3 * v['ms'] / max(v['count'], 1):.1f} |")
        L.append(f"| {arm} | outside | - | {a['wall_ms'] - tot:.2f} | - |")
        L.append(f"| {arm} | wall | - | {a['wall_ms']:.2f} | - |")
    return L + [""]


def verdict(result):
    out, tally = [], {}
    for t in result.get("tts", []):
        for k in sorted({a["k"] for a in t["arms"]}):
            arm = {a["arm"]: a for a in t["arms"] if a["k"] == k}
            m, r, b = (arm[x] for x in ("solve_multi", "solve_multi (repeat)",
                                        "solve_block"))
            spread = max(m["ms"], r["ms"]) / min(m["ms"], r["ms"])
            ratio = m["ms"] / b["ms"]
            word = ("ties with" if 1 / spread <= ratio <= spread else
                    "wins over" if ratio > 1 else "loses to")
            out.append(
                f"- {t['system']}, k = {k}: block CG {word} `solve_multi` "
                f"({b['ms']:.1f} ms against {m['ms']:.1f} ms, {ratio:.2f}x; "
                f"{b['max_its']} against {m['max_its']} iterations, "
                f"{b['us_per_it_per_rhs']:.1f} against "
                f"{m['us_per_it_per_rhs']:.1f} us per iteration and right-hand "
                f"side; identical-arm spread {100 * (spread - 1):.1f} %).")
            tally[word] = tally.get(word, 0) + 1
    if tally:
        out += ["", "Overall, against `solve_multi`: "
                + ", ".join(f"{w.split()[0]} on {c}" for w, c in tally.items())
                + " of the measured (system, k) pairs.  Block CG pays 12 vector "
                "streams per iteration against 9 and, at K = 8, the strided row "
                "mapping of `k_block_update`; it comes out ahead only where the "
                "iteration count falls by more than the per-iteration cost rises "
                "(the `us per iteration and right-hand side` ratio above).  The "
                "solver stays opt-in and is never auto-selected."]
    return out


def write_note(result, resources, parent):
    L = ["# Block CG for several right-hand sides", "",
         "Written by `tools/blockcg_tts.py`.  Dubrulle's block CG with "
         "orthonormalised residuals (Cholesky-QR), one group of kg <= K "
         "columns, K in {2, 4, 8}; multivectors are contiguous fp64 `(n, K)`, "
         "the block state one fp64 tensor (layout in `kernels.hip`).", "",
         EXPECTATION, ""]
    L += ["## Registers and scratch (gfx950, `-Rpass-analysis=kernel-resource-usage`)", ""]
    if resources:
        L += [resources_md(resources), ""]
        spill = [k for k, r in resources.items() if r["scratch"] or r["vgpr_spill"]]
        L += ["No instantiation uses scratch or spills.  (Without the "
              "compiler barrier at the top of the row loops the LDS "
              "coefficient reads are hoisted out of the loop and the K = 8 "
              "update and ortho kernels fill all 256 VGPRs and spill.)"
              if not spill else "Instantiations with scratch: " + ", ".join(spill), ""]
    else:
        L += ["(not recorded: run `tools/blockcg_tts.py --resources-only`)", ""]
    if not result:
        L += ["## Measurements", "",
              "**No GPU was available when this note was written: nothing "
              "above is measured.**", ""]
    for tab in result.get("kernels", []):
        L += _kernel_md(tab)
    for t in result.get("tts", []):
        L += _tts_md(t)
    for sp in result.get("spans", []):
        L += _spans_md(sp)
    runs = result.get("unchanged")
    if runs:
        s = runs[0]
        L += [f"## Unchanged paths: {s['system']}", "",
              f"{s['iterations']} iterations, res_rtol 0.  Every line is one "
              "process: medians of its two interleaved identical arms.  The "
              "processes of the two commits alternate within one job.", "",
              "| commit | process | solve | solve (repeat) | solve_multi k=4 | "
              "solve_multi k=4 (repeat) |", "|---|---:|---:|---:|---:|---:|"]
        keys = ("solve", "solve (repeat)", "solve_multi k=4",
                "solve_multi k=4 (repeat)")
        for label, rr in (("parent", parent), ("this", runs)):
            for i, r in enumerate(rr):
                L.append(f"| {label} | {i} | " + " | ".join(
                    f"{r['us_per_it'][k]:.1f}" for k in keys) + " |")
        L.append("")
        if parent:
            for key in ("solve", "solve_multi k=4"):
                pa = [statistics.median([r["us_per_it"][key],
                                         r["us_per_it"][key + " (repeat)"]])
                      for r in parent]
                th = [statistics.median([r["us_per_it"][key],
                                         r["us_per_it"][key + " (repeat)"]])
                      for r in runs]
                a, b = statistics.median(pa), statistics.median(th)
                proc = max(max(pa) / min(pa), max(th) / min(th))
                L.append(f"`{key}`: parent {a:.1f} us/it, this commit {b:.1f} "
                         f"us/it, ratio {b / a:.3f}; identical code in different "
                         f"processes differs by up to {100 * (proc - 1):.1f} %.")
            inproc = max(r["spread"] for r in parent + runs)
            L += ["", "Within one process the identical arms agree to "
                  f"{100 * (inproc - 1):.2f} %; the spread that a comparison of two "
                  "commits has to beat is the process-to-process one (placement "
                  "of the allocations), since two commits cannot share a "
                  "process.", ""]
        else:
            L += ["The parent commit was not measured in this run.", ""]
    if result.get("tts"):
        L += ["## Verdict", ""] + verdict(result) + [""]
        L += ["## Tried and not kept", "", NOT_KEPT, ""]
    NOTE.write_text("\n".join(L))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=111, help="Queen-shaped grid")
    ap.add_argument("--poisson", type=int, default=256, help="7-pt grid")
    ap.add_argument("--ill", type=int, default=160, help="scaled 7-pt grid")
    ap.add_argument("--dof", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--maxits", type=int, default=20000)
    ap.add_argument("--rtol", type=float, default=1e-9)
    ap.add_argument("--unchanged-its", type=int, default=300)
    ap.add_argument("--skip", default="",
                    help="comma list of kernels,queen,poisson,scaled,unchanged")
    ap.add_argument("--resources-only", action="store_true")
    ap.add_argument("--unchanged-only", action="store_true")
    ap.add_argument("--root", default=None,
                    help="import acg_amd from this checkout instead")
    ap.add_argument("--parent-json", default=None,
                    help="--unchanged-only --out results of the parent commit "
                         "(comma list, one per process)")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--no-note", action="store_true")
    ap.add_argument("--from-json", default=None,
                    help="write the note from saved --out results (comma list, "
                         "merged; no GPU)")
    args = ap.parse_args()
    sys.path.insert(0, str(Path(args.root).resolve() if args.root else ROOT))
    if args.resources_only:
        rows = resource_table()
        RES_JSON.write_text(json.dumps(rows, indent=1) + "\n")
        print(resources_md(rows))
        return
    resources = json.loads(RES_JSON.read_text()) if RES_JSON.exists() else None
    parent = [json.loads(Path(f).read_text())["unchanged"]
              for f in (args.parent_json or "").split(",") if f and Path(f).exists()]
    if args.from_json:
        result = {}
        for f in args.from_json.split(","):
            for key, v in json.loads(Path(f).read_text()).items():
                if isinstance(v, list):
                    result.setdefault(key, []).extend(v)
                elif key == "unchanged":
                    result.setdefault(key, []).append(v)
                else:
                    result[key] = v
        write_note(result, resources, parent)
        return
    import torch

    result = {}
    if not torch.cuda.is_available():
        if not args.no_note:
            write_note(result, resources, None)
        print("no GPU: wrote the note without measurements")
        return
    dev = torch.device("cuda:0")
    skip = set(args.skip.split(","))
    if args.unchanged_only:
        skip = {"kernels", "queen", "poisson", "scaled"}
    if "kernels" not in skip:
        result["kernels"] = []
        for system, n in ((f"rows of queen-like dof{args.dof} G{args.grid}",
                           args.dof * args.grid ** 3),
                          (f"rows of poisson 7pt G{args.poisson}",
                           args.poisson ** 3)):
            tab = kernel_table(system, n, dev, args.iters, args.reps)
            result["kernels"].append(tab)
            for a in tab["arms"]:
                print(f"KERNEL {system}: {a['arm']:26s} {a['us']:9.1f} us "
                      f"{a['GBps'] or 0:7.0f} GB/s", flush=True)
            torch.cuda.empty_cache()
    if "unchanged" not in skip:
        result["unchanged"] = unchanged_ab(args.grid, args.dof, dev, args.reps,
                                           args.unchanged_its)
        print("UNCHANGED", json.dumps(result["unchanged"]["us_per_it"]), flush=True)
        torch.cuda.empty_cache()
    for kind, G in (("queen", args.grid), ("poisson", args.poisson),
                    ("scaled", args.ill)):
        if kind not in skip:
            result.setdefault("tts", []).append(
                tts_ab(kind, G, args.dof, dev, args.reps, args.maxits, args.rtol,
                       (4, 8)))
            if kind != "poisson":
                result.setdefault("spans", []).append(
                    span_breakdown(kind, G, args.dof, dev, 4, args.maxits,
                                   args.rtol))
    print(json.dumps(result))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(result, indent=1))
    if not args.no_note and not args.unchanged_only:
        if "unchanged" in result:
            result["unchanged"] = [result["unchanged"]]
        write_note(result, resources, parent)


if __name__ == "__main__":
    main()
