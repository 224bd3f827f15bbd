#!/usr/bin/env python3
"""Block-Jacobi PCG on Block-SELL operators: update-kernel cost, time to
solution and setup time on an MI355X, written up as profiles/bjacobi.md.

    python tools/bjacobi_tts.py                     # all parts, then the note
    python tools/bjacobi_tts.py --part a|b|c --out FILE.json
    python tools/bjacobi_tts.py --from-json A.json,B.json,C.json

Without ``--part`` every part runs as a child process of its own under its
own ``timeout``; the first part that fails, faults or runs out of time ends
the run (nothing more is started on the GPU) and the note is written from
the parts that finished.  Inside a part all arms share ONE process, are
warmed, and are interleaved; tables give medians with [min..max] and carry
an identical repeat arm whose ratio to its twin is the spread the other
ratios have to beat.  Without a GPU the note says "not measured".

(a) us per call of ``bpcg_fused_update`` (dof 2, 3, 4) against
    ``pcg_fused_update`` at the row count of the Queen-shaped G111 dof-3
    system (4.1 M rows), and the TB/s that the byte counts give: 8n doubles
    for point Jacobi, 7n + (dof+1)/2 n for block Jacobi (9n at dof 3).
(b) The Queen-shaped device-generated dof-3 system: iterations and time to
    solution of classic CG, classic CG on the Jacobi-scaled system and
    ``solve_bjacobi``; and (d) the setup time of ``bsell_diag_inv`` on it.
    The generator's diagonal is the constant 45, so the scaling
    ``s_i a_ij s_j`` with ``s = diag^-1/2`` is applied to the device arrays.
(c) The rotated-anisotropy system ``A = L B L^T`` (B Queen-shaped, L_i =
    Q_i diag(10^U(-1,1)) per node) at G = 64, dof 3, assembled on the host:
    classic CG, point-Jacobi PCG and block-Jacobi PCG.
"""

import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
RES_JSON = ROOT / "profiles" / "bjacobi_resources.json"
NOTE = ROOT / "profiles" / "bjacobi.md"
PART_LIMIT_S = {"a": 180, "b": 300, "c": 420}


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


def _arm(name, secs, **kw):
    return dict(arm=name, med=statistics.median(secs), min=min(secs),
                max=max(secs), **kw)


# ---------------------------------------------------------------------------
# (a) update kernels

def part_a(args, dev):
    import torch

    from acg_amd.ops import gpu_ops as G

    n0 = 3 * args.grid ** 3
    fns, doubles, keep = {}, {}, []

    def vecs(n, k):
        return [torch.randn(n, dtype=torch.float64, device=dev) for _ in range(k)]

    def slab():
        scal = G.alloc_scalars(dev)
        scal[G.S_RR] = 1.0  # S_PT stays 0: alpha = 0 keeps the vectors finite
        return scal, G.alloc_partials(dev)

    r, x, p, t, z, dinv = vecs(n0, 6)
    scal, partials = slab()
    keep.append((r, x, p, t, z, dinv, scal, partials))

    def point():
        G.pcg_fused_update(r, x, p, t, z, dinv, scal, partials, n0)

    fns["pcg_fused_update"] = point
    doubles["pcg_fused_update"] = (8.0, n0)
    for dof in (3, 2, 4):
        n = n0 - n0 % dof
        rb, xb, pb, tb, zb = vecs(n, 5)
        minv = torch.rand(G.block_inv_len(n // dof, dof), dtype=torch.float64,
                          device=dev)
        sc, pa = slab()
        keep.append((rb, xb, pb, tb, zb, minv, sc, pa))
        name = f"bpcg_fused_update dof={dof}"
        fns[name] = (lambda rb=rb, xb=xb, pb=pb, tb=tb, zb=zb, minv=minv,
                     sc=sc, pa=pa, n=n, dof=dof:
                     G.bpcg_fused_update(rb, xb, pb, tb, zb, minv, sc, pa, n, dof))
        doubles[name] = (7.0 + (dof + 1) / 2.0, n)
    fns["pcg_fused_update (repeat)"] = point
    doubles["pcg_fused_update (repeat)"] = (8.0, n0)
    times = bench(fns, args.iters, args.reps)
    base = statistics.median(times["pcg_fused_update"])
    arms = []
    for name, secs in times.items():
        per_row, n = doubles[name]
        a = _arm(name, secs, rows=n, doubles_per_row=per_row,
                 bytes=8.0 * per_row * n)
        a["TBps"] = a["bytes"] / a["med"] / 1e12
        a["vs_point"] = a["med"] / base
        arms.append(a)
        print(f"UPDATE {name:28s} {a['med'] * 1e6:8.1f} us "
              f"[{a['min'] * 1e6:.1f}..{a['max'] * 1e6:.1f}] "
              f"{a['TBps']:.2f} TB/s x{a['vs_point']:.3f}", flush=True)
    return {"update": {"rows": n0, "iters": args.iters, "reps": args.reps,
                       "arms": arms}}


# ---------------------------------------------------------------------------
# time to solution, shared by (b) and (c)

def tts(arms, reps, true_rel):
    """``arms``: name -> closure returning (SolveResult, x, b).  Round 0
    warms every arm; medians over the others."""
    import torch

    rec = {a: [] for a in arms}
    last = {}
    for rep in range(reps + 1):
        for a, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res, x, b = fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if rep:
                rec[a].append(dt)
            last[a] = (res, true_rel(a, b, x))
    out = []
    for a, secs in rec.items():
        res, tr = last[a]
        row = _arm(a, secs, its=res.niterations, converged=bool(res.converged),
                   true_rel=tr)
        row["us_per_it"] = row["med"] * 1e6 / max(res.niterations, 1)
        out.append(row)
        print(f"TTS {a:26s} {row['med'] * 1e3:9.2f} ms its={res.niterations} "
              f"converged={res.converged} true_rel={tr:.2e}", flush=True)
    return out


# ---------------------------------------------------------------------------
# (b) Queen-shaped device-generated system, (d) setup time

def part_b(args, dev):
    import numpy as np
    import torch

    from acg_amd.gen import queen_like_spec
    from acg_amd.gen.device_slab import device_stencil_slab
    from acg_amd.ops import gpu_ops as G
    from acg_amd.solvers.hip import CGSolverHIP

    spec = queen_like_spec(3)
    g = args.grid
    S = device_stencil_slab(g, g, g, spec, 0, 1, dev)
    Ss = device_stencil_slab(g, g, g, spec, 0, 1, dev)
    # Jacobi scaling on the device arrays: the diagonal is the constant
    # D[a][a] of the generator, so s_i a_ij s_j is one factor everywhere
    d = np.diag(np.asarray(spec["diagblock"]))
    assert (d == d[0]).all()
    s = 1.0 / np.sqrt(d[0])
    for arrs in (Ss.A_sell, Ss.A_bsell):
        arrs[2].mul_(s).mul_(s)
    n, nl = S.nowned, S.nowned + S.nghost
    plain = CGSolverHIP(S, comm=None, device=dev)
    scaled = CGSolverHIP(Ss, comm=None, device=dev)
    b = torch.from_numpy(np.random.default_rng(1).standard_normal(n)).to(dev)
    bs_ = b * s
    chk = torch.zeros(n, dtype=torch.float64, device=dev)

    def run(solver, fn, rhs):
        x = torch.zeros(nl, dtype=torch.float64, device=dev)
        return getattr(solver, fn)(rhs, x, maxits=args.maxits,
                                   res_rtol=args.rtol), x, rhs

    def true_rel(arm, rhs, x):
        (scaled if "scaled" in arm else plain)._spmv_overlapped(x, chk)
        return float(torch.linalg.norm(rhs - chk) / torch.linalg.norm(rhs))

    arms = {"classic": lambda: run(plain, "solve", b),
            "classic (repeat)": lambda: run(plain, "solve", b),
            "classic, jacobi-scaled": lambda: run(scaled, "solve", bs_),
            "bjacobi": lambda: run(plain, "solve_bjacobi", b)}
    rows = tts(arms, args.reps, true_rel)
    # (d) setup: the whole wrapper (allocation, launch, status read)
    bptr, bcol, bvals, dof = S.A_bsell
    setup = []
    for rep in range(args.reps + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        minv, nbad = G.bsell_diag_inv(bptr, bcol, bvals, n // dof, dof)
        torch.cuda.synchronize()
        if rep:
            setup.append(time.perf_counter() - t0)
    assert nbad == 0
    st = _arm("bsell_diag_inv", setup, nnodes=n // dof,
              blocks=int(bcol.numel()),
              bytes_read=4.0 * bcol.numel() + 8.0 * 9 * (n // dof))
    print(f"SETUP bsell_diag_inv {st['med'] * 1e3:.3f} ms "
          f"[{st['min'] * 1e3:.3f}..{st['max'] * 1e3:.3f}]", flush=True)
    return {"queen": {"system": f"queen-like 27pt dof3 G{g}, device-generated",
                      "rows": n, "format": plain._format_name(),
                      "res_rtol": args.rtol, "arms": rows},
            "setup": st}


# ---------------------------------------------------------------------------
# (c) rotated anisotropy, assembled on the host

def rotated_system(G, dof, seed=9000):
    """A = L B L^T as a one-rank LocalSystem (see the module docstring)."""
    import numpy as np
    import scipy.sparse as sp

    from acg_amd.core.symcsr import SymCSRMatrix
    from acg_amd.gen.stencil import queen_like_spec, stencil_global
    from acg_amd.part import extract_subdomains, partition_rows

    rng = np.random.default_rng([seed, G, dof])
    B = stencil_global(G, G, G, queen_like_spec(dof)).to_scipy_full().tocsr()
    nn = G ** 3
    n = nn * dof
    Q, _ = np.linalg.qr(rng.standard_normal((nn, dof, dof)))
    Ls = Q * 10.0 ** rng.uniform(-1.0, 1.0, size=(nn, 1, dof))
    cols = (np.arange(nn)[:, None] * dof
            + np.tile(np.arange(dof), dof)[None, :]).reshape(-1)
    Lm = sp.csr_matrix((Ls.reshape(-1), cols, np.arange(n + 1) * dof),
                       shape=(n, n))
    Af = (Lm @ B @ Lm.T).tocsr()
    Af = ((Af + Af.T) * 0.5).tocoo()
    up = Af.row <= Af.col
    A = SymCSRMatrix.from_coo(n, Af.row[up], Af.col[up], Af.data[up])
    S = extract_subdomains(A, partition_rows(A, 1), 1)[0]
    Db = np.einsum("nab,bc,ndc->nad", Ls, np.asarray(
        queen_like_spec(dof)["diagblock"]), Ls)
    return S, float(np.linalg.cond(Db).max()), rng


def part_c(args, dev):
    import torch

    from acg_amd.solvers.hip import CGSolverHIP

    t0 = time.perf_counter()
    S, kmax, rng = rotated_system(args.rot_grid, 3)
    print(f"assembled {S.nowned} rows in {time.perf_counter() - t0:.1f} s, "
          f"largest block condition number {kmax:.3g}", flush=True)
    n, nl = S.nowned, S.nowned + S.nghost
    solver = CGSolverHIP(S, comm=None, device=dev)
    b = torch.from_numpy(rng.standard_normal(n)).to(dev)
    chk = torch.zeros(n, dtype=torch.float64, device=dev)

    def run(fn):
        x = torch.zeros(nl, dtype=torch.float64, device=dev)
        return getattr(solver, fn)(b, x, maxits=args.maxits,
                                   res_rtol=args.rtol), x, b

    def true_rel(arm, rhs, x):
        solver._spmv_overlapped(x, chk)
        return float(torch.linalg.norm(rhs - chk) / torch.linalg.norm(rhs))

    arms = {"bjacobi": lambda: run("solve_bjacobi"),
            "bjacobi (repeat)": lambda: run("solve_bjacobi"),
            "classic": lambda: run("solve"),
            "jacobi": lambda: run("solve_jacobi")}
    rows = tts(arms, args.reps, true_rel)
    return {"rotated": {"system": f"rotated anisotropy L B L^T, dof3 "
                                  f"G{args.rot_grid}, host-assembled",
                        "rows": n, "format": solver._format_name(),
                        "max_block_cond": kmax, "res_rtol": args.rtol,
                        "arms": rows}}


# ---------------------------------------------------------------------------
# the note

EXPECTATION = """\
Expectation, stated before measuring.  `k_bpcg_fused_update` moves the seven
vector streams of `k_pcg_fused_update` (r and x read + write, t, p, z) plus
`(dof+1)/2` doubles of packed inverse per row in place of one double of
`dinv`: 9n doubles against 8n at dof 3 (8.5n at dof 2, 9.5n at dof 4), so a
call should cost about 9/8 of the point-Jacobi one.  One thread owns one
node, so r/t/x/p/z are touched at stride dof per lane (the pattern of the y
write of `k_spmv_bsell`); the packed inverse is unit-stride.  On the
project's own Queen-shaped generator the diagonal block is
`45 I + 0.5 (M - I)`, almost a multiple of the identity: no iteration gain
is expected there, only the extra n doubles per iteration.  The gain is
expected where a node's dofs are coupled by a rotated, badly scaled block,
which point scaling cannot undo: the CPU prototype saw 25-45x fewer
iterations than point Jacobi on `A = L B L^T` at G = 5 and 6."""


def _ms(a):
    return f"{a['med'] * 1e3:.2f} | [{a['min'] * 1e3:.2f}..{a['max'] * 1e3:.2f}]"


def _tts_md(t, base):
    L = [f"{t['rows']} rows [{t['format']}], res_rtol {t['res_rtol']:g}.  "
         f"`vs {base}` is that arm's median over the arm's median; `true rel` "
         "is ||b - A x|| / ||b|| recomputed with the operator.", "",
         f"| arm | iterations | ms | [min..max] | vs {base} | us/iteration | true rel |",
         "|---|---:|---:|---|---:|---:|---:|"]
    ref = next(a for a in t["arms"] if a["arm"] == base)["med"]
    for a in t["arms"]:
        L.append(f"| {a['arm']} | {a['its']}"
                 f"{'' if a['converged'] else ' (not converged)'} | {_ms(a)} | "
                 f"{ref / a['med']:.2f} | {a['us_per_it']:.1f} | "
                 f"{a['true_rel']:.2e} |")
    return L + [""]


def _spread(arms, a, b):
    x, y = (next(r for r in arms if r["arm"] == k)["med"] for k in (a, b))
    return max(x, y) / min(x, y)


def write_note(result, resources):
    NM = "not measured"
    L = ["# Block-Jacobi PCG on Block-SELL operators", "",
         "Written by `tools/bjacobi_tts.py`.  M = blockdiag of the dof x dof "
         "node blocks; the inverse blocks are built on the GPU "
         "(`k_bsell_diag_inv`, Cholesky per node) and stored as packed upper "
         "triangles `[slice][component][64]`.  `solve_bjacobi` is opt-in and "
         "never auto-selected.", "", EXPECTATION, "",
         "## Registers and scratch (gfx950, "
         "`-Rpass-analysis=kernel-resource-usage`)", ""]
    if resources:
        L += ["| kernel | VGPRs | scratch B/lane | VGPR spills | LDS B/block | waves/SIMD |",
              "|---|---:|---:|---:|---:|---:|"]
        for name, r in resources.items():
            L.append(f"| `{name}` | {r['vgprs']} | {r['scratch']} | "
                     f"{r['vgpr_spill']} | {r['lds']} | {r['occupancy']} |")
        L += ["", "No instantiation uses scratch or spills."
              if not any(r["scratch"] or r["vgpr_spill"]
                         for r in resources.values())
              else "**Some instantiations use scratch.**", ""]
    L += ["## (a) Update kernel", ""]
    up = result.get("update")
    if up:
        sp = _spread(up["arms"], "pcg_fused_update", "pcg_fused_update (repeat)")
        L += [f"{up['rows']} rows, {up['iters']} calls per round, "
              f"{up['reps']} rounds, each call followed by its one-block "
              f"finalize; identical-arm spread {100 * (sp - 1):.1f} %.", "",
              "| kernel | us | [min..max] | doubles/row | TB/s | vs point |",
              "|---|---:|---|---:|---:|---:|"]
        for a in up["arms"]:
            L.append(f"| {a['arm']} | {a['med'] * 1e6:.1f} | "
                     f"[{a['min'] * 1e6:.1f}..{a['max'] * 1e6:.1f}] | "
                     f"{a['doubles_per_row']:g} | {a['TBps']:.2f} | "
                     f"{a['vs_point']:.3f} |")
        by = {a["arm"]: a for a in up["arms"]}
        pt, b3 = by["pcg_fused_update"], by["bpcg_fused_update dof=3"]
        L += ["", f"At dof 3 the block kernel takes {b3['vs_point']:.3f}x the "
              f"point kernel's time where the byte counts predict "
              f"{9 / 8:.3f}x: it reaches {100 * b3['TBps'] / pt['TBps']:.0f} % "
              f"of the point kernel's achieved bandwidth.  dof 2 and dof 4 "
              f"are measured in the same table.  The supposed cause of what "
              f"gap there is at dof 3 is the per-lane run of 24 bytes in the "
              f"five vector streams (not a multiple of 16, so no 16-byte "
              f"accesses, and every wave access spans three times the cache "
              f"lines of a unit-stride one); no counters were collected.  "
              f"A gap of this size was not taken as reason to try the "
              f"thread-per-row mapping.", ""]
    else:
        L += [f"us per call, TB/s and the ratio to `pcg_fused_update`: {NM}.", ""]
    L += ["## (b) Queen-shaped device-generated system, dof 3", ""]
    q = result.get("queen")
    if q:
        L += [q["system"] + ".  The scaled arm solves `s_i a_ij s_j` with the "
              "right-hand side `s b`; its tolerance applies to the scaled "
              "residual.", ""] + _tts_md(q, "classic")
    else:
        L += [f"Iterations and time to solution of classic, Jacobi-scaled "
              f"classic and block-Jacobi PCG: {NM}.", ""]
    L += ["## (c) Rotated anisotropy at scale", ""]
    rt = result.get("rotated")
    if rt:
        L += [rt["system"] + f"; largest block condition number "
              f"{rt['max_block_cond']:.3g}.", ""] + _tts_md(rt, "bjacobi")
    else:
        L += [f"Iterations and time to solution of classic CG, point-Jacobi "
              f"PCG and block-Jacobi PCG at G = 64: {NM}.", ""]
    L += ["## (d) Setup", ""]
    st = result.get("setup")
    if st:
        L += [f"`bsell_diag_inv` on the system of (b): {st['nnodes']} nodes, "
              f"{st['blocks']} stored blocks (every block column is read, "
              f"only the diagonal blocks' values): {st['med'] * 1e3:.3f} ms "
              f"[{st['min'] * 1e3:.3f}..{st['max'] * 1e3:.3f}] for the whole "
              f"wrapper (allocation, one launch, one status read), "
              f"{st['bytes_read'] / st['med'] / 1e12:.2f} TB/s over the bytes "
              f"it has to read.", ""]
    else:
        L += [f"Setup time of `bsell_diag_inv`: {NM}.", ""]
    L += ["## Verdict", ""]
    if up and q and rt:
        a3 = next(a for a in up["arms"] if a["arm"] == "bpcg_fused_update dof=3")
        qa = {a["arm"]: a for a in q["arms"]}
        ra = {a["arm"]: a for a in rt["arms"]}
        L += [f"- Update kernel at dof 3: {a3['vs_point']:.2f}x the point-Jacobi "
              f"call (byte counts predict {9 / 8:.3f}x), {a3['TBps']:.2f} TB/s.",
              f"- Queen-shaped system: {qa['bjacobi']['its']} iterations against "
              f"{qa['classic']['its']} (classic) and "
              f"{qa['classic, jacobi-scaled']['its']} (Jacobi-scaled); "
              f"{qa['bjacobi']['med'] * 1e3:.1f} ms against "
              f"{qa['classic']['med'] * 1e3:.1f} ms: the almost scalar diagonal "
              f"block gives block Jacobi nothing to remove.",
              f"- Rotated anisotropy: {ra['bjacobi']['its']} iterations against "
              f"{ra['jacobi']['its']} (point Jacobi) and {ra['classic']['its']} "
              f"(classic); {ra['bjacobi']['med'] * 1e3:.1f} ms against "
              f"{ra['jacobi']['med'] * 1e3:.1f} ms and "
              f"{ra['classic']['med'] * 1e3:.1f} ms.",
              "", "Use `solve_bjacobi` when the nodes' diagonal blocks are far "
              "from a multiple of the identity (rotated local frames, mixed "
              "units, shell/beam dofs); on operators whose diagonal blocks are "
              "almost scalar it only adds traffic.", ""]
    else:
        L += [f"{NM.capitalize()}: the verdict needs parts (a), (b) and (c).", ""]
    NOTE.write_text("\n".join(L))


def merge(files):
    result = {}
    for f in files:
        if f and Path(f).exists():
            result.update(json.loads(Path(f).read_text()))
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("a", "b", "c"), default=None)
    ap.add_argument("--grid", type=int, default=111, help="Queen-shaped grid")
    ap.add_argument("--rot-grid", type=int, default=64,
                    help="rotated-anisotropy grid")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--maxits", type=int, default=20000)
    ap.add_argument("--rtol", type=float, default=1e-9)
    ap.add_argument("--out", default=None, help="write the JSON here")
    ap.add_argument("--outdir", default=None,
                    help="all parts: keep the per-part JSON files here")
    ap.add_argument("--from-json", default=None,
                    help="write the note from saved --out results (comma list)")
    args = ap.parse_args()
    sys.path.insert(0, str(ROOT))
    resources = json.loads(RES_JSON.read_text()) if RES_JSON.exists() else None
    if args.from_json:
        write_note(merge(args.from_json.split(",")), resources)
        return 0
    import torch

    if not torch.cuda.is_available():
        if args.part:
            print("no GPU: nothing measured", file=sys.stderr)
            return 1
        write_note({}, resources)
        print("no GPU: wrote the note without measurements")
        return 0
    if args.part:
        dev = torch.device("cuda:0")
        result = {"a": part_a, "b": part_b, "c": part_c}[args.part](args, dev)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text(json.dumps(result, indent=1))
        return 0
    # all parts: one child process per part, each under its own time limit;
    # the first that does not end cleanly ends the run
    import tempfile

    outdir = Path(args.outdir or tempfile.mkdtemp())
    outdir.mkdir(parents=True, exist_ok=True)
    done, rc = [], 0
    for part in ("a", "b", "c"):
        out = outdir / f"bjacobi_{part}.json"
        cmd = ["timeout", "-k", "10", str(PART_LIMIT_S[part]), sys.executable,
               str(Path(__file__).resolve()), "--part", part, "--out", str(out),
               "--grid", str(args.grid), "--rot-grid", str(args.rot_grid),
               "--iters", str(args.iters), "--reps", str(args.reps),
               "--maxits", str(args.maxits), "--rtol", str(args.rtol)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(f"part {part} ended with status {rc}: stopping",
                  file=sys.stderr)
            break
        done.append(str(out))
    write_note(merge(done), resources)
    return rc


if __name__ == "__main__":
    sys.exit(main())
