#!/usr/bin/env python3
"""Flagship benchmark: distributed CG iterations/s on Queen_4147-shaped SPD.

Driver contract: `python bench.py --gpus N --steps K --warmup W` (launched
via torch.distributed.run for N>1, one rank per GPU over RCCL).  Does W
untimed warmup CG iterations, then times EXACTLY K iterations bracketed by
barrier + torch.cuda.synchronize on both sides, takes the MAX time over
ranks, and rank 0 prints ONE JSON line.

Metric (BASELINE.json): CG iter/s (whole node) on Queen_4147-shaped data
(4.1M rows / ~330M nnz fp64; synthetic 27-pt dof-3 stencil -- no network,
no SuiteSparse downloads), strong scaling across 1/2/4/8 MI355X.

A plain run does only what the headline needs: setup, solver selection,
warmup, the K timed iterations, the JSON line.  `--full` adds the checks
and diagnostics that take GPU work of their own (true-residual integrity
check, per-rank span profile).  `--dump-outputs DIR` writes what the timed
solve returned (final iterate, residual norms) as DIR/<name>.npy so two
builds can be compared output for output; inputs are seeded, hence
identical from run to run for the same arguments.  `--solver auto` may
pick classic or pipelined CG by a timing probe (mathematically equivalent,
different rounding); DIR/solver.txt records the choice, and a comparison
that wants the same algorithm on both sides passes `--solver` explicitly.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

# --dump-outputs: bytes of iterate written over all ranks (float64)
DUMP_X_BYTES = 48 << 20


def dump_sample(n: int, cap: int, seed: int) -> np.ndarray:
    """Fixed seeded sample of ``cap`` distinct sorted indices out of
    ``n > cap``: one uniformly drawn index from each of ``cap`` contiguous
    strata, so the sample spans the whole vector without duplicates."""
    edges = (np.arange(cap + 1, dtype=np.int64) * n) // cap
    lo, hi = edges[:-1], edges[1:]
    return lo + np.random.default_rng(seed).integers(0, hi - lo)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--solver", choices=["auto", "pipelined", "classic"],
                    default="auto",
                    help="auto = measured policy (profiles/RESULTS.md): "
                         "megafused pipelined for narrow rows; pipelined "
                         "(overlapped allreduce) for multi-GPU; on 1 GPU "
                         "wide rows a 30-it warmup probe picks classic vs "
                         "pipelined (their ordering flips per instance)")
    ap.add_argument("--config", choices=["queen", "flan", "poisson7", "irregular"],
                    default="queen",
                    help="queen: 27-pt dof-3 Queen_4147-shaped (BASELINE configs 3-4); "
                         "flan: Flan_1565-shaped, 1.56M rows (BASELINE config 2); "
                         "poisson7: 7-pt 3D Poisson (BASELINE config 5 sizing); "
                         "irregular: power-law-degree SPD (the merge-path "
                         "regime -- heavy-tailed rows, no block structure)")
    ap.add_argument("--rows", type=int, default=2_000_000,
                    help="irregular config: global row count")
    ap.add_argument("--mean-nnz", type=float, default=40.0,
                    help="irregular config: target mean nonzeros/row")
    ap.add_argument("--format", choices=["auto", "sell", "sigma", "csr",
                                         "bsell", "hybrid", "binned"],
                    default="auto",
                    help="force the matA operator format (A/B measurement)")
    ap.add_argument("--grid", type=int, default=None,
                    help="grid edge G (queen default 111 -> 4.10M rows; "
                         "poisson7 default 512)")
    ap.add_argument("--dof", type=int, default=None)
    ap.add_argument("--gen", choices=["device", "host"], default="device",
                    help="matrix generation: on-GPU SELL (default) or host numpy")
    ap.add_argument("--lanes", type=int, default=None,
                    help="override SpMV lanes-per-row (4/8/16/32/64)")
    ap.add_argument("--matfree", action="store_true",
                    help="matrix-free analytic operator (dof=1 stencil "
                         "configs only; beyond-reference opt-in -- the "
                         "default keeps the assembled, memory-resident "
                         "operator so numbers reflect the sparse-matrix "
                         "workload BASELINE names)")
    ap.add_argument("--full", action="store_true",
                    help="also run what the headline figure does not need: "
                         "the true-residual integrity check and the "
                         "per-rank span profile (multi-GPU, or "
                         "ACG_BENCH_SPANS=1)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write what the timed solve "
                         "returned as DIR/<name>.npy (float64): the owned "
                         "part of the final iterate x (a fixed seeded "
                         "sample when larger than 48 MB over all ranks) "
                         "and the residual norms; solver.txt names the "
                         "solver that ran (pass --solver to pin it)")
    args = ap.parse_args()

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", str(rank)))
    ngpus = max(world, 1)

    from acg_amd.dist.comm import Comm
    from acg_amd.gen import STENCIL_7PT_3D, queen_like_spec, stencil_local_slab
    from acg_amd.solvers.hip import CGSolverHIP

    device = torch.device("cuda", local_rank % max(torch.cuda.device_count(), 1))
    torch.cuda.set_device(device)
    # init RCCL whenever torchrun launched us (even world=1: exercises the
    # same bootstrap the driver's multi-GPU runs use).  ACG_BENCH_COMM=gloo
    # is test-only: it lets the full multi-rank bench flow run 2-process on
    # ONE GPU via the CPU-staged gloo path (tests/test_gpu_dist_gloo.py).
    kind = os.environ.get("ACG_BENCH_COMM", "rccl")
    comm = Comm(kind, device=device) if "RANK" in os.environ else None

    if args.config == "queen":
        dof = args.dof or 3
        G = args.grid or 111
        spec = queen_like_spec(dof)
        model = f"queen4147-like-27pt-dof{dof}-G{G}"
    elif args.config == "flan":
        # Flan_1565: 1.56M rows / 117M nnz (SuiteSparse shell problem,
        # 3 dof/node); G=80 -> 1.536M rows / 121M nnz
        dof = args.dof or 3
        G = args.grid or 80
        spec = queen_like_spec(dof)
        model = f"flan1565-like-27pt-dof{dof}-G{G}"
    elif args.config == "irregular":
        dof, G = 1, 0
        model = f"powerlaw-n{args.rows}-m{args.mean_nnz:g}"
    else:
        dof = args.dof or 1
        G = args.grid or 512
        spec = dict(STENCIL_7PT_3D)
        spec["dof"] = dof
        model = f"poisson3d-7pt-G{G}"
    if args.matfree and (dof != 1 or args.gen != "device"):
        raise SystemExit("--matfree needs a dof=1 stencil config with --gen device")
    if args.config == "irregular":
        # host-generated power-law SPD, deterministic across ranks: every
        # rank builds the same global matrix and extracts its own part
        # through the GENERIC extractor (the path real .mtx input takes)
        from acg_amd.gen.irregular import powerlaw_spd
        from acg_amd.part import extract_subdomains, partition_rows

        A = powerlaw_spd(args.rows, mean_nnz=args.mean_nnz, seed=12345)
        part = partition_rows(A, ngpus, seed=0,
                              method="auto" if ngpus > 1 else "block")
        S = extract_subdomains(A, part, ngpus, only_parts=[rank])[rank] \
            if ngpus > 1 else extract_subdomains(A, part, 1)[0]
        del A
        nrows_global = args.rows
    elif args.gen == "device":
        from acg_amd.gen.device_slab import device_stencil_slab, preflight_slab

        # pre-flight memory assertion (config-5 rehearsal): fail in
        # seconds with a clear message instead of OOMing the box mid-way
        est = preflight_slab(G, G, G, spec, rank, ngpus, args.matfree,
                             torch.cuda.get_device_properties(device).total_memory)
        if rank == 0:
            print(f"# preflight: ~{est:.1f} GiB/rank "
                  f"({'matfree' if args.matfree else 'assembled'})",
                  file=sys.stderr, flush=True)
        S = device_stencil_slab(G, G, G, spec, rank, ngpus, device,
                                operator=not args.matfree)
        nrows_global = dof * G * G * G
    else:
        S = stencil_local_slab(G, G, G, spec, rank, ngpus)
        nrows_global = dof * G * G * G
    solver = CGSolverHIP(S, comm=comm, device=device, lanes=args.lanes,
                         matfree=args.matfree,
                         force_format=None if args.format == "auto"
                         else args.format)
    if rank == 0:
        fmt = ("matfree" if solver.matfree is not None else
               "bsell" if solver.bsell is not None else
               "sigma-sell" if solver.sell_perm is not None else
               "sell" if solver.sell is not None else
               "hybrid-binned" if solver.hybrid is not None else "csr-vector")
        print(f"# operator format: {fmt}", file=sys.stderr, flush=True)

    # dry-run halo audit: collective cross-rank check of pairing symmetry
    # and in-place ghost-tail global-id agreement, so the first N>=2 run
    # fails loudly at setup instead of deadlocking mid-solve
    if comm is not None and comm.size > 1:
        from acg_amd.dist.verify import verify_halo

        verify_halo(S, comm)

    rloc = np.random.default_rng(10_000 + rank)
    b = torch.from_numpy(rloc.standard_normal(S.nowned)).to(device)
    x = torch.zeros(S.nowned + S.nghost, dtype=torch.float64, device=device)

    def _probe_pair():
        """Time classic vs pipelined briefly and agree on the winner
        collectively (MAX over ranks per arm, identical collective
        sequence on every rank)."""
        def _probe(fn):
            fn(b, x.clone(), maxits=5, res_rtol=0.0)
            torch.cuda.synchronize(device)
            if comm is not None:
                comm.barrier()
            t0 = time.perf_counter()
            fn(b, x.clone(), maxits=30, res_rtol=0.0)
            torch.cuda.synchronize(device)
            el = time.perf_counter() - t0
            if comm is not None:
                import torch.distributed as dist

                et = torch.tensor([el], dtype=torch.float64, device=red_dev)
                dist.all_reduce(et, op=dist.ReduceOp.MAX)
                el = float(et.item())
            return el
        tc = _probe(solver.solve)
        tp = _probe(solver.solve_pipelined)
        kind_ = "classic" if tc <= tp else "pipelined"
        if rank == 0:
            print(f"# auto probe: classic {tc * 1e6 / 30:.1f} us/it, "
                  f"pipelined {tp * 1e6 / 30:.1f} -> {kind_}",
                  file=sys.stderr, flush=True)
        return kind_

    red_dev = device if kind == "rccl" else "cpu"
    if args.solver == "auto":
        if solver.megafuse_auto:
            # narrow rows: megafused pipelined (measured policy)
            solver_kind = "pipelined"
        elif ngpus > 1:
            # multi-GPU: both solvers are graph-captured; their ordering
            # depends on halo/allreduce overlap on the actual fabric --
            # probe both (collective decision, MAX over ranks)
            solver_kind = _probe_pair()
        else:
            # serial wide rows: classic and pipelined are within ~10% of
            # each other and the WINNER flips with the per-instance
            # allocation-placement lottery (profiles/RESULTS.md) -- probe
            # both briefly and keep the faster (selection + its warmup
            # happen outside the timed region, like any autotuner)
            solver_kind = _probe_pair()
    else:
        solver_kind = args.solver
    solve = solver.solve_pipelined if solver_kind == "pipelined" else solver.solve

    # warmup (untimed; also JITs RCCL channels and fills caches)
    if args.warmup > 0:
        solve(b, x.clone(), maxits=args.warmup, res_rtol=0.0)

    if comm is not None:
        comm.barrier()
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    res = solve(b, x, maxits=args.steps, res_rtol=0.0)
    torch.cuda.synchronize(device)
    if comm is not None:
        comm.barrier()
    t1 = time.perf_counter()
    elapsed = t1 - t0
    # MAX over ranks
    red_dev = device if kind == "rccl" else "cpu"
    if comm is not None:
        et = torch.tensor([elapsed], dtype=torch.float64, device=red_dev)
        import torch.distributed as dist

        dist.all_reduce(et, op=dist.ReduceOp.MAX)
        elapsed = float(et.item())

    assert res.niterations == args.steps, (res.niterations, args.steps)

    # what the timed solve handed back: the owned part of the final iterate
    # and the residual norms.  Every rank writes its own files; the 48 MB
    # iterate budget is shared, larger iterates are cut to a fixed seeded
    # sample.  solver.txt names the algorithm the auto policy timed.
    if args.dump_outputs:
        os.makedirs(args.dump_outputs, exist_ok=True)
        sfx = f"_rank{rank}" if ngpus > 1 else ""
        cap = DUMP_X_BYTES // 8 // ngpus
        xo = x[:S.nowned]
        if S.nowned > cap:
            pick = dump_sample(S.nowned, cap, 777 + rank)
            xo = xo[torch.from_numpy(pick).to(device)]
        if rank == 0:
            with open(os.path.join(args.dump_outputs, "solver.txt"), "w") as f:
                f.write(f"cg-{solver_kind}\n")
        np.save(os.path.join(args.dump_outputs, f"x{sfx}.npy"),
                xo.cpu().numpy().astype(np.float64, copy=False))
        np.save(os.path.join(args.dump_outputs, f"residual_norms{sfx}.npy"),
                np.array([res.bnrm2, res.r0nrm2, res.rnrm2], dtype=np.float64))

    # integrity check (outside the timed region, --full): the TRUE residual
    # of the final iterate must agree with the recursion residual the solver
    # reports -- silent corruption anywhere (kernels, halo, captured
    # graphs, collectives) would make these diverge or go non-finite.
    # (Expected benign gap: pipelined CG's recursion residual drifts a few
    # orders below the true one at tight tolerances -- textbook behaviour,
    # e.g. true 5e-11 vs recursion 2e-15 after 200 Queen iterations.)
    true_rel = None
    if args.full:
        tchk = torch.zeros(S.nowned, dtype=torch.float64, device=device)
        solver._spmv_overlapped(x, tchk)
        rloc2 = float(torch.sum((b[:S.nowned] - tchk) ** 2))
        bloc2 = float(torch.sum(b[:S.nowned] ** 2))
        if comm is not None:
            import torch.distributed as dist

            rb = torch.tensor([rloc2, bloc2], dtype=torch.float64,
                              device=red_dev)
            dist.all_reduce(rb, op=dist.ReduceOp.SUM)
            rloc2, bloc2 = float(rb[0]), float(rb[1])
        true_rel = (rloc2 / bloc2) ** 0.5 if bloc2 > 0 else float("nan")
        assert np.isfinite(true_rel), "non-finite true residual"
    recur_rel = res.rnrm2 / res.bnrm2 if res.bnrm2 > 0 else float("nan")

    # per-rank overlap diagnosis (outside the timed region, --full): a short
    # profiled EAGER pass records hipEvent spans (halo / spmvA / spmvO /
    # allreduce / update) per rank and ships them on the JSON line, so the
    # first real N=8 run is diagnosable -- not just a single number.
    # (Profiling forces the eager path; the timed number above still
    # reflects the captured-graph hot loop.)
    rank_spans = None
    if args.full and (ngpus > 1 or os.environ.get("ACG_BENCH_SPANS")):
        solver.prof.enabled = True
        pres = solve(b, x.clone(), maxits=16, res_rtol=0.0)
        solver.prof.enabled = False
        mine = {nm: [round(st.seconds * 1e6 / max(st.count, 1), 1), st.count]
                for nm, st in (pres.ops or {}).items()}
        mine["halo_B_per_it"] = 8 * (S.halo.sendsize + S.halo.recvsize)
        allspans = comm.gather_object(mine) if comm is not None else [mine]
        if rank == 0:
            rank_spans = {f"r{i}": d for i, d in enumerate(allspans)}

    nnz_local = S.nnzA + S.nnzO
    if comm is not None:
        import torch.distributed as dist

        nt = torch.tensor([float(nnz_local)], dtype=torch.float64,
                          device=red_dev)
        dist.all_reduce(nt, op=dist.ReduceOp.SUM)
        nnz_global = float(nt.item())
    else:
        nnz_global = float(nnz_local)

    iters_per_s = args.steps / elapsed
    ms_per_step = 1000.0 * elapsed / args.steps
    if rank == 0:
        out = {
            "metric": {"queen": "CG iter/s (whole node), Queen_4147-shaped fp64",
                       "flan": "CG iter/s (whole node), Flan_1565-shaped fp64",
                       "poisson7": "CG iter/s (whole node), 7-pt 3D Poisson fp64",
                       "irregular": "CG iter/s (whole node), power-law SPD fp64",
                       }[args.config],
            "value": iters_per_s,
            "unit": "iter/s",
            "n_gpus": ngpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "fp64",
            "data": {"queen": "synthetic SPD (27-pt dof-3 stencil, Queen_4147 shape; random RHS)",
                     "flan": "synthetic SPD (27-pt dof-3 stencil, Flan_1565 shape; random RHS)",
                     "poisson7": "synthetic SPD (7-pt 3D Poisson; random RHS)",
                     "irregular": "synthetic SPD (power-law degrees, "
                                  "Laplace-local columns; random RHS)",
                     }[args.config],
            "config": {
                "model": model,
                "rows": nrows_global,
                "nnz": nnz_global,
                "solver": f"cg-{solver_kind}" + ("-matfree" if args.matfree else ""),
                "time_to_solution_s": elapsed,
                "rel_residual_true": true_rel,
                "rel_residual_recursion": recur_rel,
                "gflops": args.steps * (2.0 * nnz_global + 10.0 * nrows_global) / elapsed / 1e9,
                "parallelism": f"slab{ngpus}-rccl",
                "rank_spans_us_per_call": rank_spans,
            },
        }
        print(json.dumps(out), flush=True)
    if comm is not None:
        comm.finalize()
    return 0


if __name__ == "__main__":
    sys.exit(main())
