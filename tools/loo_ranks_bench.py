#!/usr/bin/env python3
"""Fused leave-one-out ranks (hpf_loo_ranks) against the materialising path (hpf_item_ranks, one query per user)
on one handle with C2's sides: n = 10^6 users, m = 10^5 items, K = 100, -hier, a synthetic CSR from synth.py, E set
directly.  hpf_item_ranks is the code the project had before the fused kernel, on the same box in the same process.

    python tools/loo_ranks_bench.py --out profiles/r07/loo_ranks.json [--sel 16384] [--runs 3] [--no-full]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- \\
        python tools/loo_ranks_bench.py --sel 16384 --runs 1 --no-full --no-check
    python tools/loo_ranks_bench.py --merge-trace DIR --out profiles/r07/loo_ranks.json      # no GPU needed

Wall times are those of the whole call (uploads of the user and mask lists, the kernels, the copy back of one rank
and one score per user).  Kernel-only times come from the rocprofv3 run: --merge-trace reads its *kernel_stats.csv and
*kernel_trace.csv and adds to the JSON of the first command "kernel_ms" (per path: the sum over its kernels of one
call at --sel users, first launches of 64 users included, and each kernel's share) and "fused_kernel_resources" (the
registers, LDS and scratch the trace reports for loo_rank_kernel, and the waves per SIMD that follow from them).
--n / --m / --nnz scale the problem down for a quick look."""
from __future__ import annotations

import argparse
import csv
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


FUSED = ("loo_mask_kernel", "loo_rank_kernel")
MATERIALISING = ("score_tile_kernel", "mask_scores_kernel", "rank_query_kernel")


def merge_trace(trace_dir, out_path):
    """kernel-only times and the fused kernel's resources, from a rocprofv3 --kernel-trace --stats directory"""
    d = Path(trace_dir)
    out = json.loads(Path(out_path).read_text()) if Path(out_path).exists() else {}
    per = {}
    for f in d.rglob("*kernel_stats.csv"):
        for r in csv.DictReader(open(f)):
            for k in FUSED + MATERIALISING:
                if k in r["Name"]:
                    e = per.setdefault(k, {"calls": 0, "total_ms": 0.0})
                    e["calls"] += int(r["Calls"])
                    e["total_ms"] += float(r["TotalDurationNs"]) / 1e6
    if not per:
        sys.exit(f"{trace_dir}: no *kernel_stats.csv with the ranking kernels")
    km = {"fused_ms": sum(v["total_ms"] for k, v in per.items() if k in FUSED),
          "materialising_ms": sum(v["total_ms"] for k, v in per.items() if k in MATERIALISING),
          "per_kernel": per}
    km["ratio_materialising_over_fused"] = km["materialising_ms"] / km["fused_ms"]
    out["kernel_ms"] = km
    for f in d.rglob("*kernel_trace.csv"):
        for r in csv.DictReader(open(f)):
            if "loo_rank_kernel" not in r["Kernel_Name"] or int(r["Grid_Size_X"]) <= 256:
                continue                                                   # skip the 64-user first launch
            g = lambda *names: next((int(r[x]) for x in names if r.get(x) not in (None, "")), 0)
            vgpr, agpr = g("VGPR_Count", "Arch_VGPR_Count"), g("Accum_VGPR_Count")
            regs = -(-vgpr // 8) * 8 + -(-agpr // 8) * 8                  # gfx950: 512 registers per lane and SIMD, in eights
            out["fused_kernel_resources"] = {
                "kernel": r["Kernel_Name"], "vgpr": vgpr, "agpr": agpr, "sgpr": g("SGPR_Count"),
                "lds_bytes_per_workgroup": g("LDS_Block_Size", "LDS_Block_Size_v"), "scratch_bytes": g("Scratch_Size", "Private_Segment_Size"),
                "workgroup": g("Workgroup_Size_X", "Workgroup_Size"), "grid_x": g("Grid_Size_X"), "grid_y": g("Grid_Size_Y"),
                "waves_per_simd": min(8, 512 // max(regs, 1)),
            }
            break
    Path(out_path).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps({k: out[k] for k in ("kernel_ms", "fused_kernel_resources") if k in out}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--merge-trace", default=None, metavar="DIR",
                    help="add kernel-only times and the fused kernel's resources from a rocprofv3 directory to --out; no GPU run")
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--m", type=int, default=100_000)
    ap.add_argument("--K", type=int, default=100)
    ap.add_argument("--nnz", type=int, default=50_000_000)
    ap.add_argument("--sel", type=int, default=16384)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--no-full", action="store_true", help="skip the run over all n users (fused path only)")
    ap.add_argument("--no-check", action="store_true", help="skip the comparison of the two paths' results")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.merge_trace:
        if not args.out:
            ap.error("--merge-trace needs --out")
        return merge_trace(args.merge_trace, args.out)

    import torch
    from hgaprec_amd import synth
    from hgaprec_amd.capi import Hpf
    n, m, K = args.n, args.m, args.K
    dev = torch.device("cuda", 0)
    rowptr, col, val = synth.generate_device(n, m, args.nnz, 0.5, 0.8, seed=2, device=dev)
    D = Hpf(n, m, K, hier=True, bias=False, device=0)
    D.upload_csr_device(rowptr, col, val)
    nnz = int(rowptr[-1])
    del rowptr, col, val
    torch.cuda.empty_cache()
    D.set_state_device("THETA_E", synth.initial_state_device(n, K, 11, dev)["E"])
    D.set_state_device("BETA_E", synth.initial_state_device(m, K, 12, dev)["E"])
    torch.cuda.empty_cache()

    rng = np.random.default_rng(5)
    users = np.sort(rng.choice(n, min(args.sel, n), replace=False)).astype(np.uint32)
    q = rng.integers(0, m, users.size).astype(np.uint32)
    mptr = (np.arange(users.size + 1) * 2).astype(np.uint64)               # two "validation" items per user
    mitems = rng.integers(0, m, 2 * users.size).astype(np.uint32)
    qsel = np.arange(users.size, dtype=np.uint32)

    def timed(fn, runs):
        ts, res = [], None
        for _ in range(runs):
            t0 = time.perf_counter()
            res = fn()
            ts.append(time.perf_counter() - t0)
        return ts, res

    D.loo_ranks(users[:64], q[:64])                                        # first launch of each path: code upload
    D.item_ranks(users[:64], qsel[:64], q[:64])
    t_f, r_f = timed(lambda: D.loo_ranks(users, q, mptr, mitems), args.runs)
    t_m, r_m = timed(lambda: D.item_ranks(users, qsel, q, mptr, mitems), args.runs)
    out = {
        "workload": f"{n} users x {m} items, {nnz} nonzeros, K={K}, -hier; one query item and two mask items per user",
        "n_sel": int(users.size),
        "fused_s": t_f, "materialising_s": t_m,
        "fused_median_s": statistics.median(t_f), "materialising_median_s": statistics.median(t_m),
    }
    out["ratio_materialising_over_fused"] = out["materialising_median_s"] / out["fused_median_s"]
    if not args.no_check:
        out["identical"] = bool(np.array_equal(r_f[0], r_m[0]) and np.array_equal(r_f[1], r_m[1]))
    if not args.no_full:
        allu = np.arange(n, dtype=np.uint32)
        qa = rng.integers(0, m, n).astype(np.uint32)
        t0 = time.perf_counter()
        rank, sc, masked = D.loo_ranks(allu, qa, item_limit=m - 1)
        out["fused_all_users_s"] = time.perf_counter() - t0
        out["fused_all_users_mean_rank"] = float(rank.mean())
    D.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        p = Path(args.out)
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
