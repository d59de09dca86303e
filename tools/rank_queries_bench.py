#!/usr/bin/env python3
"""Every test item of a user in one pass (hpf_rank_queries) against the two routes the project had: hpf_loo_ranks with
one selected "user" per (user, query) pair, and the materialising hpf_item_ranks.  One handle with C2's sides (n = 10^6
users, m = 10^5 items, K = 100, -hier, synthetic CSR from synth.py, E set directly), as tools/loo_ranks_bench.py.

    python tools/rank_queries_bench.py --out profiles/r07/rank_queries.json [--queries 4,10,32] [--sel 16384] [--runs 5]
    rocprofv3 --kernel-trace --output-format csv -d DIR -- \\
        python tools/rank_queries_bench.py --queries 10 --runs 1 --no-full --no-check
    python tools/rank_queries_bench.py --merge-trace DIR --out profiles/r07/rank_queries.json      # no GPU needed

Per number of queries per user, on the same --sel users: (a) hpf_rank_queries, (b) hpf_loo_ranks on the expanded pairs,
(c) hpf_item_ranks; and (a) over all n users.  Wall times are those of the whole call (uploads of the lists, kernels,
copy back); each path runs once unmeasured, then --runs rounds alternate the paths: the median, the smallest and the
largest are kept.
Kernel-only times come from the rocprofv3 run: --merge-trace walks its *kernel_trace.csv in start order, gives each
loo_mask_kernel dispatch to the path whose rank kernel follows it, and adds "kernel_ms" to the JSON (the 64-user
first launches included).  --n / --m / --nnz scale the problem down for a quick look."""
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

from tools.loo_ranks_bench import MATERIALISING  # noqa: E402

QUERIES = ("rq_threshold_kernel", "rank_queries_kernel")
PER_PAIR = ("loo_rank_kernel",)


def merge_trace(trace_dir, out_path):
    rows = []
    for f in Path(trace_dir).rglob("*kernel_trace.csv"):
        for r in csv.DictReader(open(f)):
            rows.append((int(r["Start_Timestamp"]), r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6))
    if not rows:
        sys.exit(f"{trace_dir}: no *kernel_trace.csv")
    rows.sort()
    ms = {"rank_queries": {}, "loo_ranks_per_pair": {}, "item_ranks": {}}
    pending = 0.0

    def add(path, name, t):
        e = ms[path].setdefault(name, {"calls": 0, "total_ms": 0.0})
        e["calls"] += 1
        e["total_ms"] += t
    for _, name, t in rows:
        short = next((k for k in QUERIES + PER_PAIR + MATERIALISING + ("loo_mask_kernel",) if k in name), None)
        if short == "loo_mask_kernel":
            pending += t
        elif short in QUERIES + PER_PAIR:
            path = "rank_queries" if short in QUERIES else "loo_ranks_per_pair"
            if pending:
                add(path, "loo_mask_kernel", pending)
                pending = 0.0
            add(path, short, t)
        elif short in MATERIALISING:
            add("item_ranks", short, t)
    out = json.loads(Path(out_path).read_text()) if Path(out_path).exists() else {}
    out["kernel_ms"] = {p: {"total_ms": sum(v["total_ms"] for v in k.values()), "per_kernel": k} for p, k in ms.items()}
    Path(out_path).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out["kernel_ms"]))


def timed(fns, runs):
    """{name: fn} -> ({name: times}, {name: last result}): every path once unmeasured (first touch of its buffers), then
    --runs rounds that alternate the paths, so a drift of the machine meets all of them alike"""
    res = {k: fn() for k, fn in fns.items()}
    ts = {k: [] for k in fns}
    for _ in range(runs):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            res[k] = fn()
            ts[k].append(time.perf_counter() - t0)
    return {k: {"s": v, "median_s": statistics.median(v), "min_s": min(v), "max_s": max(v)} for k, v in ts.items()}, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--merge-trace", default=None, metavar="DIR",
                    help="add kernel-only times from a rocprofv3 --kernel-trace directory to --out; no GPU run")
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--m", type=int, default=100_000)
    ap.add_argument("--K", type=int, default=100)
    ap.add_argument("--nnz", type=int, default=50_000_000)
    ap.add_argument("--sel", type=int, default=16384)
    ap.add_argument("--queries", default="4,10,32", help="queries per user, comma separated")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--full-runs", type=int, default=3)
    ap.add_argument("--no-full", action="store_true", help="skip hpf_rank_queries over all n users")
    ap.add_argument("--no-check", action="store_true", help="skip the comparison of the three paths' results")
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
    S = users.size
    mptr = (np.arange(S + 1) * 2).astype(np.uint64)                        # two "validation" items per user
    mitems = rng.integers(0, m, 2 * S).astype(np.uint32)
    D.rank_queries(users[:64], np.arange(65, dtype=np.uint64), np.zeros(64, np.uint32))   # first launch of each path
    D.loo_ranks(users[:64], np.zeros(64, np.uint32))
    D.item_ranks(users[:64], np.arange(64, dtype=np.uint32), np.zeros(64, np.uint32))

    out = {"workload": f"{n} users x {m} items, {nnz} nonzeros, K={K}, -hier; two mask items per user", "n_sel": int(S),
           "runs": args.runs, "per_queries": {}}
    for qn in [int(x) for x in args.queries.split(",")]:
        q_ptr = (np.arange(S + 1) * qn).astype(np.uint64)
        q_items = rng.integers(0, m, S * qn).astype(np.uint32)
        q_sel = np.repeat(np.arange(S, dtype=np.uint32), qn)
        eptr = (np.arange(S * qn + 1) * 2).astype(np.uint64)               # the pair's user's mask list, once per pair
        eitems = np.repeat(mitems.reshape(S, 2), qn, axis=0).reshape(-1)
        eusers = users[q_sel]
        e, res = timed({"rank_queries": lambda: D.rank_queries(users, q_ptr, q_items, mptr, mitems),
                        "loo_ranks_per_pair": lambda: D.loo_ranks(eusers, q_items, eptr, eitems),
                        "item_ranks": lambda: D.item_ranks(users, q_sel, q_items, mptr, mitems)}, args.runs)
        ra, rb, rc = res["rank_queries"], res["loo_ranks_per_pair"], res["item_ranks"]
        e["loo_over_rank_queries"] = e["loo_ranks_per_pair"]["median_s"] / e["rank_queries"]["median_s"]
        e["item_ranks_over_rank_queries"] = e["item_ranks"]["median_s"] / e["rank_queries"]["median_s"]
        if not args.no_check:
            e["identical"] = bool(np.array_equal(ra[0], rb[0]) and np.array_equal(ra[0], rc[0]) and
                                  np.array_equal(ra[1].view(np.uint64), rb[1].view(np.uint64)) and
                                  np.array_equal(ra[1].view(np.uint64), rc[1].view(np.uint64)))
        if not args.no_full:
            allu = np.arange(n, dtype=np.uint32)
            ap_ = (np.arange(n + 1, dtype=np.uint64) * np.uint64(qn))
            ai = rng.integers(0, m, n * qn).astype(np.uint32)
            t, rf = timed({"rank_queries_all_users": lambda: D.rank_queries(allu, ap_, ai)}, args.full_runs)
            e.update(t)
            e["all_users_mean_rank"] = float(rf["rank_queries_all_users"][0].mean())
            del allu, ap_, ai, rf
        out["per_queries"][str(qn)] = e
        print(json.dumps({qn: e}), flush=True)
    D.close()
    if args.out:
        p = Path(args.out)
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
