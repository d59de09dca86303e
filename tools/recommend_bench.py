#!/usr/bin/env python3
"""Top-N for every user: the fused hpf_recommend (one item sweep, candidate buffers, a merge) against the materialising
hpf_rank_topn (scores of a batch of users in memory, masked, radix-selected).  One handle with C2's sides (n = 10^6 users,
m = 10^5 items, K = 100, -hier, synthetic CSR from synth.py, E set directly), as tools/rank_queries_bench.py.

    python tools/recommend_bench.py --out profiles/r07/recommend.json [--topn 10,100,256] [--sel 16384] [--runs 5]

Per topn, on the same --sel users: (a) hpf_recommend, (b) hpf_rank_topn; then (a) over all n users in chunks of 65 536, as
`hgaprec -recommend` calls it.  Wall times are those of the whole call (uploads of the lists, kernels, copy back); each path
runs once unmeasured, then --runs rounds alternate the paths: the median, the smallest and the largest are kept.
"fused_not_slower" applies the rule of DESIGN.md section 4c: the fused median is not above the materialising median by more
than that route's own smallest-to-largest spread.  --n / --m / --nnz scale the problem down for a quick look."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tools.rank_queries_bench import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--m", type=int, default=100_000)
    ap.add_argument("--K", type=int, default=100)
    ap.add_argument("--nnz", type=int, default=50_000_000)
    ap.add_argument("--sel", type=int, default=16384)
    ap.add_argument("--topn", default="10,100,256", help="list lengths, comma separated")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--full-runs", type=int, default=2)
    ap.add_argument("--no-full", action="store_true", help="skip hpf_recommend over all n users")
    ap.add_argument("--no-check", action="store_true", help="skip the comparison of the two paths' results")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from hgaprec_amd import capi, synth
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
    D.recommend(users[:64], 10)                                            # first launch of each path
    D.rank_topn(users[:64], 10)

    out = {"workload": f"{n} users x {m} items, {nnz} nonzeros, K={K}, -hier; two mask items per user", "n_sel": int(S),
           "runs": args.runs, "per_topn": {}}
    for topn in [int(x) for x in args.topn.split(",")]:
        e, res = timed({"recommend": lambda: D.recommend(users, topn, mptr, mitems),
                        "rank_topn": lambda: D.rank_topn(users, topn, mptr, mitems)}, args.runs)
        blocks, splits, tps = capi.recommend_grid(S, m, topn)
        e["grid"] = {"blocks": blocks, "splits": splits, "tiles_per_split": tps, "cap": capi.recommend_cap(topn)}
        e["rank_topn_over_recommend"] = e["rank_topn"]["median_s"] / e["recommend"]["median_s"]
        spread = e["rank_topn"]["max_s"] - e["rank_topn"]["min_s"]
        e["fused_not_slower"] = bool(e["recommend"]["median_s"] <= e["rank_topn"]["median_s"] + spread)
        if not args.no_check:
            ra, rb = res["recommend"], res["rank_topn"]
            e["identical"] = bool(np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1].view(np.uint64), rb[1].view(np.uint64)))
        if not args.no_full:
            def all_users():
                last = None
                for u0 in range(0, n, 1 << 16):
                    last = D.recommend(np.arange(u0, min(n, u0 + (1 << 16)), dtype=np.uint32), topn)
                return last
            all_users()                                                    # unmeasured: every chunk shape once
            ts = []
            for _ in range(args.full_runs):
                t0 = time.perf_counter()
                all_users()
                ts.append(time.perf_counter() - t0)
            t = {"recommend_all_users": {"s": ts, "median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts),
                                         "users_per_s": n / statistics.median(ts)}}
            e.update(t)
        out["per_topn"][str(topn)] = e
        print(json.dumps({topn: e}), flush=True)
    D.close()
    if args.out:
        p = Path(args.out)
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
