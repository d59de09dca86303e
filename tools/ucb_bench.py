#!/usr/bin/env python3
"""Optimistic top-N: hpf_recommend_ucb beside hpf_recommend on the same handle at C2's shape (n = 10^6 users, m = 10^5
items, K = 100, -hier, synthetic CSR from synth.py, E and the shapes set directly), for a chunk of --sel users as
`hgaprec -recommend N -ucb Z` calls it.

    python tools/ucb_bench.py --out profiles/r15/ucb.json [--topn 100] [--runs 5] [--sel 65536]

Wall times are those of the whole calls (uploads of the lists, the derived rows, kernels, copy back); each path runs once
unmeasured, then --runs rounds alternate the paths.  hpf_score_moments over sel x topn pairs is timed too: what the lists'
means and variances cost apart from the sweep.  Kernel times come from a run of their own under rocprofv3 --kernel-trace
--stats (--runs 1).  --n / --m / --nnz scale the problem down for a quick look."""
from __future__ import annotations

import argparse
import json
import sys
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
    ap.add_argument("--sel", type=int, default=65536)
    ap.add_argument("--topn", type=int, default=100)
    ap.add_argument("--z", type=float, default=2.0)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from hgaprec_amd import synth
    from hgaprec_amd.capi import Hpf
    n, m, K, N = args.n, args.m, args.K, args.topn
    dev = torch.device("cuda", 0)
    rowptr, col, val = synth.generate_device(n, m, args.nnz, 0.5, 0.8, seed=2, device=dev)
    D = Hpf(n, m, K, hier=True, bias=False, device=0)
    D.upload_csr_device(rowptr, col, val)
    nnz = int(rowptr[-1])
    del rowptr, col, val
    torch.cuda.empty_cache()
    for side, rows, seed in (("THETA", n, 11), ("BETA", m, 12)):
        st = synth.initial_state_device(rows, K, seed, dev)
        D.set_state_device(side + "_E", st["E"])
        D.set_state_device(side + "_SHAPE", st["shape"])
        del st
    torch.cuda.empty_cache()

    users = np.arange(min(args.sel, n), dtype=np.uint32)
    rng = np.random.default_rng(1)
    pu = np.repeat(users, N)
    pi = rng.integers(0, m, pu.size).astype(np.uint32)
    e, res = timed({"recommend": lambda: D.recommend(users, N),
                    "recommend_ucb": lambda: D.recommend_ucb(users, N, args.z),
                    "recommend_ucb_z0": lambda: D.recommend_ucb(users, N, 0.0),
                    "score_moments_pairs": lambda: D.score_moments(pu, pi)}, args.runs)
    same = bool(np.array_equal(res["recommend"][0], res["recommend_ucb_z0"][0]))
    plan = {"C": 2 * K, "derived_bytes_Y": m * ((2 * K + 3) & ~3) * 8}
    out = {"workload": f"{n} users x {m} items, {nnz} nonzeros, K={K}, -hier; {users.size} selected users, topn={N}, z={args.z}; no mask list",
           "runs": args.runs, "times": e, "plan": plan, "z0_lists_equal_recommend": same,
           "ucb_over_recommend": e["recommend_ucb"]["median_s"] / e["recommend"]["median_s"]}
    print(json.dumps(out), flush=True)
    D.close()
    if args.out:
        p = Path(args.out)
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
