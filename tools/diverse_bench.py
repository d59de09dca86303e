#!/usr/bin/env python3
"""Diversified top-N: hpf_recommend_diverse beside hpf_recommend(topn = pool) on the same handle at C2's shape (n = 10^6
users, m = 10^5 items, K = 100, -hier, synthetic CSR from synth.py, E set directly), for a chunk of --sel users as `hgaprec
-recommend N -diverse L -diverse-pool P` calls it.

    python tools/diverse_bench.py --out profiles/r10/diverse.json [--topn 100] [--pools 256,128] [--runs 5] [--sel 100000]

Wall times are those of the whole calls (uploads of the lists, kernels, copy back); each path runs once unmeasured, then
--runs rounds alternate the paths; the median and the range are kept.  hpf_recommend(topn = pool) is the yardstick: the call
finds its pool with the same sweep and merge, so the difference is unit_rows_kernel, mmr_kernel and the two extra outputs.
The per-kernel split comes from a run of this tool under rocprofv3 --kernel-trace --stats (--runs 1), a run of its own.
On a build without the call (the parent commit) only the yardstick runs.  --n / --m / --nnz scale the problem down."""
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
    ap.add_argument("--sel", type=int, default=100_000)
    ap.add_argument("--topn", type=int, default=100)
    ap.add_argument("--pools", default="256,128")
    ap.add_argument("--lam", type=float, default=0.7)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from hgaprec_amd import synth
    from hgaprec_amd.capi import Hpf
    n, m, K, N = args.n, args.m, args.K, args.topn
    pools = [int(p) for p in args.pools.split(",")]
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
        del st
    torch.cuda.empty_cache()

    users = np.arange(min(args.sel, n), dtype=np.uint32)
    has = hasattr(Hpf, "recommend_diverse")
    fns = {}
    for P in pools:
        fns[f"recommend_{P}"] = lambda P=P: D.recommend(users, P)
        if has:
            fns[f"recommend_diverse_{P}"] = lambda P=P: D.recommend_diverse(users, min(N, P), pool=P, lam=args.lam)
    e, res = timed(fns, args.runs)
    out = {"workload": f"{n} users x {m} items, {nnz} nonzeros, K={K}, -hier; {users.size} selected users, topn={N}, "
                       f"lambda={args.lam}; no mask list",
           "runs": args.runs, "times": e}
    if has:
        out["diverse_over_recommend"] = {str(P): e[f"recommend_diverse_{P}"]["median_s"] / e[f"recommend_{P}"]["median_s"] for P in pools}
        out["mean_maxsim"] = {str(P): float(res[f"recommend_diverse_{P}"][2].mean()) for P in pools}
        lam1 = D.recommend_diverse(users[:4096], min(N, pools[0]), pool=pools[0], lam=1.0)
        out["mean_maxsim_lambda_1_first_4096_users"] = float(lam1[2].mean())
        ident = D.recommend(users[:4096], min(N, pools[0]))
        out["lambda_1_is_recommend"] = bool(np.array_equal(lam1[0], ident[0]) and np.array_equal(lam1[1].view(np.uint64), ident[1].view(np.uint64)))
    print(json.dumps(out), flush=True)
    D.close()
    if args.out:
        p = Path(args.out)
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
