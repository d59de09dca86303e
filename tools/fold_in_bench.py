#!/usr/bin/env python3
"""Fold-in of new users: hpf_fold_in's one fused launch (fold_in_kernel: a wave per user, state in registers, gathered
rows in LDS when they fit) against the same call through the training kernels (HPF_FOLD_ROUTE=sweeps under
HPF_EXPERIMENTAL=1: n_iters x (user-major phi pass + user sweep)).  C2's item side -- m = 10^5 items, K = 100, -hier, a
synthetic state from synth.py -- and 10^5 new users whose degrees synth.py draws as it does C2's (50 ratings per user).

    python tools/fold_in_bench.py --out profiles/r08/fold_in.json [--iters 10] [--runs 5]

The knobs are read when a handle is created, so the two routes are two handles of one process over the same CSR and the
same item side.  Wall times are those of the whole synchronous call (the fused route derives its copy of W and the column
sums inside it; the sweeps route sets the prior, derives both sides' W and materialises the state inside it); each route
runs once unmeasured, then --runs rounds alternate the routes: median [smallest - largest].  The states the two routes
leave are compared in the same run.  One more row: the fused route with tol = 1e-6 and the distribution of the iterations
it ran.  --n / --m / --nnz scale the problem down for a quick look."""
from __future__ import annotations

import argparse
import json
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tools.rank_queries_bench import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--m", type=int, default=100_000)
    ap.add_argument("--K", type=int, default=100)
    ap.add_argument("--nnz", type=int, default=5_000_000)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--cap", type=int, default=100, help="n_iters of the tol > 0 row")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from hgaprec_amd import capi, synth
    from hgaprec_amd.capi import Hpf
    n, m, K = args.n, args.m, args.K
    dev = torch.device("cuda", 0)
    rowptr, col, val = synth.generate_device(n, m, args.nnz, 0.5, 0.8, seed=3, device=dev)
    nnz = int(rowptr[-1])
    deg = torch.diff(rowptr).cpu().numpy()
    item = synth.initial_state_device(m, K, 12, dev)
    plan = capi.fold_plan(K)

    def handle(route):
        for k in ("HPF_EXPERIMENTAL", "HPF_FOLD_ROUTE"):
            os.environ.pop(k, None)
        if route == "sweeps":
            os.environ.update(HPF_EXPERIMENTAL="1", HPF_FOLD_ROUTE="sweeps")
        D = Hpf(n, m, K, hier=True, bias=False, device=0)
        D.upload_csr_device(rowptr, col, val)
        D.set_state_device("BETA_E", item["E"])
        D.set_state_device("BETA_ELOG", item["Elog"])
        return D

    F, S = handle("fused"), handle("sweeps")
    for k in ("HPF_EXPERIMENTAL", "HPF_FOLD_ROUTE"):
        os.environ.pop(k, None)
    T = args.iters
    e, _ = timed({"fused": lambda: F.fold_in(T, 0.0, want_iters=False), "sweeps": lambda: S.fold_in(T, 0.0, want_iters=False)}, args.runs)
    worst = {}
    for w in ("THETA_SHAPE", "THETA_RATE", "THETA_E", "THETA_ELOG", "XI_RATE", "XI_E", "XI_ELOG"):
        a, b = F.get_state(w), S.get_state(w)
        worst[w] = float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))
    out = {"workload": f"{n} new users x {m} items, {nnz} nonzeros, K={K}, -hier; T={T}, tol=0",
           "degrees": {"min": int(deg.min()), "median": float(np.median(deg)), "mean": float(deg.mean()), "max": int(deg.max()),
                       "share_of_users_held_in_lds": float(np.mean(deg <= plan["rows_held"]))},
           "plan": plan, "grid": capi.fold_grid(n), "runs": args.runs, "tol0": e,
           "sweeps_over_fused": e["sweeps"]["median_s"] / e["fused"]["median_s"],
           "max_rel_diff_between_routes": worst}
    print(json.dumps(out), flush=True)
    et, res = timed({"fused_tol": lambda: F.fold_in(args.cap, args.tol)}, args.runs)
    it = res["fused_tol"]
    q = [0, 5, 25, 50, 75, 95, 100]
    out["tol"] = {"tol": args.tol, "n_iters": args.cap, **et["fused_tol"],
                  "iterations": {"mean": float(it.mean()), "percentiles": {str(p): float(np.percentile(it, p)) for p in q},
                                 "share_at_cap": float(np.mean(it == args.cap))}}
    print(json.dumps(out["tol"]), flush=True)
    F.close()
    S.close()
    if args.out:
        p = Path(args.out)
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
