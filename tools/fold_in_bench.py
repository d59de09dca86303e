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
it ran.  --n / --m / --nnz scale the problem down for a quick look.

    python tools/fold_in_bench.py --side items --out profiles/r12/fold_in_items.json [--iters 10] [--runs 5]

The mirror, hpf_fold_in_items: C2's user side -- n = 10^6 users, K = 100, -hier, synth.py's state -- and 10^4 new items
with synth.py's item degrees (5 * 10^6 ratings).  Three routes, the same protocol: the default (fold_in_kernel for the
items below FOLD_LONG_MIN ratings, fold_in_long_kernel for the others), HPF_FOLD_LONG_MIN at its maximum (every item on
the wave kernel) and HPF_FOLD_ROUTE=sweeps; then HPF_FOLD_LONG_MIN over {128, 256, 512, 1024, 2048}, alternating too."""
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


LONG_MIN_SWEEP = (128, 256, 512, 1024, 2048)
KNOBS = ("HPF_EXPERIMENTAL", "HPF_FOLD_ROUTE", "HPF_FOLD_LONG_MIN")


def items_side(args):
    """--side items: hpf_fold_in_items, three routes and the FOLD_LONG_MIN sweep"""
    import torch
    from hgaprec_amd import capi, synth
    from hgaprec_amd.capi import Hpf
    n, m, K, T = args.n or 1_000_000, args.m or 10_000, args.K, args.iters
    dev = torch.device("cuda", 0)
    rowptr, col, val = synth.generate_device(n, m, args.nnz, 0.5, 0.8, seed=3, device=dev)
    nnz = int(rowptr[-1])
    deg = torch.bincount(col.to(torch.int64), minlength=m).cpu().numpy()
    users = synth.initial_state_device(n, K, 11, dev)
    plan = capi.fold_items_plan(K)

    def handle(**knobs):
        for k in KNOBS:
            os.environ.pop(k, None)
        if knobs:
            os.environ.update(HPF_EXPERIMENTAL="1", **{k: str(v) for k, v in knobs.items()})
        D = Hpf(n, m, K, hier=True, bias=False, device=0)
        D.upload_csr_device(rowptr, col, val)
        D.set_state_device("THETA_E", users["E"])
        D.set_state_device("THETA_ELOG", users["Elog"])
        for k in KNOBS:
            os.environ.pop(k, None)
        return D

    def run(handles):
        e, _ = timed({k: (lambda D=D: D.fold_in_items(T, 0.0, want_iters=False)) for k, D in handles.items()}, args.runs)
        return e

    H = {"default": handle(), "wave_only": handle(HPF_FOLD_LONG_MIN=2 ** 32 - 1), "sweeps": handle(HPF_FOLD_ROUTE="sweeps")}
    e = run(H)
    worst = {}
    for w in ("BETA_SHAPE", "BETA_RATE", "BETA_E", "BETA_ELOG", "ETA_RATE", "ETA_E", "ETA_ELOG"):
        a = H["default"].get_state(w)
        worst[w] = {k: float(np.max(np.abs(a - H[k].get_state(w)) / np.maximum(np.abs(a), 1e-300))) for k in ("wave_only", "sweeps")}
    for D in H.values():
        D.close()
    out = {"workload": f"{n} users x {m} new items, {nnz} nonzeros, K={K}, -hier; T={T}, tol=0",
           "degrees": {"min": int(deg.min()), "median": float(np.median(deg)), "mean": float(deg.mean()), "max": int(deg.max()),
                       "items_held_in_lds": int(np.sum(deg <= plan["rows_held"])),
                       "long_items": {str(L): int(np.sum(deg >= L)) for L in LONG_MIN_SWEEP},
                       "share_of_ratings_in_long_items": {str(L): float(deg[deg >= L].sum() / max(nnz, 1)) for L in LONG_MIN_SWEEP}},
           "plan": plan, "runs": args.runs, "routes": e, "max_rel_diff_from_default": worst}
    print(json.dumps(out), flush=True)
    H = {str(L): handle(HPF_FOLD_LONG_MIN=L) for L in LONG_MIN_SWEEP}
    out["long_min_sweep"] = run(H)
    for D in H.values():
        D.close()
    print(json.dumps(out["long_min_sweep"]), flush=True)
    if args.out:
        p = Path(args.out)
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_text(json.dumps(out, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", choices=("users", "items"), default="users")
    ap.add_argument("--n", type=int, default=0, help="users (default 10^5 new users; --side items: C2's 10^6)")
    ap.add_argument("--m", type=int, default=0, help="items (default C2's 10^5; --side items: 10^4 new items)")
    ap.add_argument("--K", type=int, default=100)
    ap.add_argument("--nnz", type=int, default=5_000_000)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--cap", type=int, default=100, help="n_iters of the tol > 0 row")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.side == "items":
        return items_side(args)
    args.n, args.m = args.n or 100_000, args.m or 100_000

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
