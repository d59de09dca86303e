#!/usr/bin/env python3
"""Because you rated: the wall time of hpf_because for 16 384 users x their 100 recommended items at C2's shape
(m = 10^5 items, K = 100, -hier, 50 ratings per user drawn as synth.py draws C2's, a synthetic state from synth.py), T = 5 --
beside hpf_recommend(topn = 100) for the same users in the same process, as context only.

    python tools/because_bench.py --out profiles/r13/because.json [--sel 16384] [--m 100000] [--K 100] [--topn 100] [--T 5] [--runs 5]

Wall times are those of the whole synchronous call (upload of the targets, the gathered copy of the item side, both kernels,
copy back); each call runs once unmeasured, then --runs rounds alternate the two (tools/rank_queries_bench.py's `timed`):
the median, the smallest and the largest are kept.  No kernel trace is taken.  A look at what came back: for the first
users the sums against the definition in numpy (tests/because_ref.py).  --sel / --m scale the problem down."""
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
    ap.add_argument("--sel", type=int, default=16384)
    ap.add_argument("--m", type=int, default=100_000)
    ap.add_argument("--K", type=int, default=100)
    ap.add_argument("--per-user", type=int, default=50)
    ap.add_argument("--topn", type=int, default=100)
    ap.add_argument("--T", type=int, default=5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from hgaprec_amd import capi, synth
    from hgaprec_amd.capi import Hpf
    from tests import because_ref as R
    n, m, K, N, T = args.sel, args.m, args.K, args.topn, args.T
    dev = torch.device("cuda", 0)
    rowptr, col, val = synth.generate_device(n, m, n * args.per_user, 0.5, 0.8, seed=3, device=dev)
    D = Hpf(n, m, K, hier=True, bias=False, device=0)
    D.upload_csr_device(rowptr, col, val)
    for side, rows, seed in (("BETA", m, 12), ("THETA", n, 13)):
        st = synth.initial_state_device(rows, K, seed, dev)
        D.set_state_device(side + "_E", st["E"])
        D.set_state_device(side + "_ELOG", st["Elog"])
    del st
    torch.cuda.empty_cache()
    users = np.arange(n, dtype=np.uint32)
    items, _ = D.recommend(users, N)
    assert not np.any(items == 0xFFFFFFFF)
    t_ptr = (np.arange(n + 1, dtype=np.uint64) * N)
    t_items = np.ascontiguousarray(items.reshape(-1))
    fns = {"because": lambda: D.because(users, t_ptr, t_items, T),
           "recommend": lambda: D.recommend(users, N)}
    e, res = timed(fns, args.runs)
    # the definition in numpy for the first users' first targets
    rp, cc, vv = rowptr.cpu().numpy(), col.cpu().numpy().view(np.uint32), val.cpu().numpy()
    stt = R.State(D.get_state("THETA_E"), D.get_state("THETA_ELOG"), D.get_state("BETA_E"), D.get_state("BETA_ELOG"))
    worst = 0.0
    for u in range(min(n, 8)):
        hist = cc[rp[u]:rp[u + 1]]
        yy = np.where(vv[rp[u]:rp[u + 1]] > 1, vv[rp[u]:rp[u + 1]], 1).astype(np.float64)
        ts = t_items[u * N:u * N + 4]
        for k, (con, prior) in enumerate(R.numpy64(stt, hist, yy, u, ts)):
            q = u * N + k
            worst = max(worst, abs(res["because"][2][q] - con.sum()) / con.sum(), abs(res["because"][3][q] - prior) / prior)
    deg = np.diff(rp)
    out = {"workload": f"{n} users x their {N} recommended items of {m} = {t_items.size} pairs, K={K}, -hier, T={T}; "
                       f"histories {int(deg.min())} .. {int(deg.max())}, mean {float(deg.mean()):.1f}",
           "library": Path(str(capi.load_library()._name)).name, "runs": args.runs, "wall": e,
           "because_over_recommend": e["because"]["median_s"] / e["recommend"]["median_s"],
           "because_plan": capi.because_plan(K, False), "because_grid": capi.because_grid(n, t_items.size),
           "first_users_sum_and_prior_max_rel_diff_from_numpy": worst,
           "not_covered": "no kernel trace (wall time of the whole call only); a synthetic start state, not a trained model"}
    print(json.dumps(out), flush=True)
    D.close()
    if args.out:
        p = Path(args.out)
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
