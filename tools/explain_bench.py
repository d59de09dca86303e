#!/usr/bin/env python3
"""Why a score is what it is: hpf_explain on C2's item side (m = 10^5 items, K = 100, E from synth.py), the pairs of the
hpf_recommend lists of 10^5 users (N = 100 items each: 10^7 pairs in list order, so runs of 100 pairs share a user), T = 5 --
against hpf_predict on the same pairs in the same process: the same two row gathers per pair, a sum instead of a selection,
one double back per pair instead of T ids and T doubles.  Also hpf_factor_top(1, 100) and hpf_factor_top(0, 100).

    python tools/explain_bench.py --out profiles/r10/explain.json [--n 100000] [--m 100000] [--K 100] [--topn 100] [--T 5] [--runs 5]

Wall times are those of the whole synchronous call (upload of the pairs, kernel, copy back); each path runs once unmeasured,
then --runs rounds alternate the paths (tools/rank_queries_bench.py's `timed`): the median, the smallest and the largest are
kept.  No kernel trace is taken: the figures do not say how the time of a call divides between its copies and its kernel.
The model is synthetic (synth.py's start state), not a trained one: a trained model's rows are sparser, which changes no
instruction the kernels execute.  --n / --m scale the problem down for a quick look."""
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
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--m", type=int, default=100_000)
    ap.add_argument("--K", type=int, default=100)
    ap.add_argument("--topn", type=int, default=100)
    ap.add_argument("--T", type=int, default=5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from hgaprec_amd import capi, synth
    from hgaprec_amd.capi import Hpf
    n, m, K, N, T = args.n, args.m, args.K, args.topn, args.T
    dev = torch.device("cuda", 0)
    # hpf_recommend wants a CSR: one nonzero per user, stored with rating 0 (nothing is masked by it)
    D = Hpf(n, m, K, hier=True, bias=False, device=0)
    D.upload_csr(np.arange(n + 1, dtype=np.int64), (np.arange(n, dtype=np.uint32) % m).astype(np.uint32), np.zeros(n, np.uint8))
    E = synth.initial_state_device(m, K, 12, dev)["E"]
    D.set_state_device("BETA_E", E)
    E = synth.initial_state_device(n, K, 13, dev)["E"]
    D.set_state_device("THETA_E", E)
    del E
    torch.cuda.empty_cache()
    items, _ = D.recommend(np.arange(n, dtype=np.uint32), N)
    assert not np.any(items == 0xFFFFFFFF)
    u = np.repeat(np.arange(n, dtype=np.uint32), N)
    i = np.ascontiguousarray(items.reshape(-1))
    del items

    fns = {"predict": lambda: D.predict(u, i),
           "explain": lambda: D.explain(u, i, T),
           "factor_top_items": lambda: D.factor_top(1, N),
           "factor_top_users": lambda: D.factor_top(0, N)}
    e, res = timed(fns, args.runs)
    # a look at what came back: the first pairs against numpy on the host's copies of the rows
    Et, Eb = D.get_state("THETA_E"), D.get_state("BETA_E")
    c = Et[u[:4096]] * Eb[i[:4096]]
    order = np.argsort(-c, axis=1, kind="stable")[:, :T]
    ok = bool(np.array_equal(res["explain"][0][:4096], order) and
              np.array_equal(res["explain"][1][:4096].view(np.uint64), np.take_along_axis(c, order, axis=1).view(np.uint64)))
    col = np.argsort(-Eb[:, 0], kind="stable")[:N]
    ok_top = bool(np.array_equal(res["factor_top_items"][0][0], col))
    out = {"workload": f"{n} users x their {N} recommended items of {m} = {u.size} pairs, K={K}, T={T}; "
                       f"hpf_factor_top(1, {N}) over {m} rows, hpf_factor_top(0, {N}) over {n} rows",
           "library": Path(str(capi.load_library()._name)).name, "runs": args.runs, "wall": e,
           "explain_over_predict": e["explain"]["median_s"] / e["predict"]["median_s"],
           "bytes_back": {"predict": int(u.size) * 8, "explain": int(u.size) * T * 12},
           "explain_grid": capi.explain_grid(u.size), "explain_plan": capi.explain_plan(K, False),
           "first_4096_pairs_equal_numpy": ok, "factor_0_items_equal_numpy": ok_top,
           "not_covered": "no kernel trace (wall time of the whole call only); a synthetic start state, not a trained model"}
    print(json.dumps(out), flush=True)
    D.close()
    if args.out:
        p = Path(args.out)
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
