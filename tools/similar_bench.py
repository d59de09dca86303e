#!/usr/bin/env python3
"""Nearest neighbours in factor space: hpf_similar on C2's item side (m = 10^5 items, K = 100, E from synth.py), every item
selected, N = 100, cosine and dot -- against hpf_recommend at the same shape (10^5 selected users of a 10^5-user handle, no
mask list, N = 100), which runs the same sweep with the bit rows on top.

    python tools/similar_bench.py --out profiles/r09/similar.json [--m 100000] [--K 100] [--topn 100] [--runs 5]

Wall times are those of the whole synchronous call (upload of the ids, kernels, copy back of m x N ids and scores); each
path runs once unmeasured, then --runs rounds alternate the paths (tools/rank_queries_bench.py's `timed`): the median, the
smallest and the largest are kept.  "similar_not_slower" applies the rule of DESIGN.md section 4c: the median is not above
hpf_recommend's by more than that call's own smallest-to-largest spread.  HPF_LIB=<another build> times that build's
hpf_recommend as the yardstick in a run of its own (--yardstick-only).  --m scales the problem down for a quick look."""
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
    ap.add_argument("--m", type=int, default=100_000)
    ap.add_argument("--K", type=int, default=100)
    ap.add_argument("--topn", type=int, default=100)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--yardstick-only", action="store_true", help="time hpf_recommend alone (a build without hpf_similar)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from hgaprec_amd import capi, synth
    from hgaprec_amd.capi import Hpf
    m, K, N = args.m, args.K, args.topn
    dev = torch.device("cuda", 0)
    # one handle serves both: its users and its items are the same m rows of factors, so hpf_recommend sweeps what
    # hpf_similar sweeps.  hpf_recommend wants a CSR: one nonzero per user, stored with rating 0 (nothing is masked by it)
    D = Hpf(m, m, K, hier=True, bias=False, device=0)
    D.upload_csr(np.arange(m + 1, dtype=np.int64), np.arange(m, dtype=np.uint32), np.zeros(m, np.uint8))
    E = synth.initial_state_device(m, K, 12, dev)["E"]
    D.set_state_device("THETA_E", E)
    D.set_state_device("BETA_E", E)
    del E
    torch.cuda.empty_cache()
    ids = np.arange(m, dtype=np.uint32)

    fns = {"recommend": lambda: D.recommend(ids, N)}
    if not args.yardstick_only:
        fns["similar_dot"] = lambda: D.similar(1, ids, N, "dot")
        fns["similar_cosine"] = lambda: D.similar(1, ids, N, "cosine")
    e, res = timed(fns, args.runs)
    blocks, splits, tps = capi.recommend_grid(min(m, 1 << 16), m, N)
    out = {"workload": f"{m} rows, K={K}, N={N}, every row selected; hpf_recommend: {m} users x {m} items, no mask list",
           "library": Path(str(capi.load_library()._name)).name, "runs": args.runs, "wall": e,
           "grid_of_65536_rows": {"blocks": blocks, "splits": splits, "tiles_per_split": tps, "cap": capi.recommend_cap(N)}}
    if not args.yardstick_only:
        spread = e["recommend"]["max_s"] - e["recommend"]["min_s"]
        for k in ("similar_dot", "similar_cosine"):
            out[k + "_over_recommend"] = e[k]["median_s"] / e["recommend"]["median_s"]
            out[k + "_not_slower"] = bool(e[k]["median_s"] <= e["recommend"]["median_s"] + spread)
        # the dot lists are hpf_recommend's with the row itself taken out (E[theta] = E[beta], nothing masked)
        ri, si = res["recommend"][0][:256], res["similar_dot"][0][:256]
        out["dot_is_recommend_without_self"] = bool(all(
            np.array_equal(si[b][:N - 1], ri[b][ri[b] != b][:N - 1]) for b in range(ri.shape[0])))
    print(json.dumps(out), flush=True)
    D.close()
    if args.out:
        p = Path(args.out)
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
