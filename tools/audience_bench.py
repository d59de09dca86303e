#!/usr/bin/env python3
"""The top-N users of every item: hpf_audience over ALL items of C2's shape (n = 10^6 users, m = 10^5 items, K = 100, -hier,
synthetic CSR from synth.py, E set directly), in chunks of 65 536 items as `hgaprec -audience` calls it, beside hpf_recommend
over all users of the same handle at the same N (the same flop count; 2 112 items a batch against 21 440 users).

    python tools/audience_bench.py --out profiles/r14/audience.json [--topn 100] [--runs 2]

Wall times are those of the whole calls (uploads of the lists, kernels, copy back); each path runs once unmeasured, then
--runs rounds alternate the paths.  The share of the mask rows is taken as a difference: the same call on a second handle
with the same factors whose CSR masks nothing (one nonzero per user, stored with rating 0) still clears the bit rows and
launches audience_mask_kernel, but walks no column.  --n / --m / --nnz scale the problem down for a quick look."""
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
    ap.add_argument("--topn", type=int, default=100)
    ap.add_argument("--runs", type=int, default=2)
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
    Et, Eb = synth.initial_state_device(n, K, 11, dev)["E"], synth.initial_state_device(m, K, 12, dev)["E"]
    D.set_state_device("THETA_E", Et)
    D.set_state_device("BETA_E", Eb)
    colptr = D.get_csc(with_vals=False)[0]
    longest = int(np.diff(colptr).max())
    # the same factors, nothing masked
    Z = Hpf(n, m, K, hier=True, bias=False, device=0)
    Z.upload_csr(np.arange(n + 1, dtype=np.int64), (np.arange(n) % m).astype(np.uint32), np.zeros(n, np.uint8))
    Z.set_state_device("THETA_E", Et)
    Z.set_state_device("BETA_E", Eb)
    del Et, Eb
    torch.cuda.empty_cache()

    def all_items(H):
        last = None
        for i0 in range(0, m, 1 << 16):
            last = H.audience(np.arange(i0, min(m, i0 + (1 << 16)), dtype=np.uint32), N)
        return last

    def all_users():
        last = None
        for u0 in range(0, n, 1 << 16):
            last = D.recommend(np.arange(u0, min(n, u0 + (1 << 16)), dtype=np.uint32), N)
        return last

    e, _ = timed({"audience_all_items": lambda: all_items(D), "audience_nothing_masked": lambda: all_items(Z),
                  "recommend_all_users": all_users}, args.runs)
    full, bare = e["audience_all_items"]["median_s"], e["audience_nothing_masked"]["median_s"]
    out = {"workload": f"{n} users x {m} items, {nnz} nonzeros (longest column {longest}), K={K}, -hier; topn={N}; no mask list",
           "runs": args.runs, "times": e, "mask_rows_share": (full - bare) / full,
           "audience_over_recommend": full / e["recommend_all_users"]["median_s"]}
    print(json.dumps(out), flush=True)
    D.close()
    Z.close()
    if args.out:
        p = Path(args.out)
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
