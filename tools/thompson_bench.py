#!/usr/bin/env python3
"""Thompson sampling: hpf_recommend_thompson beside hpf_recommend on the same handle at C2's shape (n = 10^6 users,
m = 10^5 items, K = 100, -hier, synthetic CSR from synth.py, E and the shapes set directly), for a chunk of --sel users as
`hgaprec -recommend N -thompson D` calls it once per draw; and gamma_rows_kernel over C2's item matrix.

    python tools/thompson_bench.py --out profiles/r16/thompson.json [--topn 100] [--runs 5] [--sel 65536]

Wall times are those of the whole calls (uploads of the lists, the sampled rows, kernels, copy back); each path runs once
unmeasured, then --runs rounds alternate the paths and the median is kept.  "sample_items" is hpf_sample_state of all m
items: gamma_rows_kernel over C2's item matrix, the dense copy and 8 m K bytes back to the host.  The kernel's own time
comes from a run of this tool under rocprofv3 --kernel-trace --stats (--runs 1), where it stands beside topn_sweep_kernel
and topn_merge_kernel.  --n / --m / --nnz scale the problem down for a quick look."""
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
    ap.add_argument("--seed", type=int, default=0)
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
    draw = [0]

    def thompson():
        draw[0] += 1                                              # a new draw per call, as the CLI's loop over t
        return D.recommend_thompson(users, N, args.seed, draw[0])
    e, res = timed({"recommend": lambda: D.recommend(users, N),
                    "recommend_thompson": thompson,
                    "sample_items": lambda: D.sample_state(1, args.seed, 0)}, args.runs)
    ld = D.work_info()["ld"]
    beta = res["sample_items"]
    out = {"workload": f"{n} users x {m} items, {nnz} nonzeros, K={K}, -hier; {users.size} selected users, topn={N}; no mask list",
           "runs": args.runs, "times": e,
           "plan": {"ld": ld, "item_draw_bytes": m * ld * 8, "elements_items": m * ld},
           "samples_finite_nonnegative": bool(np.all(np.isfinite(beta)) and np.all(beta >= 0)),
           "thompson_over_recommend": e["recommend_thompson"]["median_s"] / e["recommend"]["median_s"]}
    print(json.dumps(out), flush=True)
    D.close()
    if args.out:
        p = Path(args.out)
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
