"""No GPU: -eval-all's arithmetic from ranks to metrics (eval_from_ranks in hgaprec_host.cpp, through hostlib) against
numpy on hand-made ranks, and the flag's way through the CLI's parser."""
import subprocess
from pathlib import Path

import numpy as np

from hgaprec_amd import hostlib

ROOT = Path(__file__).resolve().parent.parent
EXE = str(ROOT / "hgaprec_amd" / "hgaprec")
M_ITEMS = 500

# (ranks of the user's test items in the caller's order, nranked)
USERS = [
    ([0], 480),                              # one query at rank 0: precision@10 = .1, recall = 1, mrr = 1
    ([9, 10], 470),                          # the precision@10 edge: rank 9 is a hit, rank 10 is not
    ([99, 100, 250], 499),                   # ... and precision@100's
    ([100, 10, 499], M_ITEMS),               # every training item rated 0: nranked = m; no hit at all; best rank not first
    ([3, 1, 2], 123),                        # mrr = 1 / 2 in real division (the reference's integer 1 / 2 is 0)
    ([7, 7], 300),                           # an item asked twice
]


def _numpy(users):
    rows, sums = [], np.zeros(5)
    for ranks, nranked in users:
        r = np.array(ranks, np.int64)
        row = [r.size, int(np.count_nonzero(r < 10)), int(np.count_nonzero(r < 100)), int(r.min()), int((r + 1).sum()), nranked]
        rows.append(row)
        sums += [row[1] / 10, row[2] / 100, row[2] / r.size, 1.0 / (row[3] + 1), (row[4] / nranked) / r.size]
    return np.array(rows, np.uint64), sums / len(users)


def _call(users):
    q_ptr = np.zeros(len(users) + 1, np.uint64)
    q_ptr[1:] = np.cumsum([len(r) for r, _ in users])
    rank = np.concatenate([np.array(r, np.uint32) for r, _ in users]) if users else np.zeros(0, np.uint32)
    return hostlib.eval_from_ranks(q_ptr, rank, np.array([nr for _, nr in users], np.uint32))


def test_metrics_from_ranks_against_numpy():
    per, means = _call(USERS)
    want_rows, want_means = _numpy(USERS)
    assert np.array_equal(per, want_rows)
    assert means["users"] == len(USERS) and means["pairs"] == sum(len(r) for r, _ in USERS)
    got = np.array([means[k] for k in ("precision10", "precision100", "recall100", "mrr", "meanrank")])
    assert np.array_equal(got, want_means)                          # the same sums in the same order: the same doubles
    assert hostlib.EVAL_USER_FIELDS == ("ntest", "hits10", "hits100", "best_rank", "sum_rank", "nranked")


def test_each_edge_by_hand():
    col = {k: j for j, k in enumerate(hostlib.EVAL_USER_FIELDS)}
    per, means = _call(USERS[:1])
    assert per[0].tolist() == [1, 1, 1, 0, 1, 480]
    assert means["precision10"] == 0.1 and means["precision100"] == 0.01 and means["recall100"] == 1.0 and means["mrr"] == 1.0
    assert means["meanrank"] == (1 / 480) / 1
    per, means = _call(USERS[1:2])
    assert per[0, col["hits10"]] == 1 and per[0, col["hits100"]] == 2 and per[0, col["sum_rank"]] == 21
    per, means = _call(USERS[2:3])
    assert per[0, col["hits10"]] == 0 and per[0, col["hits100"]] == 1 and means["recall100"] == 1 / 3
    per, means = _call(USERS[3:4])
    assert per[0, col["hits100"]] == 1 and per[0, col["best_rank"]] == 10 and means["mrr"] == 1 / 11
    assert means["meanrank"] == ((101 + 11 + 500) / M_ITEMS) / 3
    per, means = _call(USERS[4:5])
    assert means["mrr"] == 0.5                                       # not the reference's integer division
    per, means = _call([])
    assert per.shape == (0, 6) and means["users"] == 0 and means["pairs"] == 0 and means["mrr"] == 0.0


def test_a_sum_rank_beyond_32_bits():
    ranks = [4_000_000_000, 4_000_000_001]
    per, means = _call([(ranks, 4_100_000_000)])
    assert int(per[0, 4]) == sum(r + 1 for r in ranks) and int(per[0, 3]) == ranks[0] and per[0, 1] == 0


def test_cli_takes_eval_all_and_refuses_it_with_ngpus(tmp_path):
    base = [EXE, "-dir", str(tmp_path / "missing"), "-n", "5", "-m", "5", "-k", "2", "-eval-all"]
    r = subprocess.run(base, cwd=tmp_path, capture_output=True, text=True)
    assert "unknown option" not in r.stdout and "outside the MI355X hot-path build" not in r.stderr
    assert "ONE GPU" not in r.stderr                                 # accepted (fails later: no data)
    r = subprocess.run(base + ["-ngpus", "2", "-label", "two"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 1 and "-eval-all" in r.stderr and "ONE GPU" in r.stderr and "without -ngpus" in r.stderr
    assert not list(tmp_path.glob("*two*"))                          # refused before the output directory exists
