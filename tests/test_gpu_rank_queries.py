"""-m gpu: hpf_rank_queries, the fused multi-query kernel -- where EVERY queried item of a user stands among all items,
the user's row of scores computed once and never stored.  Its contract: rank and score equal, bit for bit, what
hpf_item_ranks returns for the expanded (q_sel, q_item) list."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests.test_gpu_loo_ranks import N, SHAPES, _case

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _qcase(K, bias, m):
    """test_gpu_loo_ranks' 37 users (a duplicate, mask lists of 0-5 items, user 3 with every item masked) with query
    counts 0, 1, 2, QCAP - 1, QCAP, QCAP + 1 and 3 QCAP + 2 (a row of the kernel holds QCAP queries: one row, one full row,
    two rows, four rows).  Items are drawn with replacement, so the long lists ask for items twice (at m = 64 and 70 they
    must); user 2 does so by construction.  The first query of a user is that case's single query: user 5's is masked
    through the list, user 7's is a training item, user 11 asks for item m - 1, user 12 for item 0.  User 3 has five
    queries and every score +0.0: its thresholds tie with each other and with every item."""
    from hgaprec_amd.capi import RANK_QUERIES_QCAP as QC
    D, rowptr, col, val, users, mask, mptr, mitems, q = _case(K, bias, m)
    rng = np.random.default_rng(1000 + K)
    pattern = [1, 2, QC - 1, QC, QC + 1, 3 * QC + 2, 0]
    counts = [pattern[b % 7] for b in range(users.size)]
    counts[3] = 5
    qs = []
    for b, c in enumerate(counts):
        x = rng.integers(0, m, c).astype(np.uint32)
        if c:
            x[0] = q[b]
        qs.append(x)
    qs[2][5] = qs[2][1]                                             # asked twice by one user
    qs[2][6] = qs[2][1]
    assert sorted(set(counts)) == sorted({0, 1, 2, 5, QC - 1, QC, QC + 1, 3 * QC + 2})
    assert counts[5] and counts[7] and qs[11][0] == m - 1 and qs[12][0] == 0 and mask[5][0] == qs[5][0]
    assert qs[7][0] in col[rowptr[users[7]]:rowptr[users[7] + 1]]
    q_ptr = np.zeros(users.size + 1, np.uint64)
    q_ptr[1:] = np.cumsum(counts)
    q_items = np.concatenate(qs).astype(np.uint32)
    q_sel = np.repeat(np.arange(users.size, dtype=np.uint32), counts)
    return D, rowptr, col, val, users, mask, mptr, mitems, q_ptr, q_items, q_sel


@pytest.mark.parametrize("K,bias,m", SHAPES)
def test_rank_queries_equal_item_ranks_bit_for_bit(K, bias, m):
    D, rowptr, col, val, users, mask, mptr, mitems, q_ptr, q_items, q_sel = _qcase(K, bias, m)
    want_r, want_s = D.item_ranks(users, q_sel, q_items, mptr, mitems)
    rank, sc = D.rank_queries(users, q_ptr, q_items, mptr, mitems)
    assert rank.size == q_items.size and sc.size == q_items.size
    assert np.array_equal(rank, want_r)
    assert np.array_equal(sc.view(np.uint64), want_s.view(np.uint64))
    u3 = slice(int(q_ptr[3]), int(q_ptr[4]))                        # every item masked: +0.0, item ascending decides
    assert np.all(sc[u3].view(np.uint64) == 0) and np.array_equal(rank[u3], q_items[u3])
    assert sc[int(q_ptr[5])] == 0.0 and sc[int(q_ptr[7])] == 0.0 and np.count_nonzero(sc) >= 100
    # without a mask list only the training items are zeroed
    want_r, want_s = D.item_ranks(users, q_sel, q_items)
    rank, sc = D.rank_queries(users, q_ptr, q_items)
    assert np.array_equal(rank, want_r) and np.array_equal(sc.view(np.uint64), want_s.view(np.uint64))
    D.close()


@pytest.mark.parametrize("K,bias,m", SHAPES)
def test_one_pass_equals_one_pass_per_query(K, bias, m):
    """hpf_loo_ranks with one selected "user" per (user, query) pair -- the only fused route before -- gives the same"""
    D, rowptr, col, val, users, mask, mptr, mitems, q_ptr, q_items, q_sel = _qcase(K, bias, m)
    emask = [mask[b] for b in q_sel]
    emptr = np.zeros(q_sel.size + 1, np.uint64)
    emptr[1:] = np.cumsum([x.size for x in emask])
    want_r, want_s, _ = D.loo_ranks(users[q_sel], q_items, emptr, np.concatenate(emask).astype(np.uint32))
    rank, sc = D.rank_queries(users, q_ptr, q_items, mptr, mitems)
    assert np.array_equal(rank, want_r) and np.array_equal(sc.view(np.uint64), want_s.view(np.uint64))
    D.close()


_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from tests.test_gpu_rank_queries import _qcase, SHAPES
out = []
for K, bias, m in SHAPES:
    D, rowptr, col, val, users, mask, mptr, mitems, q_ptr, q_items, q_sel = _qcase(K, bias, m)
    rank, sc = D.rank_queries(users, q_ptr, q_items, mptr, mitems)
    out.append([rank.tolist(), sc.view(np.uint64).tolist()])
    D.close()
print("RESULT " + json.dumps(out))
"""


def test_batch_boundary_gives_the_same_ranks():
    """HPF_LOO_BATCH=16: the 37 users go through in three batches (16, 16, 5), each with bit rows and rows of queries of
    its own.  The library reads the variable, hence a fresh process."""
    env = dict(os.environ, HPF_LOO_BATCH="16")
    r = subprocess.run([sys.executable, "-c", _CHILD, str(ROOT)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][0][7:])
    for (K, bias, m), (rank, scbits) in zip(SHAPES, got):
        D, rowptr, col, val, users, mask, mptr, mitems, q_ptr, q_items, q_sel = _qcase(K, bias, m)
        r1, s1 = D.rank_queries(users, q_ptr, q_items, mptr, mitems)
        assert np.array_equal(np.array(rank, np.uint32), r1)
        assert np.array_equal(np.array(scbits, np.uint64), s1.view(np.uint64))
        D.close()


def test_a_workgroup_sweeps_several_tiles():
    """The launch policy is hpf_loo_ranks', over rows: ceil(rows / 64) blocks of rows, and the ceil(m / 64) tiles cut so
    that some 1024 workgroups exist.  150 users with 1-3 queries are 150 rows = 3 blocks, so 342 splits; m = 25 000 is
    391 tiles: two tiles per workgroup, the item range cut 196 ways, the last split with one tile."""
    from tests.test_gpu_ranking import _setup
    from oracle import orc
    n, m, K = 150, 25000, 5
    M, D, rowptr, col, val = _setup(orc, n, m, K, 6000, False, seed=11)
    rng = np.random.default_rng(11)
    users = np.arange(n, dtype=np.uint32)
    counts = rng.integers(1, 4, n)
    q_ptr = np.zeros(n + 1, np.uint64)
    q_ptr[1:] = np.cumsum(counts)
    q_items = rng.integers(0, m, int(q_ptr[-1])).astype(np.uint32)
    q_items[0], q_items[1] = m - 1, 0
    mptr = (np.arange(n + 1) * 3).astype(np.uint64)
    mitems = rng.integers(0, m, 3 * n).astype(np.uint32)
    want_r, want_s = D.item_ranks(users, np.repeat(users, counts), q_items, mptr, mitems)
    rank, sc = D.rank_queries(users, q_ptr, q_items, mptr, mitems)
    assert np.array_equal(rank, want_r) and np.array_equal(sc.view(np.uint64), want_s.view(np.uint64))
    assert np.unique(rank).size > 100
    D.close()


def test_more_than_1024_blocks_of_rows_and_one_split():
    """70 000 users, all selected, two queries each: 70 000 rows = 1094 blocks of rows, more than the 1024 workgroups the
    policy aims at, so the item range (m = 128, two tiles) is not cut: every workgroup sweeps both tiles"""
    from hgaprec_amd.capi import Hpf
    n, m, K = 70000, 128, 5
    rng = np.random.default_rng(12)
    # (a handle with E set directly and two training items per user, ratings 0-2: the oracle's start state and
    # make_problem's per-user draws would take longer than everything the test checks)
    first = rng.integers(0, m, n)
    col = np.stack([first, (first + 1 + rng.integers(0, m - 1, n)) % m], axis=1).reshape(-1).astype(np.uint32)
    rowptr = (np.arange(n + 1) * 2).astype(np.int64)
    val = rng.integers(0, 3, 2 * n).astype(np.uint8)
    D = Hpf(n, m, K, hier=False, bias=False)
    D.upload_csr(rowptr, col, val)
    D.set_state("THETA_E", rng.gamma(0.3, 1.0, (n, K)) + 1e-3)
    D.set_state("BETA_E", rng.gamma(0.3, 1.0, (m, K)) + 1e-3)
    users = np.arange(n, dtype=np.uint32)
    q_ptr = (np.arange(n + 1) * 2).astype(np.uint64)
    q_items = rng.integers(0, m, 2 * n).astype(np.uint32)
    want_r, want_s = D.item_ranks(users, np.repeat(users, 2), q_items)
    rank, sc = D.rank_queries(users, q_ptr, q_items)
    assert np.array_equal(rank, want_r) and np.array_equal(sc.view(np.uint64), want_s.view(np.uint64))
    D.close()


def test_against_numpy_alone():
    """independent of the library's ranking code: hpf_scores' exact device scores, zeroed in numpy, stable argsort"""
    K, bias, m = SHAPES[2]
    D, rowptr, col, val, users, mask, mptr, mitems, q_ptr, q_items, q_sel = _qcase(K, bias, m)
    dev = D.scores(users)
    for b, u in enumerate(users):
        js = np.arange(rowptr[u], rowptr[u + 1])
        dev[b, col[js][val[js] > 0]] = 0.0
        dev[b, mask[b]] = 0.0
    rank, sc = D.rank_queries(users, q_ptr, q_items, mptr, mitems)
    for b in range(users.size):
        pos = np.empty(m, np.int64)
        pos[np.argsort(-dev[b], kind="stable")] = np.arange(m)      # score descending, item ascending
        sl = slice(int(q_ptr[b]), int(q_ptr[b + 1]))
        assert np.array_equal(rank[sl], pos[q_items[sl]])
        assert np.array_equal(sc[sl], dev[b, q_items[sl]])
    D.close()


def test_invalid_queries_and_empty_selections():
    from hgaprec_amd.capi import HpfError
    K, bias, m = SHAPES[0]
    D, rowptr, col, val, users, mask, mptr, mitems, q_ptr, q_items, q_sel = _qcase(K, bias, m)
    bad = q_items.copy()
    bad[20] = m
    with pytest.raises(HpfError):
        D.rank_queries(users, q_ptr, bad, mptr, mitems)
    with pytest.raises(HpfError):
        D.rank_queries(np.array([N], np.uint32), np.array([0, 1], np.uint64), np.array([0], np.uint32))
    with pytest.raises(HpfError):
        D.rank_queries(users[:2], np.array([1, 2, 3], np.uint64), q_items)
    with pytest.raises(HpfError):
        D.rank_queries(users[:2], np.array([0, 5, 3], np.uint64), q_items)
    r, s = D.rank_queries(np.zeros(0, np.uint32), np.zeros(1, np.uint64), np.zeros(0, np.uint32))
    assert r.size == 0 and s.size == 0
    r, s = D.rank_queries(users, np.zeros(users.size + 1, np.uint64), np.zeros(0, np.uint32), mptr, mitems)
    assert r.size == 0 and s.size == 0
    D.close()


def test_several_workgroups_and_the_two_chunk_register_path():
    """test_gpu_loo_ranks' shape of the same name, over rows: K = 40 (two staged chunks, A in registers:
    rank_queries_kernel<2>), every user selected with 1-3 queries -- 150 users are three workgroups of 64 rows or more --
    and m = 333 (five full tiles and one of 13 items)"""
    from tests.test_gpu_ranking import _setup
    from oracle import orc
    n, m, K = 150, 333, 40
    M, D, rowptr, col, val = _setup(orc, n, m, K, 5000, True, seed=3)
    rng = np.random.default_rng(3)
    users = np.arange(n, dtype=np.uint32)
    counts = rng.integers(1, 4, n)
    q_ptr = np.zeros(n + 1, np.uint64)
    q_ptr[1:] = np.cumsum(counts)
    q_items = rng.integers(0, m, int(q_ptr[-1])).astype(np.uint32)
    q_items[0], q_items[1] = m - 1, 0
    mptr = (np.arange(n + 1) * 3).astype(np.uint64)
    mitems = rng.integers(0, m, 3 * n).astype(np.uint32)
    want_r, want_s = D.item_ranks(users, np.repeat(users, counts), q_items, mptr, mitems)
    rank, sc = D.rank_queries(users, q_ptr, q_items, mptr, mitems)
    assert np.array_equal(rank, want_r) and np.array_equal(sc.view(np.uint64), want_s.view(np.uint64))
    assert np.unique(rank).size > 50
    D.close()


@pytest.mark.parametrize("K", [32, 33, 64, 65, 128, 129])
def test_chunk_count_boundaries_of_both_fused_kernels(K):
    """The column counts at which the fused kernels change instance (NCH = 1 | 2 | 4 chunks of 32 columns in registers,
    0 = A re-read per step): at K = 32, 64, 128 every unrolled step of the last chunk is live, at K = 33, 65, 129 one
    step of a new chunk (or of the re-read path) is.  m = 70: one full tile and one of 6 items.  hpf_loo_ranks and
    hpf_rank_queries each equal hpf_item_ranks bit for bit."""
    D, rowptr, col, val, users, mask, mptr, mitems, q = _case(K, True, 70)
    sel = np.arange(users.size, dtype=np.uint32)
    want_r, want_s = D.item_ranks(users, sel, q, mptr, mitems)
    rank, sc, _ = D.loo_ranks(users, q, mptr, mitems)
    assert rank.dtype.kind == "u" and np.array_equal(rank, want_r)
    assert np.array_equal(sc.view(np.uint64), want_s.view(np.uint64))
    rank, sc = D.rank_queries(users, np.arange(users.size + 1, dtype=np.uint64), q, mptr, mitems)
    assert rank.dtype.kind == "u" and np.array_equal(rank, want_r)
    assert np.array_equal(sc.view(np.uint64), want_s.view(np.uint64))
    assert np.count_nonzero(want_s) >= 10 and np.unique(want_r).size >= 10
    D.close()
