"""-m gpu: hpf_loo_ranks, the fused score-and-count kernel -- where one item per user stands among all items,
without the score matrix.  Its contract: with item_limit = 0 rank and score equal hpf_item_ranks' bit for bit."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent

# K not a multiple of 4 / above the register path (128); m below one tile / no multiple of 64 / several tiles
SHAPES = [(5, False, 200), (7, True, 70), (100, False, 1000), (260, True, 64)]
N = 150


def _case(K, bias, m):
    """37 selected users (no multiple of 16): a duplicate, one with every item masked, one whose query item is
    masked through the list, one whose query is a training item; mask lists of 0-5 items"""
    from tests.test_gpu_ranking import _setup
    from oracle import orc
    M, D, rowptr, col, val = _setup(orc, N, m, K, 4000, bias, seed=K)
    rng = np.random.default_rng(K)
    users = np.sort(rng.choice(N, 36, replace=False)).astype(np.uint32)
    users = np.concatenate([users, users[4:5]])                     # 37, a duplicate
    mask = [np.sort(rng.choice(m, rng.integers(0, 6), replace=False)).astype(np.uint32) for _ in users]
    mask[3] = np.arange(m, dtype=np.uint32)                         # every item masked
    mask[9] = np.concatenate([mask[9], mask[9][:1]]) if mask[9].size else np.array([1, 1], np.uint32)   # a repeated entry
    q = rng.integers(0, m, users.size).astype(np.uint32)
    mask[5] = np.array([q[5]], np.uint32)                           # the query item itself is masked
    u7 = users[7]
    q[7] = col[rowptr[u7]]                                          # ... or a training item
    q[11] = m - 1
    q[12] = 0
    mptr = np.zeros(users.size + 1, np.uint64)
    mptr[1:] = np.cumsum([x.size for x in mask])
    mitems = np.concatenate(mask).astype(np.uint32)
    return D, rowptr, col, val, users, mask, mptr, mitems, q


@pytest.mark.parametrize("K,bias,m", SHAPES)
def test_loo_ranks_equal_item_ranks_bit_for_bit(K, bias, m):
    D, rowptr, col, val, users, mask, mptr, mitems, q = _case(K, bias, m)
    want_r, want_s = D.item_ranks(users, np.arange(users.size, dtype=np.uint32), q, mptr, mitems)
    rank, sc, masked = D.loo_ranks(users, q, mptr, mitems)
    assert np.array_equal(rank, want_r)
    assert np.array_equal(sc, want_s)
    assert want_s[3] == 0.0 and want_s[5] == 0.0 and want_s[7] == 0.0 and np.count_nonzero(want_s) >= 10
    # without a mask list only the training items are zeroed
    want_r, want_s = D.item_ranks(users, np.arange(users.size, dtype=np.uint32), q)
    rank, sc, _ = D.loo_ranks(users, q)
    assert np.array_equal(rank, want_r) and np.array_equal(sc, want_s)
    D.close()


_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from tests.test_gpu_loo_ranks import _case, SHAPES
out = []
for K, bias, m in SHAPES:
    D, rowptr, col, val, users, mask, mptr, mitems, q = _case(K, bias, m)
    rank, sc, masked = D.loo_ranks(users, q, mptr, mitems)
    out.append([rank.tolist(), sc.view(np.uint64).tolist(), masked.tolist()])
    D.close()
print("RESULT " + json.dumps(out))
"""


def test_batch_boundary_gives_the_same_ranks():
    """HPF_LOO_BATCH=16: the 37 users go through the kernel in three batches (16, 16, 5), each with bit rows of its
    own.  The library reads the variable, hence a fresh process."""
    env = dict(os.environ, HPF_LOO_BATCH="16")
    r = subprocess.run([sys.executable, "-c", _CHILD, str(ROOT)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][0][7:])
    for (K, bias, m), (rank, scbits, masked) in zip(SHAPES, got):
        D, rowptr, col, val, users, mask, mptr, mitems, q = _case(K, bias, m)
        r1, s1, m1 = D.loo_ranks(users, q, mptr, mitems)
        assert np.array_equal(np.array(rank, np.uint32), r1)
        assert np.array_equal(np.array(scbits, np.uint64), s1.view(np.uint64))
        assert np.array_equal(np.array(masked, np.uint32), m1)
        D.close()


@pytest.mark.parametrize("K,bias,m", SHAPES)
def test_item_limit_against_numpy(K, bias, m):
    D, rowptr, col, val, users, mask, mptr, mitems, q = _case(K, bias, m)
    lim = m - 1
    dev = D.scores(users)                                           # exact device scores, masked like the kernel
    distinct = []
    for b, u in enumerate(users):
        js = np.arange(rowptr[u], rowptr[u + 1])
        z = np.concatenate([col[js][val[js] > 0], mask[b]])
        dev[b, z] = 0.0
        distinct.append(np.unique(z[z < lim]).size)
    rank, sc, masked = D.loo_ranks(users, q, mptr, mitems, item_limit=lim)
    assert np.array_equal(masked, np.array(distinct, np.uint32))
    for b in range(users.size):
        if q[b] >= lim:
            assert rank[b] == 0 and sc[b] == 0.0                    # item m - 1 is never scored
            continue
        order = np.argsort(-dev[b, :lim], kind="stable")            # score descending, item ascending
        assert rank[b] == int(np.flatnonzero(order == q[b])[0])
        assert sc[b] == dev[b, q[b]]
    assert q[11] == m - 1 and masked[3] == lim
    D.close()


def test_invalid_queries_and_empty_selection():
    from hgaprec_amd.capi import HpfError
    K, bias, m = SHAPES[0]
    D, rowptr, col, val, users, mask, mptr, mitems, q = _case(K, bias, m)
    bad = q.copy()
    bad[20] = m
    with pytest.raises(HpfError):
        D.loo_ranks(users, bad, mptr, mitems)
    with pytest.raises(HpfError):
        D.loo_ranks(users, q, mptr, mitems, item_limit=m + 1)
    with pytest.raises(HpfError):
        D.loo_ranks(np.array([N], np.uint32), np.array([0], np.uint32))
    r, s, k = D.loo_ranks(np.zeros(0, np.uint32), np.zeros(0, np.uint32))
    assert r.size == 0 and s.size == 0 and k.size == 0
    D.close()


def test_several_workgroups_and_the_two_chunk_register_path():
    """beyond the four shapes: K = 40 (two staged chunks, A in registers), every user selected -- 150 users are three
    workgroups of 64, the last with 22 -- and m = 333 (five full tiles and one of 13 items)"""
    from tests.test_gpu_ranking import _setup
    from oracle import orc
    n, m, K = 150, 333, 40
    M, D, rowptr, col, val = _setup(orc, n, m, K, 5000, True, seed=3)
    rng = np.random.default_rng(3)
    users = np.arange(n, dtype=np.uint32)
    q = rng.integers(0, m, n).astype(np.uint32)
    mptr = (np.arange(n + 1) * 3).astype(np.uint64)
    mitems = rng.integers(0, m, 3 * n).astype(np.uint32)
    want_r, want_s = D.item_ranks(users, users, q, mptr, mitems)
    rank, sc, masked = D.loo_ranks(users, q, mptr, mitems)
    assert np.array_equal(rank, want_r) and np.array_equal(sc, want_s)
    for b in range(n):
        js = np.arange(rowptr[b], rowptr[b + 1])
        assert masked[b] == np.unique(np.concatenate([col[js][val[js] > 0], mitems[3 * b:3 * b + 3]])).size
    D.close()
