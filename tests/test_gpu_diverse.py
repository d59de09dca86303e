"""-m gpu: hpf_recommend_diverse -- greedy maximal marginal relevance over the pool hpf_recommend finds (unit_rows_kernel,
the unchanged topn_sweep_kernel / topn_merge_kernel at topn = pool, then mmr_kernel: the pool's Gram matrix on the fp64
matrix cores and the selection).

Every comparison is bit for bit.  The oracle is tests/diverse_ref.py, the numpy statement of the selection, fed from
EXISTING calls: the pool from Hpf.recommend, the Gram matrix from hpf_scores on a square handle whose E[theta] = E[beta] =
the probe's unit rows (probe_unit_rows).  Ties, exact cosines and pool sizes are set directly through probe_mmr, which
launches mmr_kernel as the call does on a pool and a U of the test's."""
import ctypes as C

import numpy as np
import pytest

from hgaprec_amd.capi import Hpf, HpfError
from tests import diverse_ref as R
from tests.test_gpu_rank_edges import _train
from tests.test_gpu_similar import _probe_lib, _square_scores, unit_rows

pytestmark = pytest.mark.gpu
INVALID, UNSUPPORTED, STATE = -1, -5, -6
PAD = R.PAD
N_USERS, N_ITEMS = 24, 600
KS, POOLS, LAMBDAS = (1, 3, 100, 129), (1, 16, 17, 33, 100, 256), (0.0, 0.3, 0.7, 1.0)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _eq(got, want, what):
    names = ("items", "scores", "maxsim", "mmr")
    for k, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, f"{what}: {names[k]} shape"
        same = np.array_equal(g, w) if g.dtype != np.float64 else np.array_equal(_bits(g), _bits(w))
        if not same:
            bad = np.argwhere((g != w) if g.dtype != np.float64 else (_bits(g) != _bits(w)))
            assert False, f"{what}: {names[k]} differ at {bad[:4].tolist()}: {g[tuple(bad[0])]!r} vs {w[tuple(bad[0])]!r} ({bad.shape[0]} in all)"


def _raises(code, f, msg=None):
    with pytest.raises(HpfError) as e:
        f()
    assert f"({code})" in str(e.value) and (msg is None or msg in str(e.value)), str(e.value)


def _mask_csr(lists):
    mptr = np.zeros(len(lists) + 1, np.uint64)
    mptr[1:] = np.cumsum([len(x) for x in lists])
    return mptr, np.concatenate([np.asarray(x, np.uint32) for x in lists] + [np.zeros(0, np.uint32)]).astype(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------
# the clustered model: re-ranking has something to move
# ---------------------------------------------------------------------------------------------------------------------
def clustered(n, m, K, seed):
    """items in groups of 5 to 10 around a sparse centre with a small perturbation; users weighted on two or three
    clusters, every second one with a faint dense background (so that some pools are full and some are short)"""
    rng = np.random.default_rng(seed)
    beta = np.zeros((m, K))
    cluster_of = np.zeros(m, np.int64)
    centres, i = [], 0
    while i < m:
        size = min(int(rng.integers(5, 11)), m - i)
        c = np.zeros(K)
        act = rng.choice(K, min(K, int(rng.integers(2, 5))), replace=False)
        c[act] = rng.gamma(2.0, 1.0, act.size) + 0.2
        for j in range(size):
            beta[i + j] = c * (1.0 + 0.05 * rng.random(K)) * float(rng.uniform(0.5, 2.0))
        cluster_of[i:i + size] = len(centres)
        centres.append(c)
        i += size
    theta = np.zeros((n, K))
    for u in range(n):
        for c in rng.choice(len(centres), int(rng.integers(2, 4)), replace=False):
            theta[u] += float(rng.uniform(0.5, 2.0)) * centres[c]
        if u % 2 == 0:
            theta[u] += 1e-3 * rng.random(K)
    return theta, beta, cluster_of


_models, _grams = {}, {}


def model(K):
    if K not in _models:
        _models[K] = clustered(N_USERS, N_ITEMS, K, 77 + K)
    return _models[K]


def gram(K):
    """the cosines of every pair of items of model(K) from existing calls: hpf_scores on a square handle of the unit rows.
    Computed once per K and left unchanged"""
    if K not in _grams:
        U = unit_rows(model(K)[1])
        G = _square_scores(U, np.arange(N_ITEMS, dtype=np.uint32))
        assert np.array_equal(_bits(G), _bits(G.T)), "G is symmetric bit for bit"
        G.setflags(write=False)
        _grams[K] = G
    return _grams[K]


def handle(K, bias, n=N_USERS, m=N_ITEMS, theta=None, beta=None, seed=5):
    if theta is None:
        theta, beta, _ = model(K)
    D = Hpf(n, m, K, hier=False, bias=bias)
    rowptr, col, val, _ = _train(n, m)
    D.upload_csr(rowptr, col, val)
    D.set_state("THETA_E", theta)
    D.set_state("BETA_E", beta)
    if bias:                                                     # enters the scores and never G
        rng = np.random.default_rng(seed)
        D.set_state("UBIAS_E", rng.gamma(1.0, 0.05, n))
        D.set_state("IBIAS_E", rng.gamma(1.0, 0.05, m))
    return D


def reference(D, G, users, topn, pool, lam, mptr=None, mitems=None):
    items, scores = D.recommend(users, pool, mptr, mitems)
    return R.mmr_lists(items, scores, lambda c: G[np.ix_(c, c)], topn, lam)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the hand-checked fixture
# ---------------------------------------------------------------------------------------------------------------------
def test_fixture_all_four_outputs_exact():
    theta, beta, topn, want = R.fixture()
    D = Hpf(1, 7, 2, hier=False, bias=False)
    try:
        D.upload_csr(np.array([0, 1], np.int64), np.array([6], np.uint32), np.array([1], np.uint8))    # item 6: the one training item
        D.set_state("THETA_E", theta)
        D.set_state("BETA_E", beta)
        got = D.recommend_diverse(np.zeros(1, np.uint32), topn, pool=topn, lam=0.5)
        _eq([g[0] for g in got], (want["items"], want["scores"], want["maxsim"], want["mmr"]), "the fixture")
        # a longer list and a pool beyond the items: P = 6, then padding
        got = D.recommend_diverse(np.zeros(1, np.uint32), 9, pool=32, lam=0.5)
        _eq([g[0][:6] for g in got], (want["items"], want["scores"], want["maxsim"], want["mmr"]), "the fixture, topn 9")
        assert (got[0][0][6:] == PAD).all() and not any(_bits(g[0][6:]).any() for g in got[1:])
    finally:
        D.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. against the reference
# ---------------------------------------------------------------------------------------------------------------------
def test_the_fixture_moves_on_the_reference_alone():
    """Before anything is compared: at lambda = 0.3 every user's reference list differs from its lambda = 1 list.  Asserted
    for every pool and list of the comparison below where the definition lets a list move at all: with K = 1 every cosine
    is 1, so after the first pick all keys drop by the same (1 - lambda) and the order of hpf_recommend stands for every
    lambda; a list of one entry (topn = 1, pool = 1) is always c_0.  Those cases are compared all the same: they pin
    exactly that."""
    for K in (3, 100, 129):
        G = gram(K)
        D = handle(K, False)
        try:
            users = np.arange(N_USERS, dtype=np.uint32)
            for pool in (16, 17, 33, 100, 256):
                for topn in (pool // 2, pool):
                    a = reference(D, G, users, topn, pool, 0.3)[0]
                    b = reference(D, G, users, topn, pool, 1.0)[0]
                    moved = (a != b).any(axis=1)
                    assert moved.all(), f"K={K} pool={pool} topn={topn}: users {np.flatnonzero(~moved).tolist()} keep their list"
        finally:
            D.close()


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("K", KS)
def test_against_the_reference_bit_for_bit(K, bias):
    G = gram(K)
    D = handle(K, bias)
    try:
        users = np.arange(N_USERS, dtype=np.uint32)
        short = 0
        for pool in POOLS:
            lists = D.recommend(users, pool)
            short += int((lists[1] <= 0.0).any())
            for topn in sorted({1, max(1, pool // 2), pool}):
                for lam in LAMBDAS:
                    want = R.mmr_lists(lists[0], lists[1], lambda c: G[np.ix_(c, c)], topn, lam)
                    got = D.recommend_diverse(users, topn, pool=pool, lam=lam)
                    _eq(got, want, f"K={K} bias={bias} pool={pool} topn={topn} lambda={lam}")
        assert bias or K < 100 or short > 0, "without bias some pools are shorter than asked (a user's clusters have fewer items)"
    finally:
        D.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. lambda = 1, pool == topn, padding
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,bias", [(3, True), (100, False)])
def test_lambda_one_is_recommend_and_pool_equal_topn_is_a_permutation(K, bias):
    D = handle(K, bias)
    try:
        users = np.arange(N_USERS, dtype=np.uint32)
        lists = [np.sort(np.random.default_rng(b).choice(N_ITEMS, b % 4, replace=False)) for b in range(N_USERS)]
        mptr, mitems = _mask_csr(lists)
        for topn in (1, 20, 100, 256):
            items, scores = D.recommend(users, topn, mptr, mitems)
            pos = scores > 0.0
            want = (np.where(pos, items, PAD).astype(np.uint32), np.where(pos, scores, 0.0))
            for pool in sorted({topn, min(256, 4 * topn), 256}):
                got = D.recommend_diverse(users, topn, pool=pool, lam=1.0, mask_ptr=mptr, mask_items=mitems)
                _eq(got[:2], want, f"lambda=1 topn={topn} pool={pool}")
                assert not _bits(got[2])[~pos].any() and not _bits(got[3])[~pos].any()
            for lam in (0.0, 0.5):
                got = D.recommend_diverse(users, topn, pool=topn, lam=lam, mask_ptr=mptr, mask_items=mitems)
                for b in range(N_USERS):
                    assert sorted(got[0][b].tolist()) == sorted(want[0][b].tolist()), f"pool == topn == {topn} lambda={lam} user {b}"
                    assert got[0][b][0] == want[0][b][0], "the first pick is c_0"
                    order = {int(it): j for j, it in enumerate(want[0][b]) if it != PAD}
                    assert all(_bits(got[1][b])[t] == _bits(want[1][b])[order[int(it)]] for t, it in enumerate(got[0][b]) if it != PAD)
    finally:
        D.close()


def test_padding_short_pools_and_fewer_items_than_the_pool():
    # a user whose positive scores number fewer than topn: user 0 loads on one factor only three items have
    K, n, m = 4, 3, 40
    beta = np.zeros((m, K))
    beta[:, 1] = np.linspace(1.0, 2.0, m)
    beta[[7, 20, 33], 0] = [3.0, 1.0, 2.0]
    theta = np.array([[1.0, 0, 0, 0], [0.5, 1.0, 0, 0], [0, 0, 1.0, 0]])             # user 2: no positive score at all
    G = _square_scores(unit_rows(beta), np.arange(m, dtype=np.uint32))
    D = handle(K, False, n, m, theta, beta)
    try:
        users = np.arange(n, dtype=np.uint32)
        for topn, pool in ((10, 10), (10, 64), (64, 64), (41, 256)):                # n_items = 40 < pool
            want = reference(D, G, users, topn, pool, 0.4)
            got = D.recommend_diverse(users, topn, pool=pool, lam=0.4)
            _eq(got, want, f"topn={topn} pool={pool}")
            mine = set(_train(n, m)[3][0])
            listed = [it for it in (7, 33, 20) if it not in mine]
            assert got[0][0][:len(listed)].tolist() == listed and (got[0][0][len(listed):] == PAD).all()
            assert (got[0][2] == PAD).all() and not any(_bits(g[2]).any() for g in got[1:])
            assert (got[0][1] != PAD).sum() == min(topn, (D.recommend(users[1:2], min(pool, 256))[1] > 0).sum())
    finally:
        D.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. ties and exact cosines, through probe_mmr
# ---------------------------------------------------------------------------------------------------------------------
def probe_mmr(U, K, pool_items, pool_scores, topn, lam):
    lib = _probe_lib()
    u32p, dp = C.POINTER(C.c_uint32), C.POINTER(C.c_double)
    lib.probe_mmr.argtypes = [dp, C.c_uint32, C.c_uint32, C.c_uint32, u32p, dp, C.c_uint32, C.c_uint32, C.c_double, u32p, dp, dp, dp]
    U = np.ascontiguousarray(U, np.float64)
    rows, ld = U.shape
    pi, ps = np.ascontiguousarray(pool_items, np.uint32), np.ascontiguousarray(pool_scores, np.float64)
    oi = np.empty(topn, np.uint32)
    os_, om, ok = (np.empty(topn, np.float64) for _ in range(3))
    rc = lib.probe_mmr(U.ctypes.data_as(dp), rows, ld, K, pi.ctypes.data_as(u32p), ps.ctypes.data_as(dp), pi.size, topn, float(lam),
                       oi.ctypes.data_as(u32p), os_.ctypes.data_as(dp), om.ctypes.data_as(dp), ok.ctypes.data_as(dp))
    assert rc == 0, f"probe_mmr: HIP error {rc}"
    return oi, os_, om, ok


def _padded(U):
    """a matrix of even stride whose columns from K on hold junk: they take no part"""
    rows, K = U.shape
    buf = np.full((rows, (K + 3) & ~1), 1e300)
    buf[:, :K] = U
    return buf


def test_probe_ties_identical_rows_equal_scores_and_a_zero_row():
    K = 3
    # rows 0, 1 and 4, 5 are bit-identical; row 6 is all zero
    U = np.array([[1.0, 0, 0], [1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0], [0, 0.6, 0.8], [0, 0.6, 0.8], [0, 0, 0], [0.6, 0, 0.8]])
    G = _square_scores(U, np.arange(8, dtype=np.uint32))
    assert G[0, 1] == 1.0 and G[6].tolist() == [0.0] * 8 and not np.signbit(G[6]).any() and not np.isnan(G).any()
    assert np.array_equal(_bits(G[4]), _bits(G[5])) and np.array_equal(_bits(G), _bits(G.T))
    buf = _padded(U)
    # (a) bit-identical item rows with equal scores: their cosine to everything is equal, so their keys are equal in every
    # round and the earlier pool position wins
    r = np.array([2.0, 2.0, 1.0, 1.0, 0.5])
    for order in ([1, 0, 5, 4, 2], [0, 1, 4, 5, 2], [5, 4, 1, 0, 7], [3, 7, 4, 5, 0]):
        c = np.array(order, np.uint32)
        for lam in (0.0, 0.25, 0.5, 1.0):
            want = R.mmr(c, r, G[np.ix_(c, c)], 5, lam)
            _eq(probe_mmr(buf, K, c, r, 5, lam), want, f"identical rows {order} lambda={lam}")
    got = probe_mmr(buf, K, np.array([1, 0, 2], np.uint32), np.array([2.0, 2.0, 2.0]), 3, 0.5)
    assert got[0].tolist() == [1, 2, 0] and got[2].tolist() == [0.0, 0.0, 1.0] and got[3].tolist() == [0.5, 0.5, 0.0]
    # (b) all-equal scores over a pool of every size class, orthogonal and repeated directions: ties at every round
    rng = np.random.default_rng(12)
    for P in (1, 2, 16, 17, 64, 65, 200, 256):
        rows = rng.integers(0, 4, P)                                                 # only rows 0 .. 3: cosines exactly 0 or 1
        Ubig = _padded(U[rows])
        Gb = _square_scores(U[rows], np.arange(P, dtype=np.uint32))
        c = rng.permutation(P).astype(np.uint32)
        r = np.full(P, 0.75)
        for lam in (0.0, 0.5, 1.0):
            for topn in sorted({1, P, min(256, P + 3)}):
                want = R.mmr(c, r, Gb[np.ix_(c, c)], topn, lam)
                _eq(probe_mmr(Ubig, K, c, r, topn, lam), want, f"equal scores P={P} topn={topn} lambda={lam}")
    # (c) an all-zero U row: its cosine to everything is +0.0, no NaN; with lambda = 0 it ties with what is orthogonal
    c = np.array([7, 6, 0, 3, 2], np.uint32)
    r = np.array([4.0, 3.0, 2.0, 1.0, 0.5])
    for lam in (0.0, 0.5):
        got = probe_mmr(buf, K, c, r, 5, lam)
        _eq(got, R.mmr(c, r, G[np.ix_(c, c)], 5, lam), f"a zero row, lambda={lam}")
        assert not np.isnan(got[2]).any() and not np.isnan(got[3]).any()
        assert _bits(got[2])[got[0] == 6][0] == 0, "the zero row's maxsim is +0.0"
    # (d) the pool is the positive prefix: a zero score ends it, whatever follows
    got = probe_mmr(buf, K, np.array([0, 2, 3, 4], np.uint32), np.array([2.0, 1.0, 0.0, 0.0]), 4, 0.5)
    assert got[0].tolist() == [0, 2, PAD, PAD] and got[1].tolist() == [2.0, 1.0, 0.0, 0.0]


# ---------------------------------------------------------------------------------------------------------------------
# 5. independence: batches, selection, call order, the state
# ---------------------------------------------------------------------------------------------------------------------
def test_a_list_does_not_depend_on_batches_selection_or_order(monkeypatch):
    K, bias = 100, True
    D = handle(K, bias)
    names = ("THETA_E", "BETA_E", "UBIAS_E", "IBIAS_E")
    try:
        before = {w: D.get_state(w) for w in names}
        users = np.random.default_rng(8).permutation(N_USERS).astype(np.uint32)
        lists = [np.sort(np.random.default_rng(b).choice(N_ITEMS, b % 5, replace=False)) for b in range(N_USERS)]
        mptr, mitems = _mask_csr(lists)
        one = D.recommend_diverse(users, 20, pool=80, lam=0.3, mask_ptr=mptr, mask_items=mitems)
        for knob in (8, 10):                                                         # three batches
            monkeypatch.setenv("HPF_LOO_BATCH", str(knob))                           # read when the handle is created
            B = handle(K, bias)
            try:
                _eq(B.recommend_diverse(users, 20, pool=80, lam=0.3, mask_ptr=mptr, mask_items=mitems), one, f"HPF_LOO_BATCH={knob}")
            finally:
                B.close()
        monkeypatch.delenv("HPF_LOO_BATCH")
        # a subset, in another order, a user twice: the rows of the full selection
        pick = np.array([20, 3, 20, 23, 0, 17], np.int64)
        sptr, sitems = _mask_csr([lists[b] for b in pick])
        got = D.recommend_diverse(users[pick], 20, pool=80, lam=0.3, mask_ptr=sptr, mask_items=sitems)
        _eq(got, [o[pick] for o in one], "a subset, a user twice")
        _eq([g[0] for g in got], [g[2] for g in got], "a user selected twice gives two equal rows")
        # other scoring calls in between
        D.recommend(users, 256, mptr, mitems)
        D.similar(1, np.arange(5, dtype=np.uint32), 10)
        D.scores(users[:3])
        D.recommend_diverse(users[:4], 256, pool=256, lam=0.9)
        _eq(D.recommend_diverse(users, 20, pool=80, lam=0.3, mask_ptr=mptr, mask_items=mitems), one, "after other calls")
        for w in names:
            assert np.array_equal(_bits(D.get_state(w)), _bits(before[w])), f"{w} was written"
    finally:
        D.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. refusals: each on the host before a launch, with a message; the handle stays usable
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals():
    """(An odd row stride -- HPF_ERR_UNSUPPORTED, as for the other fused calls -- cannot be produced through hpf_create:
    every planned stride is a multiple of four.)"""
    K = 3
    theta, beta, _ = model(K)
    D = handle(K, True)
    n, m = N_USERS, N_ITEMS
    try:
        users = np.array([3, 7, 3, 23, 0], np.uint32)
        mptr, mitems = _mask_csr([[1], [], [1], [2, 3], []])
        want = D.recommend_diverse(users, 10, pool=40, lam=0.5, mask_ptr=mptr, mask_items=mitems)
        e = D.recommend_diverse(np.zeros(0, np.uint32), 10)
        assert all(a.shape == (0, 10) for a in e)
        assert D.lib.hpf_recommend_diverse(D._h, None, 0, None, None, 10, 40, 0.5, None, None, None, None) == 0      # n_sel = 0
        bad_users, bad_items, bad_ptr0, bad_ptr = users.copy(), mitems.copy(), mptr.copy(), mptr.copy()
        bad_users[1] = n
        bad_items[-1] = m
        bad_ptr0[0] = 1
        bad_ptr[2] = bad_ptr[1] - 1
        nan = float("nan")
        for (us, topn, pool, lam, mp, mi), msg in (
                ((users, 0, 40, 0.5, mptr, mitems), "topn is 1 .. 256"), ((users, 257, 257, 0.5, mptr, mitems), "topn is 1 .. 256"),
                ((users, 10, 9, 0.5, mptr, mitems), "pool is topn .. 256"), ((users, 10, 257, 0.5, mptr, mitems), "pool is topn .. 256"),
                ((users, 10, 0, 0.5, mptr, mitems), "pool is topn .. 256"),
                ((users, 10, 40, nan, mptr, mitems), "lambda is in [0, 1]"), ((users, 10, 40, -1e-9, mptr, mitems), "lambda is in [0, 1]"),
                ((users, 10, 40, 1.0000001, mptr, mitems), "lambda is in [0, 1]"), ((users, 10, 40, float("inf"), mptr, mitems), "lambda is in [0, 1]"),
                ((bad_users, 10, 40, 0.5, mptr, mitems), "user index out of range"),
                ((users, 10, 40, 0.5, mptr, bad_items), "mask item out of range"),
                ((users, 10, 40, 0.5, bad_ptr0, mitems), "mask_ptr[0]"), ((users, 10, 40, 0.5, bad_ptr, mitems), "mask_ptr not monotone")):
            _raises(INVALID, lambda: D.recommend_diverse(us, topn, pool=pool, lam=lam, mask_ptr=mp, mask_items=mi), msg)
            assert msg.encode() in D.lib.hpf_last_error(D._h)
        u32p, dp = C.POINTER(C.c_uint32), C.POINTER(C.c_double)
        oi, od = np.zeros(50, np.uint32), np.zeros(50)
        pu, pi, pd = users.ctypes.data_as(u32p), oi.ctypes.data_as(u32p), od.ctypes.data_as(dp)
        assert D.lib.hpf_recommend_diverse(D._h, None, 5, None, None, 10, 40, 0.5, pi, pd, None, None) == INVALID    # null pointers with work to do
        assert D.lib.hpf_recommend_diverse(D._h, pu, 5, None, None, 10, 40, 0.5, None, pd, None, None) == INVALID
        assert D.lib.hpf_recommend_diverse(D._h, pu, 5, None, None, 10, 40, 0.5, pi, None, None, None) == INVALID
        assert D.lib.hpf_recommend_diverse(D._h, pu, 5, None, None, 10, 40, 0.5, pi, pd, None, None) == 0            # maxsim and mmr may be NULL
        assert np.array_equal(oi.reshape(5, 10), D.recommend_diverse(users, 10, pool=40, lam=0.5)[0])
        _eq(D.recommend_diverse(users, 10, pool=40, lam=0.5, mask_ptr=mptr, mask_items=mitems), want, "after the refused calls")
    finally:
        D.close()
    sel = np.arange(3, dtype=np.uint32)
    # HPF_ERR_STATE: no E on either side
    for missing in ("THETA_E", "BETA_E"):
        F = Hpf(n, m, K, hier=False, bias=False)
        try:
            F.upload_csr(*_train(n, m)[:3])
            F.set_state("BETA_E" if missing == "THETA_E" else "THETA_E", beta if missing == "THETA_E" else theta)
            _raises(STATE, lambda: F.recommend_diverse(sel, 5))
            F.set_state(missing, theta if missing == "THETA_E" else beta)
            assert F.recommend_diverse(sel, 5)[0].shape == (3, 5)
        finally:
            F.close()
    # HPF_ERR_STATE: no CSR
    G = Hpf(n, m, K, hier=False, bias=False)
    try:
        G.set_state("THETA_E", theta)
        G.set_state("BETA_E", beta)
        _raises(STATE, lambda: G.recommend_diverse(sel, 5), "hpf_upload_csr")
    finally:
        G.close()
