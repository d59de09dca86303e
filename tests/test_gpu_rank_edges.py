"""-m gpu: the three kernels the whole ranking family stands on -- score_tile_kernel, topn_kernel, rank_query_kernel --
and the two fused ones (loo_rank_kernel, rank_queries_kernel) against an EXACT reference, at the places the scores of a
trained model never reach: keys that differ only in their last byte, rows that span 2000 binades, plateaus of exactly
equal nonzero scores across the 256-item chunks of the top-N tie loop, every top-N size class, rows of zeros.

No oracle, no trained model: a handle without -hier, a tiny CSR (1 to 3 training items per user, one of them stored
with rating 0, which is NOT zeroed) and THETA_E / BETA_E (/ UBIAS_E / IBIAS_E) set directly.  In families a to d every
entry is an integer or a power of two (times 1 + j 2^-52 with K = 1), so every score is exactly representable and does
not depend on the order of summation: the reference is Python integer / fractions.Fraction arithmetic, the expected
order is sorted(range(m), key=lambda i: (-score[i], i)) after zeroing, device scores must be BIT-equal and items and
ranks equal.  The exactness conditions are asserted on the CPU before the GPU is touched.

Family e (accuracy where float64 is no reference): entries 2^U(-150,150) U(1,2), exact dot products in integer
arithmetic, |dev - exact| <= (K + 3) 2^-53 (sum_k |theta_k beta_k| + |b_u| + |b_i|) -- the bound of ANY summation
order of K products and two additions, derived and therefore fixed.

MEASURED on an MI355X (gfx950), largest error / bound over the 32 x 70 pairs (the bound is never approached: the terms of
a row span 600 binades, so a handful of them carry the sum):
    K     bias    hpf_scores  hpf_predict
    7     no      0.1935      0.1990
    7     yes     0.2084      0.2334
    100   no      0.0346      0.0266
    100   yes     0.0346      0.0266
    260   no      0.0134      0.0110
    260   yes     0.0134      0.0110

OBSERVED for scores below 2^-1022 (family b, the user with theta = 2^-60; nothing is asserted about their values): the
fp64 MFMA chain KEEPS subnormals.  Of 257 exact products 5 lie below 2^-1022; hpf_scores returned all 5 exactly and
none as 0.0, and the scores of item_ranks, loo_ranks, rank_queries and rank_topn carried the same bits.
"""
from collections import Counter
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
TWO53 = 2 ** 53



def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _exact_float(x):
    """float(x) for an exact number that must be representable: the generator is broken otherwise"""
    f = float(x)
    assert Fraction(f) == Fraction(x), f"{x} is not a double"
    return f


# ---------------------------------------------------------------------------------------------------------------------
# training matrix, masks, the exact reference
# ---------------------------------------------------------------------------------------------------------------------
def _train(n, m):
    """1 to 3 distinct training items per user.  A user with two or three has the first stored with rating 0; a user
    with one has rating 0 (even user) or 2 (odd user).  -> rowptr, col, val, zeroed[u] = the items with rating > 0"""
    rowptr, col, val, zeroed = [0], [], [], []
    for u in range(n):
        cnt = min(1 + u % 3, m)
        start, step = (37 * u + 11) % m, max(1, m // 3)
        items = [(start + j * step) % m for j in range(cnt)]
        assert len(set(items)) == cnt
        vals = [0 if u % 2 == 0 else 2] if cnt == 1 else [0] + [1 + (u + j) % 5 for j in range(1, cnt)]
        col += items
        val += vals
        rowptr.append(len(col))
        zeroed.append({i for i, v in zip(items, vals) if v > 0})
    return np.array(rowptr, np.int64), np.array(col, np.uint32), np.array(val, np.uint8), zeroed


class State:
    """a handle with E set directly, and the exact score of every (user, item): exact[u][i], an int or a Fraction"""

    def __init__(self, theta, beta, exact, ub=None, ib=None, loose_users=()):
        from hgaprec_amd.capi import Hpf
        theta, beta = np.asarray(theta, np.float64), np.asarray(beta, np.float64)
        self.n, self.K = theta.shape
        self.m = beta.shape[0]
        self.bias = ub is not None
        self.exact = exact
        self.loose = set(loose_users)                    # users whose scores leave the normal range: not in the reference
        assert len(exact) == self.n and all(len(r) == self.m for r in exact)
        # every score is a double, and a normal one (or zero): checked before the GPU is touched
        self.f64 = np.empty((self.n, self.m))
        for u in range(self.n):
            self.f64[u] = [_exact_float(x) for x in exact[u]]
            if u not in self.loose:
                nz = self.f64[u][self.f64[u] != 0.0]
                assert np.all(nz >= 2.0 ** -1022) and np.all(nz < 2.0 ** 1023), "a score outside the normal range"
        self.rowptr, self.col, self.val, self.zeroed = _train(self.n, self.m)
        assert np.any(self.val == 0) and (self.m == 1 or np.any(self.val > 0))
        self.D = Hpf(self.n, self.m, self.K, hier=False, bias=self.bias)
        self.D.upload_csr(self.rowptr, self.col, self.val)
        self.D.set_state("THETA_E", theta)
        self.D.set_state("BETA_E", beta)
        if self.bias:
            self.D.set_state("UBIAS_E", np.asarray(ub, np.float64))
            self.D.set_state("IBIAS_E", np.asarray(ib, np.float64))

    def close(self):
        self.D.close()


class Selection:
    """selected users with one mask list each, and what the reference expects of them"""

    def __init__(self, S, users, masks):
        self.S, self.users, self.masks = S, np.asarray(users, np.uint32), [list(x) for x in masks]
        assert len(self.masks) == len(users)
        self.mptr = np.zeros(len(users) + 1, np.uint64)
        self.mptr[1:] = np.cumsum([len(x) for x in self.masks])
        self.mitems = np.array([i for x in self.masks for i in x], np.uint32)
        self._cache = {}

    def sub(self, sel):
        return Selection(self.S, self.users[sel], [self.masks[b] for b in sel])

    def gone(self, b):
        return self.S.zeroed[int(self.users[b])] | set(self.masks[b])

    def expect(self, b):
        """-> vals (exact, zeroed), f64 (the same as doubles), order, pos"""
        key = (int(self.users[b]), tuple(self.masks[b]))
        if key not in self._cache:
            u, m = key[0], self.S.m
            vals = list(self.S.exact[u])
            f64 = self.S.f64[u].copy()
            for i in self.gone(b):
                vals[i] = 0
                f64[i] = 0.0
            order = sorted(range(m), key=lambda i: (-vals[i], i))
            pos = np.empty(m, np.int64)
            pos[order] = np.arange(m)
            self._cache[key] = (vals, f64, np.array(order, np.int64), pos)
        return self._cache[key]


def _masks_small(S, users):
    """no mask for most users (user 0 among them), a few items with a duplicate and a training item for every fourth"""
    out = []
    for u in users:
        if u % 4 == 3:
            z = sorted(S.zeroed[u])
            out.append([i % S.m for i in (5, 5, 120, 256, 300, 555)] + z[:1])
        else:
            out.append([])
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the four routes against the reference
# ---------------------------------------------------------------------------------------------------------------------
def check_topn(sel, N):
    """rank_topn and recommend (the same selection over a row of scores and over the sweep's lists), each against the reference"""
    S = sel.S
    Ne = min(N, S.m)
    for route in (S.D.rank_topn, S.D.recommend):
        name = route.__name__
        items, sc = route(sel.users, N, sel.mptr, sel.mitems)
        assert items.shape == sc.shape == (len(sel.users), N)
        for b, u in enumerate(sel.users):
            if int(u) in S.loose:
                continue
            _, f64, order, _ = sel.expect(b)
            assert np.array_equal(items[b, :Ne], order[:Ne].astype(np.uint32)), f"{name}: top-{N} items of user {u} (m = {S.m})"
            assert np.array_equal(_bits(sc[b, :Ne]), _bits(f64[order[:Ne]])), f"{name}: top-{N} scores of user {u}"
            assert np.all(items[b, Ne:] == NONE) and np.all(_bits(sc[b, Ne:]) == 0), f"{name}: entries beyond m of user {u}"


def check_item_ranks(sel, three):
    S, m = sel.S, sel.S.m
    qs = np.repeat(np.array(three, np.uint32), m)
    qi = np.tile(np.arange(m, dtype=np.uint32), len(three))
    rank, sc = S.D.item_ranks(sel.users, qs, qi, sel.mptr, sel.mitems)
    for b in three:
        _, f64, _, pos = sel.expect(b)
        assert np.array_equal(rank[qs == b], pos.astype(np.uint32)), f"item_ranks of user {sel.users[b]}"
        assert np.array_equal(_bits(sc[qs == b]), _bits(f64)), f"item_ranks scores of user {sel.users[b]}"


def check_loo(sel, limits):
    """one call per block of 256 items: every item is the query once, for users taken in turn"""
    S, m = sel.S, sel.S.m
    strict = [b for b, u in enumerate(sel.users) if int(u) not in S.loose]
    idx = np.arange(m)
    for limit in [0] + [x for x in limits if 1 <= x <= m]:
        L = limit if limit else m
        for c0 in range(0, m, 256):
            q = np.arange(c0, min(m, c0 + 256))
            pick = [strict[(int(t) + c0 // 256 + limit) % len(strict)] for t in q]
            part = sel.sub(pick)
            rank, sc, masked = S.D.loo_ranks(part.users, q.astype(np.uint32), part.mptr, part.mitems, item_limit=limit)
            for j, (t, b) in enumerate(zip(q, pick)):
                _, f64, _, pos = sel.expect(b)
                if t >= L:
                    want_r, want_s = 0, 0.0
                elif L == m:
                    want_r, want_s = pos[t], f64[t]
                else:
                    v = f64[:L]                         # exact doubles: comparing them is comparing the exact scores
                    want_r, want_s = int(np.sum((v > v[t]) | ((v == v[t]) & (idx[:L] < t)))), f64[t]
                what = f"loo_ranks user {sel.users[b]} item {t} limit {limit}"
                assert rank[j] == want_r, what
                assert _bits(sc[j])[()] == _bits(want_s)[()], what
                assert masked[j] == sum(1 for i in sel.gone(b) if i < L), what + ": distinct masked items"


def _query_list(m, seed):
    """all m items in a fixed permuted order, some of them asked twice"""
    rng = np.random.default_rng(seed)
    q = list(rng.permutation(m))
    for t in rng.integers(0, m, max(2, m // 16)):
        q.insert(int(rng.integers(0, len(q) + 1)), int(t))
    return q


def check_rank_queries(sel, b_all, b_none, b_zero):
    """selected user b_all asks for every item in permuted order with repeats, b_none for nothing, b_zero (the all-zero
    user) for every item in index order and once more in reverse"""
    S, m = sel.S, sel.S.m
    part = sel.sub([b_all, b_none, b_zero])
    qa = _query_list(m, 3)
    qz = list(range(m)) + list(range(m - 1, -1, -1))
    q_ptr = np.array([0, len(qa), len(qa), len(qa) + len(qz)], np.uint64)
    q_items = np.array(qa + qz, np.uint32)
    rank, sc = S.D.rank_queries(part.users, q_ptr, q_items, part.mptr, part.mitems)
    for b, lo, hi in ((0, 0, len(qa)), (2, len(qa), len(qa) + len(qz))):
        _, f64, _, pos = part.expect(b)
        assert np.array_equal(rank[lo:hi], pos[q_items[lo:hi]].astype(np.uint32)), f"rank_queries of user {part.users[b]}"
        assert np.array_equal(_bits(sc[lo:hi]), _bits(f64[q_items[lo:hi]])), f"rank_queries scores of user {part.users[b]}"
    return len(qa)


def check_all_routes(S, masks, topns, three, rq, limits):
    sel = Selection(S, np.arange(S.n), masks)
    dev = S.D.scores(sel.users)
    for u in range(S.n):
        if u not in S.loose:
            assert np.array_equal(_bits(dev[u]), _bits(S.f64[u])), f"hpf_scores of user {u} differs from the exact scores"
    for N in topns:
        check_topn(sel, N)
    check_item_ranks(sel, three)
    check_loo(sel, limits)
    return check_rank_queries(sel, *rq)


# ---------------------------------------------------------------------------------------------------------------------
# a. low byte: K = 1, beta_i = 1 + pi(i) 2^-52
# ---------------------------------------------------------------------------------------------------------------------
def _k1_state(theta, beta, loose_users=()):
    """K = 1: theta and beta are lists of Fractions, every product must be a double"""
    exact = [[t * x for x in beta] for t in theta]
    return State([[_exact_float(t)] for t in theta], [[_exact_float(x)] for x in beta], exact, loose_users=loose_users)


@pytest.mark.parametrize("m", [256, 600])
def test_low_byte_keys(m):
    """all keys of a row agree in their top seven (m = 256) or six (m = 600) bytes: only the last radix passes have a
    histogram with more than one bin, and the walk ends at digit 0 under a nonzero prefix when the worst item is asked
    for.  User 1 carries the same mantissas under the exponent of 2^-600, user 2 is all zero."""
    pi = [(77 * i + 13) % m for i in range(m)]
    assert sorted(pi) == list(range(m))
    beta = [1 + Fraction(p, 2 ** 52) for p in pi]
    S = _k1_state([Fraction(1), Fraction(1, 2 ** 600), Fraction(0)], beta)
    try:
        assert not S.zeroed[0]                           # user 0: one training item, stored with rating 0 -> a pure row
        for u in (0, 1):
            keys = _bits(S.f64[u])
            low = 8 if m == 256 else 16
            assert np.unique(keys >> np.uint64(low)).size == 1, "the keys differ above the low byte(s)"
            assert np.unique(keys).size == m and np.unique(keys >> np.uint64(low - 8)).size > 1
            if m == 256:
                assert sorted((keys & np.uint64(255)).tolist()) == list(range(256))     # pass 8 alone separates them
            else:
                assert np.unique(keys >> np.uint64(8)).size == 3                        # pass 7 sees three bins
        masks = [[], [5, 5, m - 1], []]
        topns = [1, 2, 100, 255, 256, 257] if m == 256 else [1, 3, 100, 256, 257, 599, 600, 1024]
        nq = check_all_routes(S, masks, topns, [0, 1, 2], (0, 1, 2), [1, 64, 257, m - 1])
        assert nq > m and (m != 600 or -(-nq // 32) >= 19)                              # 19 rows of RANK_QUERIES_QCAP at m = 600
    finally:
        S.close()


# ---------------------------------------------------------------------------------------------------------------------
# b. exponent ladder: K = 1, beta_i = 2^e_i over [-1000, 1000]
# ---------------------------------------------------------------------------------------------------------------------
def _ladder(m):
    rungs = [-1000 + (2000 * j) // (m - 1) for j in range(m)]
    assert len(set(rungs)) == m and rungs[0] == -1000 and rungs[-1] == 1000
    e = [rungs[(389 * i + 7) % m] for i in range(m)]
    assert sorted(e) == rungs
    beta = [Fraction(2) ** x for x in e]
    theta = [Fraction(1), Fraction(1, 2 ** 20), Fraction(2 ** 20), Fraction(0), Fraction(1, 2 ** 60)]
    return _k1_state(theta, beta, loose_users=(4,)), e


@pytest.mark.parametrize("m", [257, 1025])
def test_exponent_ladder(m):
    """one item per rung of a ladder of 2000 binades: the FIRST radix passes decide, every bin of pass 1 and 2 is in
    use, and all products are normal and exact"""
    S, e = _ladder(m)
    try:
        assert max(e) - min(e) > 1900
        for u in (0, 1, 2):
            assert np.log2(S.f64[u].max()) - np.log2(S.f64[u].min()) > 1900             # the ladder spans > 1900 binades
            assert np.unique(_bits(S.f64[u]) >> np.uint64(56)).size > 100                # pass 1 has > 100 bins in use
        masks = [[], [3, 3, m - 1, 100], [0], [], []]
        topns = [1, 10, 256, 257, 1024]
        check_all_routes(S, masks, topns, [0, 2, 3], (1, 3, 3), [1, 64, 257, m - 1])
    finally:
        S.close()


def test_ladder_below_the_normal_range_orders_by_its_own_scores(capsys):
    """theta = 2^-60 puts the low rungs below 2^-1022.  Whether the MFMA chain keeps fp64 subnormals has not been
    specified anywhere, so nothing is asserted about their VALUES: each route must order by the scores it returns
    itself.  What is seen is printed (and recorded in this file's docstring)."""
    m = 257
    S, e = _ladder(m)
    try:
        u = 4
        exact = S.f64[u]                                 # float(Fraction) of 2^(e - 60): exact, subnormal below 2^-1022
        users = np.array([u], np.uint32)
        mptr, mitems = np.array([0, 2], np.uint64), np.array([9, 200], np.uint32)
        nsub = int(np.sum((exact > 0) & (exact < 2.0 ** -1022)))
        assert nsub >= 5
        idx = np.arange(m)

        def own_order(sc):
            return np.lexsort((idx, -sc))                # score descending, item ascending

        dev = S.D.scores(users)[0]
        rank, sc = S.D.item_ranks(users, np.zeros(m, np.uint32), idx.astype(np.uint32), mptr, mitems)
        pos = np.empty(m, np.int64)
        pos[own_order(sc)] = idx
        assert np.array_equal(rank, pos), "item_ranks does not order by its own scores"
        lr, lsc, _ = S.D.loo_ranks(np.full(m, u, np.uint32), idx.astype(np.uint32),
                                   np.arange(m + 1, dtype=np.uint64) * 2, np.tile(mitems, m))
        pos[own_order(lsc)] = idx
        assert np.array_equal(lr, pos), "loo_ranks does not order by its own scores"
        qr, qsc = S.D.rank_queries(users, np.array([0, m], np.uint64), idx.astype(np.uint32), mptr, mitems)
        pos[own_order(qsc)] = idx
        assert np.array_equal(qr, pos), "rank_queries does not order by its own scores"
        items, tsc = S.D.rank_topn(users, 1024, mptr, mitems)
        assert sorted(items[0, :m].tolist()) == list(range(m)) and np.all(items[0, m:] == NONE)
        keys = list(zip((-tsc[0, :m]).tolist(), items[0, :m].tolist()))
        assert keys == sorted(keys), "rank_topn does not order by its own scores"
        sub = (exact > 0) & (exact < 2.0 ** -1022)
        gone = sorted(S.zeroed[u] | set(mitems.tolist()))
        with capsys.disabled():
            print(f"\n[subnormal scores, K = 1, theta = 2^-60] {nsub} of {m} exact products lie below 2^-1022; "
                  f"hpf_scores returns {int(np.sum(dev[sub] == exact[sub]))} of them exactly and {int(np.sum(dev[sub] == 0.0))} as 0.0; "
                  f"item_ranks' scores equal hpf_scores': {np.array_equal(_bits(np.where(np.isin(idx, gone), 0.0, dev)), _bits(sc))}, "
                  f"loo_ranks': {np.array_equal(_bits(lsc), _bits(sc))}, rank_queries': {np.array_equal(_bits(qsc), _bits(sc))}, "
                  f"rank_topn's: {np.array_equal(_bits(tsc[0, :m]), _bits(sc[items[0, :m]]))}")
    finally:
        S.close()


# ---------------------------------------------------------------------------------------------------------------------
# c, d. plateaus: five distinct rows of beta dealt to the items
# ---------------------------------------------------------------------------------------------------------------------
GROUP_SIZES = (1, 254, 257, 40, 48)


def _groups600():
    """group of each of 600 items.  Group 2 (257 items) is 100..299 and 500..556: 156 items in the first 256-item chunk
    of the top-N tie loop, 44 + 12 in the second, 45 in the third; group 0 is item 300; groups 1, 3 and 4 are dealt in
    turn to the rest"""
    g = [-1] * 600
    for i in list(range(100, 300)) + list(range(500, 557)):
        g[i] = 2
    g[300] = 0
    left = {1: GROUP_SIZES[1], 3: GROUP_SIZES[3], 4: GROUP_SIZES[4]}
    turn = [1, 3, 1, 4, 1, 1, 3, 4]
    j = 0
    for i in range(600):
        if g[i] >= 0:
            continue
        while left[turn[j % len(turn)]] == 0:
            j += 1
        g[i] = turn[j % len(turn)]
        left[g[i]] -= 1
        j += 1
    assert tuple(Counter(g)[k] for k in range(5)) == GROUP_SIZES
    chunks = Counter(i // 256 for i in range(600) if g[i] == 2)
    assert chunks[0] >= 2 and chunks[1] >= 2 and chunks[2] >= 2                # the 257-plateau crosses 256 and 512
    return g


def _plateau_state(m, K, bias, n):
    """integers only: beta rows in [0, 1024], theta rows in [0, 8] (user 1 = user 0, user 2 all zero), biases per user
    and per GROUP (so that a plateau stays one; groups 2 and 3 share theirs)"""
    rng = np.random.default_rng(1000 * K + m)
    g600 = _groups600()
    grp = [g600[i % 600] if (g600[i % 600] != 0 or i == 300) else 1 for i in range(m)]
    rows = rng.integers(0, 1025, (5, K))
    rows[rng.random((5, K)) < 0.1] = 0
    assert len({tuple(r) for r in rows.tolist()}) == 5
    beta = rows[grp]
    theta = rng.integers(0, 9, (n, K))
    if n > 1:
        theta[1] = theta[0]
    if n > 2:
        theta[2] = 0
    ub = rng.integers(0, 50, n) if bias else None
    if bias and n > 1:
        ub[1] = ub[0]
    ib = np.array([3, 0, 7, 7, 1])[grp] if bias else None
    s = theta @ beta.T                                                        # int64, exact
    if bias:
        s = s + ub[:, None] + ib[None, :]
    # exactness: integers, and every partial sum of a row in any order stays below 2^53
    assert theta.dtype.kind == "i" and beta.dtype.kind == "i" and theta.min() >= 0 and beta.min() >= 0
    assert int((theta.astype(object) @ beta.T.astype(object)).max()) + 100 < TWO53
    assert np.array_equal(theta.astype(np.float64).astype(np.int64), theta) and np.array_equal(beta.astype(np.float64).astype(np.int64), beta)
    return State(theta, beta, s.tolist(), ub, ib), grp


def _tie_case(vals, order, N):
    """what a top-N of this row asks of the tie loop -> (labels, size of the threshold's plateau)"""
    T = vals[order[N - 1]]
    ties = [i for i in range(len(vals)) if vals[i] == T]
    need = N - sum(1 for v in vals if v > T)
    assert 1 <= need <= len(ties)
    last, labels = ties[need - 1], set()
    if T == 0:
        return labels, len(ties)
    if need == 1:
        labels.add("first item")
    if need == len(ties):
        labels.add("whole plateau")
    elif ties[need] // 256 != last // 256:
        labels.add("ends on a chunk's last tied item")
    else:
        labels.add({0: "inside the first chunk", 1: "into a second chunk", 2: "into a third chunk"}[last // 256 - ties[0] // 256])
    return labels, len(ties)


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("K", [3, 33, 129])
def test_plateaus(K, bias):
    """m = 600 in plateaus of 1, 254, 257, 40 and 48 exactly tied nonzero scores; the top-N sizes are computed from the
    exact reference so that the boundary falls on every kind of place inside the 257-plateau"""
    m, n = 600, 12
    S, grp = _plateau_state(m, K, bias, n)
    try:
        masks = _masks_small(S, range(n))
        sel = Selection(S, np.arange(n), masks)
        assert S.exact[0] == S.exact[1] and (bias or set(S.exact[2]) == {0})
        topns, hit = {1, 100, 600, 601, 1024}, Counter()
        for b in range(n):
            vals, _, order, _ = sel.expect(b)
            score, size = max(((s, c) for s, c in Counter(vals).items() if s != 0), key=lambda t: t[1], default=(0, 0))
            if size != 257:
                continue                                                        # a training or masked item inside it
            ties = [i for i in range(m) if vals[i] == score]
            above = sum(1 for v in vals if v > score)
            c = Counter(i // 256 for i in ties)
            for need in (1, c[0] + c[1] // 2, c[0] + c[1] + c[2] // 2, c[0], c[0] + c[1], 257):
                N = above + need
                labels, sz = _tie_case(vals, order, N)
                assert sz == 257
                for x in labels:
                    hit[x] += 1
                topns.add(N)
        want = {"first item", "into a second chunk", "into a third chunk", "ends on a chunk's last tied item", "whole plateau"}
        assert want <= set(hit) and hit["ends on a chunk's last tied item"] >= 2, f"boundary cases reached: {dict(hit)}"
        for N in sorted(topns):
            check_topn(sel, N)
        check_item_ranks(sel, [0, 2, 7])
        check_loo(sel, [1, 64, 257, m - 1])
        nq = check_rank_queries(sel, 3, 1, 2)
        assert -(-nq // 32) >= 19
        dev = S.D.scores(sel.users)
        assert np.array_equal(_bits(dev), _bits(S.f64))
    finally:
        S.close()


SIZES = [(1, 3, False), (2, 33, True), (63, 129, False), (64, 3, True), (65, 33, False), (255, 129, True), (256, 3, False),
         (257, 33, True), (1025, 129, True)]
TOPNS = [1, 2, 3, 10, 100, 255, 256, 257, 1023, 1024]


@pytest.mark.parametrize("m,K,bias", SIZES)
def test_zeros_and_sizes(m, K, bias):
    """every size class of N and of m around the wave, the chunk and the 1024 candidates, with masks that zero a prefix,
    a suffix or everything: N = m, m - 1, m + 1, and N beyond the count of nonzero scores, where the threshold is key 0"""
    n = 40 if m == 1025 else 8
    S, grp = _plateau_state(m, K, bias, n)
    try:
        masks = []
        for u in range(n):
            kind = u % 4
            masks.append([] if kind == 0 else list(range((m + 2) // 3)) if kind == 1 else
                         list(range(m - (m + 1) // 2, m)) if kind == 2 else list(range(m)))
        sel = Selection(S, np.arange(n), masks)
        beyond = sum(1 for b in range(n) for N in TOPNS if N <= m and sel.expect(b)[0][sel.expect(b)[2][N - 1]] == 0)
        assert beyond > 0 or m < 3                                              # the threshold is key 0 somewhere
        for N in TOPNS:
            check_topn(sel, N)
        check_item_ranks(sel, [0, min(2, n - 1), min(3, n - 1)])
        check_loo(sel, [1, 64, 257, m - 1])
        check_rank_queries(sel, 0, 1, 2)
        from hgaprec_amd.capi import HpfError
        for bad in (0, 1025):
            with pytest.raises(HpfError):
                S.D.rank_topn(sel.users, bad, sel.mptr, sel.mitems)
    finally:
        S.close()


# ---------------------------------------------------------------------------------------------------------------------
# e. accuracy where float64 is no reference
# ---------------------------------------------------------------------------------------------------------------------
_SHIFT = 1000                                              # every product of two entries is a multiple of 2^-_SHIFT
_wide_cache = {}


def _split(a):
    """doubles -> (integer mantissas, exponents): a == mant * 2^exp exactly"""
    mant, ex = np.frexp(np.asarray(a, np.float64))
    return (mant * 2.0 ** 53).astype(np.int64).tolist(), (ex - 53).tolist()


def _wide_state(K):
    """32 x K and 70 x K entries 2^U(-150,150) U(1,2) with a share of exact zeros, biases alike, and the exact dot
    product of every pair as an integer multiple of 2^-1000 (computed once per K)"""
    if K not in _wide_cache:
        n, m = 32, 70
        rng = np.random.default_rng(K)

        def draw(shape):
            a = 2.0 ** rng.uniform(-150, 150, shape) * rng.uniform(1, 2, shape)
            a[rng.random(shape) < 0.15] = 0.0
            return a
        theta, beta, ub, ib = draw((n, K)), draw((m, K)), draw(n), draw(m)
        tm, te = _split(theta)
        bm, be = _split(beta)
        dots = [[sum((tm[u][k] * bm[i][k]) << (te[u][k] + be[i][k] + _SHIFT) for k in range(K) if tm[u][k] and bm[i][k])
                 for i in range(m)] for u in range(n)]
        assert Fraction(dots[3][5], 2 ** _SHIFT) == sum(Fraction(theta[3, k]) * Fraction(beta[5, k]) for k in range(K))
        _wide_cache[K] = (theta, beta, ub, ib, dots)
    return _wide_cache[K]


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("K", [7, 100, 260])
def test_accuracy_against_exact_dot_products(K, bias, capsys):
    """hpf_scores (the MFMA chain) and hpf_predict (fma per lane, then a tree) against exact arithmetic where the terms
    of a row span 600 binades: |dev - exact| <= (K + 3) 2^-53 (sum |theta_k beta_k| + |b_u| + |b_i|).  All terms are
    positive, so the sum of absolute values is the exact score itself.  The thresholds the three rank routes return
    are hpf_scores' entries, bit for bit.

    Largest error / bound measured on an MI355X (the table at the top of this file): 0.21 for hpf_scores, 0.23 for
    hpf_predict, both at K = 7 with bias."""
    from hgaprec_amd.capi import Hpf
    theta, beta, ub, ib, dots = _wide_state(K)
    n, m = theta.shape[0], beta.shape[0]
    rowptr, col, val, zeroed = _train(n, m)
    D = Hpf(n, m, K, hier=False, bias=bias)
    try:
        D.upload_csr(rowptr, col, val)
        D.set_state("THETA_E", theta)
        D.set_state("BETA_E", beta)
        if bias:
            D.set_state("UBIAS_E", ub)
            D.set_state("IBIAS_E", ib)
        users = np.arange(n, dtype=np.uint32)
        dev = D.scores(users)
        pu, pi = np.repeat(users, m), np.tile(np.arange(m, dtype=np.uint32), n)
        pred = D.predict(pu, pi).reshape(n, m)
        worst = {"scores": Fraction(0), "predict": Fraction(0)}
        one = 2 ** _SHIFT
        for u in range(n):
            for i in range(m):
                exact = Fraction(dots[u][i], one)
                if bias:
                    exact += Fraction(ub[u]) + Fraction(ib[i])
                bound = (K + 3) * exact / TWO53
                for name, got in (("scores", dev[u, i]), ("predict", pred[u, i])):
                    err = abs(Fraction(float(got)) - exact)
                    if bound == 0:
                        assert err == 0, f"{name}[{u}, {i}] = {got} where every term is zero"
                    else:
                        worst[name] = max(worst[name], err / bound)
        with capsys.disabled():
            print(f"\n[accuracy K = {K} bias = {bias}] largest error / bound: hpf_scores {float(worst['scores']):.4f}, "
                  f"hpf_predict {float(worst['predict']):.4f}")
        assert worst["scores"] <= 1, f"hpf_scores exceeds the bound of any summation order: {float(worst['scores'])}"
        assert worst["predict"] <= 1, f"hpf_predict exceeds the bound of any summation order: {float(worst['predict'])}"

        # the thresholds of the rank routes are these scores
        masks = [[] if u % 3 else [1, 1, 40, 69] for u in range(n)]
        mptr = np.zeros(n + 1, np.uint64)
        mptr[1:] = np.cumsum([len(x) for x in masks])
        mitems = np.array([i for x in masks for i in x], np.uint32)
        zd = dev.copy()
        for u in range(n):
            zd[u, sorted(zeroed[u] | set(masks[u]))] = 0.0
        three = [0, 7, 31]
        qs, qi = np.repeat(np.array(three, np.uint32), m), np.tile(np.arange(m, dtype=np.uint32), 3)
        rank, sc = D.item_ranks(users, qs, qi, mptr, mitems)
        pos = np.empty(m, np.int64)
        for b in three:
            assert np.array_equal(_bits(sc[qs == b]), _bits(zd[b])), "item_ranks' scores are not hpf_scores'"
            pos[np.argsort(-zd[b], kind="stable")] = np.arange(m)
            assert np.array_equal(rank[qs == b], pos)
        for c0 in range(0, m, n):                                               # every item the query once
            q = np.arange(c0, min(m, c0 + n), dtype=np.uint32)
            lr, lsc, _ = D.loo_ranks(users[:q.size], q, mptr[:q.size + 1], mitems[:int(mptr[q.size])])
            assert np.array_equal(_bits(lsc), _bits(zd[np.arange(q.size), q])), "loo_ranks' scores are not hpf_scores'"
        q_ptr = np.arange(n + 1, dtype=np.uint64) * m
        qr, qsc = D.rank_queries(users, q_ptr, np.tile(np.arange(m, dtype=np.uint32), n), mptr, mitems)
        assert np.array_equal(_bits(qsc), _bits(zd.reshape(-1))), "rank_queries' scores are not hpf_scores'"
    finally:
        D.close()
