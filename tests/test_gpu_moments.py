"""-m gpu: hpf_score_moments and hpf_recommend_ucb -- the posterior mean and variance of a score and the top-N by
mean + z sd (moment_rows_kernel, ucb_sweep_kernel, pair_moments_kernel, topn_merge_kernel).

The oracle is the definition of include/hpf.h.  mean(u, i) is hpf_scores of the handle.  var(u, i) is hpf_scores of a SECOND
handle with K' = C = 2 K + 2 * bias, no bias, E[theta] = X and E[beta] = Y, the derived rows formed by numpy with the five
operations of the definition (tests/moments_ref.py).  ucb, the masking and the sort are numpy's.  Every comparison of a
returned double is on its bits; the accuracy of var against rational arithmetic is the derived (C + 9) 2^-53."""
import ctypes as C

import numpy as np
import pytest

from hgaprec_amd import capi
from hgaprec_amd.capi import Hpf, HpfError
from tests import moments_ref as ref
from tests.moments_ref import NONE, bits
from tests.util import compare_states, init_states, make_problem

pytestmark = pytest.mark.gpu
INVALID, UNSUPPORTED, STATE = -1, -5, -6


def _raises(code, f, msg=None):
    with pytest.raises(HpfError) as e:
        f()
    assert f"({code})" in str(e.value) and (msg is None or msg in str(e.value)), str(e.value)


def _eq(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    if got.dtype == np.float64:
        bad = np.flatnonzero(bits(got).ravel() != bits(want).ravel())
        assert bad.size == 0, f"{what}: {bad.size} differ, first at {bad[:3]}: {got.ravel()[bad[:3]]} vs {want.ravel()[bad[:3]]}"
    else:
        assert np.array_equal(got, want), what


def _handle(n, m, K, bias, csr, st):
    rowptr, col, val = csr
    D = Hpf(n, m, K, hier=False, bias=bias, binary=val is None)
    D.upload_csr(rowptr, col, val)
    for w, a in st.items():
        D.set_state(w, a)
    return D


def _all(n):
    return np.arange(n, dtype=np.uint32)


def _var_matrix(st, bias, csr):
    """hpf_scores of the handle with K' = C, E[theta] = X, E[beta] = Y: var of every pair, by definition"""
    X, Y = ref.derived_rows(st, bias)
    H = _handle(X.shape[0], Y.shape[0], X.shape[1], False, csr, {"THETA_E": X, "BETA_E": Y})
    try:
        assert H.work_info()["ld"] % 2 == 0
        return H.scores(_all(X.shape[0]))
    finally:
        H.close()


def _exports(D, bias):
    names = ["THETA_E", "THETA_SHAPE", "BETA_E", "BETA_SHAPE"] + (["UBIAS_E", "UBIAS_SHAPE", "IBIAS_E", "IBIAS_SHAPE"] if bias else [])
    return {w: D.get_state(w) for w in names}


def _masked(csr, u, lst):
    rowptr, col, val = csr
    seg = slice(rowptr[u], rowptr[u + 1])
    own = col[seg] if val is None else col[seg][val[seg] > 0]
    return np.union1d(own, np.asarray(lst, np.uint32)).astype(np.int64)


def _mask_csr(lists):
    mptr = np.zeros(len(lists) + 1, np.uint64)
    mptr[1:] = np.cumsum([len(x) for x in lists])
    return mptr, np.concatenate([np.asarray(x, np.uint32) for x in lists] + [np.zeros(0, np.uint32)]).astype(np.uint32)


def _want_lists(S, V, csr, users, lists, topn, z):
    """S, V: mean and variance of every (user, item) -> (items, ucb, mean, var) as hpf_recommend_ucb returns them"""
    full = ref.ucb(S, V, z)
    key = full[users.astype(np.int64)].copy()
    for b, u in enumerate(users):
        key[b, _masked(csr, u, lists[b] if lists is not None else [])] = 0.0
    items = ref.top_lists(key, topn)
    return items, ref.take(full, users, items), ref.take(S, users, items), ref.take(V, users, items)


def _same_lists(got, want, what):
    for g, w, name in zip(got, want, ("items", "ucb", "mean", "var")):
        _eq(g, w, f"{what}: {name}")


# ---------------------------------------------------------------------------------------------------------------------
# 1. pair moments
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("K", ref.PAIR_KS)
def test_pair_moments(K, bias):
    """K = 5: both chains end inside an MFMA step; 16: the mean chain ends exactly on one; 511 with bias: C = 1024, the limit"""
    n, m = ref.PAIR_N, ref.PAIR_M
    st, u, i = ref.pair_case(K, bias)
    csr = make_problem(n, m, 300, seed=K)
    Cc = capi.moments_plan(K, bias)["C"]
    D = _handle(n, m, K, bias, csr, st)
    try:
        assert D.work_info()["ld"] % 2 == 0
        S = D.scores(_all(n))
        V = _var_matrix(st, bias, csr)
        mean, var = D.score_moments(u, i)
        _eq(mean, S[u, i], "mean against hpf_scores")
        _eq(var, V[u, i], "var against hpf_scores of the X / Y handle")
        for p in range(17):
            exact = ref.exact_var(st, bias, u[p], i[p])
            rel = abs(ref.Fraction(float(var[p])) - exact) / exact
            print(f"K={K} bias={bias} pair {p}: |var - exact| / exact = {float(rel) / ref.U:.2f} u (bound {Cc + 9} u)")
            assert ref.within(var[p], exact, Cc), (K, bias, p)
        # pairs given twice give equal rows
        _eq(mean[40:], mean[3:12], "repeated pairs: mean")
        _eq(var[40:], var[3:12], "repeated pairs: var")
        # the edge of the 16-pair wave; either output may be left out
        for cnt in (1, 15, 16, 17):
            mc, vc = D.score_moments(u[:cnt], i[:cnt])
            _eq(mc, mean[:cnt], f"cnt={cnt}: mean")
            _eq(vc, var[:cnt], f"cnt={cnt}: var")
        u32p, dp = C.POINTER(C.c_uint32), C.POINTER(C.c_double)
        only = np.full(17, -1.0)
        assert D.lib.hpf_score_moments(D._h, u.ctypes.data_as(u32p), i.ctypes.data_as(u32p), 17, None, only.ctypes.data_as(dp)) == 0
        _eq(only, var[:17], "var alone")
        assert D.lib.hpf_score_moments(D._h, u.ctypes.data_as(u32p), i.ctypes.data_as(u32p), 17, only.ctypes.data_as(dp), None) == 0
        _eq(only, mean[:17], "mean alone")
        assert D.lib.hpf_score_moments(D._h, None, None, 0, None, None) == 0
    finally:
        D.close()


def test_the_column_limit():
    n, m = 20, 30
    D = Hpf(n, m, 512, hier=False, bias=True)
    try:
        _raises(UNSUPPORTED, lambda: D.score_moments(np.zeros(1, np.uint32), np.zeros(1, np.uint32)), "HPF_MAX_COLUMNS")
        _raises(UNSUPPORTED, lambda: D.recommend_ucb(np.zeros(1, np.uint32), 5, 1.0), "HPF_MAX_COLUMNS")
    finally:
        D.close()
    with pytest.raises(ValueError):
        capi.moments_plan(512, True)
    assert capi.moments_plan(511, True)["C"] == 1024 and capi.moments_plan(512, False)["C"] == 1024


# ---------------------------------------------------------------------------------------------------------------------
# 2. lists: two batches, splits, compactions, masks, padding
# ---------------------------------------------------------------------------------------------------------------------
LIST_N, LIST_M, LOO_BATCH = 70, 700, 64
TOPNS = (1, 64, 65, 256)


def _batch_users(n_sel, knob):
    """hpf_plan::rank_batch_users where the bit rows are no limit: the knob rounded up to a wave's 16 users"""
    return min((knob + 15) & ~15, (n_sel + 15) & ~15)


def _check_plan(n_sel, m, topn, want_splits):
    """the shapes do what they are meant to: two batches, the splits named, and a split long enough to compact"""
    batch = _batch_users(n_sel, LOO_BATCH)
    assert batch < n_sel <= 2 * batch
    cap = capi.recommend_cap(topn)
    blocks, splits, tps = capi.recommend_grid(batch, m, topn)
    assert blocks == 1 and splits == want_splits
    # a buffer is compacted once it holds more than cap - 64 entries; before the first compaction every item is taken
    assert min(tps * 64, m) > cap - 64, (topn, tps, cap)
    return splits, tps


def _list_case(K, bias, m=LIST_M):
    n = LIST_N
    st = ref.gamma_state(n, m, K, bias, 4000 + K + int(bias))
    # duplicate item rows, bit-identical E and shape, made heavy so that they are listed: across a tile edge (63 | 64),
    # across the split edge of topn <= 64 (tile 8: 511 | 512) and inside one tile (100, 101)
    if m > 512:
        heavy = st["BETA_E"].max(0)
        for a, b, f in ((63, 64, 3.0), (511, 512, 2.5), (100, 101, 2.0)):
            st["BETA_E"][a] = f * heavy
            for w in ("BETA_E", "BETA_SHAPE"):
                st[w][b] = st[w][a]
            if bias:
                for w in ("IBIAS_E", "IBIAS_SHAPE"):
                    st[w][b] = st[w][a]
    csr = make_problem(n, m, 6 * n, seed=K + m)
    rng = np.random.default_rng(K + 17)
    users = rng.permutation(n).astype(np.uint32)              # every user once, not in order: 64 + 6 over two batches
    lists = [np.sort(rng.choice(m, rng.integers(0, 6), replace=False)) if b % 3 else [] for b in range(n)]
    lists[5] = np.arange(m)                                   # every item masked: the list is items 0 .. at +0.0
    lists[66] = np.arange(0, m, 2)                            # in the second batch: half of the items
    return n, m, st, csr, users, lists


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("K", [100, 5])
def test_lists_equal_the_reference_bit_for_bit(K, bias, monkeypatch):
    monkeypatch.setenv("HPF_LOO_BATCH", str(LOO_BATCH))       # read when the handle is created
    n, m, st, csr, users, lists = _list_case(K, bias)
    mptr, mitems = _mask_csr(lists)
    splits_seen = set()
    D = _handle(n, m, K, bias, csr, st)
    try:
        assert D.work_info()["ld"] % 2 == 0
        S, V = D.scores(_all(n)), _var_matrix(st, bias, csr)
        for topn in TOPNS:
            splits_seen.add(_check_plan(n, m, topn, 2 if topn <= 64 else 1)[0])
            for z in (2.0, 0.5):
                got = D.recommend_ucb(users, topn, z, mptr, mitems)
                _same_lists(got, _want_lists(S, V, csr, users, lists, topn, z), f"K={K} bias={bias} topn={topn} z={z}, mask list")
            got = D.recommend_ucb(users, topn, 2.0)
            _same_lists(got, _want_lists(S, V, csr, users, None, topn, 2.0), f"K={K} bias={bias} topn={topn}, no mask list")
        assert splits_seen == {1, 2}
        # user 5 of the selection has every item masked: items ascending, each with the moments and the value it would have had
        it, ucb, mean, var = D.recommend_ucb(users, 64, 2.0, mptr, mitems)
        assert np.array_equal(it[5], np.arange(64, dtype=np.uint32)) and np.all(ucb[5] > 0)
        _eq(ucb[5], ref.ucb(S[users[5], :64], V[users[5], :64], 2.0), "masked items report their own value")
        # z = 0: ucb is mean bit for bit and the lists are hpf_recommend's; where hpf_recommend reports a masked item's
        # +0.0, out_ucb reports the value the item would have had
        for topn in (64, 256):
            it0, ucb0, mean0, var0 = D.recommend_ucb(users, topn, 0.0, mptr, mitems)
            itr, scr = D.recommend(users, topn, mptr, mitems)
            _eq(it0, itr, f"z = 0, topn={topn}: items")
            _eq(ucb0, mean0, f"z = 0, topn={topn}: ucb is mean")
            msk = np.zeros(it0.shape, bool)
            for b, u in enumerate(users):
                msk[b] = np.isin(it0[b], _masked(csr, u, lists[b]))
            assert msk.any() and np.all(bits(scr[msk]) == 0)
            _eq(np.where(msk, 0.0, ucb0), scr, f"z = 0, topn={topn}: scores")
    finally:
        D.close()


def test_two_splits_at_the_largest_topn(monkeypatch):
    """m = 2100: 33 tiles, which topn = 256 (cap 512) sweeps as 32 + 1"""
    monkeypatch.setenv("HPF_LOO_BATCH", str(LOO_BATCH))
    K, bias, m = 5, True, 2100
    n, m, st, csr, users, lists = _list_case(K, bias, m)
    mptr, mitems = _mask_csr(lists)
    assert _check_plan(n, m, 256, 2) == (2, 32)
    D = _handle(n, m, K, bias, csr, st)
    try:
        S, V = D.scores(_all(n)), _var_matrix(st, bias, csr)
        _same_lists(D.recommend_ucb(users, 256, 1.5, mptr, mitems), _want_lists(S, V, csr, users, lists, 256, 1.5), "m=2100 topn=256")
    finally:
        D.close()


def test_padding_beyond_the_items(monkeypatch):
    monkeypatch.setenv("HPF_LOO_BATCH", str(LOO_BATCH))
    K, bias, m = 5, True, 40
    n, m, st, csr, users, lists = _list_case(K, bias, m)
    lists = [np.asarray(x)[np.asarray(x) < m] if len(x) else [] for x in lists]
    mptr, mitems = _mask_csr(lists)
    D = _handle(n, m, K, bias, csr, st)
    try:
        S, V = D.scores(_all(n)), _var_matrix(st, bias, csr)
        for topn in (64, 256):
            got = D.recommend_ucb(users, topn, 2.0, mptr, mitems)
            _same_lists(got, _want_lists(S, V, csr, users, lists, topn, 2.0), f"m=40 topn={topn}")
            assert np.all(got[0][:, m:] == NONE) and np.all(got[0][:, :m] < m)
            for a in got[1:]:
                assert np.all(bits(a[:, m:]) == 0)
    finally:
        D.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. ties: equal ucb lists by ascending item, across a tile edge, a split edge and inside a tile
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("topn", [64, 256])
def test_ties(topn):
    K, bias = 5, True
    n, m, st, csr, users, lists = _list_case(K, bias)
    D = _handle(n, m, K, bias, csr, st)
    try:
        S, V = D.scores(_all(n)), _var_matrix(st, bias, csr)
        got = D.recommend_ucb(users, topn, 2.0)
        want = _want_lists(S, V, csr, users, None, topn, 2.0)
        _same_lists(got, want, f"topn={topn}")
        seen = 0
        for a, b in ((63, 64), (511, 512), (100, 101)):
            for r in range(n):
                row = got[0][r].tolist()
                if a in row and b in row:                     # neither is a training item of the user: the same ucb, side by side
                    pa, pb = row.index(a), row.index(b)
                    if bits(got[1][r, pa]) == bits(got[1][r, pb]) and got[1][r, pa] > 0:
                        assert pb == pa + 1, (a, b, r)
                        seen += 1
        assert seen >= 3 * n - 30                             # the planted rows are the heaviest: listed unless a training item
    finally:
        D.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. the variance must matter
# ---------------------------------------------------------------------------------------------------------------------
def test_the_variance_decides_the_order():
    """item 7: a small mean from a tiny shape; item 300: a larger mean from a huge shape.  At z = 3 the first precedes the
    second, at z = 0 the second the first -- a sweep that ignored its second chain would pass every test above"""
    n, m, K = 70, 700, 5
    st = ref.gamma_state(n, m, K, False, 77)
    top = st["BETA_E"].max()
    st["BETA_E"][7], st["BETA_SHAPE"][7] = 40.0 * top, 0.05           # sd of a factor = E / sqrt(shape): 4.5 E
    st["BETA_E"][300], st["BETA_SHAPE"][300] = 50.0 * top, 1e6
    st["THETA_SHAPE"][:] = 1e6                                        # the users are sure: the items' shapes decide
    csr = make_problem(n, m, 4 * n, seed=1)
    D = _handle(n, m, K, False, csr, st)
    try:
        S, V = D.scores(_all(n)), _var_matrix(st, False, csr)
        users = _all(n)
        for z, first in ((0.0, (300, 7)), (3.0, (7, 300))):
            got = D.recommend_ucb(users, 10, z)
            _same_lists(got, _want_lists(S, V, csr, users, None, 10, z), f"z={z}")
            free = np.array([not np.isin([7, 300], _masked(csr, u, [])).any() for u in users])     # neither is a training item
            assert free.sum() >= n // 2
            assert np.all(got[0][free, 0] == first[0]) and np.all(got[0][free, 1] == first[1]), (z, got[0][:3, :3])
        mean, var = D.score_moments(np.zeros(2, np.uint32), np.array([7, 300], np.uint32))
        assert mean[0] < mean[1] and np.sqrt(var[0]) > 100 * np.sqrt(var[1])
    finally:
        D.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. state routes: after hpf_iterate, after hpf_fold_in
# ---------------------------------------------------------------------------------------------------------------------
def _trained(n, m, K, hier, bias, csr, iters):
    from hgaprec_amd import hostlib
    init = hostlib.initial_state(0, n, m, K, hier, bias)
    D = Hpf(n, m, K, hier=hier, bias=bias)
    D.upload_csr(*csr)
    for w in init_states(hier, bias):
        D.set_state(w, init[w])
    D.iterate(iters)
    return D


def _check_against_exports(D, bias, csr, users, topn, z, got_pairs, got_lists, up, ip, what):
    st = _exports(D, bias)
    n = st["THETA_E"].shape[0]
    S, V = D.scores(_all(n)), _var_matrix(st, bias, csr)
    _eq(got_pairs[0], S[up, ip], what + ": mean")
    _eq(got_pairs[1], V[up, ip], what + ": var")
    Cc = 2 * st["THETA_E"].shape[1] + 2 * bias
    for p in range(8):
        assert ref.within(got_pairs[1][p], ref.exact_var(st, bias, up[p], ip[p]), Cc), (what, p)
    _same_lists(got_lists, _want_lists(S, V, csr, users, None, topn, z), what)


@pytest.mark.parametrize("hier,bias", [(True, True), (False, False)])
def test_straight_after_an_iteration_and_the_state_is_not_written(hier, bias):
    n, m, K = 300, 80, 20
    csr = make_problem(n, m, 4000, seed=3)
    rng = np.random.default_rng(4)
    users = rng.permutation(n)[:100].astype(np.uint32)
    up, ip = rng.integers(0, n, 30).astype(np.uint32), rng.integers(0, m, 30).astype(np.uint32)
    A = _trained(n, m, K, hier, bias, csr, 2)
    B = _trained(n, m, K, hier, bias, csr, 2)
    try:
        got_pairs = A.score_moments(up, ip)                           # straight after hpf_iterate(2): S holds raw sums
        got_lists = A.recommend_ucb(users, 20, 2.0)
        states = compare_states(hier, bias)
        before = {w: B.get_state(w) for w in states}
        for w in states:
            _eq(A.get_state(w), before[w], w)
        _check_against_exports(A, bias, csr, users, 20, 2.0, got_pairs, got_lists, up, ip, f"hier={hier} bias={bias}")
        _same_lists(A.recommend_ucb(users, 20, 2.0), got_lists, "a second call")
        A.iterate(1)
        B.iterate(1)
        for w in states:
            _eq(A.get_state(w), B.get_state(w), "after a further iteration: " + w)
    finally:
        A.close()
        B.close()


@pytest.mark.parametrize("hier,bias", [(True, True), (False, False)])
def test_straight_after_a_fold_in(hier, bias):
    import tests.test_gpu_fold_in as fi
    n, m, K = fi.N1, fi.M1, fi.K1
    rowptr, col, val = fi.make_csr(m, fi.DEGS1, 91)
    item = fi.item_side(n, m, K, hier, bias, 92)
    D = fi.device(n, m, K, hier, bias, rowptr, col, val, item)
    try:
        D.fold_in(5)
        users = _all(n)
        up, ip = np.arange(20, dtype=np.uint32), (np.arange(20, dtype=np.uint32) * 7) % m
        got_pairs = D.score_moments(up, ip)                           # straight after hpf_fold_in: the fold-in left shapes
        got_lists = D.recommend_ucb(users, 10, 2.0)
        _check_against_exports(D, bias, (rowptr, col, val), users, 10, 2.0, got_pairs, got_lists, up, ip, f"fold-in hier={hier} bias={bias}")
        # a user with one rating is less sure of its scores than one with fifty
        deg = np.diff(rowptr)
        one, fifty = int(np.flatnonzero(deg == 1)[0]), int(np.flatnonzero(deg == 50)[0])
        mean, var = D.score_moments(np.repeat(np.array([one, fifty], np.uint32), m), np.tile(_all(m), 2))
        cv = (np.sqrt(var) / mean).reshape(2, m).mean(1)
        assert cv[0] > cv[1], cv
    finally:
        D.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. errors: each refused on the host before a launch; the handle stays usable
# ---------------------------------------------------------------------------------------------------------------------
def test_errors():
    n, m, K = 70, 90, 5
    csr = make_problem(n, m, 400, seed=9)
    st = ref.gamma_state(n, m, K, True, 60)
    D = _handle(n, m, K, True, csr, st)
    try:
        users = np.array([3, 7, 3, 69, 0], np.uint32)
        lists = [[1], [], [1], [2, 3], []]
        mptr, mitems = _mask_csr(lists)
        S, V = D.scores(_all(n)), _var_matrix(st, True, csr)
        want = _want_lists(S, V, csr, users, lists, 10, 1.0)
        got = D.recommend_ucb(users, 10, 1.0, mptr, mitems)
        _same_lists(got, want, "a repeated user")
        for a in got:
            assert np.array_equal(a[0].view(np.uint8), a[2].view(np.uint8))
        e = D.recommend_ucb(np.zeros(0, np.uint32), 10, 1.0)
        assert all(a.shape == (0, 10) for a in e)
        assert D.lib.hpf_recommend_ucb(D._h, None, 0, None, None, 10, 1.0, None, None, None, None) == 0
        bad_users, bad_items, bad_ptr0, bad_ptr = users.copy(), mitems.copy(), mptr.copy(), mptr.copy()
        bad_users[1] = n
        bad_items[-1] = m
        bad_ptr0[0] = 1
        bad_ptr[2] = bad_ptr[1] - 1
        for args, msg in (((users, 10, -1.0, mptr, mitems), "z is finite and >= 0"), ((users, 10, float("nan"), mptr, mitems), "z is finite"),
                          ((users, 10, float("inf"), mptr, mitems), "z is finite"), ((users, 10, -0.5), "z is finite"),
                          ((users, 0, 1.0, mptr, mitems), "topn"), ((users, 257, 1.0, mptr, mitems), "topn"),
                          ((bad_users, 10, 1.0, mptr, mitems), "user index out of range"),
                          ((users, 10, 1.0, mptr, bad_items), "mask item out of range"),
                          ((users, 10, 1.0, bad_ptr0, mitems), "mask_ptr[0]"), ((users, 10, 1.0, bad_ptr, mitems), "mask_ptr not monotone")):
            _raises(INVALID, lambda: D.recommend_ucb(*args), msg)
            assert msg.encode() in D.lib.hpf_last_error(D._h)
        _raises(INVALID, lambda: D.score_moments(np.array([n], np.uint32), np.array([0], np.uint32)), "index out of range")
        _raises(INVALID, lambda: D.score_moments(np.array([0], np.uint32), np.array([m], np.uint32)), "index out of range")
        _same_lists(D.recommend_ucb(users, 10, 1.0, mptr, mitems), want, "after the refused calls")
    finally:
        D.close()
    # HPF_ERR_STATE: a fresh handle with E but no shape; with bias: E and shapes but no bias shape
    sel = np.arange(3, dtype=np.uint32)
    for bias, have, msg in ((False, ("THETA_E", "BETA_E"), "THETA_SHAPE"),
                            (False, ("THETA_E", "BETA_E", "THETA_SHAPE"), "BETA_SHAPE"),
                            (True, ("THETA_E", "BETA_E", "THETA_SHAPE", "BETA_SHAPE", "UBIAS_E", "IBIAS_E"), "SHAPE of UBIAS and IBIAS"),
                            (True, ("THETA_E", "BETA_E", "THETA_SHAPE", "BETA_SHAPE", "UBIAS_E", "IBIAS_E", "UBIAS_SHAPE"), "SHAPE of UBIAS and IBIAS")):
        F = Hpf(n, m, K, hier=False, bias=bias)
        try:
            F.upload_csr(*csr)
            for w in have:
                F.set_state(w, st[w])
            _raises(STATE, lambda: F.recommend_ucb(sel, 5, 1.0), msg)
            _raises(STATE, lambda: F.score_moments(sel, sel), msg)
            assert msg.encode() in F.lib.hpf_last_error(F._h)
            assert F.recommend(sel, 5)[0].shape == (3, 5)             # usable: E is there
            for w in st:
                if w not in have and (bias or not w.startswith(("UBIAS", "IBIAS"))):
                    F.set_state(w, st[w])
            assert F.recommend_ucb(sel, 5, 1.0)[0].shape == (3, 5)
        finally:
            F.close()
    # no CSR: the pairs need none, the lists do
    G = Hpf(n, m, K, hier=False, bias=False)
    try:
        for w in ("THETA_E", "BETA_E", "THETA_SHAPE", "BETA_SHAPE"):
            G.set_state(w, st[w])
        assert G.score_moments(sel, sel)[0].shape == (3,)
        _raises(STATE, lambda: G.recommend_ucb(sel, 5, 1.0), "hpf_upload_csr")
    finally:
        G.close()
