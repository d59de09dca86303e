"""-m gpu: hpf_because -- which of a user's own ratings carry a score (because_shape_kernel: a wave per selected user writes
the shape D; because_kernel: a wave per target pair walks the history again with g in registers and the T best in its lanes).

The reference is tests/because_ref.py: the definition of include/hpf.h in mpmath at 60 digits, computed once per model and
shared.  Every returned contribution and prior is held to the DERIVED bound (4 S + H + 64) 2^-53 relative -- S the largest
Elog spread inside the user's row or a gathered row, H the history's length --, the returned items to the exact top-T
(tests/test_because_ref.py shows that these inputs need none of the exemptions for near-ties), the sum to the bits of a
sequential float64 sum, and the identity to hpf_predict.

Measured on an MI355X: the largest distance from mpmath 11.9 x 2^-53 (bounds: about 160 .. 1000 x 2^-53), the identity within
16.5 x 2^-53 of hpf_predict, no list exempted.
"""
import ctypes as C
import math

import numpy as np
import pytest

from hgaprec_amd import capi
from hgaprec_amd.capi import Hpf, HpfError
from tests import because_ref as R
from tests.util import compare_states

pytestmark = pytest.mark.gpu
NONE = R.NONE
U53 = R.U53


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def device(inp, only=None, csr=True):
    D = Hpf(inp.n, inp.m, inp.K, hier=inp.hier, bias=inp.bias, binary=inp.val is None)
    if csr:
        D.upload_csr(inp.rowptr, inp.col, inp.val)
    for w, a in inp.states().items():
        if only is None or w in only:
            D.set_state(w, a)
    return D


def readable(inp):
    return list(inp.states())


def all_bits(D, names):
    return {w: _bits(D.get_state(w)).copy() for w in names}


def csr_of(groups):
    """[(user, [targets])] -> users, t_ptr, t_items"""
    users = np.array([u for u, _ in groups], np.uint32)
    t_ptr = np.zeros(len(groups) + 1, np.uint64)
    t_ptr[1:] = np.cumsum([len(t) for _, t in groups])
    t_items = np.array([j for _, t in groups for j in t], np.uint32)
    return users, t_ptr, t_items


def check_rows(inp, st, pairs, exact, items, con, priors, T, what):
    """values, order, own order and padding of every output row -> (worst multiple of 2^-53 seen, lists that used the exemption)"""
    worst, exempt = 0.0, 0
    for q, (u, j) in enumerate(pairs):
        hist, _ = inp.history(u)
        H = len(hist)
        econ, eprior, _ = exact[q]
        bnd = R.bound(st.spread(u, hist), H)
        want_ids, order = R.top(econ, hist, T)
        real = min(T, H)
        # padding, and the row sorted by its own bits: contribution descending, item ascending
        assert np.all(items[q, real:] == NONE) and np.all(_bits(con[q, real:]) == 0), (what, q)
        keys = [(-int(k), int(i)) for k, i in zip(_bits(con[q, :real]), items[q, :real])]
        assert keys == sorted(keys) and len(set(keys)) == real, (what, q, "not in the ranking order")
        pos = {int(i): r for r, i in enumerate(hist)}
        used = False
        for r in range(real):
            got = int(items[q, r])
            assert got in pos, (what, q, r, "an item that is not in the history")
            if got != int(want_ids[r]):
                # only where the exact values on either side of the place differ by less than twice the bound
                a, b = econ[pos[got]], econ[order[r]]
                assert abs(a - b) < 2.0 * bnd * max(a, b), (what, q, r, got, int(want_ids[r]))
                used = True
            e = R.ulps(con[q, r], econ[pos[got]])
            worst = max(worst, e)
            assert e * U53 <= bnd, (what, q, r, e, bnd / U53)
        exempt += used
        e = R.ulps(priors[q], eprior)
        worst = max(worst, e)
        assert e * U53 <= bnd, (what, q, "prior", e, bnd / U53)
    return worst, exempt


# ---------------------------------------------------------------------------------------------------------------------
# 1. values, order, sum, identity and the state, for every combination of bias, hier and ratings
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_values_order_sum_and_identity(case):
    bias, hier, ratings, K, T = case
    inp, st, exact = R.reference(case)
    pairs = [(u, j) for _, u, j in inp.pairs()]
    D = device(inp)
    try:
        before = all_bits(D, readable(inp))
        items, con, sums, priors = D.because(inp.users, inp.t_ptr, inp.t_items, T)
        assert items.shape == (len(pairs), T) and con.shape == (len(pairs), T) and sums.shape == priors.shape == (len(pairs),)
        worst, exempt = check_rows(inp, st, pairs, exact, items, con, priors, T, R.case_id(case))
        assert exempt <= 0.01 * len(pairs), exempt
        print(f"{R.case_id(case)}: contributions and priors within {worst:.1f} x 2^-53 of mpmath ({len(pairs)} lists, {exempt} exempted)")

        # the sum: with H <= T = 32 the bits of the sequential float64 sum of the returned contributions in CSR order
        i32, c32, s32, p32 = (items, con, sums, priors) if T == 32 else D.because(inp.users, inp.t_ptr, inp.t_items, 32)
        assert np.array_equal(i32[:, :T], items) and np.array_equal(_bits(c32[:, :T]), _bits(con))
        assert np.array_equal(_bits(s32), _bits(sums)) and np.array_equal(_bits(p32), _bits(priors))
        summed = 0
        for q, (u, j) in enumerate(pairs):
            hist, _ = inp.history(u)
            if len(hist) > 32:
                continue
            by_item = {int(i): c for i, c in zip(i32[q], c32[q])}
            s = np.float64(0.0)
            for i in hist:
                s = s + by_item[int(i)]
            assert _bits(s) == _bits(s32[q]), (q, u, j)
            summed += 1
        assert summed >= 8

        # the identity against hpf_predict
        pred = D.predict(np.array([u for u, _ in pairs], np.uint32), np.array([j for _, j in pairs], np.uint32))
        worst_id = 0.0
        for q, (u, j) in enumerate(pairs):
            hist, _ = inp.history(u)
            tol = R.bound(st.spread(u, hist), len(hist)) + (math.ceil(K / 16) + 10) * U53
            whole = sums[q] + priors[q] + (st.ib[j] if bias else 0.0)
            worst_id = max(worst_id, abs(whole - pred[q]) / pred[q] / U53)
            assert abs(whole - pred[q]) <= tol * pred[q], (q, u, j, whole, pred[q])
        print(f"{R.case_id(case)}: sum + prior + E[ibias] within {worst_id:.1f} x 2^-53 of hpf_predict")

        after = all_bits(D, readable(inp))
        assert all(np.array_equal(before[w], after[w]) for w in before), "hpf_because wrote the state"
    finally:
        D.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. ties: identical item rows with equal ratings, anywhere in the row and at the T cut
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("copies", [2, 3])
def test_identical_rows_tie_bit_for_bit_lower_item_first(copies):
    inp = R.Inputs(True, False, True, 5, seed=50, n=4, m=120, histories=(70, 3))
    hist, _ = inp.history(0)
    a0, a1 = int(inp.rowptr[0]), int(inp.rowptr[1])
    places = [68, 3, 40][:copies]                              # in different 64-blocks of the walk
    twins = sorted(int(hist[p]) for p in places)
    for w in ("SHAPE", "E", "ELOG", "B_SHAPE", "B_E", "B_ELOG"):
        for t in twins[:-1]:
            inp.item[w][t] = inp.item[w][twins[-1]]
    inp.col[a0:a1][places] = twins                             # the smallest id stands LAST in the row
    inp.val[a0:a1] = 1
    inp.val[a0:a1][places] = 255                               # (and near the top of the list: T <= 32 reaches them)
    D = device(inp)
    try:
        users, t_ptr, t_items = csr_of([(0, [5, int(hist[0])])])
        items, con, _, _ = D.because(users, t_ptr, t_items, 32)
        for q in range(2):
            where = [int(np.flatnonzero(items[q] == t)[0]) for t in twins]
            assert where == list(range(where[0], where[0] + copies)), (q, where)          # side by side, ascending id
            assert len({int(b) for b in _bits(con[q, where])}) == 1, (q, "twins differ in bits")
            # ... and at the cut: T = the place of the first of them
            cut = where[0] + 1
            ic, cc, _, _ = D.because(users, t_ptr, t_items, cut)
            assert np.array_equal(ic[q], items[q, :cut]) and np.array_equal(_bits(cc[q]), _bits(con[q, :cut]))
            assert int(ic[q, -1]) == twins[0]
    finally:
        D.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. a pair's result depends on nothing but the user's history, the state and the target
# ---------------------------------------------------------------------------------------------------------------------
def test_same_pairs_same_bits_whatever_else_is_in_the_call():
    inp = R.Inputs(True, True, True, 65, seed=60)
    rng = np.random.default_rng(61)
    T = 5
    D = device(inp)
    try:
        groups = [(int(u), [int(j) for j in inp.t_items[int(inp.t_ptr[b]):int(inp.t_ptr[b + 1])]]) for b, u in enumerate(inp.users)]

        def run(gs):
            users, t_ptr, t_items = csr_of(gs)
            items, con, sums, priors = D.because(users, t_ptr, t_items, T)
            out, q = {}, 0
            for u, ts in gs:
                for j in ts:
                    row = (items[q].tobytes(), con[q].tobytes(), sums[q].tobytes(), priors[q].tobytes())
                    assert out.setdefault((u, j), row) == row, "equal requests, unequal rows"
                    q += 1
            return out

        base = run(groups)
        assert run(groups[::-1]) == base                                           # another selection order
        assert run(groups + [groups[7], groups[0]]) == base                        # a user selected twice
        half = run(groups[:5])
        half.update(run(groups[5:]))
        assert half == base                                                        # split over two calls
        one = run([(u, ts[:1]) for u, ts in groups])                               # one target per user ...
        many = run([(u, ts[:1] + [int(j) for j in rng.integers(0, inp.m, 31)] + ts[:1]) for u, ts in groups])   # ... and 33
        assert all(many[k] == v for k, v in one.items()) and all(base[k] == v for k, v in one.items())
    finally:
        D.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. the model state is not written: exports and a following iteration
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hier,bias", [(True, True), (False, False)])
def test_exports_and_the_next_iteration_do_not_see_the_call(hier, bias):
    inp = R.Inputs(bias, hier, True, 5, seed=70)
    names = compare_states(hier, bias)
    A, B, Cc = device(inp), device(inp), device(inp)
    try:
        A.iterate(3)
        B.iterate(3)
        A.because(inp.users, inp.t_ptr, inp.t_items, 5)
        sa, sb = all_bits(A, names), all_bits(B, names)                            # the call first, or the exports alone
        assert all(np.array_equal(sa[w], sb[w]) for w in names)
        A.because(inp.users, inp.t_ptr, inp.t_items, 5)
        sa2 = all_bits(A, names)
        assert all(np.array_equal(sa[w], sa2[w]) for w in names)                   # before and after
        # iterate(3), the call, iterate(1) against iterate(4) -- on a handle nobody exported from in between
        Cc.iterate(3)
        Cc.because(inp.users, inp.t_ptr, inp.t_items, 5)
        Cc.iterate(1)
        B.close()
        B = device(inp)
        B.iterate(4)
        sc, sb = all_bits(Cc, names), all_bits(B, names)
        assert all(np.array_equal(sc[w], sb[w]) for w in names), [w for w in names if not np.array_equal(sc[w], sb[w])]
    finally:
        A.close(); B.close(); Cc.close()


def test_on_the_state_a_fold_in_leaves():
    """the session case: the users are folded in, then asked why"""
    inp = R.Inputs(True, True, True, 5, seed=80, n=12, m=200, histories=(0, 1, 2, 63, 65))
    item_side = [w for w in inp.states() if w.split("_")[0] in ("BETA", "ETA", "IBIAS")]
    D = device(inp, only=item_side)
    try:
        D.fold_in(3)
        st = R.State(D.get_state("THETA_E"), D.get_state("THETA_ELOG"), D.get_state("BETA_E"), D.get_state("BETA_ELOG"),
                     D.get_state("UBIAS_E"), D.get_state("UBIAS_ELOG"), D.get_state("IBIAS_E"), D.get_state("IBIAS_ELOG"))
        T = 5
        items, con, sums, priors = D.because(inp.users, inp.t_ptr, inp.t_items, T)
        pairs, exact = [], {}
        for b, u in enumerate(inp.users):
            hist, yy = inp.history(u)
            ts = inp.t_items[int(inp.t_ptr[b]):int(inp.t_ptr[b + 1])]
            for j, r in zip(ts, R.exact(st, hist, yy, int(u), ts)):
                exact[len(pairs)] = r
                pairs.append((int(u), int(j)))
        worst, exempt = check_rows(inp, st, pairs, exact, items, con, priors, T, "after hpf_fold_in")
        assert exempt == 0
        print(f"after hpf_fold_in: within {worst:.1f} x 2^-53 of mpmath on the exported state")
    finally:
        D.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. errors, each before anything is launched and with the state untouched
# ---------------------------------------------------------------------------------------------------------------------
def _raises(code, f):
    with pytest.raises(HpfError) as e:
        f()
    assert f"({code})" in str(e.value), str(e.value)


def test_errors_leave_the_state_alone():
    inp = R.Inputs(True, True, True, 5, seed=90, n=6, m=40, histories=(0, 3, 5))
    users, t_ptr, t_items = csr_of([(1, [2, 3]), (2, [4])])
    D = device(inp)
    try:
        before = all_bits(D, readable(inp))
        _raises(-1, lambda: D.because(users, t_ptr, t_items, 0))
        _raises(-1, lambda: D.because(users, t_ptr, t_items, 33))
        _raises(-1, lambda: D.because([1, 6], t_ptr, t_items, 5))                  # a user out of range
        _raises(-1, lambda: D.because(users, t_ptr, [2, 40, 4], 5))                # an item out of range
        _raises(-1, lambda: D.because(users, [1, 2, 3], t_items, 5))               # t_ptr[0] != 0
        _raises(-1, lambda: D.because(users, [0, 3, 2], t_items, 5))               # a decreasing t_ptr
        lib, u32, u64 = D.lib, C.c_uint32, C.c_uint64
        pu, pp, pi = (u32 * 2)(1, 2), (u64 * 3)(0, 2, 3), (u32 * 3)(2, 3, 4)
        oi, oc = (u32 * 15)(), (C.c_double * 15)()
        assert lib.hpf_because(D._h, pu, 2, pp, pi, 5, None, oc, None, None) == -1  # a null pointer with work to do
        assert lib.hpf_because(D._h, pu, 2, pp, None, 5, oi, oc, None, None) == -1
        assert lib.hpf_because(D._h, None, 2, pp, pi, 5, oi, oc, None, None) == -1
        assert lib.hpf_because(D._h, pu, 2, None, pi, 5, oi, oc, None, None) == -1
        assert lib.hpf_because(D._h, None, 0, None, None, 5, None, None, None, None) == 0      # n_sel = 0
        assert lib.hpf_because(D._h, pu, 2, (u64 * 3)(0, 0, 0), None, 5, None, None, None, None) == 0      # nt = 0
        assert lib.hpf_because(D._h, pu, 2, pp, pi, 5, oi, oc, None, None) == 0     # sums and priors not asked for
        i2, c2, s2, p2 = D.because(users, t_ptr, t_items, 5)
        assert np.array_equal(np.frombuffer(oi, np.uint32), i2.ravel()) and np.array_equal(np.frombuffer(oc, np.uint64), _bits(c2).ravel())
        assert D.because(users, t_ptr, t_items, 5, want_sums=False)[2:] == (None, None)
        after = all_bits(D, readable(inp))
        assert all(np.array_equal(before[w], after[w]) for w in before)
    finally:
        D.close()
    # no CSR; no Elog on a side; with bias either bias
    D = device(inp, csr=False)
    try:
        _raises(-6, lambda: D.because(users, t_ptr, t_items, 5))
    finally:
        D.close()
    for missing in ("THETA_ELOG", "BETA_ELOG", "THETA_E", "BETA_E", "UBIAS_ELOG", "IBIAS_E"):
        D = device(inp, only=[w for w in inp.states() if w != missing])
        try:
            _raises(-6, lambda: D.because(users, t_ptr, t_items, 5))
            D.set_state(missing, inp.states()[missing])
            D.because(users, t_ptr, t_items, 5)
        finally:
            D.close()


def test_an_underflowing_denominator_is_reported_and_the_handle_stays_usable():
    inp = R.Inputs(False, True, False, 5, seed=95, n=6, m=40, histories=(1, 3, 5))
    item = int(inp.history(0)[0][0])
    inp.user["ELOG"][0] = [0.0, -1500.0, -1500.0, -1500.0, -1500.0]                # the maxima 1500 apart in different columns:
    inp.item["ELOG"][item] = [-1500.0, 0.0, -1500.0, -1500.0, -1500.0]             # every product of the pair underflows
    D = device(inp)
    try:
        before = all_bits(D, readable(inp))
        _raises(-6, lambda: D.because(*csr_of([(0, [3])]), 5))
        _raises(-6, lambda: D.because(*csr_of([(1, [3]), (0, [3])]), 5))
        items, con, sums, priors = D.because(*csr_of([(1, [3]), (2, [item])]), 5)  # the next valid call
        assert np.all(items[:, :3] != NONE) and np.all(con[:, :3] > 0) and np.all(sums > 0) and np.all(priors > 0)
        after = all_bits(D, readable(inp))
        assert all(np.array_equal(before[w], after[w]) for w in before)
    finally:
        D.close()
