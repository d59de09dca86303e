"""-m gpu: hpf_audience -- the top-N users of every selected item: hpf_recommend transposed (audience_mask_kernel: the
bit rows of a batch of ITEMS, one bit per user, from the item-major view; audience_sweep_kernel: topn_sweep_kernel's body
with the rows of E[beta] as query rows and the rows of E[theta] swept; topn_merge_kernel).

The oracle is the project's own exact one: hpf_scores for all users of the same handle, column i zeroed at the masked users,
sorted on the host by (bit pattern descending, user ascending).  Every comparison is exact."""
import ctypes as C
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from hgaprec_amd import capi
from hgaprec_amd.capi import Hpf, HpfError
from tests.util import compare_states, init_states, make_problem

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
NONE = 0xFFFFFFFF
INVALID, UNSUPPORTED, STATE = -1, -5, -6


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(got, want, what):
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape, what
    assert np.array_equal(got[0], want[0]), what + ": users"
    assert np.array_equal(_bits(got[1]), _bits(want[1])), what + ": scores"


def _raises(code, f, msg=None):
    with pytest.raises(HpfError) as e:
        f()
    assert f"({code})" in str(e.value) and (msg is None or msg in str(e.value)), str(e.value)


# ---------------------------------------------------------------------------------------------------------------------
# handles and the oracle
# ---------------------------------------------------------------------------------------------------------------------
def _gamma(rows, K, seed):
    """expectations of a Gamma(0.3, .) factor matrix: positive, wide in magnitude, and a few exact zeros"""
    rng = np.random.default_rng(seed)
    E = rng.gamma(0.3, 1.0, (rows, K)) / rng.gamma(3.0, 1.0, (rows, 1))
    E[rng.random((rows, K)) < 0.02] = 0.0
    return E


def _factors(n, m, K, bias, seed):
    rng = np.random.default_rng(seed + 7)
    st = {"THETA_E": _gamma(n, K, seed), "BETA_E": _gamma(m, K, seed + 1)}
    if bias:
        st["UBIAS_E"], st["IBIAS_E"] = rng.gamma(0.3, 1.0, n), rng.gamma(0.3, 1.0, m)
    return st


def _handle(n, m, K, bias, csr, st, **kw):
    rowptr, col, val = csr
    D = Hpf(n, m, K, hier=False, bias=bias, binary=val is None, **kw)
    D.upload_csr(rowptr, col, val)
    for w, a in st.items():
        D.set_state(w, a)
    return D


def _csc(n, m, csr):
    """the item-major view of a CSR, users ascending inside an item (what the upload builds)"""
    rowptr, col, val = csr
    user_of = np.repeat(np.arange(n, dtype=np.uint32), np.diff(rowptr))
    o = np.argsort(col, kind="stable")
    colptr = np.zeros(m + 1, np.int64)
    colptr[1:] = np.cumsum(np.bincount(col, minlength=m))
    return colptr, user_of[o], None if val is None else val[o]


def _from_columns(n, cols):
    """items given as (users, ratings) -> the CSR over the n users"""
    usr = np.concatenate([np.asarray(u, np.uint32) for u, _ in cols])
    val = np.concatenate([np.asarray(v, np.uint8) for _, v in cols])
    item_of = np.repeat(np.arange(len(cols), dtype=np.uint32), [len(u) for u, _ in cols])
    o = np.argsort(usr, kind="stable")
    rowptr = np.zeros(n + 1, np.int64)
    rowptr[1:] = np.cumsum(np.bincount(usr, minlength=n))
    return rowptr, item_of[o], val[o]


def _mask_csr(lists):
    mptr = np.zeros(len(lists) + 1, np.uint64)
    mptr[1:] = np.cumsum([len(x) for x in lists])
    return mptr, (np.concatenate([np.asarray(x, np.uint32) for x in lists]) if len(lists) else np.zeros(0)).astype(np.uint32)


def _masked_users(csc, i, lst):
    colptr, usr, cval = csc
    seg = slice(colptr[i], colptr[i + 1])
    mu = usr[seg] if cval is None else usr[seg][cval[seg] > 0]
    return np.union1d(mu, np.asarray(lst if lst is not None else [], np.uint32)).astype(np.int64)


def _want(S, csc, items, topn, lists=None):
    """S = hpf_scores of all users [n x m] -> what hpf_audience returns"""
    n = S.shape[0]
    out = np.full((len(items), topn), NONE, np.uint32)
    sc = np.zeros((len(items), topn), np.float64)
    users = np.arange(n)
    for b, i in enumerate(items):
        s = S[:, i].copy()
        s[_masked_users(csc, i, None if lists is None else lists[b])] = 0.0
        order = np.lexsort((users, ~_bits(s)))[:topn]             # bit pattern descending, user ascending
        out[b, :order.size] = order
        sc[b, :order.size] = s[order]
    return out, sc


def _all_scores(D):
    return D.scores(np.arange(D.n_users, dtype=np.uint32))


# ---------------------------------------------------------------------------------------------------------------------
# 1. the sweep: every NCH instance, a K that is no multiple of 4, ragged tiles, two splits, compactions
# ---------------------------------------------------------------------------------------------------------------------
M_SWEEP, N_SEL = 160, 150
# users, topn list, cap, tiles, tiles per split: ten tiles in 8 + 2 (compactions from the third tile), 16 + 2, 32 + 1
USERS = [(600, (1, 10, 64), 128, 10, 8), (1100, (100,), 256, 18, 16), (2100, (256,), 512, 33, 32)]


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("K", [5, 33, 100, 130])
@pytest.mark.parametrize("n,topns,cap,tiles,tps", USERS)
def test_sweep_equals_scores_and_a_sort_bit_for_bit(n, topns, cap, tiles, tps, K, bias):
    m = M_SWEEP
    csr = make_problem(n, m, 6 * n, seed=n + K)
    rng = np.random.default_rng(n * 1000 + K)
    items = rng.permutation(m)[:N_SEL].astype(np.uint32)           # three workgroups of query rows, the last ragged
    lists = [np.sort(rng.choice(n, rng.integers(0, 5), replace=False)) for _ in items]
    mptr, musers = _mask_csr(lists)
    D = _handle(n, m, K, bias, csr, _factors(n, m, K, bias, n + K))
    try:
        if D.work_info()["ld"] & 1:
            _raises(UNSUPPORTED, lambda: D.audience(items, topns[0], mptr, musers), "odd row stride")
            return
        S, csc = _all_scores(D), _csc(n, m, csr)
        for topn in topns:
            assert capi.recommend_cap(topn) == cap and (n + 63) // 64 == tiles
            assert capi.recommend_grid(N_SEL, n, topn) == (3, 2, tps)
            _same(D.audience(items, topn, mptr, musers), _want(S, csc, items, topn, lists), f"n={n} K={K} bias={bias} topn={topn}, list")
            _same(D.audience(items, topn), _want(S, csc, items, topn), f"n={n} K={K} bias={bias} topn={topn}, no list")
    finally:
        D.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. ties and padding
# ---------------------------------------------------------------------------------------------------------------------
def _tie_case(n, m=12, K=3):
    rng = np.random.default_rng(n)
    Et = rng.integers(0, 3, (n, K)).astype(np.float64)               # small integers: many equal scores, exact in a double
    Eb = rng.integers(0, 3, (m, K)).astype(np.float64)
    Et[n // 2:n // 2 + 10] = Et[:10]                                 # duplicated user rows
    Eb[4] = 0.0                                                      # an all-zero item row
    csr = make_problem(n, m, 3 * n, seed=n + 1)
    return csr, {"THETA_E": Et, "BETA_E": Eb}


@pytest.mark.parametrize("n,topn", [(200, 10), (200, 64), (200, 200), (40, 64)])
def test_ties_and_padding(n, topn):
    m = 12
    csr, st = _tie_case(n)
    D = _handle(n, m, 3, False, csr, st)
    try:
        items = np.arange(m, dtype=np.uint32)
        S, csc = _all_scores(D), _csc(n, m, csr)
        got = D.audience(items, topn)
        _same(got, _want(S, csc, items, topn), f"n={n} topn={topn}")
        Ne = min(topn, n)
        # the all-zero item: +0.0 throughout, users ascending
        assert np.array_equal(got[0][4, :Ne], np.arange(Ne, dtype=np.uint32)) and np.all(_bits(got[1][4]) == 0)
        assert np.all(got[0][:, Ne:] == NONE) and np.all(_bits(got[1][:, Ne:]) == 0) and np.all(got[0][:, :Ne] < n)
        # exact scores: ties are really there
        assert any(np.unique(got[1][b, :Ne]).size < Ne for b in range(m) if Ne > 3)
    finally:
        D.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. masks: column lengths, a stored 0, no values, the caller's list, masked users at +0.0
# ---------------------------------------------------------------------------------------------------------------------
def _mask_case():
    n, K = 400, 5
    rng = np.random.default_rng(31)
    lens = [0, 1, 64, 65, 300, 7]
    cols = []
    for L in lens:
        u = np.sort(rng.choice(n, L, replace=False))
        v = rng.integers(1, 6, L)
        cols.append((u, v))
    cols[3][1][10] = 0                                               # a stored rating of 0 (256 wrapped)
    cols[4][1][[0, 150, 299]] = 0
    st = {"THETA_E": rng.gamma(0.3, 1.0, (n, K)) + 2.0 ** -20, "BETA_E": rng.gamma(0.3, 1.0, (len(lens), K)) + 2.0 ** -20}   # every score > 0
    st["THETA_E"][cols[3][0][10]] += 1e3                            # ... of the user who would lead item 3's list
    return n, K, lens, cols, st


@pytest.mark.parametrize("values", [True, False])
def test_masks(values):
    n, K, lens, cols, st = _mask_case()
    m = len(lens)
    rowptr, col, val = _from_columns(n, cols)
    csr = (rowptr, col, val if values else None)
    D = _handle(n, m, K, False, csr, st)
    try:
        S, csc = _all_scores(D), _csc(n, m, csr)
        assert np.array_equal(np.diff(csc[0]), lens)
        cc, cu, cv = D.get_csc(with_vals=values)
        assert np.array_equal(cc, csc[0]) and np.array_equal(cu, csc[1]) and (not values or np.array_equal(cv, csc[2]))
        items = np.arange(m, dtype=np.uint32)
        zero3 = int(cols[3][0][10])
        # the caller's list: a duplicate, a user already in the column, users outside it
        free = np.setdiff1d(np.arange(n), cols[3][0])
        lists = [[], [5, 5], [int(cols[2][0][0]), 399], [int(free[0]), int(free[0]), int(cols[3][0][3])], [], [0, 399]]
        mptr, musers = _mask_csr(lists)
        for topn in (1, 10, 256):
            got = D.audience(items, topn, mptr, musers)
            _same(got, _want(S, csc, items, topn, lists), f"values={values} topn={topn}, list")
            _same(D.audience(items, topn), _want(S, csc, items, topn), f"values={values} topn={topn}, no list")
        # the stored 0 of item 3 is unmasked with values and masked without
        top = D.audience(items[3:4], 256)
        assert np.all(top[1][0] > 0)                                  # 335 users and more have a positive score
        assert top[0][0][0] == zero3 if values else zero3 not in top[0][0]
        # item 4: 100 (103 with values) users with a positive score, then its masked users at +0.0 in id order
        got = D.audience(items[4:5], 256)
        live = n - 300 + (3 if values else 0)
        masked = np.sort(cols[4][0][cols[4][1] > 0]) if values else cols[4][0]
        assert np.all(got[1][0][:live] > 0) and np.all(_bits(got[1][0][live:]) == 0)
        assert np.array_equal(got[0][0][live:], masked[:256 - live].astype(np.uint32))
    finally:
        D.close()


def test_a_long_column_is_walked_by_a_workgroup():
    """columns of 4095 and 4096 users stand on the two sides of AUDIENCE_LONG_MIN (hpf_kernels.hpp): a wave walks the one, a
    workgroup the other; an item with a list only, between them"""
    n, K = 4300, 5
    rng = np.random.default_rng(41)
    cols = []
    for L in (4095, 3, 4096, 4200):
        u = np.sort(rng.choice(n, L, replace=False))
        v = rng.integers(0, 3, L)                                     # a third of the stored ratings are 0
        cols.append((u, v))
    rowptr, col, val = _from_columns(n, cols)
    st = {"THETA_E": _gamma(n, K, 42), "BETA_E": _gamma(4, K, 43)}
    items = np.array([2, 0, 1, 3, 2], np.uint32)
    lists = [[0, 4299], [], [17], [1, 2, 3], []]
    mptr, musers = _mask_csr(lists)
    for values in (True, False):
        csr = (rowptr, col, val if values else None)
        D = _handle(n, 4, K, False, csr, st)
        try:
            S, csc = _all_scores(D), _csc(n, 4, csr)
            for topn in (10, 256):
                _same(D.audience(items, topn, mptr, musers), _want(S, csc, items, topn, lists), f"values={values} topn={topn}")
        finally:
            D.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. batches
# ---------------------------------------------------------------------------------------------------------------------
def _batch_case():
    """40 selected items whose columns are disjoint: a bit row that is not cleared between batches masks another item's users"""
    n, m, K = 600, 40, 33
    cols = [(np.arange(15 * i, 15 * i + 10), np.full(10, 1 + i % 5)) for i in range(m)]
    csr = _from_columns(n, cols)
    items = np.random.default_rng(5).permutation(m).astype(np.uint32)
    lists = [[(15 * int(i) + 12) % n] for i in items]
    return n, m, K, csr, _factors(n, m, K, True, 50), items, lists


_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from tests.test_gpu_audience import _batch_case, _handle, _mask_csr
n, m, K, csr, st, items, lists = _batch_case()
mptr, musers = _mask_csr(lists)
D = _handle(n, m, K, True, csr, st)
out = []
for topn in (10, 100, 256):
    users, sc = D.audience(items, topn, mptr, musers)
    out.append([users.tolist(), sc.view(np.uint64).tolist()])
D.close()
print("RESULT " + json.dumps(out))
"""


def test_batches_give_the_same_lists():
    """HPF_LOO_BATCH=16: the 40 selected items go through the kernels in three batches (16, 16, 8).  The library reads the
    variable when a handle is created, hence a fresh process."""
    env = dict(os.environ, HPF_LOO_BATCH="16")
    r = subprocess.run([sys.executable, "-c", _CHILD, str(ROOT)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][0][7:])
    n, m, K, csr, st, items, lists = _batch_case()
    mptr, musers = _mask_csr(lists)
    D = _handle(n, m, K, True, csr, st)
    try:
        S, csc = _all_scores(D), _csc(n, m, csr)
        for topn, (users, scbits) in zip((10, 100, 256), got):
            one = D.audience(items, topn, mptr, musers)
            _same(one, _want(S, csc, items, topn, lists), f"one batch, topn={topn}")
            assert np.array_equal(np.array(users, np.uint32), one[0]), topn
            assert np.array_equal(np.array(scbits, np.uint64), _bits(one[1])), topn
    finally:
        D.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. the call: a repeated item, nothing selected, every refusal of the header comment
# ---------------------------------------------------------------------------------------------------------------------
def test_call_level_cases_and_errors():
    n, m, K = 130, 20, 5
    csr = make_problem(n, m, 400, seed=9)
    st = _factors(n, m, K, True, 60)
    D = _handle(n, m, K, True, csr, st)
    u32p, u64p, dp = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_double)
    try:
        items = np.array([3, 7, 3, 19, 0], np.uint32)
        lists = [[1], [], [1], [2, 3], []]
        mptr, musers = _mask_csr(lists)
        want = _want(_all_scores(D), _csc(n, m, csr), items, 10, lists)
        got = D.audience(items, 10, mptr, musers)
        _same(got, want, "a repeated item")
        assert np.array_equal(got[0][0], got[0][2]) and np.array_equal(_bits(got[1][0]), _bits(got[1][2]))
        # n_sel = 0 is fine, also with null pointers
        e = D.audience(np.zeros(0, np.uint32), 10)
        assert e[0].shape == (0, 10) and e[1].shape == (0, 10)
        assert D.lib.hpf_audience(D._h, None, 0, None, None, 10, None, None) == 0
        # HPF_ERR_INVALID, each before anything is launched
        bad_items, bad_users, bad_ptr0, bad_ptr = items.copy(), musers.copy(), mptr.copy(), mptr.copy()
        bad_items[1] = m
        bad_users[-1] = n
        bad_ptr0[0] = 1
        bad_ptr[2] = bad_ptr[1] - 1
        for args, msg in (((items, 0, mptr, musers), "topn"), ((items, 257, mptr, musers), "topn"),
                          ((bad_items, 10, mptr, musers), "item index out of range"),
                          ((items, 10, mptr, bad_users), "mask user out of range"),
                          ((items, 10, bad_ptr0, musers), "mask_ptr[0]"), ((items, 10, bad_ptr, musers), "mask_ptr not monotone")):
            _raises(INVALID, lambda: D.audience(*args), msg)
        out_u, out_s = np.empty((5, 10), np.uint32), np.empty((5, 10), np.float64)
        pi, po, ps = items.ctypes.data_as(u32p), out_u.ctypes.data_as(u32p), out_s.ctypes.data_as(dp)
        for a in ((None, po, ps), (pi, None, ps), (pi, po, None)):
            assert D.lib.hpf_audience(D._h, a[0], 5, None, None, 10, a[1], a[2]) == INVALID
            assert b"null pointer" in D.lib.hpf_last_error(D._h)
        assert D.lib.hpf_audience(D._h, pi, 5, mptr.ctypes.data_as(u64p), None, 10, po, ps) == INVALID     # a list without its users
        _same(D.audience(items, 10, mptr, musers), want, "after the refused calls")
    finally:
        D.close()
    # HPF_ERR_STATE: no CSR, or no E on either side
    F = Hpf(n, m, K, hier=False, bias=False)
    try:
        sel = np.arange(3, dtype=np.uint32)
        _raises(STATE, lambda: F.audience(sel, 5))
        F.set_state("THETA_E", st["THETA_E"])
        F.set_state("BETA_E", st["BETA_E"])
        _raises(STATE, lambda: F.audience(sel, 5), "hpf_upload_csr")
        F.upload_csr(*csr)
        assert F.audience(sel, 5)[0].shape == (3, 5)
    finally:
        F.close()
    for missing in ("THETA_E", "BETA_E"):
        G = Hpf(n, m, K, hier=False, bias=False)
        try:
            G.upload_csr(*csr)
            G.set_state("BETA_E" if missing == "THETA_E" else "THETA_E", st["BETA_E" if missing == "THETA_E" else "THETA_E"])
            _raises(STATE, lambda: G.audience(np.arange(3, dtype=np.uint32), 5))
        finally:
            G.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. the handle with the sides exchanged: its hpf_recommend returns the same bits
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,bias", [(5, True), (33, False), (100, True)])
def test_the_transposed_handle_recommends_the_same_bits(K, bias):
    n, m = 700, 90
    csr = make_problem(n, m, 5000, seed=K)
    st = _factors(n, m, K, bias, 70 + K)
    rng = np.random.default_rng(K)
    items = rng.permutation(m)[:70].astype(np.uint32)
    lists = [np.sort(rng.choice(n, rng.integers(0, 4), replace=False)) for _ in items]
    mptr, musers = _mask_csr(lists)
    D = _handle(n, m, K, bias, csr, st)
    T = None
    try:
        colptr, usr, cval = D.get_csc()
        swapped = {"THETA_E": st["BETA_E"], "BETA_E": st["THETA_E"]}
        if bias:
            swapped.update(UBIAS_E=st["IBIAS_E"], IBIAS_E=st["UBIAS_E"])
        T = _handle(m, n, K, bias, (colptr, usr, cval), swapped)
        for topn in (10, 100, 256):
            _same(D.audience(items, topn, mptr, musers), T.recommend(items, topn, mptr, musers), f"K={K} bias={bias} topn={topn}")
    finally:
        D.close()
        if T is not None:
            T.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. state: nothing is written, and the call sees what hpf_get_state would export
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


@pytest.mark.parametrize("hier,bias", [(True, True), (False, False)])
def test_the_state_is_read_and_not_written(hier, bias):
    n, m, K = 300, 80, 20
    csr = make_problem(n, m, 4000, seed=3)
    items = np.random.default_rng(3).permutation(m).astype(np.uint32)
    A = _trained(n, m, K, hier, bias, csr, 2)
    B = _trained(n, m, K, hier, bias, csr, 2)
    R = None
    try:
        got = A.audience(items, 50)                                   # straight after hpf_iterate(2)
        states = compare_states(hier, bias)
        before = {w: B.get_state(w) for w in states}
        for w in states:
            assert np.array_equal(_bits(A.get_state(w)), _bits(before[w])), w
        _same(A.audience(items, 50), got, "a second call")
        # ... equals a call after exporting and importing E again
        R = Hpf(n, m, K, hier=hier, bias=bias)
        R.upload_csr(*csr)
        for w in ["THETA_E", "BETA_E"] + (["UBIAS_E", "IBIAS_E"] if bias else []):
            R.set_state(w, before[w])
        _same(got, R.audience(items, 50), "after export and import")
        _same(got, _want(_all_scores(R), _csc(n, m, csr), items, 50), "the oracle on the imported state")
        # an iteration after the call gives the bits it gives without it
        A.iterate(1)
        B.iterate(1)
        for w in states:
            assert np.array_equal(_bits(A.get_state(w)), _bits(B.get_state(w))), w
    finally:
        A.close()
        B.close()
        if R is not None:
            R.close()


@pytest.mark.parametrize("hier,bias", [(True, True), (False, False)])
def test_after_fold_in_items_the_folded_in_side_is_ranked(hier, bias):
    import tests.test_gpu_fold_in_items as fi
    n, m, K = fi.N1, fi.M1, fi.K1
    imajor, umajor = fi.make_items(n, fi.DEGS1, 81)
    users = fi.user_side(n, m, K, hier, bias, 82)
    D = fi.device(n, m, K, hier, bias, umajor, users)
    try:
        D.fold_in_items(5)
        items = np.arange(m, dtype=np.uint32)
        got = D.audience(items, 20)                                   # straight after hpf_fold_in_items
        Eb = D.get_state("BETA_E")
        _same(got, _want(_all_scores(D), _csc(n, m, umajor), items, 20), "against hpf_scores")
        sc = Eb @ users["THETA_E"].T
        if bias:
            sc = sc + D.get_state("IBIAS_E")[:, None] + users["UBIAS_E"][None, :]
        live = got[1] > 0
        ref = np.take_along_axis(sc, np.where(got[0] == NONE, 0, got[0]).astype(np.int64), 1)
        assert live.any() and np.all(np.abs(got[1][live] - ref[live]) <= 1e-12 * ref[live])
    finally:
        D.close()
