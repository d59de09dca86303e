"""-m gpu: hpf_sample_state and hpf_recommend_thompson -- one draw of the model from its Gamma posterior and the top-N of
that draw (gamma_rows_kernel, sample_pack_kernel, then the unchanged topn_sweep_kernel / topn_merge_kernel).

The sampler's oracle is tests/thompson_ref.py, the numpy statement of hgaprec_amd/csrc/hpf_rng.hpp: every element within
(32 + 16 / (1 + w) + 4 |log(u4) / a|) 2^-52 of it, and -- independent of it -- the Kolmogorov-Smirnov distance of a column
from the Gamma distribution.  The lists' oracle is hpf_recommend on a second handle whose E are the sampled rows: items and
scores bit for bit."""
import numpy as np
import pytest

from hgaprec_amd.capi import Hpf, HpfError
from tests import thompson_ref as ref
from tests.thompson_ref import bits
from tests.util import compare_states, init_states, make_problem

pytestmark = pytest.mark.gpu
INVALID, UNSUPPORTED, STATE = -1, -5, -6
NONE = 0xFFFFFFFF
SEED, DRAW = ref.SEED, ref.DRAW


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
    D = Hpf(n, m, K, hier=False, bias=bias, binary=csr is not None and csr[2] is None)
    if csr is not None:
        D.upload_csr(*csr)
    for w, a in st.items():
        D.set_state(w, a)
    return D


def _all(n):
    return np.arange(n, dtype=np.uint32)


def _names(bias):
    return ["THETA_E", "THETA_SHAPE", "BETA_E", "BETA_SHAPE"] + (["UBIAS_E", "UBIAS_SHAPE", "IBIAS_E", "IBIAS_SHAPE"] if bias else [])


def _exports(D, bias):
    return {w: D.get_state(w) for w in _names(bias)}


def _as_E(theta, beta, K, bias):
    """the two hpf_sample_state outputs as the E arrays of a handle"""
    st = {"THETA_E": np.ascontiguousarray(theta[:, :K]), "BETA_E": np.ascontiguousarray(beta[:, :K])}
    if bias:
        st.update(UBIAS_E=np.ascontiguousarray(theta[:, K]), IBIAS_E=np.ascontiguousarray(beta[:, K]))
    return st


def _mask_csr(lists):
    mptr = np.zeros(len(lists) + 1, np.uint64)
    mptr[1:] = np.cumsum([len(x) for x in lists])
    return mptr, np.concatenate([np.asarray(x, np.uint32) for x in lists] + [np.zeros(0, np.uint32)]).astype(np.uint32)


def _mask_lists(n_sel, m, seed):
    rng = np.random.default_rng(seed)
    lists = [np.sort(rng.choice(m, rng.integers(0, 6), replace=False)) if b % 3 else [] for b in range(n_sel)]
    lists[5] = np.arange(m)                                     # every item masked: the list is items 0 .. at +0.0
    return lists


def _lists_by_construction(D, K, bias, csr, seed, draw):
    """a second handle with the same CSR whose E are D's two hpf_sample_state outputs"""
    theta, beta = D.sample_state(0, seed, draw), D.sample_state(1, seed, draw)
    return _handle(theta.shape[0], beta.shape[0], K, bias, csr, _as_E(theta, beta, K, bias)), theta, beta


# ---------------------------------------------------------------------------------------------------------------------
# 1. values against the numpy statement of the sampler
# ---------------------------------------------------------------------------------------------------------------------
VALUE_CASES = [(5, True), (100, False)]


@pytest.mark.parametrize("K,bias", VALUE_CASES)
def test_values_against_the_reference(K, bias):
    """observed on an MI355X: see DESIGN.md section 4k for the largest error / bound"""
    n, m = 257, 130
    st = ref.value_case(K, bias, n, m)
    D = _handle(n, m, K, bias, None, st)
    try:
        worst = 0.0
        for side, (want, tr, shapes) in enumerate(ref.reference_sides(st, K, bias, SEED, DRAW)):
            got = D.sample_state(side, SEED, DRAW)
            assert got.shape == want.shape == (n if side == 0 else m, K + bias)
            # the precondition (tests/test_thompson_ref.py asserts it without a GPU): no decision near its edge
            assert np.all(tr["attempt"] >= 0) and tr["ratio"].min() >= ref.MARGIN_MIN and np.abs(tr["t"]).min() >= ref.T_MIN
            assert np.all(np.isfinite(got)) and np.all(got >= 0.0) and not np.any(np.signbit(got))
            E = np.hstack([st["THETA_E" if side == 0 else "BETA_E"]] + ([st["UBIAS_E" if side == 0 else "IBIAS_E"][:, None]] if bias else []))
            assert (E == 0.0).sum() >= 1 and np.all(bits(got[E == 0.0]) == 0), "E = +0.0 gives +0.0"
            live = E != 0.0
            tiny = live & (want < 2.0 ** -1000)                  # they would be compared as "both below 2^-990"
            assert tiny.mean() == 0.0 and np.all(want[live] > 0.0), "reference values below 2^-1000 on these inputs"
            rel = np.abs(got[live] - want[live]) / want[live]
            b = ref.bound(tr, shapes)[live]
            r = float((rel / b).max())
            worst = max(worst, r)
            print(f"K={K} bias={bias} side={side}: max error / bound = {r:.4f}, max error = {rel.max() / ref.U:.2f} x 2^-52, "
                  f"bit-equal share {np.mean(bits(got) == bits(want)):.4f}")
            bad = np.flatnonzero(rel > b)
            assert bad.size == 0, (side, bad[:5], rel[bad[:5]] / ref.U, b[bad[:5]] / ref.U)
        print(f"K={K} bias={bias}: worst error / bound {worst:.4f}")
    finally:
        D.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the distribution, independent of the reference
# ---------------------------------------------------------------------------------------------------------------------
def test_distribution_of_a_column_per_shape():
    shapes = np.array(ref.KS_SHAPES)
    n, m, K = ref.KS_DRAWS, 16, len(shapes)
    S = np.tile(shapes, (n, 1))
    st = {"THETA_E": S.copy(), "THETA_SHAPE": S, "BETA_E": np.ones((m, K)), "BETA_SHAPE": np.ones((m, K))}      # E / shape = 1: the sample is g
    D = _handle(n, m, K, False, None, st)
    try:
        g = D.sample_state(0, 99, 3)
        for j, a in enumerate(shapes):
            d = ref.ks_distance(g[:, j], a)
            mean = g[:, j].mean() / a
            print(f"shape {a:g}: KS distance {d:.4f} (cap {ref.KS_CAP:.4f}), sample mean / a = {mean:.5f}")
            assert d <= ref.KS_CAP, (a, d)
            assert abs(mean - 1.0) <= 6.0 / np.sqrt(a * n), (a, mean)
        z = (g - g.mean(0)) / g.std(0)
        for j in range(K - 1):                                   # adjacent columns and adjacent rows: independent streams
            assert abs(np.mean(z[:, j] * z[:, j + 1])) <= 6.0 / np.sqrt(n), j
        for j in range(K):
            assert abs(np.mean(z[:-1, j] * z[1:, j])) <= 6.0 / np.sqrt(n), j
    finally:
        D.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the lists, exact: hpf_recommend of a handle whose E are the sampled rows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,bias,n,m", [(5, True, 257, 130), (100, False, 257, 130), (5, True, 70, 700)])
def test_lists_equal_recommend_on_the_sampled_rows(K, bias, n, m):
    """m = 130: three tiles, topn = 256 > m pads; m = 700: two splits at topn <= 64 and compactions"""
    st = ref.value_case(K, bias, n, m)
    csr = make_problem(n, m, 6 * n, seed=K + m)
    users = np.random.default_rng(K).permutation(n).astype(np.uint32)
    lists = _mask_lists(n, m, K + 1)
    mptr, mitems = _mask_csr(lists)
    D = _handle(n, m, K, bias, csr, st)
    H, theta, beta = _lists_by_construction(D, K, bias, csr, SEED, 2)
    try:
        assert D.work_info()["ld"] % 2 == 0
        for topn in (1, 64, 256):
            it, sc = D.recommend_thompson(users, topn, SEED, 2, mptr, mitems)
            wit, wsc = H.recommend(users, topn, mptr, mitems)
            _eq(it, wit, f"K={K} bias={bias} m={m} topn={topn}, mask list: items")
            _eq(sc, wsc, f"K={K} bias={bias} m={m} topn={topn}, mask list: scores")
            it, sc = D.recommend_thompson(users, topn, SEED, 2)
            wit, wsc = H.recommend(users, topn)
            _eq(it, wit, f"K={K} bias={bias} m={m} topn={topn}: items")
            _eq(sc, wsc, f"K={K} bias={bias} m={m} topn={topn}: scores")
            if topn > m:
                assert np.all(it[:, m:] == NONE) and np.all(bits(sc[:, m:]) == 0) and np.all(it[:, :m] < m)
            # the scores are those of the draw: theta~ . beta~ (+ the biases), not the posterior mean's
            b = 9
            u, i = int(users[b]), int(it[b, 0])
            s = float(theta[u, :K] @ beta[i, :K]) + (float(theta[u, K] + beta[i, K]) if bias else 0.0)
            assert abs(sc[b, 0] - s) <= 1e-12 * s
        it, sc = D.recommend_thompson(users, 64, SEED, 2, mptr, mitems)
        assert np.array_equal(it[5], np.arange(min(64, m), dtype=np.uint32)) and np.all(bits(sc[5]) == 0)      # all masked
        # and they differ from the mean's lists: a draw is not the mean
        mi, _ = D.recommend(users, 64, mptr, mitems)
        assert np.mean(mi != it) > 0.2
    finally:
        D.close()
        H.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. a draw is a function of (seed, draw, row, column) only
# ---------------------------------------------------------------------------------------------------------------------
def test_a_draw_does_not_depend_on_batches_selection_or_order(monkeypatch):
    K, bias, n, m = 5, True, 70, 130
    st = ref.value_case(K, bias, n, m)
    csr = make_problem(n, m, 6 * n, seed=3)
    users = np.random.default_rng(8).permutation(n).astype(np.uint32)
    lists = _mask_lists(n, m, 4)
    mptr, mitems = _mask_csr(lists)
    D = _handle(n, m, K, bias, csr, st)
    try:
        one = D.recommend_thompson(users, 20, 7, 1, mptr, mitems)
        theta, beta = D.sample_state(0, 7, 1), D.sample_state(1, 7, 1)
        for knob in (16, 48):                                     # five batches, two batches
            monkeypatch.setenv("HPF_LOO_BATCH", str(knob))        # read when the handle is created
            B = _handle(n, m, K, bias, csr, st)
            try:
                got = B.recommend_thompson(users, 20, 7, 1, mptr, mitems)
                _eq(got[0], one[0], f"HPF_LOO_BATCH={knob}: items")
                _eq(got[1], one[1], f"HPF_LOO_BATCH={knob}: scores")
            finally:
                B.close()
        monkeypatch.delenv("HPF_LOO_BATCH")
        # a subset, in another order, a user twice: the rows of the full selection
        pick = np.array([40, 3, 40, 69, 0, 17], np.int64)
        sub, (sptr, sitems) = users[pick], _mask_csr([lists[b] for b in pick])
        got = D.recommend_thompson(sub, 20, 7, 1, sptr, sitems)
        _eq(got[0], one[0][pick], "a subset: items")
        _eq(got[1], one[1][pick], "a subset: scores")
        again = D.recommend_thompson(users, 20, 7, 1, mptr, mitems)
        _eq(again[0], one[0], "the same call twice: items")
        _eq(again[1], one[1], "the same call twice: scores")
        _eq(D.sample_state(0, 7, 1), theta, "the same sample twice")
        # another draw, another seed (low or high half): another sample
        for seed, draw in ((7, 2), (8, 1), (7 + (1 << 32), 1)):
            t2 = D.sample_state(0, seed, draw)
            assert np.mean(bits(t2) == bits(theta)) < 0.01 + np.mean(theta == 0.0), (seed, draw)      # (E = +0.0 gives +0.0 in every draw)
            assert not np.array_equal(D.recommend_thompson(users, 20, seed, draw, mptr, mitems)[0], one[0])
        # ids: the rows of the call without
        ids = np.array([69, 0, 5, 5, 33], np.uint32)
        _eq(D.sample_state(0, 7, 1, ids), theta[ids.astype(np.int64)], "ids, users")
        _eq(D.sample_state(1, 7, 1, ids), beta[ids.astype(np.int64)], "ids, items")
        _eq(D.sample_state(1, 7, 1, n_sel=17), beta[:17], "the first rows")
    finally:
        D.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. state: not written; after hpf_iterate and after hpf_fold_in the calls are those of the exported E and shapes
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


def _check_against_exports(D, K, bias, csr, users, got_lists, got_theta, got_beta, seed, draw, what):
    """a fresh handle handed D's exported E and shapes makes the same calls"""
    st = _exports(D, bias)
    F = _handle(st["THETA_E"].shape[0], st["BETA_E"].shape[0], K, bias, csr, st)
    try:
        _eq(got_theta, F.sample_state(0, seed, draw), what + ": theta~")
        _eq(got_beta, F.sample_state(1, seed, draw), what + ": beta~")
        want = F.recommend_thompson(users, got_lists[0].shape[1], seed, draw)
        _eq(got_lists[0], want[0], what + ": items")
        _eq(got_lists[1], want[1], what + ": scores")
    finally:
        F.close()
    assert np.all(np.isfinite(got_theta)) and np.all(got_theta >= 0) and got_theta.max() > 0


@pytest.mark.parametrize("hier,bias", [(True, True), (False, False)])
def test_straight_after_an_iteration_and_the_state_is_not_written(hier, bias):
    n, m, K = 300, 80, 20
    csr = make_problem(n, m, 4000, seed=3)
    users = np.random.default_rng(4).permutation(n)[:100].astype(np.uint32)
    A = _trained(n, m, K, hier, bias, csr, 2)
    B = _trained(n, m, K, hier, bias, csr, 2)
    try:
        lists = A.recommend_thompson(users, 20, 11, 0)                # straight after hpf_iterate(2): S holds raw sums
        theta, beta = A.sample_state(0, 11, 0), A.sample_state(1, 11, 0)
        states = compare_states(hier, bias)
        for w in states:
            _eq(A.get_state(w), B.get_state(w), w)
        _check_against_exports(A, K, bias, csr, users, lists, theta, beta, 11, 0, f"hier={hier} bias={bias}")
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
        lists = D.recommend_thompson(users, 10, 5, 4)                 # straight after hpf_fold_in: the fold-in left shapes
        theta, beta = D.sample_state(0, 5, 4), D.sample_state(1, 5, 4)
        _check_against_exports(D, K, bias, (rowptr, col, val), users, lists, theta, beta, 5, 4, f"fold-in hier={hier} bias={bias}")
    finally:
        D.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. errors: each refused on the host before a launch; the handle stays usable
# ---------------------------------------------------------------------------------------------------------------------
def test_errors():
    n, m, K = 70, 90, 5
    csr = make_problem(n, m, 400, seed=9)
    st = ref.value_case(K, True, n, m)
    D = _handle(n, m, K, True, csr, st)
    try:
        users = np.array([3, 7, 3, 69, 0], np.uint32)
        mptr, mitems = _mask_csr([[1], [], [1], [2, 3], []])
        want = D.recommend_thompson(users, 10, 1, 0, mptr, mitems)
        _eq(want[0][0], want[0][2], "a repeated user: items")
        _eq(want[1][0], want[1][2], "a repeated user: scores")
        e = D.recommend_thompson(np.zeros(0, np.uint32), 10, 1, 0)
        assert all(a.shape == (0, 10) for a in e)
        assert D.lib.hpf_recommend_thompson(D._h, None, 0, None, None, 10, 1, 0, None, None) == 0
        assert D.lib.hpf_sample_state(D._h, 0, None, 0, 1, 0, None) == 0
        bad_users, bad_items, bad_ptr0, bad_ptr = users.copy(), mitems.copy(), mptr.copy(), mptr.copy()
        bad_users[1] = n
        bad_items[-1] = m
        bad_ptr0[0] = 1
        bad_ptr[2] = bad_ptr[1] - 1
        for args, msg in (((users, 0, 1, 0, mptr, mitems), "topn"), ((users, 257, 1, 0, mptr, mitems), "topn"),
                          ((bad_users, 10, 1, 0, mptr, mitems), "user index out of range"),
                          ((users, 10, 1, 0, mptr, bad_items), "mask item out of range"),
                          ((users, 10, 1, 0, bad_ptr0, mitems), "mask_ptr[0]"), ((users, 10, 1, 0, bad_ptr, mitems), "mask_ptr not monotone")):
            _raises(INVALID, lambda: D.recommend_thompson(*args), msg)
            assert msg.encode() in D.lib.hpf_last_error(D._h)
        for side in (2, -1):
            _raises(INVALID, lambda: D.sample_state(side, 1, 0, n_sel=3), "side is 0 (users) or 1 (items)")
        _raises(INVALID, lambda: D.sample_state(0, 1, 0, np.array([0, n], np.uint32)), "user index out of range")
        _raises(INVALID, lambda: D.sample_state(1, 1, 0, np.array([m], np.uint32)), "item index out of range")
        _raises(INVALID, lambda: D.sample_state(1, 1, 0, n_sel=m + 1), "item index out of range")
        assert D.lib.hpf_sample_state(D._h, 0, None, 3, 1, 0, None) == INVALID
        got = D.recommend_thompson(users, 10, 1, 0, mptr, mitems)
        _eq(got[0], want[0], "after the refused calls: items")
        _eq(got[1], want[1], "after the refused calls: scores")
    finally:
        D.close()
    # HPF_ERR_STATE: a fresh handle with E but no shape
    sel = np.arange(3, dtype=np.uint32)
    st = ref.value_case(K, False, n, m)
    F = Hpf(n, m, K, hier=False, bias=False)
    try:
        F.upload_csr(*csr)
        for w in ("THETA_E", "BETA_E"):
            F.set_state(w, st[w])
        _raises(STATE, lambda: F.recommend_thompson(sel, 5, 1, 0), "THETA_SHAPE")
        _raises(STATE, lambda: F.sample_state(0, 1, 0), "THETA_SHAPE")
        assert F.recommend(sel, 5)[0].shape == (3, 5)                 # usable: E is there
        for w in ("THETA_SHAPE", "BETA_SHAPE"):
            F.set_state(w, st[w])
        assert F.recommend_thompson(sel, 5, 1, 0)[0].shape == (3, 5)
    finally:
        F.close()
    # no CSR: the sample needs none, the lists do
    G = Hpf(n, m, K, hier=False, bias=False)
    try:
        for w in _names(False):
            G.set_state(w, st[w])
        assert G.sample_state(1, 1, 0).shape == (m, K)
        _raises(STATE, lambda: G.recommend_thompson(sel, 5, 1, 0), "hpf_upload_csr")
    finally:
        G.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. tiny shapes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a", [1e-3, 1e-6])
def test_tiny_shapes(a):
    """u^(1 / a) underflows for most elements: zeros are allowed, nothing else than finite and >= +0.0"""
    K, bias, n, m = 5, True, 70, 130
    st = ref.value_case(K, bias, n, m)
    for w in st:
        if w.endswith("_SHAPE"):
            st[w][...] = a
    csr = make_problem(n, m, 6 * n, seed=5)
    D = _handle(n, m, K, bias, csr, st)
    H, theta, beta = _lists_by_construction(D, K, bias, csr, 3, 0)
    try:
        for x in (theta, beta):
            assert np.all(np.isfinite(x)) and np.all(x >= 0.0) and not np.any(np.signbit(x))
        print(f"a={a:g}: share of zeros {np.mean(theta == 0):.3f} (users), {np.mean(beta == 0):.3f} (items)")
        users = _all(n)
        for topn in (10, 256):
            got, want = D.recommend_thompson(users, topn, 3, 0), H.recommend(users, topn)
            _eq(got[0], want[0], f"a={a:g} topn={topn}: items")
            _eq(got[1], want[1], f"a={a:g} topn={topn}: scores")
    finally:
        D.close()
        H.close()
