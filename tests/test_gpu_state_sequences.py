"""-m gpu: laziness must not be observable (tests/statemodel.py).

The library keeps its model lazily: what a call finds pending depends on the calls before it.  Here the same
operations run on the oracle (independent arrays: the semantics), on a handle that does exactly them, and on a twin
that exports everything after every operation so that nothing is ever pending on it.  lazy and twin agree bit for bit;
both agree with the oracle at the bars of tests/test_gpu_parity.py.  test_random_call_orders draws what the library
could do when the model was written; test_random_serving_call_orders adds the two fold-ins, which write a whole side, and
every scoring call (lists and ranks against numpy on the oracle's arrays through tests/toplist.py).  The directed tests pin
the call orders the random ones led to: the first consumer after a fall-back from the packed rows, a refused call, an
export before a set, a snapshot taken before the first sweep."""
import ctypes as C

import numpy as np
import pytest

from tests import statemodel as sm
from tests.test_state_sequences_host import PACKED_SEEDS, SERVING_PACKED, SERVING_SEEDS, STATE_SEEDS
from tests.util import compare_states, copy_state, heldout_pairs, init_states, make_problem, rel_err

pytestmark = pytest.mark.gpu

RTOL = sm.RTOL


@pytest.mark.parametrize("seed", STATE_SEEDS)
def test_random_call_orders(orc, monkeypatch, seed):
    config, ops = sm.sequence(seed)
    sm.set_env(monkeypatch, config)
    lazy, twin, _ = sm.run_three(orc, config, ops, f"seed {seed}")
    lazy.close(); twin.close()


@pytest.mark.parametrize("seed", PACKED_SEEDS)
def test_random_call_orders_around_a_fall_back(orc, monkeypatch, seed):
    """K = 100 in packed rows, and somewhere in the sequence a user sweep that cannot pack its rows inside a call of two
    iterations: whatever comes next is the first consumer after the fall-back"""
    config, ops = sm.sequence(seed)
    ops = sm.with_fall_back(seed, ops)
    sm.set_env(monkeypatch, config)
    lazy, twin, _ = sm.run_three(orc, config, ops, f"seed {seed} (packed)")
    try:
        for D in (lazy.D, twin.D):
            wi = D.work_info()
            assert wi["w_fallbacks"] == 1 and wi["w_layout"] == 4, (seed, wi)
    finally:
        lazy.close(); twin.close()


@pytest.mark.parametrize("seed", SERVING_SEEDS)
def test_random_serving_call_orders(orc, monkeypatch, seed):
    """the fold-ins and the scoring calls among the operations of test_random_call_orders: whatever a call returns is the
    same bits on lazy and twin, and within 1e-9 of numpy on the oracle's arrays (prints the worst error per call)"""
    config, ops = sm.serving_sequence(seed)
    sm.set_env(monkeypatch, config)
    lazy, twin, _ = sm.run_three(orc, config, ops, f"serving seed {seed}")
    lazy.close(); twin.close()


@pytest.mark.parametrize("seed", SERVING_PACKED)
def test_random_serving_call_orders_around_a_fall_back(orc, monkeypatch, seed):
    """the serving sequences whose config is K = 100 in packed rows, with the fall-back of
    test_random_call_orders_around_a_fall_back woven in: a fold-in or a scoring call may be its first consumer"""
    config, ops = sm.serving_sequence(seed)
    ops = sm.with_fall_back(seed, ops)
    sm.set_env(monkeypatch, config)
    lazy, twin, _ = sm.run_three(orc, config, ops, f"serving seed {seed} (packed)")
    try:
        for D in (lazy.D, twin.D):
            wi = D.work_info()
            assert wi["w_fallbacks"] == 1 and wi["w_layout"] == 4, (seed, wi)
    finally:
        lazy.close(); twin.close()


# ---- the first consumer after a fall-back ---------------------------------------------------------------------------------

def _held(n, m):
    return heldout_pairs(n, m, 200, seed=5)


def _scenario(orc, which):
    """-> (M, D, P, dims): the oracle, a packing handle on which the fall-back is due or done, a w_storage = 3 handle
    after the same calls.  A: test_default_packs_k100_rows_and_falls_back_when_a_state_does_not_fit (the THETA_ELOG
    column - 120 handed in mid-run), B: test_a_sweep_that_cannot_pack_its_row_... (BETA_E[:, 0] = 1e40, four iterations
    in one call)."""
    from hgaprec_amd.capi import Hpf
    if which == "A":
        n, m, K, prob = 200, 150, 100, make_problem(200, 150, 4000, 3)
        seed = 3
    else:
        n, m, K, prob = 300, 200, 100, make_problem(300, 200, 8000, 7, heavy_item=True)
        seed = 7
    M = orc.Model(n, m, K, True, False, False)
    M.set_csr(*prob); M.initialize(seed)
    if which == "B":
        be = M.state("BETA_E").copy()
        be[:, 0] = 1e40
        M.set_state("BETA_E", be)
    D, P = (Hpf(n, m, K, hier=True, w_storage=ws) for ws in (0, 3))
    for X in (D, P):
        X.upload_csr(*prob)
        X.heldout_bind(0, *_held(n, m))
        copy_state(M, X, True, False)
    assert D.work_info()["w_layout"] == 3 and P.work_info()["w_layout"] == 4
    if which == "A":
        D.iterate(2); M.iterate(2)
        st = {w: D.get_state(w) for w in init_states(True, False)}
        st["THETA_ELOG"][:, 0] -= 120.0
        for X in (D, P, M):
            for w, v in st.items():
                X.set_state(w, v)
        D.iterate(3); P.iterate(3); M.iterate(3)
    else:
        D.iterate(4); P.iterate(4); M.iterate(4)
    return M, D, P, (n, m, K, prob)


def _get(w):
    def run(M, D, P, dims):
        a, b = D.get_state(w), P.get_state(w)
        assert sm.same_bits(a, b), w
        assert sm.oracle_error(w, a, M.state(w)) < RTOL, (w, sm.oracle_error(w, a, M.state(w)))
        return D, P
    return run


def _get_device(w):
    def run(M, D, P, dims):
        a, b = D.get_state_device(w).cpu().numpy(), P.get_state_device(w).cpu().numpy()
        assert sm.same_bits(a, b), w
        assert sm.oracle_error(w, a, M.state(w)) < RTOL, (w, sm.oracle_error(w, a, M.state(w)))
        return D, P
    return run


def _exchange_read(M, D, P, dims):
    a, b = D.exchange_read(), P.exchange_read()
    assert sm.same_bits(a, b), int(np.sum(a != b))
    return D, P


def _heldout(bound):
    def run(M, D, P, dims):
        held = _held(dims[0], dims[1])
        a, b = (X.heldout_ll_bound(0) if bound else X.heldout_ll(*held) for X in (D, P))
        assert a == b, (a, b)
        assert a[1] == held[0].size and abs(a[0] - M.heldout_sum(*held)) / a[1] < 1e-9, (a, M.heldout_sum(*held))
        return D, P
    return run


def _elbo(M, D, P, dims):
    a, b, ref = D.elbo(), P.elbo(), M.elbo()
    assert a == b, (a, b)
    assert abs(a - ref) <= 1e-10 * abs(ref), (a, ref)
    return D, P


def _predict(M, D, P, dims):
    pu, pi, _ = heldout_pairs(dims[0], dims[1], 50, seed=6)
    a, b = D.predict(pu, pi), P.predict(pu, pi)
    assert sm.same_bits(a, b)
    assert rel_err(a, sm.oracle_predict(M, False, pu, pi)) < 1e-9
    return D, P


def _snapshot_restore(M, D, P, dims):
    from hgaprec_amd.capi import Hpf
    n, m, K, prob = dims
    out = []
    for X, ws in ((D, 0), (P, 3)):
        blob = X.snapshot()
        F = Hpf(n, m, K, hier=True, w_storage=ws)
        F.upload_csr(*prob)
        F.restore(blob)
        X.close()
        out.append(F)
    return out


def _refused_set_state(M, D, P, dims):
    from hgaprec_amd.capi import STATE
    buf = np.full(dims[0] * dims[2] + 8, 0.5)
    for X in (D, P):
        rc = X.lib.hpf_set_state(X._h, STATE["THETA_E"], buf.ctypes.data_as(C.POINTER(C.c_double)), dims[0] * dims[2] + 1)
        assert rc == -1
    return D, P


def _iterate(M, D, P, dims):
    D.iterate(1); P.iterate(1); M.iterate(1)
    return D, P


def _same_on_both(call):
    """a scoring call as the first consumer: everything it returns, bit for bit on both handles"""
    def run(M, D, P, dims):
        a, b = call(D, dims), call(P, dims)
        a, b = (a, b) if isinstance(a, tuple) else ((a,), (b,))
        assert len(a) == len(b) and all(x.size for x in a)
        for k, (x, y) in enumerate(zip(a, b)):
            assert sm.same_bits(x, y), (k, int(np.sum(x != y)))
        return D, P
    return run


def _users(dims):
    return np.array([0, 7, dims[0] // 2, dims[0] - 1], dtype=np.uint32)


def _queries(dims):
    """two queried items for each of _users -> (q_ptr, q_items)"""
    q = (np.arange(8, dtype=np.uint32) * 37 + 5) % dims[1]
    return np.arange(0, 9, 2, dtype=np.uint64), q.astype(np.uint32)


def _pairs(dims):
    return heldout_pairs(dims[0], dims[1], 6, seed=8)[:2]


SCORING_CONSUMERS = {
    "scores": lambda X, d: X.scores(_users(d)),
    "rank_topn": lambda X, d: X.rank_topn(_users(d), topn=10),
    "item_ranks": lambda X, d: X.item_ranks(_users(d), np.repeat(np.arange(4, dtype=np.uint32), 2), _queries(d)[1]),
    "loo_ranks": lambda X, d: X.loo_ranks(_users(d), _queries(d)[1][:4]),
    "rank_queries": lambda X, d: X.rank_queries(_users(d), *_queries(d)),
    "recommend": lambda X, d: X.recommend(_users(d), topn=10),
    "similar_users": lambda X, d: X.similar(0, _users(d), 10),
    "similar_items": lambda X, d: X.similar(1, _queries(d)[1][:4], 10),
    "explain": lambda X, d: X.explain(*_pairs(d), 4),
    "factor_top_users": lambda X, d: X.factor_top(0, 10),
    "factor_top_items": lambda X, d: X.factor_top(1, 10),
    "audience": lambda X, d: X.audience(_queries(d)[1][:4], topn=10),
    "because": lambda X, d: X.because(_users(d), *_queries(d), 4),
    "score_moments": lambda X, d: X.score_moments(*_pairs(d)),
    "recommend_ucb": lambda X, d: X.recommend_ucb(_users(d), topn=10, z=1.5),
}


def _fold(items):
    """a fold-in as the first consumer: the whole side replaced on both handles and in the oracle (the final comparison
    of the test holds all three together)"""
    def run(M, D, P, dims):
        n, m, K, prob = dims
        a, b = ((X.fold_in_items if items else X.fold_in)(2, 0.0) for X in (D, P))
        assert np.array_equal(a, b) and np.all(a == 2)
        sm.oracle_fold_into(M, n, m, K, True, False, prob, items, 2)
        return D, P
    return run


CONSUMERS = {
    "THETA_RATE": _get("THETA_RATE"), "BETA_RATE": _get("BETA_RATE"), "XI_E": _get("XI_E"), "XI_RATE": _get("XI_RATE"),
    "XI_ELOG": _get("XI_ELOG"), "ETA_E": _get("ETA_E"), "THETA_E": _get("THETA_E"), "BETA_ELOG": _get("BETA_ELOG"),
    "THETA_RATE_device": _get_device("THETA_RATE"), "exchange_read": _exchange_read, "heldout_ll": _heldout(False),
    "heldout_ll_bound": _heldout(True), "elbo": _elbo, "predict": _predict, "snapshot_restore": _snapshot_restore,
    "refused_set_state": _refused_set_state, "iterate": _iterate, "fold_in": _fold(False), "fold_in_items": _fold(True),
}
CONSUMERS.update({name: _same_on_both(call) for name, call in SCORING_CONSUMERS.items()})


@pytest.mark.parametrize("consumer", list(CONSUMERS))
@pytest.mark.parametrize("scenario", ["A", "B-graph0", "B-graph1"])
def test_first_consumer_after_a_fall_back(orc, monkeypatch, scenario, consumer):
    """Whatever is called first after a fall-back is due sees the state of the last iteration the call returned for:
    the w_storage = 3 handle's bits, the oracle's values.  (One rank does not look at the flag before an iteration, so
    in B the call has returned with three iterations skipped.)"""
    if scenario != "A":
        monkeypatch.setenv("HPF_EXPERIMENTAL", "1")
        monkeypatch.setenv("HPF_GRAPH", scenario[-1])
    M, D, P, dims = _scenario(orc, scenario[0])
    try:
        D, P = CONSUMERS[consumer](M, D, P, dims)
        for w in compare_states(True, False):
            a = D.get_state(w)
            assert sm.same_bits(a, P.get_state(w)), (scenario, consumer, w)
            e = sm.oracle_error(w, a, M.state(w))
            assert e < RTOL, (scenario, consumer, w, e)
        wd, wp = D.work_info(), P.work_info()
        assert wd["w_fallbacks"] == 1 and wd["w_layout"] == 4 and wp["w_fallbacks"] == 0, (wd, wp)
    finally:
        D.close(); P.close()


# ---- a snapshot before the first sweep hides nothing -------------------------------------------------------------------

def _same_answer(call, A, B, what):
    """a call on two handles: the same status and message, or the same bits"""
    from hgaprec_amd.capi import HpfError
    out = []
    for X in (A, B):
        try:
            r = call(X)
            out.append(r if isinstance(r, tuple) else (r,))
        except HpfError as e:
            out.append(str(e))
    a, b = out
    if isinstance(a, str) or isinstance(b, str):
        assert a == b, f"{what}: the old handle answers {a if isinstance(a, str) else 'HPF_OK'!r}, the restored one {b if isinstance(b, str) else 'HPF_OK'!r}"
    else:
        assert sm.same_results(a, b), f"{what}: the old and the restored handle return different bits"
    return a


@pytest.mark.parametrize("fold", ["fold_in", "fold_in_items"])
@pytest.mark.parametrize("hier", [False, True], ids=["flat", "hier"])
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
def test_a_snapshot_before_the_first_sweep_hides_nothing(orc, bias, hier, fold):
    """A fresh handle is handed E, Elog and the shapes and folds one side in; then snapshot, restore into a fresh handle
    with the same CSR.  Every export of compare_states, the bias rates, score_moments, because and recommend_ucb answer
    alike on the old and on the restored handle -- the same status and message, or the same bits -- and what the fold-in
    left exportable (the shapes and rates of its side, the moments) is answered, not refused."""
    from hgaprec_amd.capi import Hpf
    n, m, K = 150, 120, 21
    prob = make_problem(n, m, 3000, 11)
    M = orc.Model(n, m, K, hier, bias, False)
    M.set_csr(*prob); M.initialize(11)
    users, pairs = _users((n, m)), _pairs((n, m))
    q_ptr, q_items = _queries((n, m))
    old, new = Hpf(n, m, K, hier=hier, bias=bias), Hpf(n, m, K, hier=hier, bias=bias)
    try:
        for X in (old, new):
            X.upload_csr(*prob)
        copy_state(M, old, hier, bias)
        getattr(old, fold)(2, 0.0)
        new.restore(old.snapshot())
        mine = ("THETA", "XI", "UBIAS") if fold == "fold_in" else ("BETA", "ETA", "IBIAS")
        for w in compare_states(hier, bias):
            r = _same_answer(lambda X: X.get_state(w), old, new, w)
            if w.split("_")[0] in mine:
                assert not isinstance(r, str), f"{w} after {fold}: {r}"
        calls = {"score_moments": lambda X: X.score_moments(*pairs), "because": lambda X: X.because(users, q_ptr, q_items, 4),
                 "recommend_ucb": lambda X: X.recommend_ucb(users, topn=10, z=1.5), "recommend": lambda X: X.recommend(users, topn=10)}
        for name, call in calls.items():
            r = _same_answer(call, old, new, name)
            assert not isinstance(r, str), f"{name} after {fold}: {r}"
        # and both go on alike
        old.iterate(1); new.iterate(1)
        for w in compare_states(hier, bias):
            assert sm.same_bits(old.get_state(w), new.get_state(w)), w
    finally:
        old.close(); new.close()


def test_a_snapshot_does_not_grant_a_bias_column_that_was_never_handed_in(orc):
    """-bias, THETA_E and THETA_ELOG handed in but no UBIAS_*: hpf_fold_in_items is refused, with the same message before
    and after a snapshot round trip"""
    from hgaprec_amd.capi import Hpf
    n, m, K = 60, 40, 5
    prob = make_problem(n, m, 1000, 5)
    M = orc.Model(n, m, K, True, True, False)
    M.set_csr(*prob); M.initialize(5)
    old, new = Hpf(n, m, K, hier=True, bias=True), Hpf(n, m, K, hier=True, bias=True)
    try:
        for X in (old, new):
            X.upload_csr(*prob)
        for w in ("THETA_E", "THETA_ELOG"):
            old.set_state(w, M.state(w))
        new.restore(old.snapshot())
        r = _same_answer(lambda X: X.fold_in_items(2, 0.0), old, new, "fold_in_items without UBIAS_*")
        assert isinstance(r, str) and "UBIAS_E" in r, r
    finally:
        old.close(); new.close()


# ---- a refused call hides nothing ---------------------------------------------------------------------------------------

def _underflowing_handle(orc, bias):
    """test_softmax_underflow_is_reported_not_hidden's state on f32-stored W, one iteration launched: flag bit 0 is up
    and nobody has looked yet.  With bias the two bias columns vanish like the factors, so that every product does."""
    from hgaprec_amd.capi import Hpf
    n, m, K = 30, 20, 2
    rowptr, col, val = make_problem(n, m, 200, 3)
    M = orc.Model(n, m, K, True, bias, False)
    M.set_csr(rowptr, col, val)
    M.initialize(1)
    D = Hpf(n, m, K, hier=True, bias=bias, w_storage=1)
    D.upload_csr(rowptr, col, val)
    copy_state(M, D, True, bias)
    D.set_state("THETA_ELOG", np.tile(np.array([0.0, -150.0]), (n, 1)))
    D.set_state("BETA_ELOG", np.tile(np.array([-150.0, 0.0]), (m, 1)))
    if bias:
        D.set_state("UBIAS_ELOG", np.full(n, -150.0))
        D.set_state("IBIAS_ELOG", np.full(m, -150.0))
    D.iterate(1)
    return D, (n, m, K)


def _refused_calls(bias):
    """name -> (call(lib, h, buffer pointer), documented status)"""
    from hgaprec_amd.capi import STATE
    n, m, K = 30, 20, 2
    calls = {
        "set_state, wrong count": (lambda lib, h, p: lib.hpf_set_state(h, STATE["THETA_E"], p, n * K + 1), -1),
        "set_state of a rate, wrong count": (lambda lib, h, p: lib.hpf_set_state(h, STATE["THETA_RATE"], p, 1), -1),
        "set_state of XI_E, wrong count": (lambda lib, h, p: lib.hpf_set_state(h, STATE["XI_E"], p, n + 1), -1),
        "get_state, wrong count": (lambda lib, h, p: lib.hpf_get_state(h, STATE["THETA_E"], p, n * K - 1), -1),
        "get_state of a rate, wrong count": (lambda lib, h, p: lib.hpf_get_state(h, STATE["BETA_RATE"], p, 1), -1),
        "bias-rate set": (lambda lib, h, p: lib.hpf_set_state(h, STATE["UBIAS_RATE"], p, n), 0 if bias else -1),
    }
    if not bias:
        calls["set_state of a state that is not part of the model"] = (lambda lib, h, p: lib.hpf_set_state(h, STATE["UBIAS_E"], p, n), -1)
        calls["get_state of a state that is not part of the model"] = (lambda lib, h, p: lib.hpf_get_state(h, STATE["IBIAS_E"], p, m), -1)
    return calls


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
def test_a_refused_call_hides_nothing(orc, bias):
    """a pending underflow report survives every call that is refused (and the bias-rate set, which is accepted and does
    nothing): hpf_synchronize still fails afterwards"""
    from hgaprec_amd.capi import HpfError
    D, _ = _underflowing_handle(orc, bias)
    with pytest.raises(HpfError, match="underflow"):      # the scenario does what it is for
        D.synchronize()
    D.close()
    erased = []
    for name, (call, status) in _refused_calls(bias).items():
        D, _ = _underflowing_handle(orc, bias)
        buf = np.full(256, 0.5)
        rc = call(D.lib, D._h, buf.ctypes.data_as(C.POINTER(C.c_double)))
        assert rc == status, (name, rc)
        try:
            D.synchronize()
            erased.append(name)
        except HpfError as e:
            assert "underflow" in str(e), (name, str(e))
        D.close()
    assert not erased, f"the underflow report was erased by: {erased}"


# ---- what was exported earlier does not change an export --------------------------------------------------------------

@pytest.mark.parametrize("kind", ["SHAPE", "E"])
@pytest.mark.parametrize("obj", ["THETA", "BETA", "UBIAS"])
def test_export_history_does_not_change_an_export(orc, obj, kind):
    """iterate, hand in one array of an object, export the others -- with and without an export of its Elog before the
    set.  The four arrays of a Gamma object are independent (the oracle's orc_model_set_state): both orders give the same
    bits, and the oracle's values."""
    from hgaprec_amd.capi import Hpf
    n, m, K = 150, 120, 21
    prob = make_problem(n, m, 3000, 21)
    M = orc.Model(n, m, K, True, True, False)
    M.set_csr(*prob); M.initialize(21)
    handles = []
    for _ in range(2):
        D = Hpf(n, m, K, hier=True, bias=True)
        D.upload_csr(*prob)
        copy_state(M, D, True, True)
        D.iterate(2)
        handles.append(D)
    M.iterate(2)
    early, late = handles
    try:
        before = early.get_state(f"{obj}_ELOG")
        assert sm.oracle_error(f"{obj}_ELOG", before, M.state(f"{obj}_ELOG")) < RTOL
        new = sm.perturbed(M.state(f"{obj}_{kind}"), f"{obj}_{kind}", 5)
        for X in (early, late, M):
            X.set_state(f"{obj}_{kind}", new)
        for w in (f"{obj}_ELOG", f"{obj}_E", f"{obj}_RATE", f"{obj}_SHAPE"):
            a, b = early.get_state(w), late.get_state(w)
            e = max(sm.oracle_error(w, a, M.state(w)), sm.oracle_error(w, b, M.state(w)))
            print(f"{obj}_{kind} set, {w}: {int(np.sum(a != b))} entries differ between the orders, worst error against the oracle {e:.3e}")
            assert sm.same_bits(a, b), f"{w} after a set of {obj}_{kind} depends on whether {obj}_ELOG was exported before it"
            assert e < RTOL, (w, e)
        assert sm.same_bits(late.get_state(f"{obj}_ELOG"), before)      # neither set touches Elog
    finally:
        early.close(); late.close()
