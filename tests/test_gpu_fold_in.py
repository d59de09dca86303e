"""-m gpu: hpf_fold_in -- new users folded in against a frozen item side (fold_in_kernel: one launch, a wave per user, the
user's state in registers and its gathered item rows in LDS when they fit, a stopping time per user).

The CPU reference is the oracle itself (tests/fold_ref.py): oracle.orc.Model on the same CSR, the user side at the prior,
the item side a random trained-like state; per iteration iterate(1), then every item-side array is put back.  The oracle's
user half reads only the OLD item side, so that is one fold-in iteration -- test_oracle_loop_is_the_fold_in_equations checks the claim against a
numpy restatement of the equations of include/hpf.h at 1e-12.  The bar is test_gpu_parity.py's: rel_err < 1e-9 on every
user-side array of compare_states."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from hgaprec_amd import capi
from hgaprec_amd.capi import Hpf, HpfError
from oracle import orc
from tests.fold_ref import item_states, oracle_fold, psi, user_states  # noqa: F401  (test_gpu_fold_in_items.py takes them from here)
from tests.util import compare_states, rel_err

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
RTOL = 1e-9
S0 = R0 = 0.3


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def item_side(n, m, K, hier, bias, seed):
    """a trained-like item side: every array of every item-side Gamma object, consistent with each other"""
    rng = np.random.default_rng(seed)
    st = {}
    sh = S0 + rng.gamma(1.0, 0.5, (m, K))
    rt = (R0 + rng.gamma(2.0, 1.0, (m, 1)) + rng.uniform(0.5, 3.0, (1, K))) if hier else R0 + rng.uniform(0.5, 3.0, K)
    st["BETA_SHAPE"], st["BETA_RATE"] = sh, rt
    st["BETA_E"], st["BETA_ELOG"] = sh / rt, psi(sh) - np.log(rt)
    if hier:
        es, er = np.full(m, S0 + K * S0), R0 + st["BETA_E"].sum(1)
        st.update(ETA_SHAPE=es, ETA_RATE=er, ETA_E=es / er, ETA_ELOG=psi(es) - np.log(er))
    if bias:
        bs, br = S0 + rng.gamma(1.0, 0.5, m), np.full(m, R0 + n)
        st.update(IBIAS_SHAPE=bs, IBIAS_RATE=br, IBIAS_E=bs / br, IBIAS_ELOG=psi(bs) - np.log(br))
    return st


def make_csr(m, degs, seed, binary=False):
    rng = np.random.default_rng(seed)
    rows = [rng.permutation(m)[:d].astype(np.uint32) for d in degs]
    rowptr = np.zeros(len(degs) + 1, np.int64)
    rowptr[1:] = np.cumsum([r.size for r in rows])
    col = np.concatenate(rows).astype(np.uint32) if rows else np.zeros(0, np.uint32)
    val = None if binary else rng.integers(1, 6, col.size).astype(np.uint8)
    return rowptr, col, val


def numpy_fold(n, K, hier, bias, rowptr, col, val, item, T):
    """the equations of hpf_fold_in (include/hpf.h), restated"""
    Eb, Lb = item["BETA_E"], item["BETA_ELOG"]
    c, m = Eb.sum(0), Eb.shape[0]
    sh, rt = np.full((n, K), S0), np.full((n, K), R0)
    xs, xr, bs, br = np.full(n, S0), np.full(n, R0), np.full(n, S0), np.full(n, R0)
    for _ in range(T):
        Lt, Exi, Lub = psi(sh) - np.log(rt), xs / xr, psi(bs) - np.log(br)
        nsh, nbs = np.full((n, K), S0), np.full(n, S0)
        for u in range(n):
            for j in range(rowptr[u], rowptr[u + 1]):
                i, y = col[j], 1 if val is None else int(val[j])
                lg = np.concatenate([Lt[u] + Lb[i], [Lub[u], item["IBIAS_ELOG"][i]]]) if bias else Lt[u] + Lb[i]
                p = np.exp(lg - lg.max())
                p *= max(y, 1) / p.sum()
                nsh[u] += p[:K]
                nbs[u] += p[K] if bias else 0.0
        sh, rt = nsh, (Exi[:, None] if hier else R0) + np.broadcast_to(c, (n, K))
        bs, br = nbs, np.full(n, R0 + m)
        xs, xr = np.full(n, S0 + K * S0), R0 + (sh / rt).sum(1)
    out = dict(THETA_SHAPE=sh, THETA_RATE=rt if hier else rt[0], THETA_E=sh / rt, THETA_ELOG=psi(sh) - np.log(rt))
    if hier:
        out.update(XI_SHAPE=xs, XI_RATE=xr, XI_E=xs / xr, XI_ELOG=psi(xs) - np.log(xr))
    if bias:
        out.update(UBIAS_SHAPE=bs, UBIAS_RATE=br, UBIAS_E=bs / br, UBIAS_ELOG=psi(bs) - np.log(br))
    return out


def device(n, m, K, hier, bias, rowptr, col, val, item, only=None, **kw):
    """a handle over the new users with the item side handed in (only: just these arrays)"""
    D = Hpf(n, m, K, hier=hier, bias=bias, binary=val is None, **kw)
    D.upload_csr(rowptr, col, val)
    for w in (only if only is not None else item_states(hier, bias)):
        D.set_state(w, item[w])
    return D


def needed(bias):
    return ["BETA_E", "BETA_ELOG"] + (["IBIAS_E", "IBIAS_ELOG"] if bias else [])


def check_against(D, want, hier, bias, what):
    for w in user_states(hier, bias):
        got = D.get_state(w)
        assert got.shape == want[w].shape, (what, w)
        err = rel_err(got, want[w])
        print(f"{what} {w}: rel err {err:.3e}")
        assert err < RTOL, (what, w, err)


# ---------------------------------------------------------------------------------------------------------------------
# 0. the reference is what it claims to be
# ---------------------------------------------------------------------------------------------------------------------
N1, M1, K1 = 37, 50, 7
DEGS1 = [0, 1, 2, 50] + [int(d) for d in np.random.default_rng(5).integers(1, 21, N1 - 4)]
FLAGS = [(True, False, False), (True, True, False), (False, False, False), (False, True, False), (True, False, True)]


@pytest.mark.parametrize("hier,bias", [(True, True), (False, True), (True, False)])
def test_oracle_loop_is_the_fold_in_equations(hier, bias):
    rowptr, col, val = make_csr(M1, DEGS1, 11)
    item = item_side(N1, M1, K1, hier, bias, 12)
    a = oracle_fold(N1, M1, K1, hier, bias, rowptr, col, val, item, 3)
    b = numpy_fold(N1, K1, hier, bias, rowptr, col, val, item, 3)
    for w in user_states(hier, bias):
        assert rel_err(a[w], b[w]) < 1e-12, (w, rel_err(a[w], b[w]))


# ---------------------------------------------------------------------------------------------------------------------
# 1. parity with the oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hier,bias,binary", FLAGS)
def test_parity_with_the_oracle(hier, bias, binary):
    rowptr, col, val = make_csr(M1, DEGS1, 21, binary)
    item = item_side(N1, M1, K1, hier, bias, 22)
    D = device(N1, M1, K1, hier, bias, rowptr, col, val, item, only=needed(bias))
    try:
        for T in (1, 2, 5):
            iters = D.fold_in(T)
            assert iters.dtype == np.uint32 and np.all(iters == T)
            check_against(D, oracle_fold(N1, M1, K1, hier, bias, rowptr, col, val, item, T), hier, bias, f"T={T}")
        sh = D.get_state("THETA_SHAPE")
        assert np.all(sh[0] == S0)                                   # no ratings: the shape stays at the prior
    finally:
        D.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. column and lane edges
# ---------------------------------------------------------------------------------------------------------------------
R_EDGES = [(k, False) for k in (64, 128, 192, 256, 300)]              # the largest K of R = 1 .. 4, and R = 5 up to 300
COLS = [(1, False), (3, False), (62, True), (64, False), (65, False), (100, False), (100, True), (129, False)] + R_EDGES[1:]


@pytest.mark.parametrize("K,bias", COLS)
def test_column_and_lane_edges(K, bias):
    n, m = 9, 40
    assert [capi.fold_plan(k)["R"] for k, _ in R_EDGES] == [1, 2, 3, 4, 5] and capi.fold_plan(65)["R"] == 2 and capi.fold_plan(62, True)["ld"] == 64
    rowptr, col, val = make_csr(m, [0, 1, 40, 7, 13, 2, 25, 3, 9], 31)
    item = item_side(n, m, K, True, bias, 32)
    D = device(n, m, K, True, bias, rowptr, col, val, item, only=needed(bias))
    try:
        D.fold_in(3)
        check_against(D, oracle_fold(n, m, K, True, bias, rowptr, col, val, item, 3), True, bias, f"K={K} bias={bias}")
    finally:
        D.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the LDS boundary: the same user from LDS or from memory, here or there in the list
# ---------------------------------------------------------------------------------------------------------------------
def test_lds_boundary_and_independence_of_position():
    K, m = 100, 60
    H = capi.fold_plan(K)["rows_held"]
    degs = [H - 1, H, H + 1, 4 * H + 3]
    assert H == 13 and degs[-1] <= m
    rowptr, col, val = make_csr(m, degs, 41)
    item = item_side(4, m, K, True, False, 42)
    rows = [(col[rowptr[u]:rowptr[u + 1]], val[rowptr[u]:rowptr[u + 1]]) for u in range(4)]
    D = device(4, m, K, True, False, rowptr, col, val, item, only=needed(False))
    try:
        D.fold_in(4)
        check_against(D, oracle_fold(4, m, K, True, False, rowptr, col, val, item, 4), True, False, "alone")
        alone = {w: D.get_state(w) for w in user_states(True, False)}
    finally:
        D.close()
    # the same four users, in another order, among 300 others
    rp2, col2, val2 = make_csr(m, [int(d) for d in np.random.default_rng(43).integers(0, 41, 304)], 44)
    pos = [301, 17, 150, 2]
    r2 = [(col2[rp2[u]:rp2[u + 1]], val2[rp2[u]:rp2[u + 1]]) for u in range(304)]
    for p, r in zip(pos, rows):
        r2[p] = r
    rp2 = np.zeros(305, np.int64)
    rp2[1:] = np.cumsum([r[0].size for r in r2])
    col2, val2 = np.concatenate([r[0] for r in r2]), np.concatenate([r[1] for r in r2])
    D = device(304, m, K, True, False, rp2, col2, val2, item, only=needed(False))
    try:
        D.fold_in(4)
        for w in user_states(True, False):
            got = D.get_state(w)
            assert np.array_equal(_bits(got[pos]), _bits(alone[w])), w
    finally:
        D.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. grid edges and a row longer than a training segment
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 4, 5, 257])
def test_grid_edges_and_a_long_row(n):
    m, K = 2000, 5
    degs = [int(d) for d in np.random.default_rng(51).integers(0, 30, n)]
    degs[n // 2] = 1500
    rowptr, col, val = make_csr(m, degs, 52)
    item = item_side(n, m, K, True, True, 53)
    D = device(n, m, K, True, True, rowptr, col, val, item, only=needed(True))
    try:
        assert np.all(D.fold_in(2) == 2)
        check_against(D, oracle_fold(n, m, K, True, True, rowptr, col, val, item, 2), True, True, f"n={n}")
    finally:
        D.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. stopping
# ---------------------------------------------------------------------------------------------------------------------
STOP = dict(n=64, m=80, K=20, tol=1e-3, cap=30, seed=61)


def _stop_case():
    n, m, K = STOP["n"], STOP["m"], STOP["K"]
    degs = [int(d) for d in np.random.default_rng(STOP["seed"]).integers(0, 60, n)]
    rowptr, col, val = make_csr(m, degs, STOP["seed"] + 1)
    return n, m, K, rowptr, col, val, item_side(n, m, K, True, False, STOP["seed"] + 2)


def reference_counts(steps, tol, cap):
    """the stopping rule on the oracle's own trajectory"""
    n = steps[0].shape[0]
    cnt = np.full(n, cap, np.int64)
    for u in range(n):
        for t in range(2, cap + 1):
            if np.max(np.abs(steps[t - 1][u] - steps[t - 2][u])) <= tol * np.max(steps[t - 1][u]):
                cnt[u] = t
                break
    return cnt


def test_stopping_per_user():
    n, m, K, rowptr, col, val, item = _stop_case()
    tol, cap = STOP["tol"], STOP["cap"]
    _, steps = oracle_fold(n, m, K, True, False, rowptr, col, val, item, cap, trace=True)
    ref = reference_counts(steps, tol, cap)
    print("reference iteration counts:", np.unique(ref, return_counts=True))
    assert np.unique(ref).size >= 3 and np.any(ref == cap), "the inputs do not exercise the stopping rule"
    D = device(n, m, K, True, False, rowptr, col, val, item, only=needed(False))
    try:
        iters = D.fold_in(cap, tol)
        assert iters.min() >= 2 and iters.max() <= cap
        assert np.unique(iters).size >= 3 and np.any(iters == cap)
        stopped = {w: D.get_state(w) for w in user_states(True, False)}
        assert D.fold_in(cap, tol, want_iters=False) is None            # iters_out = NULL
        for w in user_states(True, False):
            assert np.array_equal(_bits(D.get_state(w)), _bits(stopped[w])), w
        for t in np.unique(iters):
            assert np.all(D.fold_in(int(t), 0.0) == t)
            who = np.flatnonzero(iters == t)
            for w in user_states(True, False):
                assert np.array_equal(_bits(D.get_state(w)[who]), _bits(stopped[w][who])), (int(t), w)
    finally:
        D.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. the other route as a witness (a child process: the knobs are read when the handle is created)
# ---------------------------------------------------------------------------------------------------------------------
def _witness(hier, bias, binary):
    rowptr, col, val = make_csr(M1, DEGS1, 21, binary)
    item = item_side(N1, M1, K1, hier, bias, 22)
    D = device(N1, M1, K1, hier, bias, rowptr, col, val, item, only=needed(bias))
    try:
        for T in (1, 2, 5):
            assert np.all(D.fold_in(T) == T)
            check_against(D, oracle_fold(N1, M1, K1, hier, bias, rowptr, col, val, item, T), hier, bias, f"sweeps route T={T}")
        try:
            D.fold_in(5, 1e-3)
        except HpfError as e:
            assert "(-5)" in str(e), str(e)                           # HPF_ERR_UNSUPPORTED
        else:
            raise AssertionError("tol > 0 was accepted by the sweeps route")
    finally:
        D.close()


def test_sweeps_route_is_a_second_witness():
    code = ("import tests.test_gpu_fold_in as t\n"
            "for f in t.FLAGS:\n"
            "    t._witness(*f)\n"
            "print('witness ok')\n")
    env = dict(os.environ, HPF_EXPERIMENTAL="1", HPF_FOLD_ROUTE="sweeps")
    r = subprocess.run([sys.executable, "-c", code], cwd=str(ROOT), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "witness ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


# ---------------------------------------------------------------------------------------------------------------------
# 7. nothing else moved, and the scoring calls see the result
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hier,bias", [(True, True), (False, False)])
def test_item_side_untouched_and_consumers_see_the_state(hier, bias):
    n, m, K = 37, 50, 7
    rowptr, col, val = make_csr(m, DEGS1, 71)
    item = item_side(n, m, K, hier, bias, 72)
    readable = [w for w in item_states(hier, bias) if w != "IBIAS_RATE"]     # (the constant r_prior + n: defined after a sweep)
    D = device(n, m, K, hier, bias, rowptr, col, val, item)
    F = None
    try:
        before = {w: D.get_state(w) for w in readable}
        D.fold_in(5)
        for w in readable:
            assert np.array_equal(_bits(D.get_state(w)), _bits(before[w])), w
        users = np.arange(n, dtype=np.uint32)
        ri, rs = D.recommend(users, 10)
        ti, ts = D.rank_topn(users, 10)
        assert np.array_equal(ri, ti) and np.array_equal(_bits(rs), _bits(ts))
        sc = D.get_state("THETA_E") @ item["BETA_E"].T
        if bias:
            sc = sc + D.get_state("UBIAS_E")[:, None] + item["IBIAS_E"][None, :]
        for u in range(n):
            sc[u, col[rowptr[u]:rowptr[u + 1]]] = 0.0
        order = np.lexsort((np.broadcast_to(np.arange(m), sc.shape), -sc), axis=1)[:, :10]
        live = np.take_along_axis(sc, order, 1) > 0                         # (a user who rated nearly everything: zeros tie by item)
        assert np.array_equal(ri[live], order[live].astype(np.uint32))
        assert rel_err(rs[live], np.take_along_axis(sc, order, 1)[live]) < 1e-12
        # a later iteration starts from the folded-in state
        F = device(n, m, K, hier, bias, rowptr, col, val, item)
        for w in user_states(hier, bias):
            if w.endswith("_RATE") and (w.startswith("UBIAS") or (w.startswith("THETA"))):
                continue                                                    # not part of a start state (tests.util.init_states)
            F.set_state(w, D.get_state(w))
        D.iterate(1)
        F.iterate(1)
        for w in compare_states(hier, bias):
            assert rel_err(D.get_state(w), F.get_state(w)) < RTOL, w
    finally:
        D.close()
        if F is not None:
            F.close()


# ---------------------------------------------------------------------------------------------------------------------
# 8. errors, each before anything is launched
# ---------------------------------------------------------------------------------------------------------------------
def _raises(code, f):
    with pytest.raises(HpfError) as e:
        f()
    assert f"({code})" in str(e.value), str(e.value)


def test_errors():
    n, m, K = 6, 20, 4
    rowptr, col, val = make_csr(m, [3, 0, 5, 1, 2, 4], 81)
    item = item_side(n, m, K, True, True, 82)
    D = Hpf(n, m, K, hier=True, bias=True)
    try:
        for w in needed(True):
            D.set_state(w, item[w])
        _raises(-6, lambda: D.fold_in(3))                               # no CSR: HPF_ERR_STATE
        _raises(-1, lambda: D.fold_in(0))
    finally:
        D.close()
    D = device(n, m, K, True, True, rowptr, col, val, item, only=["BETA_E"])
    try:
        _raises(-6, lambda: D.fold_in(3))                               # no BETA_ELOG
        D.set_state("BETA_ELOG", item["BETA_ELOG"])
        D.set_state("IBIAS_E", item["IBIAS_E"])
        _raises(-6, lambda: D.fold_in(3))                               # -bias without IBIAS_ELOG
        D.set_state("IBIAS_ELOG", item["IBIAS_ELOG"])
        _raises(-1, lambda: D.fold_in(0))
        _raises(-1, lambda: D.fold_in(3, -1e-3))
        _raises(-1, lambda: D.fold_in(3, float("nan")))
        assert np.all(D.fold_in(3) == 3)
    finally:
        D.close()
    Z = Hpf(0, m, K, hier=True, bias=True)
    try:
        Z.upload_csr(np.zeros(1, np.int64), np.zeros(0, np.uint32), np.zeros(0, np.uint8))
        for w in needed(True):
            Z.set_state(w, item[w])
        assert Z.fold_in(3).size == 0                                   # zero users: HPF_OK
    finally:
        Z.close()
