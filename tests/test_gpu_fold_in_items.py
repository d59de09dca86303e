"""-m gpu: hpf_fold_in_items -- new items folded in against a frozen user side (fold_in_kernel, a wave per item, for the
items with fewer than FOLD_LONG_MIN ratings; fold_in_long_kernel, a workgroup per item, for the others).

The reference.  Item fold-in of (R, user side U) IS user fold-in of (R^T, item side := U) with the names exchanged, so the
oracle is tests.fold_ref.oracle_fold on the item-major lists (users ascending inside an item, as the upload builds
them) with THETA <-> BETA, XI <-> ETA, UBIAS <-> IBIAS swapped.  test_oracle_loop_is_the_item_equations checks the claim
against a numpy restatement of the item equations of include/hpf.h at 1e-12.  The bar everywhere else is the project's:
rel_err < 1e-9 on every item-side array.

Tests that need a knob (HPF_FOLD_LONG_MIN, HPF_FOLD_ROUTE under HPF_EXPERIMENTAL=1: read when a handle is created) run in a
child process with a timeout."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import tests.test_gpu_fold_in as t
from hgaprec_amd import capi
from hgaprec_amd.capi import Hpf, HpfError
from tests.fold_ref import SWAP, oracle_items, swap  # noqa: F401
from tests.util import compare_states, rel_err

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
RTOL = 1e-9
S0 = R0 = t.S0
_bits = t._bits
item_states = t.item_states
user_states = t.user_states


def user_side(n, m, K, hier, bias, seed):
    """a trained-like user side of n users (every array of every user-side Gamma object) for m new items"""
    return {swap(w): a for w, a in t.item_side(m, n, K, hier, bias, seed).items()}


def needed(bias):
    return ["THETA_E", "THETA_ELOG"] + (["UBIAS_E", "UBIAS_ELOG"] if bias else [])


def make_items(n, degs, seed, binary=False):
    """ratings of len(degs) new items by n users -> the item-major lists (colptr, user, val), users ascending inside an
    item, and the CSR over the users they come from (rowptr, col, val)"""
    colptr, usr, val = t.make_csr(n, degs, seed, binary)
    for i in range(len(degs)):
        a, b = colptr[i], colptr[i + 1]
        o = np.argsort(usr[a:b], kind="stable")
        usr[a:b] = usr[a:b][o]
        if val is not None:
            val[a:b] = val[a:b][o]
    item_of = np.repeat(np.arange(len(degs), dtype=np.uint32), np.diff(colptr))
    o = np.argsort(usr, kind="stable")
    rowptr = np.zeros(n + 1, np.int64)
    rowptr[1:] = np.cumsum(np.bincount(usr, minlength=n))
    return (colptr, usr, val), (rowptr, item_of[o], None if val is None else val[o])


def from_lists(n, lists):
    """items given as (users ascending, ratings) -> what make_items returns"""
    colptr = np.zeros(len(lists) + 1, np.int64)
    colptr[1:] = np.cumsum([u.size for u, _ in lists])
    usr = np.concatenate([u for u, _ in lists]).astype(np.uint32)
    val = np.concatenate([v for _, v in lists]).astype(np.uint8)
    item_of = np.repeat(np.arange(len(lists), dtype=np.uint32), np.diff(colptr))
    o = np.argsort(usr, kind="stable")
    rowptr = np.zeros(n + 1, np.int64)
    rowptr[1:] = np.cumsum(np.bincount(usr, minlength=n))
    return (colptr, usr, val), (rowptr, item_of[o], val[o])


def numpy_items(n, m, K, hier, bias, imajor, users, T):
    """the equations of hpf_fold_in_items (include/hpf.h), restated"""
    colptr, usr, val = imajor
    Et, Lt = users["THETA_E"], users["THETA_ELOG"]
    c = Et.sum(0)
    sh, rt = np.full((m, K), S0), np.full((m, K), R0)
    es, er, bs, br = np.full(m, S0), np.full(m, R0), np.full(m, S0), np.full(m, R0)
    for _ in range(T):
        Lb, Eeta, Lib = t.psi(sh) - np.log(rt), es / er, t.psi(bs) - np.log(br)
        nsh, nbs = np.full((m, K), S0), np.full(m, S0)
        for i in range(m):
            for j in range(colptr[i], colptr[i + 1]):
                u, y = usr[j], 1 if val is None else int(val[j])
                lg = np.concatenate([Lt[u] + Lb[i], [users["UBIAS_ELOG"][u], Lib[i]]]) if bias else Lt[u] + Lb[i]
                p = np.exp(lg - lg.max())
                p *= max(y, 1) / p.sum()
                nsh[i] += p[:K]
                nbs[i] += p[K + 1] if bias else 0.0
        sh, rt = nsh, (Eeta[:, None] if hier else R0) + np.broadcast_to(c, (m, K))
        bs, br = nbs, np.full(m, R0 + n)
        es, er = np.full(m, S0 + K * S0), R0 + (sh / rt).sum(1)
    out = dict(BETA_SHAPE=sh, BETA_RATE=rt if hier else rt[0], BETA_E=sh / rt, BETA_ELOG=t.psi(sh) - np.log(rt))
    if hier:
        out.update(ETA_SHAPE=es, ETA_RATE=er, ETA_E=es / er, ETA_ELOG=t.psi(es) - np.log(er))
    if bias:
        out.update(IBIAS_SHAPE=bs, IBIAS_RATE=br, IBIAS_E=bs / br, IBIAS_ELOG=t.psi(bs) - np.log(br))
    return out


def device(n, m, K, hier, bias, umajor, users, only=None, **kw):
    """a handle of n trained users x m new items with the user side handed in (only: just these arrays)"""
    rowptr, col, val = umajor
    D = Hpf(n, m, K, hier=hier, bias=bias, binary=val is None, **kw)
    D.upload_csr(rowptr, col, val)
    for w in (only if only is not None else user_states(hier, bias)):
        D.set_state(w, users[w])
    return D


def check_against(D, want, hier, bias, what, rows=None):
    worst = 0.0
    for w in item_states(hier, bias):
        got, ref = D.get_state(w), want[w]
        assert got.shape == ref.shape, (what, w)
        if rows is not None and got.shape[:1] == (D.n_items,):
            got, ref = got[rows], ref[rows]
        err = rel_err(got, ref)
        worst = max(worst, err)
        assert err < RTOL, (what, w, err)
    print(f"{what}: worst rel err {worst:.3e}")


def run_child(code, **env):
    e = dict(os.environ, HPF_EXPERIMENTAL="1", **{k: str(v) for k, v in env.items()})
    r = subprocess.run([sys.executable, "-c", "import tests.test_gpu_fold_in_items as f\n" + code + "\nprint('child ok')\n"],
                       cwd=str(ROOT), env=e, capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:])
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def parity(n, degs, K, hier, bias, binary, Ts, seed, what):
    """the call against the oracle on one handle, for every T of Ts; returns the states after the last"""
    m = len(degs)
    imajor, umajor = make_items(n, degs, seed, binary)
    users = user_side(n, m, K, hier, bias, seed + 1)
    D = device(n, m, K, hier, bias, umajor, users, only=needed(bias))
    try:
        for T in Ts:
            iters = D.fold_in_items(T)
            assert iters.dtype == np.uint32 and iters.shape == (m,) and np.all(iters == T)
            check_against(D, oracle_items(n, m, K, hier, bias, imajor, users, T), hier, bias, f"{what} T={T}")
        return {w: D.get_state(w) for w in item_states(hier, bias)}
    finally:
        D.close()


# ---------------------------------------------------------------------------------------------------------------------
# 0. the reference is what it claims to be
# ---------------------------------------------------------------------------------------------------------------------
N1, M1, K1 = 50, 37, 7                                               # 50 frozen users, 37 new items
DEGS1 = t.DEGS1
FLAGS = t.FLAGS


@pytest.mark.parametrize("hier,bias,binary", FLAGS)
@pytest.mark.parametrize("T", [1, 3])
def test_oracle_loop_is_the_item_equations(hier, bias, binary, T):
    imajor, _ = make_items(N1, DEGS1, 11, binary)
    users = user_side(N1, M1, K1, hier, bias, 12)
    a = oracle_items(N1, M1, K1, hier, bias, imajor, users, T)
    b = numpy_items(N1, M1, K1, hier, bias, imajor, users, T)
    for w in item_states(hier, bias):
        assert rel_err(a[w], b[w]) < 1e-12, (w, rel_err(a[w], b[w]))


# ---------------------------------------------------------------------------------------------------------------------
# 1. parity with the oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hier,bias,binary", FLAGS)
def test_parity_with_the_oracle(hier, bias, binary):
    st = parity(N1, DEGS1, K1, hier, bias, binary, (1, 2, 5), 21, "parity")
    assert DEGS1[0] == 0 and np.all(st["BETA_SHAPE"][0] == S0)           # no ratings: the shape stays at the prior


# ---------------------------------------------------------------------------------------------------------------------
# 2. column and lane edges, through the wave kernel and through every instance of the workgroup kernel the list reaches
# ---------------------------------------------------------------------------------------------------------------------
COL_DEGS = [0, 1, 40, 7, 13, 2, 25, 3, 9]


@pytest.mark.parametrize("K,bias", t.COLS)
def test_column_and_lane_edges(K, bias):
    parity(40, COL_DEGS, K, True, bias, False, (3,), 31, f"K={K} bias={bias}")


def _cols_long():
    for K, bias in t.COLS:
        parity(40, COL_DEGS, K, True, bias, False, (3,), 31, f"long rows K={K} bias={bias}")


def test_column_and_lane_edges_long_rows():
    run_child("f._cols_long()", HPF_FOLD_LONG_MIN=8)                    # 40, 13, 25 and 9 ratings: a workgroup each


# ---------------------------------------------------------------------------------------------------------------------
# 3. the route boundary at the shipped threshold
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,bias", [(5, True), (100, False)])
def test_route_boundary(K, bias):
    L, W = capi.FOLD_LONG_MIN, capi.fold_items_plan(K, bias)["waves"]
    n = 2 * W * 64 + 8
    assert L + 1 < 2 * W * 64 + 1 <= n
    parity(n, [L - 1, L, L + 1, 2 * W * 64 + 1], K, True, bias, False, (3,), 41, f"boundary K={K}")


# ---------------------------------------------------------------------------------------------------------------------
# 4. empty and ragged parts: every non-empty row to the workgroup kernel
# ---------------------------------------------------------------------------------------------------------------------
def _ragged(K, bias):
    W = capi.fold_items_plan(K, bias)["waves"]
    degs = [1, 2, 63, 64, 65, W * 64 - 1, W * 64, W * 64 + 1]
    n, m, T = W * 64 + 8, len(degs), 3
    imajor, umajor = make_items(n, degs, 51)
    users = user_side(n, m, K, True, bias, 52)
    want = oracle_items(n, m, K, True, bias, imajor, users, T)
    got = {}
    for knob in ("1", str(2 ** 32 - 1)):                                 # the knobs are read when the handle is created
        os.environ["HPF_FOLD_LONG_MIN"] = knob
        D = device(n, m, K, True, bias, umajor, users, only=needed(bias))
        try:
            D.fold_in_items(T)
            check_against(D, want, True, bias, f"K={K} W={W} HPF_FOLD_LONG_MIN={knob}")
            got[knob] = {w: D.get_state(w) for w in item_states(True, bias)}
        finally:
            D.close()
    for w in item_states(True, bias):
        a, b = got["1"][w], got[str(2 ** 32 - 1)][w]
        print(f"K={K} {w}: workgroup route against wave route, rel diff {rel_err(a, b):.3e}")
        # up to 64 ratings are one wave's part: the other waves add +0.0, so the two routes give the same bits
        assert np.array_equal(_bits(a[:4]), _bits(b[:4])), w


def test_empty_and_ragged_parts():
    run_child("f._ragged(7, True)\nf._ragged(520, False)", HPF_FOLD_LONG_MIN=1)      # R = 1: eight waves; R = 9: four


# ---------------------------------------------------------------------------------------------------------------------
# 5. independence of position (default route: one of the four items is long)
# ---------------------------------------------------------------------------------------------------------------------
def test_independence_of_position():
    K, n, T = 100, 720, 4
    degs = [12, 13, 60, capi.FOLD_LONG_MIN + 188]
    (colptr, usr, val), umajor = make_items(n, degs, 61)
    users = user_side(n, 304, K, True, False, 62)
    mine = [(usr[colptr[i]:colptr[i + 1]], val[colptr[i]:colptr[i + 1]]) for i in range(4)]
    D = device(n, 4, K, True, False, umajor, users, only=needed(False))
    try:
        D.fold_in_items(T)
        check_against(D, oracle_items(n, 4, K, True, False, (colptr, usr, val), users, T), True, False, "alone")
        alone = {w: D.get_state(w) for w in item_states(True, False)}
    finally:
        D.close()
    (cp2, us2, va2), _ = make_items(n, [int(d) for d in np.random.default_rng(63).integers(0, 41, 304)], 64)
    lists = [(us2[cp2[i]:cp2[i + 1]], va2[cp2[i]:cp2[i + 1]]) for i in range(304)]
    pos = [301, 17, 150, 2]
    for p, r in zip(pos, mine):
        lists[p] = r
    _, umajor2 = from_lists(n, lists)
    D = device(n, 304, K, True, False, umajor2, users, only=needed(False))
    try:
        D.fold_in_items(T)
        for w in item_states(True, False):
            assert np.array_equal(_bits(D.get_state(w)[pos]), _bits(alone[w])), w
    finally:
        D.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. grid edges
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 4, 5, 257])
def test_grid_edges_and_a_long_row(m):
    degs = [int(d) for d in np.random.default_rng(71).integers(0, 30, m)]
    degs[m // 2] = capi.FOLD_LONG_MIN + 88
    parity(700, degs, 5, True, True, False, (2,), 72, f"m={m}")


def _many_long():
    m = capi.FOLD_LONG_BLOCKS_MAX + 104                                  # more long rows than workgroups: they stride
    degs = [int(d) for d in np.random.default_rng(73).integers(1, 4, m)]
    parity(50, degs, 5, True, True, False, (2,), 74, f"{m} long rows")


def test_more_long_rows_than_workgroups():
    run_child("f._many_long()", HPF_FOLD_LONG_MIN=1)


# ---------------------------------------------------------------------------------------------------------------------
# 7. stopping: per item; in the workgroup kernel the decision is taken once and shared
# ---------------------------------------------------------------------------------------------------------------------
def _stopping(tol):
    m, n, K, colptr, usr, val, as_items = t._stop_case()                 # transposed: 64 new items, 80 users
    cap = t.STOP["cap"]
    for i in range(m):
        a, b = colptr[i], colptr[i + 1]
        o = np.argsort(usr[a:b], kind="stable")
        usr[a:b], val[a:b] = usr[a:b][o], val[a:b][o]
    lists = [(usr[colptr[i]:colptr[i + 1]], val[colptr[i]:colptr[i + 1]]) for i in range(m)]
    imajor, umajor = from_lists(n, lists)
    users = {swap(w): a for w, a in as_items.items()}
    _, steps = oracle_items(n, m, K, True, False, imajor, users, cap, trace=True)
    ref = t.reference_counts(steps, tol, cap)
    print("reference iteration counts:", np.unique(ref, return_counts=True))
    assert np.unique(ref).size >= 3 and np.any(ref == cap), "the inputs do not exercise the stopping rule"
    D = device(n, m, K, True, False, umajor, users, only=needed(False))
    try:
        iters = D.fold_in_items(cap, tol)
        print("device iteration counts:", np.unique(iters, return_counts=True))
        assert iters.min() >= 2 and iters.max() <= cap
        assert np.unique(iters).size >= 3 and np.any(iters == cap)
        stopped = {w: D.get_state(w) for w in item_states(True, False)}
        assert D.fold_in_items(cap, tol, want_iters=False) is None       # iters_out = NULL
        for w in item_states(True, False):
            assert np.array_equal(_bits(D.get_state(w)), _bits(stopped[w])), w
        for c in np.unique(iters):
            assert np.all(D.fold_in_items(int(c), 0.0) == c)
            who = np.flatnonzero(iters == c)
            for w in item_states(True, False):
                assert np.array_equal(_bits(D.get_state(w)[who]), _bits(stopped[w][who])), (int(c), w)
    finally:
        D.close()


def test_stopping_per_item():
    _stopping(t.STOP["tol"])


def test_stopping_per_item_in_the_workgroup_kernel():
    run_child("f._stopping(1e-2)", HPF_FOLD_LONG_MIN=8)                  # early and late stops in one launch


# ---------------------------------------------------------------------------------------------------------------------
# 8. the sweeps route as a second witness
# ---------------------------------------------------------------------------------------------------------------------
def _witness(hier, bias, binary):
    imajor, umajor = make_items(N1, DEGS1, 21, binary)
    users = user_side(N1, M1, K1, hier, bias, 22)
    D = device(N1, M1, K1, hier, bias, umajor, users, only=needed(bias))
    try:
        for T in (1, 2, 5):
            assert np.all(D.fold_in_items(T) == T)
            check_against(D, oracle_items(N1, M1, K1, hier, bias, imajor, users, T), hier, bias, f"sweeps route T={T}")
        try:
            D.fold_in_items(5, 1e-3)
        except HpfError as e:
            assert "(-5)" in str(e), str(e)                               # HPF_ERR_UNSUPPORTED
        else:
            raise AssertionError("tol > 0 was accepted by the sweeps route")
    finally:
        D.close()


def test_sweeps_route_is_a_second_witness():
    run_child("for fl in f.FLAGS:\n    f._witness(*fl)", HPF_FOLD_ROUTE="sweeps")


# ---------------------------------------------------------------------------------------------------------------------
# 9. nothing else moved, and the scoring calls see the result
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hier,bias", [(True, True), (False, False)])
def test_user_side_untouched_and_consumers_see_the_state(hier, bias):
    n, m, K = N1, M1, K1
    imajor, umajor = make_items(n, DEGS1, 81)
    rowptr, col, _ = umajor
    users = user_side(n, m, K, hier, bias, 82)
    readable = [w for w in user_states(hier, bias) if w != "UBIAS_RATE"]      # (the constant r_prior + m: defined after a sweep)
    D = device(n, m, K, hier, bias, umajor, users)
    F = None
    try:
        before = {w: D.get_state(w) for w in readable}
        D.fold_in_items(5)
        for w in readable:
            assert np.array_equal(_bits(D.get_state(w)), _bits(before[w])), w
        sel = np.arange(n, dtype=np.uint32)
        ri, rs = D.recommend(sel, 10)
        ti, ts = D.rank_topn(sel, 10)
        assert np.array_equal(ri, ti) and np.array_equal(_bits(rs), _bits(ts))
        sc = users["THETA_E"] @ D.get_state("BETA_E").T
        if bias:
            sc = sc + users["UBIAS_E"][:, None] + D.get_state("IBIAS_E")[None, :]
        for u in range(n):
            sc[u, col[rowptr[u]:rowptr[u + 1]]] = 0.0
        order = np.lexsort((np.broadcast_to(np.arange(m), sc.shape), -sc), axis=1)[:, :10]
        live = np.take_along_axis(sc, order, 1) > 0
        assert np.array_equal(ri[live], order[live].astype(np.uint32))
        assert rel_err(rs[live], np.take_along_axis(sc, order, 1)[live]) < 1e-12
        # a later iteration starts from the folded-in state
        F = device(n, m, K, hier, bias, umajor, users)
        for w in item_states(hier, bias):
            if w.endswith("_RATE") and (w.startswith("IBIAS") or w.startswith("BETA")):
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
# 10. errors, each before anything is launched
# ---------------------------------------------------------------------------------------------------------------------
def test_errors():
    n, m, K = 20, 6, 4
    _, umajor = make_items(n, [3, 0, 5, 1, 2, 4], 91)
    users = user_side(n, m, K, True, True, 92)
    D = Hpf(n, m, K, hier=True, bias=True)
    try:
        for w in needed(True):
            D.set_state(w, users[w])
        t._raises(-6, lambda: D.fold_in_items(3))                       # no CSR: HPF_ERR_STATE
        t._raises(-1, lambda: D.fold_in_items(0))
    finally:
        D.close()
    D = device(n, m, K, True, True, umajor, users, only=["THETA_E"])
    try:
        t._raises(-6, lambda: D.fold_in_items(3))                       # no THETA_ELOG
        D.set_state("THETA_ELOG", users["THETA_ELOG"])
        D.set_state("UBIAS_E", users["UBIAS_E"])
        t._raises(-6, lambda: D.fold_in_items(3))                       # -bias without UBIAS_ELOG
        D.set_state("UBIAS_ELOG", users["UBIAS_ELOG"])
        t._raises(-1, lambda: D.fold_in_items(0))
        t._raises(-1, lambda: D.fold_in_items(3, -1e-3))
        t._raises(-1, lambda: D.fold_in_items(3, float("nan")))
        assert np.all(D.fold_in_items(3) == 3)
    finally:
        D.close()
    P = device(n, m, K, True, True, umajor, users, n_ranks=2, rank=0, n_users_total=2 * n)
    try:
        t._raises(-5, lambda: P.fold_in_items(3))                       # users are sharded across ranks: HPF_ERR_UNSUPPORTED
    finally:
        P.close()
    # zero items is HPF_OK in the call, but no such handle exists: hpf_create has always refused n_items = 0
    with pytest.raises(HpfError) as e:
        Hpf(n, 0, K, hier=True, bias=True)
    assert "(-1)" in str(e.value)
