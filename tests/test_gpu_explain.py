"""-m gpu: hpf_explain -- the T largest terms of a pair's score (explain_kernel: a wave per pair, the terms in registers, T
rounds of a wave-wide arg-best).

The reference is numpy: c = Et[u] * Eb[i] (one IEEE multiplication per term) with the two bias copies appended, ordered by a
stable argsort of -c.  Factors and the bit patterns of the contributions are compared for equality; only the sum of a row is
compared with hpf_predict under a derived bound (the two calls add in different orders)."""
import ctypes as C
import math

import numpy as np
import pytest

from hgaprec_amd import capi

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF
U53 = 2.0 ** -53
N_USERS, N_ITEMS = 37, 41


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _gamma(rows, K, seed):
    """expectations of a Gamma(0.3, .) factor matrix: positive, wide in magnitude, and a few exact zeros"""
    rng = np.random.default_rng(seed)
    E = rng.gamma(0.3, 1.0, (rows, K)) / rng.gamma(3.0, 1.0, (rows, 1))
    E[rng.random((rows, K)) < 0.02] = 0.0
    return E


class Model:
    """a handle that holds E of both sides (and of both biases) and nothing else: no CSR, no iteration"""

    def __init__(self, Et, Eb, ub=None, ib=None, hier=False):
        self.Et, self.Eb = np.ascontiguousarray(Et, np.float64), np.ascontiguousarray(Eb, np.float64)
        self.bias = ub is not None
        self.ub = np.ascontiguousarray(ub, np.float64) if self.bias else None
        self.ib = np.ascontiguousarray(ib, np.float64) if self.bias else None
        self.K = self.Et.shape[1]
        self.D = capi.Hpf(self.Et.shape[0], self.Eb.shape[0], self.K, hier=hier, bias=self.bias)
        self.D.set_state("THETA_E", self.Et)
        self.D.set_state("BETA_E", self.Eb)
        if self.bias:
            self.D.set_state("UBIAS_E", self.ub)
            self.D.set_state("IBIAS_E", self.ib)

    def names(self):
        return ["THETA_E", "BETA_E"] + (["UBIAS_E", "IBIAS_E"] if self.bias else [])

    def state(self):
        return [_bits(self.D.get_state(w)).copy() for w in self.names()]

    def terms(self, u, i):
        c = self.Et[u] * self.Eb[i]
        if self.bias:
            c = np.concatenate([c, self.ub[u][:, None], self.ib[i][:, None]], axis=1)
        return c

    def reference(self, u, i, T):
        c = self.terms(np.asarray(u, np.int64), np.asarray(i, np.int64))
        order = np.argsort(-c, axis=1, kind="stable")[:, :T]
        fac = np.full((len(u), T), NONE, np.uint32)
        con = np.zeros((len(u), T), np.float64)
        fac[:, :order.shape[1]] = order
        con[:, :order.shape[1]] = np.take_along_axis(c, order, axis=1)
        return fac, con

    def check(self, u, i, T, what):
        fac, con = self.D.explain(u, i, T)
        wf, wc = self.reference(u, i, T)
        assert fac.shape == wf.shape and con.shape == wc.shape, what
        assert fac.dtype == np.uint32 and con.dtype == np.float64, what
        assert np.array_equal(fac, wf), f"{what}: factors, first bad pair {np.argwhere((fac != wf).any(axis=1))[:1]}"
        assert np.array_equal(_bits(con), _bits(wc)), what + ": contributions"
        return fac, con

    def close(self):
        self.D.close()


def _random_model(K, bias, hier, seed=3):
    rng = np.random.default_rng(seed + K)
    return Model(_gamma(N_USERS, K, seed), _gamma(N_ITEMS, K, seed + 1),
                 rng.gamma(0.3, 1.0, N_USERS) if bias else None, rng.gamma(0.3, 1.0, N_ITEMS) if bias else None, hier)


def _pairs(cnt, seed, n=N_USERS, m=N_ITEMS):
    rng = np.random.default_rng(seed)
    return rng.integers(0, n, cnt).astype(np.uint32), rng.integers(0, m, cnt).astype(np.uint32)


SHAPES = [(K, bias, hier) for K in (1, 3, 63, 64, 65, 100, 129) for bias in (False, True) for hier in (False, True)]
SHAPES += [(1022, True, False), (1022, True, True)]                # K + 2 = HPF_MAX_COLUMNS: R = 16


@pytest.mark.parametrize("K,bias,hier", SHAPES)
def test_terms_are_numpys_products_in_the_ranking_order(K, bias, hier):
    M = _random_model(K, bias, hier)
    try:
        before = M.state()
        for cnt in (1, 5, 4099):
            u, i = _pairs(cnt, 11 + cnt)
            for T in (1, 5, 32):                                   # T > K + 2 * bias: the padding
                fac, con = M.check(u, i, T, f"K={K} bias={bias} hier={hier} cnt={cnt} T={T}")
                real = min(T, K + 2 * bias)
                assert np.all(fac[:, real:] == NONE) and np.all(_bits(con[:, real:]) == 0)
        assert all(np.array_equal(a, b) for a, b in zip(before, M.state())), "hpf_explain wrote the state"
    finally:
        M.close()


def test_every_lane_count_from_one_to_sixteen():
    """R = ceil((K + 2 bias) / 64): one column count per kernel instance, each at the last column of its R"""
    for R in range(1, 17):
        K = 64 * R - 2
        assert capi.explain_plan(K, True)["R"] == R
        M = _random_model(K, True, False, seed=R)
        try:
            u, i = _pairs(67, R)
            M.check(u, i, 32, f"R={R}")
        finally:
            M.close()


def test_second_grid_stride_trip():
    K = 3
    probe = capi.explain_grid(10 ** 9) * capi.EXPLAIN_WAVES * capi.EXPLAIN_RUN       # pairs of one trip of the capped grid
    cnt = probe + 3
    assert capi.explain_grid(cnt) == capi.EXPLAIN_BLOCKS_MAX
    M = _random_model(K, True, True)
    try:
        u, i = _pairs(cnt, 5)
        M.check(u, i, 5, "two trips")
    finally:
        M.close()


def test_ties_go_to_the_smaller_factor():
    K, T = 200, 32
    # all-equal rows: factors 0, 1, ... ascending
    M = Model(np.full((N_USERS, K), 0.5), np.full((N_ITEMS, K), 0.25))
    try:
        u, i = _pairs(9, 1)
        fac, con = M.check(u, i, T, "all equal")
        assert np.array_equal(fac, np.tile(np.arange(T, dtype=np.uint32), (9, 1))) and np.all(con == 0.125)
    finally:
        M.close()
    # equal terms in different lanes and different register slots: k, k + 1, k + 64, k + 128 tie at the top, then a
    # second tied group below it, among random smaller terms
    rng = np.random.default_rng(2)
    Et, Eb = rng.random((N_USERS, K)) * 0.5, rng.random((N_ITEMS, K)) * 0.5
    for k in (0, 5, 62, 63):
        for c in (k, k + 1, k + 64, k + 128):
            Et[:, c], Eb[:, c] = 2.0, 3.0
        for c in (k + 2, k + 66, k + 130):
            Et[:, c], Eb[:, c] = 1.0, 1.0
        M = Model(Et, Eb)
        try:
            fac, _ = M.check(u, i, T, f"ties at {k}")
            want = sorted({k, k + 1, k + 64, k + 128})
            assert fac[0, :len(want)].tolist() == want
        finally:
            M.close()
        Et, Eb = rng.random((N_USERS, K)) * 0.5, rng.random((N_ITEMS, K)) * 0.5
    # all-zero rows, without and with bias; and a row whose only non-zero terms are the two biases
    for bias in (False, True):
        M = Model(np.zeros((N_USERS, K)), _gamma(N_ITEMS, K, 4), np.zeros(N_USERS) if bias else None, np.zeros(N_ITEMS) if bias else None)
        try:
            fac, con = M.check(u, i, T, "all zero")
            assert np.array_equal(fac, np.tile(np.arange(T, dtype=np.uint32), (9, 1))) and np.all(_bits(con) == 0)
        finally:
            M.close()
    M = Model(np.zeros((N_USERS, K)), _gamma(N_ITEMS, K, 4), np.full(N_USERS, 0.25), np.full(N_ITEMS, 0.5))
    try:
        fac, con = M.check(u, i, 5, "biases only")
        assert np.all(fac[:, 0] == K + 1) and np.all(fac[:, 1] == K) and np.array_equal(fac[:, 2:], np.tile(np.arange(3, dtype=np.uint32), (9, 1)))
        assert np.all(con[:, 0] == 0.5) and np.all(con[:, 1] == 0.25)
    finally:
        M.close()


def test_wide_range_products_stay_finite_and_order_by_pattern():
    """entries from 2^-545 to 2^500: products up to 2^1000, down through the subnormals to those that round to +0.0"""
    K = 130
    rng = np.random.default_rng(8)
    Et = np.ldexp(1.0 + rng.random((N_USERS, K)), rng.integers(-545, 500, (N_USERS, K)))
    Eb = np.ldexp(1.0 + rng.random((N_ITEMS, K)), rng.integers(-545, 500, (N_ITEMS, K)))
    Et[:, 100:], Eb[:, 100:] = np.ldexp(1.0 + rng.random((N_USERS, 30)), rng.integers(-545, -500, (N_USERS, 30))), \
        np.ldexp(1.0 + rng.random((N_ITEMS, 30)), rng.integers(-545, -500, (N_ITEMS, 30)))
    M = Model(Et, Eb, np.ldexp(1.0, rng.integers(-1000, 1000, N_USERS)), np.ldexp(1.0, rng.integers(-1000, 1000, N_ITEMS)))
    try:
        u, i = _pairs(300, 3)
        with np.errstate(under="ignore"):
            c = M.terms(u.astype(np.int64), i.astype(np.int64))
            assert np.all(np.isfinite(c)) and np.any((c > 0) & (c < 2.0 ** -1022)) and np.any(c[:, :K] == 0)
            for T in (5, 32):
                M.check(u, i, T, f"wide range T={T}")
        # the tail of every row, where the subnormal and the zero terms are: all K + 2 terms cannot be asked for at once
        # (T <= 32), so rows of 30 tiny columns alone
        M2 = Model(Et[:, 100:], Eb[:, 100:])
        try:
            with np.errstate(under="ignore"):
                M2.check(u, i, 32, "subnormal and zero products")
        finally:
            M2.close()
    finally:
        M.close()


def test_runs_of_one_user_and_duplicated_pairs():
    M = _random_model(100, True, True)
    try:
        # a run of one user, a change of user in the middle of a wave's run of EXPLAIN_RUN pairs, and single-pair calls
        u = np.array([4] * 13 + [9] * 3 + [4] * 7 + [0] + [36] * 20, np.uint32)
        i = (np.arange(u.size, dtype=np.uint32) * 7) % N_ITEMS
        assert u.size > 2 * capi.EXPLAIN_RUN and (13 % capi.EXPLAIN_RUN) != 0
        fac, con = M.check(u, i, 5, "runs")
        for p in range(u.size):
            f1, c1 = M.D.explain(u[p:p + 1], i[p:p + 1], 5)
            assert np.array_equal(f1[0], fac[p]) and np.array_equal(_bits(c1[0]), _bits(con[p])), p
        # a pair given twice (next to each other and a trip apart): equal rows
        u2 = np.concatenate([u[:3], u[:3], u]); i2 = np.concatenate([i[:3], i[:3], i])
        fac, con = M.check(u2, i2, 32, "duplicates")
        assert np.array_equal(fac[:3], fac[3:6]) and np.array_equal(_bits(con[:3]), _bits(con[3:6]))
        assert np.array_equal(fac[:3], fac[6:9]) and np.array_equal(_bits(con[:3]), _bits(con[6:9]))
    finally:
        M.close()


@pytest.mark.parametrize("K,bias", [(1, False), (7, True), (16, False), (17, True), (30, True), (30, False)])
def test_sum_of_all_terms_against_hpf_predict(K, bias):
    """|hpf_predict - fsum(row)| <= (ceil(K / 16) + 10) 2^-53 fsum: predict_kernel does at most ceil(K / 16) FMAs per chain,
    4 adds in group_sum<16> and 2 bias adds; each contribution carries one rounding and fsum adds one; all terms are >= 0,
    so the sum is its own condition number"""
    M = _random_model(K, bias, True)
    try:
        u, i = _pairs(500, 21)
        T = K + 2 * bias
        _, con = M.check(u, i, T, "all terms")
        pred = M.D.predict(u, i)
        worst = 0.0
        for p in range(u.size):
            s = math.fsum(con[p])
            bound = (-(-K // 16) + 10) * U53 * s
            worst = max(worst, abs(pred[p] - s) / (U53 * s) if s > 0 else 0.0)
            assert abs(pred[p] - s) <= bound, (p, pred[p], s, bound)
        print(f"K={K} bias={bias}: worst |predict - fsum| = {worst:.2f} x 2^-53 sum (bound {-(-K // 16) + 10})")
    finally:
        M.close()


def test_refusals_launch_nothing():
    M = _random_model(20, True, False)
    try:
        lib, h = M.D.lib, M.D._h
        u32p, dp = C.POINTER(C.c_uint32), C.POINTER(C.c_double)
        u, i = _pairs(6, 2)
        fac, con = np.zeros((6, 32), np.uint32), np.zeros((6, 32), np.float64)
        pu, pi, pf, pc = (a.ctypes.data_as(t) for a, t in ((u, u32p), (i, u32p), (fac, u32p), (con, dp)))
        before = M.state()
        for T in (0, 33, 0xFFFFFFFF):
            assert lib.hpf_explain(h, pu, pi, 6, T, pf, pc) == -1, T
            with pytest.raises(capi.HpfError):
                M.D.explain(u, i, T)
        bad_u, bad_i = u.copy(), i.copy()
        bad_u[4], bad_i[5] = N_USERS, N_ITEMS
        assert lib.hpf_explain(h, bad_u.ctypes.data_as(u32p), pi, 6, 5, pf, pc) == -1
        assert lib.hpf_explain(h, pu, bad_i.ctypes.data_as(u32p), 6, 5, pf, pc) == -1
        assert b"out of range" in lib.hpf_last_error(h)
        for args in ((None, pi, pf, pc), (pu, None, pf, pc), (pu, pi, None, pc), (pu, pi, pf, None)):
            assert lib.hpf_explain(h, args[0], args[1], 6, 5, args[2], args[3]) == -1
        assert lib.hpf_explain(h, None, None, 0, 5, None, None) == 0          # cnt = 0 is fine, whatever the pointers
        assert not fac.any() and not con.any()                                # nothing was written
        assert all(np.array_equal(a, b) for a, b in zip(before, M.state()))   # the state is still readable and the same
        M.check(u, i, 5, "a good call after the refusals")
    finally:
        M.close()
    # no E on one side: HPF_ERR_STATE through hpf_predict's readiness path
    D = capi.Hpf(N_USERS, N_ITEMS, 20, hier=False, bias=False)
    try:
        D.set_state("BETA_E", _gamma(N_ITEMS, 20, 1))
        with pytest.raises(capi.HpfError, match=r"\(-6\)"):
            D.explain(u, i, 5)
        with pytest.raises(capi.HpfError, match=r"\(-6\)"):
            D.predict(u, i)
        D.set_state("THETA_E", _gamma(N_USERS, 20, 2))
        assert D.explain(u, i, 5)[0].shape == (6, 5)
    finally:
        D.close()
