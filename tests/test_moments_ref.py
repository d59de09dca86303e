"""CPU: the reference of hpf_score_moments (tests/moments_ref.py) against what it stands for.

1. The algebra: under a factorised posterior sum_k (E[t^2] E[b^2] - E[t]^2 E[b]^2) + the bias variances is X . Y, exactly,
   on random rationals.
2. A Gamma(shape a, rate r) has E[x] = a / r and E[x^2] = a (a + 1) / r^2 (mpmath integrates the density), so
   Var = E[x]^2 / a and E[x^2] = E^2 + E^2 / a: what the derived rows are made of.
3. numpy's X . Y stays within (C + 9) 2^-53 of the exact value on the very inputs tests/test_gpu_moments.py hands the GPU:
   the reference alone is inside the bound the GPU test imposes.
"""
import random
from fractions import Fraction

import numpy as np
import pytest

from tests import moments_ref as ref


def test_the_variance_is_one_dot_product_of_derived_rows():
    rnd = random.Random(7)
    F = lambda: Fraction(rnd.randint(1, 10 ** 6), rnd.randint(1, 10 ** 6))
    for K, bias in ((1, False), (3, True), (8, False), (17, True)):
        m_, a, n_, b = ([F() for _ in range(K)] for _ in range(4))
        direct, X, Y = Fraction(0), [], []
        for k in range(K):
            et2 = m_[k] ** 2 + m_[k] ** 2 / a[k]                       # E[theta^2] = E^2 + Var
            eb2 = n_[k] ** 2 + n_[k] ** 2 / b[k]
            direct += et2 * eb2 - m_[k] ** 2 * n_[k] ** 2
        X += [m_[k] ** 2 / a[k] for k in range(K)] + [m_[k] ** 2 for k in range(K)]
        Y += [n_[k] ** 2 + n_[k] ** 2 / b[k] for k in range(K)] + [n_[k] ** 2 / b[k] for k in range(K)]
        if bias:
            ue, ua, ie, ia = F(), F(), F(), F()
            direct += ue ** 2 / ua + ie ** 2 / ia
            X += [ue ** 2 / ua, Fraction(1)]
            Y += [Fraction(1), ie ** 2 / ia]
        assert len(X) == len(Y) == 2 * K + 2 * bias
        assert sum(x * y for x, y in zip(X, Y)) == direct


def test_second_moment_of_a_gamma():
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 40
    for a, r in ((0.3, 0.3), (0.31, 7.5), (2.0, 1.0), (37.25, 0.125), (1500.0, 900.0)):
        a_, r_ = mp.mpf(a), mp.mpf(r)
        dens = lambda x: r_ ** a_ / mp.gamma(a_) * x ** (a_ - 1) * mp.exp(-r_ * x)
        peak = max(a_ / r_, mp.mpf(1) / r_)
        cuts = [0, peak / 100, peak, 4 * peak, 40 * peak, mp.inf]
        e1 = mp.quad(lambda x: x * dens(x), cuts)
        e2 = mp.quad(lambda x: x * x * dens(x), cuts)
        assert abs(e1 - a_ / r_) <= mp.mpf(10) ** -20 * e1
        assert abs(e2 - a_ * (a_ + 1) / r_ ** 2) <= mp.mpf(10) ** -20 * e2
        E = a_ / r_
        assert abs((E * E + E * E / a_) - e2) <= mp.mpf(10) ** -20 * e2            # E[x^2] = q + q / shape


def test_derived_rows_layout_and_bits():
    st = ref.gamma_state(3, 4, 2, True, 5)
    X, Y = ref.derived_rows(st, True)
    assert X.shape == (3, 6) and Y.shape == (4, 6)
    m_, a, n_, b = st["THETA_E"], st["THETA_SHAPE"], st["BETA_E"], st["BETA_SHAPE"]
    for u in range(3):
        for k in range(2):
            q = float(m_[u, k]) * float(m_[u, k])
            assert X[u, k] == q / float(a[u, k]) and X[u, 2 + k] == q
        assert X[u, 4] == float(st["UBIAS_E"][u]) * float(st["UBIAS_E"][u]) / float(st["UBIAS_SHAPE"][u]) and X[u, 5] == 1.0
    for i in range(4):
        for k in range(2):
            p = float(n_[i, k]) * float(n_[i, k])
            vb = p / float(b[i, k])
            assert Y[i, k] == p + vb and Y[i, 2 + k] == vb
        assert Y[i, 4] == 1.0 and Y[i, 5] == float(st["IBIAS_E"][i]) * float(st["IBIAS_E"][i]) / float(st["IBIAS_SHAPE"][i])
    X0, Y0 = ref.derived_rows(st, False)
    assert np.array_equal(X0, X[:, :4]) and np.array_equal(Y0, Y[:, :4])


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("K", ref.PAIR_KS)
def test_the_reference_is_inside_its_own_bound(K, bias):
    st, u, i = ref.pair_case(K, bias)
    X, Y = ref.derived_rows(st, bias)
    C = 2 * K + 2 * bias
    assert X.shape[1] == C and np.all(X >= 0) and np.all(Y >= 0)
    tiny = np.finfo(np.float64).tiny
    for v in (st["THETA_E"] ** 2, st["BETA_E"] ** 2, X[X > 0], Y[Y > 0]):          # no intermediate is subnormal
        assert np.all(v >= tiny)
    var = X @ Y.T
    chain = np.zeros((len(X), len(Y)))                                             # one accumulator, columns in order
    for c in range(C):
        chain += X[:, c:c + 1] * Y[None, :, c]
    for p in range(17):
        exact = ref.exact_var(st, bias, u[p], i[p])
        assert exact > 0
        assert ref.within(var[u[p], i[p]], exact, C), (K, bias, p)
        assert ref.within(chain[u[p], i[p]], exact, C), (K, bias, p)


def test_ucb_and_the_order():
    mean, var = np.array([1.0, 2.0, 0.5, 2.0]), np.array([4.0, 0.0, 9.0, 0.0])
    assert np.array_equal(ref.ucb(mean, var, 0.0), mean) and np.array_equal(ref.ucb(mean, var, 3.0), [7.0, 2.0, 9.5, 2.0])
    key = np.array([[7.0, 2.0, 9.5, 2.0, 0.0]])
    assert ref.top_lists(key, 7).tolist() == [[2, 0, 1, 3, 4, ref.NONE, ref.NONE]]
    assert ref.take(np.arange(10.0).reshape(2, 5), [1], np.array([[4, ref.NONE]], np.uint32)).tolist() == [[9.0, 0.0]]
