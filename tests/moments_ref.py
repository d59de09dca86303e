"""The definition of hpf_score_moments / hpf_recommend_ucb (include/hpf.h) in numpy and in exact
arithmetic: the derived rows X, Y bit for bit, the variance of a pair as a Fraction, the optimistic score, the ordering
rule -- and the inputs the CPU and the GPU tests share.

numpy's elementwise *, / and + are single IEEE fp64 operations and np.sqrt is correctly rounded, so X, Y and ucb below are
the doubles the definition names.  The dot product X_u . Y_i itself is NOT formed here in the library's order: the GPU
tests take it from hpf_scores on a second handle with K' = C, E[theta] = X, E[beta] = Y."""
from fractions import Fraction

import numpy as np

NONE = 0xFFFFFFFF
U = 2.0 ** -53


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def derived_rows(st, bias):
    """st: THETA_E, THETA_SHAPE, BETA_E, BETA_SHAPE [rows x K] and with bias UBIAS_* / IBIAS_* [rows] -> X [n x C], Y [m x C],
    C = 2 K + 2 * bias: the five operations of the definition, each one rounding"""
    m_, a = np.asarray(st["THETA_E"], np.float64), np.asarray(st["THETA_SHAPE"], np.float64)
    n_, b = np.asarray(st["BETA_E"], np.float64), np.asarray(st["BETA_SHAPE"], np.float64)
    q = m_ * m_
    vt = q / a
    p = n_ * n_
    vb = p / b
    s = p + vb
    X, Y = [vt, q], [s, vb]
    if bias:
        ue, ie = np.asarray(st["UBIAS_E"], np.float64), np.asarray(st["IBIAS_E"], np.float64)
        uv = (ue * ue) / np.asarray(st["UBIAS_SHAPE"], np.float64)
        iv = (ie * ie) / np.asarray(st["IBIAS_SHAPE"], np.float64)
        X += [uv[:, None], np.ones((len(ue), 1))]
        Y += [np.ones((len(ie), 1)), iv[:, None]]
    return np.ascontiguousarray(np.hstack(X)), np.ascontiguousarray(np.hstack(Y))


def exact_sum(terms):
    """the sum of Fractions without a gcd per addition (a thousand denominators of 100 bits: the reduced running sum would
    cost a long gcd at every step)"""
    num, den = 0, 1
    for t in terms:
        num, den = num * t.denominator + t.numerator * den, den * t.denominator
    return Fraction(num, den)


def exact_var(st, bias, u, i):
    """the variance of the score of (u, i) in rational arithmetic from the doubles E and shape:
    sum_k (vt s + q vb) = sum_k m^2 n^2 (1 / a + 1 / (a b) + 1 / b), + Var ubias_u + Var ibias_i"""
    F = Fraction
    terms = []
    for m_, a, n_, b in zip(st["THETA_E"][u], st["THETA_SHAPE"][u], st["BETA_E"][i], st["BETA_SHAPE"][i]):
        m_, a, n_, b = F(float(m_)), F(float(a)), F(float(n_)), F(float(b))
        q, p = m_ * m_, n_ * n_
        vt, vb = q / a, p / b
        terms.append(vt * (p + vb) + q * vb)
    if bias:
        terms.append(F(float(st["UBIAS_E"][u])) ** 2 / F(float(st["UBIAS_SHAPE"][u])))
        terms.append(F(float(st["IBIAS_E"][i])) ** 2 / F(float(st["IBIAS_SHAPE"][i])))
    return exact_sum(terms)


def within(got, exact, C):
    """|got - exact| <= (C + 9) 2^-53 exact, decided in rational arithmetic"""
    return abs(Fraction(float(got)) - exact) <= (C + 9) * Fraction(1, 2 ** 53) * exact


def ucb(mean, var, z):
    """sd = sqrt(var), t = z * sd, ucb = mean + t: three operations"""
    sd = np.sqrt(np.asarray(var, np.float64))
    t = np.float64(z) * sd
    return np.asarray(mean, np.float64) + t


def top_lists(key, topn):
    """key [rows x m], masked entries already +0.0 -> items [rows x topn] by (bit pattern descending, item ascending);
    entries beyond m are NONE"""
    rows, m = key.shape
    out = np.full((rows, topn), NONE, np.uint32)
    ids = np.arange(m)
    for r in range(rows):
        order = np.lexsort((ids, ~bits(key[r])))[:topn]
        out[r, :order.size] = order
    return out


def take(mat, rows, items):
    """mat[rows[b], items[b, j]], 0.0 where items is NONE"""
    pad = items == NONE
    v = mat[np.asarray(rows, np.int64)[:, None], np.where(pad, 0, items).astype(np.int64)]
    return np.where(pad, 0.0, v)


# ---------------------------------------------------------------------------------------------------------------------
# the inputs of the pair tests (tests/test_moments_ref.py checks the reference on them, tests/test_gpu_moments.py the GPU)
# ---------------------------------------------------------------------------------------------------------------------
PAIR_N, PAIR_M = 37, 131
PAIR_KS = (1, 5, 16, 100, 511)


def gamma_state(n, m, K, bias, seed):
    """E and shape of a Gamma(0.3, .) model after some ratings: positive expectations wide in magnitude, shapes from the
    prior's 0.3 up to thousands.  Every value is a normal double well inside the range: no intermediate of the definition is
    subnormal"""
    rng = np.random.default_rng(seed)

    def side(rows, cols):
        shape = 0.3 + rng.gamma(0.5, 40.0, (rows, cols))
        rate = 0.3 + rng.gamma(2.0, 3.0, (rows, 1)) * np.ones((1, cols))
        return np.ascontiguousarray(shape / rate), np.ascontiguousarray(shape)

    st = {}
    st["THETA_E"], st["THETA_SHAPE"] = side(n, K)
    st["BETA_E"], st["BETA_SHAPE"] = side(m, K)
    if bias:
        e, s = side(n, 1)
        st["UBIAS_E"], st["UBIAS_SHAPE"] = e[:, 0].copy(), s[:, 0].copy()
        e, s = side(m, 1)
        st["IBIAS_E"], st["IBIAS_SHAPE"] = e[:, 0].copy(), s[:, 0].copy()
    return st


def pair_case(K, bias):
    """-> (state, u, i): 49 pairs over PAIR_N users and PAIR_M items, the last nine repeating earlier ones"""
    st = gamma_state(PAIR_N, PAIR_M, K, bias, 1000 + 2 * K + int(bias))
    rng = np.random.default_rng(K)
    u = rng.integers(0, PAIR_N, 40).astype(np.uint32)
    i = rng.integers(0, PAIR_M, 40).astype(np.uint32)
    u[0], i[0], u[1], i[1] = 0, 0, PAIR_N - 1, PAIR_M - 1
    return st, np.concatenate([u, u[3:12]]), np.concatenate([i, i[3:12]])
