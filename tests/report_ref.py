"""High-precision references of the report quantities, term by term -- the held-out likelihood of a pair, the ELBO's
term of a nonzero and its Gamma term of a matrix or prior-array element -- for tests/test_report_ref.py (against the CPU
oracle) and tests/test_gpu_report_terms.py (against the kernels).  Test infrastructure.

Every evaluator takes the doubles a kernel is handed, evaluates the reference program's formula on them with mpmath at
DPS digits -- nothing is rounded on the way and no value is recomputed from another -- and returns

    (exact, A)      exact: the term, an mpf;   A: the sum of the absolute values of the term's addends, a float

A is what an error is measured in: a comparison is |computed - exact| <= c u A with u = 2^-53.  An addend is whatever
the arithmetic rounds: each product of a dot product (A = sum |Et Eb|), each summand of the formula, and for a
log-sum-exp the maximum, the logarithm of the sum, and -- weighted by its share p_c of the sum, through which an error
of the exponent reaches the result -- per column 1 (the exponential and its place in the sum), |x_c| (the rounding of
x_c = Lt_c + Lb_c) and |x_c - max| (the rounding of the difference).  For the binary likelihood log(1 - exp(-s)) it is
1 / (1 - exp(-s)) + |ll|: a relative error of exp(-s) enters divided by 1 - exp(-s).

The plain_* functions restate the reference program's own double arithmetic (hgaprec.cc / gpbase.hh as oracle/hpf_oracle.c
restates them): numpy doubles, glibc's log / exp / lgamma through `math`, serial order, log y! as the serial sum of
log i.  c_ref(...) is the largest |plain - exact| / (u A) over a set of terms: what the formula costs in doubles when
nothing but rounding goes wrong, measured on the very inputs of a test.  A kernel gets c = 4 max(1, c_ref).
"""
from __future__ import annotations

import math

import mpmath as mp
import numpy as np

DPS = 50
U = 2.0 ** -53
CLAMP = 1e-30


def _f(x):
    return mp.mpf(float(x))


def c_for(c_ref):
    """the factor a kernel is held to: its libm takes a few ulp where glibc takes one, it contracts to fma and it sums
    a dot product as a 16-lane tree -- each changes the rounding of an addend by a small factor, never its magnitude"""
    return 4.0 * max(1.0, float(c_ref))


def ratio(computed, exact, A):
    """|computed - exact| / (u A), inf for a value that is not finite (or an A of 0 with any error at all)"""
    if not math.isfinite(computed):
        return math.inf
    with mp.workdps(DPS):
        err = abs(_f(computed) - exact)
        if err == 0:
            return 0.0
        return float(err / (mp.mpf(U) * _f(A))) if A > 0.0 else math.inf


def abs_err(computed, exact):
    """|computed - exact| as a float; inf for a value that is not finite"""
    if not math.isfinite(computed):
        return math.inf
    with mp.workdps(DPS):
        return float(abs(_f(computed) - exact))


# ---- held-out likelihood of one pair (rating_likelihood / rating_likelihood_hier) ------------------------------------
_LOGFACT = {}


def _mp_logfact(y):
    if y not in _LOGFACT:
        _LOGFACT[y] = mp.loggamma(mp.mpf(y + 1))
    return _LOGFACT[y]


def _mp_score(et, eb, ubias, ibias):
    s, A = mp.mpf(0), mp.mpf(0)
    for a, b in zip(et, eb):
        p = _f(a) * _f(b)
        s += p
        A += abs(p)
    if ubias is not None:
        s += _f(ubias) + _f(ibias)
        A += abs(_f(ubias)) + abs(_f(ibias))
    return s, A


def pair_ll(et, eb, y, ubias=None, ibias=None, binary=False):
    """s = sum_k et_k eb_k (+ ubias + ibias), clamped at 1e-30; Poisson: y log s - s - log y!; binary: -s for y = 0, else
    log(1 - exp(-s)).  y is the rating as handed in: the reference's yval_t keeps its low 8 bits"""
    with mp.workdps(DPS):
        s, As = _mp_score(et, eb, ubias, ibias)
        if s < _f(CLAMP):
            s, As = _f(CLAMP), _f(CLAMP)
        y = int(y) & 0xFF
        if binary:
            if y == 0:
                return -s, float(As)
            q = 1 - mp.exp(-s)
            ll = mp.log(q)
            return ll, float(1 / q + abs(ll))
        ll = y * mp.log(s) - s - _mp_logfact(y)
        return ll, float(abs(y * mp.log(s)) + As + abs(_mp_logfact(y)))


def plain_logfact_table():
    lf = np.zeros(256)
    for y in range(2, 256):
        lf[y] = lf[y - 1] + math.log(float(y))
    return lf


_PLAIN_LF = plain_logfact_table()


def plain_pair_ll(et, eb, y, ubias=None, ibias=None, binary=False):
    s = 0.0
    for a, b in zip(et, eb):
        s += float(a) * float(b)
    if ubias is not None:
        s += float(ubias) + float(ibias)
    if s < CLAMP:
        s = CLAMP
    y = int(y) & 0xFF
    if binary:
        if y == 0:
            return -s
        q = 1.0 - math.exp(-s)
        return math.log(q) if q > 0.0 else -math.inf
    return y * math.log(s) - s - _PLAIN_LF[y]


# ---- the ELBO's term of one nonzero (HGAPRec::logl) ----------------------------------------------------------------------
def _yy(y):
    y = 1 if y is None else int(y)
    return y, max(y, 1)


def _dot_part(et, eb, ubias, ibias):
    s, A = _mp_score(et, eb, ubias, ibias)
    return s, A


def nnz_term(lt, lb, et, eb, y, ubias=None, ibias=None):
    """y yy (logsumexp_c(lt_c + lb_c) - log yy) - sum_k et_k eb_k (- ubias - ibias), yy = max(y, 1); y None: 1.
    lt, lb: the C live columns of the two Elog rows (with -bias: the own bias in its slot, 0 in the other side's);
    et, eb: the K columns of E; ubias, ibias: the two E of the biases"""
    with mp.workdps(DPS):
        y, yy = _yy(y)
        x = [_f(a) + _f(b) for a, b in zip(lt, lb)]
        mx = max(x)
        e = [mp.exp(v - mx) for v in x]
        se = sum(e)
        lse = mx + mp.log(se)
        A_lse = abs(mx) + abs(mp.log(se)) + sum(p / se * (1 + abs(v) + abs(v - mx)) for p, v in zip(e, x))
        dot, A_dot = _dot_part(et, eb, ubias, ibias)
        exact = y * yy * (lse - mp.log(yy)) - dot
        return exact, float(y * yy * (A_lse + abs(mp.log(yy))) + A_dot)


def nnz_term_w(wt, wb, mt, mb, et, eb, y, ubias=None, ibias=None):
    """the same from the rows of W = exp(Elog - M) and the row maxima as given: logsumexp = log(sum_c wt_c wb_c) + mt + mb
    (over the whole stride: padding columns hold 0).  -inf where the sum is 0"""
    with mp.workdps(DPS):
        y, yy = _yy(y)
        z = sum(_f(a) * _f(b) for a, b in zip(wt, wb))
        dot, A_dot = _dot_part(et, eb, ubias, ibias)
        if z == 0:
            return -mp.inf, math.inf
        lz = mp.log(z)
        lse = lz + _f(mt) + _f(mb)
        A_lse = abs(lz) + abs(_f(mt)) + abs(_f(mb)) + 1
        exact = y * yy * (lse - mp.log(yy)) - dot
        return exact, float(y * yy * (A_lse + abs(mp.log(yy))) + A_dot)


def plain_logsum(x):
    """matrix.hh logsum: the running pairwise form"""
    r = float(x[0])
    for v in x[1:]:
        v = float(v)
        if v < r:
            r = r + math.log(1.0 + math.exp(v - r))
        else:
            r = v + math.log(1.0 + math.exp(r - v))
    return r


def plain_nnz_term(lt, lb, et, eb, y, ubias=None, ibias=None):
    """as HGAPRec::logl walks a nonzero: phi = yy lognormalize(x), sum_k y phi_k (x_k - log phi_k), minus the products"""
    y, yy = _yy(y)
    x = [float(a) + float(b) for a, b in zip(lt, lb)]
    ls = plain_logsum(x)
    phi = [math.exp(v - ls) for v in x]
    if y > 1:
        phi = [p * y for p in phi]
    K = len(et)
    v = 0.0
    for k in range(K):
        v += y * phi[k] * (x[k] - math.log(phi[k])) if phi[k] > 0.0 else 0.0
    s = v
    for k in range(K, len(x)):
        s += y * phi[k] * (x[k] - math.log(phi[k])) if phi[k] > 0.0 else 0.0
    for k in range(K):
        s -= float(et[k]) * float(eb[k])
    if ubias is not None:
        s -= float(ubias)
        s -= float(ibias)
    return s


# ---- the ELBO's Gamma term of one element (compute_elbo_term_helper; gp_elbo_term of oracle/hpf_oracle.c) ----------------
_LGAMMA = {}


def _mp_lgamma(a):
    a = float(a)
    if a not in _LGAMMA:
        _LGAMMA[a] = mp.loggamma(mp.mpf(a))
    return _LGAMMA[a]


def gamma_term(shape, rate, ev, el, s_prior, r, log_r=None):
    """s0 log_r + (s0 - 1) el - (r ev + lgamma(s0)) - (a log b + (a - 1) el) + (b ev + lgamma(a)) with a = shape and
    b = rate, each replaced by 1e-30 unless > 0.  r, log_r: E and E[log] of the rate's prior -- the row's xi (eta) for a
    hierarchical matrix element, else r = r_prior and log_r = None: log(r_prior).  A prior-array element is the same
    formula with its own shape and rate and the fixed prior.  The lgamma of a shape is taken from a table of unique shapes"""
    with mp.workdps(DPS):
        a = _f(shape) if shape > 0.0 else _f(CLAMP)
        b = _f(rate) if rate > 0.0 else _f(CLAMP)
        s0, r, ev, el = _f(s_prior), _f(r), _f(ev), _f(el)
        lr = mp.log(r) if log_r is None else _f(log_r)
        adds = [s0 * lr, (s0 - 1) * el, -(r * ev), -_mp_lgamma(s_prior), -(a * mp.log(b)), -((a - 1) * el), b * ev,
                _mp_lgamma(float(a))]
        return sum(adds), float(sum(abs(t) for t in adds))


def plain_gamma_term(shape, rate, ev, el, s_prior, r, log_r=None):
    a = shape if shape > 0.0 else CLAMP
    b = rate if rate > 0.0 else CLAMP
    lr = math.log(r) if log_r is None else log_r
    s = 0.0
    s += s_prior * lr + (s_prior - 1) * el
    s -= r * ev + math.lgamma(s_prior)
    s -= a * math.log(b) + (a - 1) * el
    s += b * ev + math.lgamma(a)
    return s


# ---- sums and c_ref -------------------------------------------------------------------------------------------------------
def c_ref(plain, terms):
    """the largest |plain_k - exact_k| / (u A_k); terms: (exact, A) pairs.  Terms the plain arithmetic itself gives as
    -inf where the exact one is finite (or the reverse) are the caller's to keep out: they have no error in u A"""
    return max([ratio(p, e, A) for p, (e, A) in zip(plain, terms)], default=0.0)


def sum_bound(terms, c):
    """-> (exact sum, bound) of a sum of terms computed one by one within c u A and added in doubles in any order:
    the terms' bounds plus n u sum |term| for the additions"""
    with mp.workdps(DPS):
        total = sum((e for e, _ in terms), mp.mpf(0))
        mag = sum((abs(e) for e, _ in terms), mp.mpf(0))
        bound = c * U * math.fsum(A for _, A in terms) + len(terms) * U * float(mag)
        return total, bound


# ---- the whole ELBO from an exported state ----------------------------------------------------------------------------------
def elbo_terms(st, used, pairs, K, hier, bias, s_prior, r_prior):
    """every term of the ELBO of a state as the C-ABI or the oracle exports it.
    st: {"THETA_SHAPE": ..., "THETA_RATE": ..., "THETA_E": ..., "THETA_ELOG": ..., "BETA_...", "XI_...", ...};
    used: with hier {"XI": (E, ELOG), "ETA": (E, ELOG)} as they stood BEFORE the last iteration -- theta's rates were built
    from them (set_prior_rate runs before xi is updated), and the ELBO reads them as the prior of theta's rate;
    pairs: (user, item, rating or None, multiplicity) of every unique line.
    -> (nnz, gamma): lists of (exact, A, plain, multiplicity)"""
    nnz, gamma = [], []
    TE, TL, BE, BL = st["THETA_E"], st["THETA_ELOG"], st["BETA_E"], st["BETA_ELOG"]
    for u, i, y, mult in pairs:
        lt, lb = list(TL[u]), list(BL[i])
        ub = ib = None
        if bias:
            lt += [st["UBIAS_ELOG"][u], 0.0]
            lb += [0.0, st["IBIAS_ELOG"][i]]
            ub, ib = st["UBIAS_E"][u], st["IBIAS_E"][i]
        e, A = nnz_term(lt, lb, TE[u], BE[i], y, ub, ib)
        nnz.append((e, A, plain_nnz_term(lt, lb, TE[u], BE[i], y, ub, ib), int(mult)))
    for name, prior in (("THETA", "XI"), ("BETA", "ETA")):
        S, R, E, L = (st[f"{name}_{k}"] for k in ("SHAPE", "RATE", "E", "ELOG"))
        for row in range(S.shape[0]):
            r, lr = (float(used[prior][0][row]), float(used[prior][1][row])) if hier else (r_prior, None)
            for k in range(K):
                rate = float(R[row, k] if hier else R[k])
                args = (float(S[row, k]), rate, float(E[row, k]), float(L[row, k]), s_prior, r, lr)
                gamma.append(gamma_term(*args) + (plain_gamma_term(*args), 1))
    arrays = (["XI", "ETA"] if hier else []) + (["UBIAS", "IBIAS"] if bias else [])
    for name in arrays:
        S, R, E, L = (st[f"{name}_{k}"] for k in ("SHAPE", "RATE", "E", "ELOG"))
        for row in range(S.shape[0]):
            args = (float(S[row]), float(R[row]), float(E[row]), float(L[row]), s_prior, r_prior, None)
            gamma.append(gamma_term(*args) + (plain_gamma_term(*args), 1))
    return nnz, gamma


def elbo_bound(nnz, gamma, c_nnz, c_gamma):
    """-> (exact ELBO, bound): every line of the data adds its term (a unique pair `multiplicity` times), every term within
    its c u A, and the n additions cost n u sum |term|"""
    with mp.workdps(DPS):
        total = mp.mpf(0)
        mag = mp.mpf(0)
        n = 0
        bound = 0.0
        for terms, c in ((nnz, c_nnz), (gamma, c_gamma)):
            for e, A, _, mult in terms:
                total += mult * e
                mag += mult * abs(e)
                n += mult
                bound += c * U * A * mult
        return total, bound + n * U * float(mag)


def total_A(*term_lists):
    """sum of multiplicity x A over lists of (exact, A, plain, multiplicity): the unit an error of a total is reported in"""
    return math.fsum(t[3] * t[1] for terms in term_lists for t in terms)
