"""The sampler of hpf_sample_state / hpf_recommend_thompson (hgaprec_amd/csrc/hpf_rng.hpp) in numpy,
line by line: Philox4x32-10 in uint64 arithmetic, the 52-bit uniforms, Marsaglia-Tsang with the acceptance test in the
form in which nothing cancels at large shapes -- and the inputs the CPU and the GPU tests share.

numpy's elementwise +, -, *, / and np.sqrt are single correctly rounded fp64 operations; log, log1p, cos and exp are the
host's, each within a few units of the last place like the device's (ocml).  A sample therefore agrees with the device's
within the bound below wherever both take the same decisions, and the trace says how far each decision was from its edge."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)
ATTEMPTS = 32
TWO_PI = 2.0 * np.pi                  # the double nearest 2 pi (a power of two times the double nearest pi)
U = 2.0 ** -52


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 of the counters (c0, c1, c2, c3) and keys (k0, k1): arrays (or scalars) of 32-bit values held in
    uint64 -> four uint64 arrays of 32-bit words"""
    c0, c1, c2, c3, k0, k1 = (np.asarray(x, dtype=np.uint64) & MASK32 for x in (c0, c1, c2, c3, k0, k1))
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(c0, c1, c2, c3, k0, k1)
    m0, m1, w0, w1, s32 = np.uint64(M0), np.uint64(M1), np.uint64(W0), np.uint64(W1), np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2                       # 32 x 32 -> 64 bits: no overflow
        hi0, lo0, hi1, lo1 = p0 >> s32, p0 & MASK32, p1 >> s32, p1 & MASK32
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + w0) & MASK32, (k1 + w1) & MASK32
    return c0, c1, c2, c3


def philox_int(c, k):
    """the same in plain Python integers, for the known answers: c a 4-tuple, k a 2-tuple -> 4-tuple"""
    c0, c1, c2, c3 = c
    k0, k1 = k
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c3 ^ k1, p0 & 0xFFFFFFFF
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def uniform(x, y):
    """u = (n + 0.5) 2^-52 of n = (x >> 6) 2^26 + (y >> 6): exact, strictly inside (0, 1)"""
    n = ((np.asarray(x, np.uint64) >> np.uint64(6)) << np.uint64(26)) + (np.asarray(y, np.uint64) >> np.uint64(6))
    return (n.astype(np.float64) + 0.5) * U


def element_block(seed, draw, obj, row, col, b, j):
    seed = int(seed)
    return philox(col, row, draw, int(obj) | (int(b) << 4) | (int(j) << 8), seed & 0xFFFFFFFF, seed >> 32)


def gamma_unit(seed, draw, obj, row, col, a):
    """Gamma(a, 1) variates of the elements (row, col) (arrays of one shape, like a) of side obj in draw `draw` -> (g, trace)
    trace: attempt  the accepted attempt (-1: none)
           t        1 + w of the accepted attempt (0.0 where none)
           q        log(u4) / a where a < 1, else 0.0
           ratio    the smallest margin / A over the decisions taken for the element, margin = |log u3 - rhs|,
                    A = 0.5 z^2 + d (|l| + |p|) + |log u3| (inf where no decision was taken)
           tries    attempts made"""
    a = np.asarray(a, np.float64)
    row = np.broadcast_to(np.asarray(row, np.uint64), a.shape).ravel()
    col = np.broadcast_to(np.asarray(col, np.uint64), a.shape).ravel()
    shape, a = a.shape, a.ravel()
    with np.errstate(all="ignore"):
        small = a < 1.0
        ap = np.where(small, a + 1.0, a)
        d = ap - 1.0 / 3.0
        cc = 1.0 / np.sqrt(9.0 * d)
        g, u4 = ap.copy(), np.ones_like(a)
        attempt = np.full(a.shape, -1, np.int64)
        t_acc = np.zeros_like(a)
        ratio = np.full(a.shape, np.inf)
        tries = np.zeros(a.shape, np.int64)
        live = np.arange(a.size)
        for j in range(ATTEMPTS):
            if not live.size:
                break
            tries[live] += 1
            w0, w1, w2, w3 = element_block(seed, draw, obj, row[live], col[live], 0, j)
            u1, u2 = uniform(w0, w1), uniform(w2, w3)
            z = np.sqrt(-2.0 * np.log(u1)) * np.cos(TWO_PI * u2)
            w = cc[live] * z
            ok = w > -1.0
            idx, z, w = live[ok], z[ok], w[ok]
            w0, w1, w2, w3 = element_block(seed, draw, obj, row[idx], col[idx], 1, j)
            u3, u4j = uniform(w0, w1), uniform(w2, w3)
            l = 3.0 * np.log1p(w)
            p = w * (3.0 + w * (3.0 + w))
            h = l - p
            l3 = np.log(u3)
            zz = (0.5 * z) * z
            rhs = zz + d[idx] * h
            acc = l3 < rhs
            A = zz + d[idx] * (np.abs(l) + np.abs(p)) + np.abs(l3)
            ratio[idx] = np.minimum(ratio[idx], np.abs(l3 - rhs) / A)
            t = 1.0 + w
            hit = idx[acc]
            g[hit] = d[hit] * ((t[acc] * t[acc]) * t[acc])
            u4[hit] = u4j[acc]
            attempt[hit] = j
            t_acc[hit] = t[acc]
            done = np.zeros(a.size, bool)
            done[hit] = True
            live = live[~done[live]]
        q = np.where(small, np.log(u4) / a, 0.0)
        g = np.where(small, g * np.exp(q), g)
    tr = {"attempt": attempt.reshape(shape), "t": t_acc.reshape(shape), "q": q.reshape(shape), "ratio": ratio.reshape(shape),
          "tries": tries.reshape(shape)}
    return g.reshape(shape), tr


def sample_side(seed, draw, obj, E, S, ids=None, bias_E=None, bias_S=None, bias_col=None):
    """hpf_sample_state of one side: E, S [rows x K] (and with bias bias_E, bias_S [rows], the side's bias at column
    bias_col of the handle's row layout); ids: the rows' ids on their side (default 0 .. rows - 1) -> (out [rows x C], trace)"""
    E, S = np.asarray(E, np.float64), np.asarray(S, np.float64)
    rows, K = E.shape
    ids = np.arange(rows, dtype=np.uint64) if ids is None else np.asarray(ids, np.uint64)
    cols = np.arange(K, dtype=np.uint64)
    if bias_E is not None:
        E = np.hstack([E, np.asarray(bias_E, np.float64)[:, None]])
        S = np.hstack([S, np.asarray(bias_S, np.float64)[:, None]])
        cols = np.append(cols, np.uint64(bias_col))
    r = np.broadcast_to(ids[:, None], E.shape)
    c = np.broadcast_to(cols[None, :], E.shape)
    g, tr = gamma_unit(seed, draw, obj, r, c, S)
    with np.errstate(all="ignore"):
        out = g * (E / S)
    return out, tr


def bound(tr, a):
    """the relative bound of a device sample against this reference, in units of 2^-52: 32 + 16 / (1 + w) + 4 |log(u4) / a|,
    the last term only for a < 1 (at most 2 ulp per ocml call through the condition of each step)"""
    with np.errstate(all="ignore"):
        b = 32.0 + 16.0 / tr["t"]
    return (b + np.where(np.asarray(a) < 1.0, 4.0 * np.abs(tr["q"]), 0.0)) * U


# ---- what the tests share --------------------------------------------------------------------------------------------------
KS_SHAPES = [0.05, 0.3, float(np.nextafter(1.0, 0.0)), 1.0, 3.7, 100.0, 1e4, 1e8]
KS_DRAWS = 4096
KS_CAP = float(np.sqrt(np.log(2.0 / 1e-6) / 2.0) / 64.0)          # DKW-Massart at a false-alarm rate of 1e-6 per shape: 0.0421
MARGIN_MIN, T_MIN = 2.0 ** -44, 2.0 ** -40                         # the precondition of the GPU value test
SEED, DRAW = 20261021, 0                                           # of the value test


def ks_distance(x, a):
    """Kolmogorov-Smirnov distance of the sample x from Gamma(a, 1)"""
    from scipy.special import gammainc
    x = np.sort(np.asarray(x, np.float64))
    n = x.size
    F = gammainc(a, x)
    return float(max(np.max(np.arange(1, n + 1) / n - F), np.max(F - np.arange(n) / n)))


def value_case(K, bias, n=257, m=130, rng_seed=7):
    """the inputs of the GPU value test: E random in [0, 3) with a few exact zeros, shapes log-uniform in [0.05, 1e8] with
    0.3, 1 and its two neighbours planted -> dict of hpf_set_state arrays (dense, the host layout)"""
    r = np.random.default_rng(rng_seed + 1000 * K + (1 if bias else 0))
    st = {}
    for side, rows, en, sn, be, bs in (("u", n, "THETA_E", "THETA_SHAPE", "UBIAS_E", "UBIAS_SHAPE"),
                                        ("i", m, "BETA_E", "BETA_SHAPE", "IBIAS_E", "IBIAS_SHAPE")):
        C = K + (1 if bias else 0)
        E = r.random((rows, C)) * 3.0
        S = np.exp(r.uniform(np.log(0.05), np.log(1e8), (rows, C)))
        E.ravel()[r.choice(E.size, 7, replace=False)] = 0.0
        planted = [0.3, 1.0, float(np.nextafter(1.0, 0.0)), float(np.nextafter(1.0, 2.0))]
        S.ravel()[r.choice(S.size, len(planted), replace=False)] = planted
        st[en], st[sn] = np.ascontiguousarray(E[:, :K]), np.ascontiguousarray(S[:, :K])
        if bias:
            st[be], st[bs] = np.ascontiguousarray(E[:, K]), np.ascontiguousarray(S[:, K])
    return st


def reference_sides(st, K, bias, seed, draw, u_ids=None, i_ids=None):
    """both sides' hpf_sample_state outputs from a value_case-style dict: ((theta~, trace, shapes), (beta~, trace, shapes))"""
    out = []
    for obj, en, sn, be, bs, bc, ids in ((0, "THETA_E", "THETA_SHAPE", "UBIAS_E", "UBIAS_SHAPE", K, u_ids),
                                         (1, "BETA_E", "BETA_SHAPE", "IBIAS_E", "IBIAS_SHAPE", K + 1, i_ids)):
        E, S = st[en], st[sn]
        bE, bS = (st[be], st[bs]) if bias else (None, None)
        if ids is not None:
            E, S = E[ids], S[ids]
            if bias:
                bE, bS = bE[ids], bS[ids]
        x, tr = sample_side(seed, draw, obj, E, S, ids, bE, bS, bc)
        shapes = np.hstack([S, bS[:, None]]) if bias else S
        out.append((x, tr, shapes))
    return out
