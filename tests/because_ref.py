"""The definition of hpf_because (include/hpf.h), twice: exact() in mpmath at 60 digits and numpy64() in plain float64 --
and the inputs tests/test_gpu_because.py runs, so that tests/test_because_ref.py can check on a CPU what the GPU test
assumes about them (the identity, the distance of float64 from the exact values, the gaps between neighbours of a list).

For a user u with history hist(u) (the nonzeros of the CSR row in CSR order, yy = y if y > 1 else 1):
  phi_uic = exp(Elog theta_uc + Elog beta_ic) / sum_c' exp(...)   c over the K factors and, with bias, entry K = Elog ubias_u
                                                                  and entry K + 1 = Elog ibias_i (denominator only)
  D_uc    = s_prior + sum_i yy_i phi_uic                          c < K, with bias also c = K
  g_c     = E[theta_uc] E[beta_jc] / D_uc ,  g_K = E[ubias_u] / D_uK
  c(i->j) = yy_i sum_c phi_uic g_c ,  prior(j) = s_prior sum_c g_c
"""
import functools
import math

import mpmath
import numpy as np

S0 = R0 = 0.3
U53 = 2.0 ** -53
NONE = 0xFFFFFFFF
N_USERS, N_ITEMS = 40, 800
HISTORIES = (0, 1, 2, 63, 64, 65, 129, 700)       # the 64-block edges of the walk; users 0 .. 7
MP = mpmath.mp.clone()
MP.dps = 60

# (bias, hier, ratings, K, T): every combination of the three flags; every K of {1, 5, 64, 65, 100, 130} and every T of
# {1, 5, 32} at least once.  K = 1 goes with bias: without, phi is 1 for every history item and all contributions of a
# binary user tie exactly.
CASES = [
    (False, False, False, 5, 5),
    (False, False, True, 64, 32),
    (False, True, False, 65, 1),
    (False, True, True, 130, 5),
    (True, False, False, 1, 32),
    (True, False, True, 100, 5),
    (True, True, False, 100, 1),
    (True, True, True, 5, 32),
]


def case_id(c):
    return "bias%d-hier%d-val%d-K%d-T%d" % tuple(int(x) for x in c)


def digamma(x):
    """psi(x) for x > 0 in float64: the recurrence up to x >= 12, then the asymptotic series (the states are INPUTS of the
    definition, so this needs to be no better than a plausible Elog)"""
    x = np.asarray(x, np.float64).copy()
    s = np.zeros_like(x)
    for _ in range(12):
        small = x < 12.0
        s = np.where(small, s - 1.0 / x, s)
        x = np.where(small, x + 1.0, x)
    r = 1.0 / (x * x)
    return s + np.log(x) - 0.5 / x - r * (1.0 / 12 - r * (1.0 / 120 - r * (1.0 / 252 - r * (1.0 / 240 - r / 132))))


def gamma_side(rows, K, hier, bias, bias_rate, rng):
    """shape, rate, E = shape / rate, Elog = psi(shape) - log(rate) of one side: Gamma(0.3)-like shapes above 0.05 (Elog
    spreads up to about 25 inside a row) with one entry in a hundred near 0.0175 (psi = -57: spreads up to about 60).  A
    history item whose phi sits in ONE column to 2^-53 contributes g of that column whatever else its row holds, and two
    such items tie: the floor keeps the inputs away from that, tests/test_because_ref.py checks that it does"""
    sh = 0.05 + rng.gamma(0.3, 1.0, (rows, K))
    sh = np.where(rng.random((rows, K)) < 0.01, 0.0175 + 0.001 * rng.random((rows, K)), sh)
    rt = (R0 + rng.gamma(2.0, 1.0, (rows, 1)) + rng.uniform(0.5, 3.0, (1, K))) if hier else np.broadcast_to(R0 + rng.uniform(0.5, 3.0, K), (rows, K))
    st = {"SHAPE": sh, "RATE": rt if hier else rt[0].copy(), "E": sh / rt, "ELOG": digamma(sh) - np.log(rt)}
    if hier:
        ps, pr = np.full(rows, S0 + K * S0), R0 + st["E"].sum(1)
        st.update(P_SHAPE=ps, P_RATE=pr, P_E=ps / pr, P_ELOG=digamma(ps) - np.log(pr))
    if bias:
        bs, br = S0 + rng.gamma(0.3, 1.0, rows), np.full(rows, R0 + bias_rate)
        st.update(B_SHAPE=bs, B_E=bs / br, B_ELOG=digamma(bs) - np.log(br))
    return st


class Inputs:
    """one model of the GPU test: the CSR, the state of both sides as float64 arrays, and the targets"""

    def __init__(self, bias, hier, ratings, K, seed=0, n=N_USERS, m=N_ITEMS, histories=HISTORIES):
        rng = np.random.default_rng(1000 + seed + 7 * K + 2 * bias + hier)
        self.bias, self.hier, self.K, self.n, self.m = bool(bias), bool(hier), K, n, m
        degs = list(histories) + [int(d) for d in rng.integers(1, 21, n - len(histories))]
        rows = [rng.permutation(m)[:d].astype(np.uint32) for d in degs]
        self.rowptr = np.zeros(n + 1, np.int64)
        self.rowptr[1:] = np.cumsum(degs)
        self.col = np.concatenate(rows).astype(np.uint32)
        self.val = rng.choice(np.array([0, 1, 2, 255], np.uint8), self.col.size) if ratings else None
        self.user = gamma_side(n, K, hier, bias, m, rng)
        self.item = gamma_side(m, K, hier, bias, n, rng)
        # the selected users: those of the block edges and eight others; one to three targets each, the first of a user
        # with a history out of that history
        self.users = np.concatenate([np.arange(len(histories)), len(histories) + rng.permutation(n - len(histories))[:8]]).astype(np.uint32)
        t_ptr, t_items = [0], []
        for u in self.users:
            t = [int(x) for x in rng.integers(0, m, int(rng.integers(1, 4)))]
            h = self.history(u)[0]
            if h.size:
                t[0] = int(h[rng.integers(0, h.size)])
            t_items += t
            t_ptr.append(len(t_items))
        self.t_ptr, self.t_items = np.array(t_ptr, np.uint64), np.array(t_items, np.uint32)

    def history(self, u):
        a, b = int(self.rowptr[u]), int(self.rowptr[u + 1])
        items = self.col[a:b]
        yy = np.ones(b - a) if self.val is None else np.where(self.val[a:b] > 1, self.val[a:b], 1).astype(np.float64)
        return items, yy

    def states(self):
        """name -> array, everything hpf_set_state takes for a start state of this model"""
        out = {}
        for side, o, p, b in ((self.user, "THETA", "XI", "UBIAS"), (self.item, "BETA", "ETA", "IBIAS")):
            out.update({o + "_SHAPE": side["SHAPE"], o + "_E": side["E"], o + "_ELOG": side["ELOG"]})
            if self.hier:
                out.update({p + "_SHAPE": side["P_SHAPE"], p + "_RATE": side["P_RATE"], p + "_E": side["P_E"], p + "_ELOG": side["P_ELOG"]})
            if self.bias:
                out.update({b + "_SHAPE": side["B_SHAPE"], b + "_E": side["B_E"], b + "_ELOG": side["B_ELOG"]})
        return out

    def pairs(self):
        """(selected index, user, target item) of every target, in the outputs' order"""
        return [(b, int(self.users[b]), int(self.t_items[q])) for b in range(len(self.users)) for q in range(int(self.t_ptr[b]), int(self.t_ptr[b + 1]))]


class State:
    """E and Elog of both sides as a call reads them (hpf_get_state's arrays)"""

    def __init__(self, Et, Lt, Eb, Lb, ub=None, lub=None, ib=None, lib=None):
        self.Et, self.Lt, self.Eb, self.Lb, self.ub, self.lub, self.ib, self.lib = Et, Lt, Eb, Lb, ub, lub, ib, lib
        self.bias = ub is not None

    @classmethod
    def of(cls, inp):
        u, i = inp.user, inp.item
        return cls(u["E"], u["ELOG"], i["E"], i["ELOG"], *((u["B_E"], u["B_ELOG"], i["B_E"], i["B_ELOG"]) if inp.bias else ()))

    def spread(self, u, items):
        """S: the largest Elog spread inside the user's row or a gathered row (bias entries included)"""
        rows = [np.append(self.Lt[u], self.lub[u]) if self.bias else self.Lt[u]]
        rows += [np.append(self.Lb[i], self.lib[i]) if self.bias else self.Lb[i] for i in items]
        return max(float(r.max() - r.min()) for r in rows)


def bound(S, H):
    """relative, in units of 1: (4 S + H + 64) 2^-53 (include/hpf.h)"""
    return (4.0 * S + H + 64.0) * U53


def _mpf(a):
    return [MP.mpf(float(x)) for x in np.asarray(a, np.float64).ravel()]


def exact(st, items, yy, u, targets, s0=S0):
    """mpmath: for user u with the given history, per target j -> (contributions [H], prior, score)"""
    K = st.Et.shape[1]
    eu = [MP.exp(x) for x in _mpf(st.Lt[u])]
    eub = MP.exp(MP.mpf(float(st.lub[u]))) if st.bias else None
    C = K + 1 if st.bias else K
    phi, D = [], [MP.mpf(s0)] * C
    for i, y in zip(items, yy):
        w = [a * MP.exp(b) for a, b in zip(eu, _mpf(st.Lb[i]))]
        den = MP.fsum(w)
        if st.bias:
            w.append(eub)
            den += eub + MP.exp(MP.mpf(float(st.lib[i])))
        p = [x / den for x in w]
        phi.append(p)
        D = [d + MP.mpf(float(y)) * x for d, x in zip(D, p)]
    out = []
    et = _mpf(st.Et[u])
    for j in targets:
        eb = _mpf(st.Eb[j])
        terms = [a * b for a, b in zip(et, eb)]
        if st.bias:
            terms.append(MP.mpf(float(st.ub[u])))
        g = [t / d for t, d in zip(terms, D)]
        con = [MP.mpf(float(y)) * MP.fdot(p, g) for p, y in zip(phi, yy)]
        score = MP.fsum(terms) + (MP.mpf(float(st.ib[j])) if st.bias else 0)
        out.append((con, MP.mpf(s0) * MP.fsum(g), score))
    return out


def numpy64(st, items, yy, u, targets, s0=S0):
    """plain float64: the same definition, one row max taken off each exponent -> per target (contributions [H], prior)"""
    K = st.Et.shape[1]
    lu = np.append(st.Lt[u], [st.lub[u], 0.0]) if st.bias else st.Lt[u]
    C = K + 1 if st.bias else K
    phi = np.zeros((len(items), C))
    for r, i in enumerate(items):
        lg = lu + (np.append(st.Lb[i], [0.0, st.lib[i]]) if st.bias else st.Lb[i])
        w = np.exp(lg - lg.max())
        phi[r] = (w / w.sum())[:C]
    D = s0 + (phi * np.asarray(yy, np.float64)[:, None]).sum(0) if len(items) else np.full(C, s0)
    out = []
    for j in targets:
        terms = st.Et[u] * st.Eb[j]
        if st.bias:
            terms = np.append(terms, st.ub[u])
        g = terms / D
        out.append((np.asarray(yy, np.float64) * (phi @ g) if len(items) else np.zeros(0), s0 * g.sum()))
    return out


def top(con, items, T):
    """the exact top-T of a list: contribution descending, item ascending -> (item ids [T] padded with NONE, positions)"""
    order = sorted(range(len(con)), key=lambda r: (-con[r], int(items[r])))[:T]
    ids = np.full(T, NONE, np.uint32)
    ids[:len(order)] = [items[r] for r in order]
    return ids, order


@functools.lru_cache(maxsize=None)
def reference(case):
    """the inputs of one case and their exact results, computed once: (Inputs, State, {q: (con, prior, score)})"""
    bias, hier, ratings, K, _ = case
    inp = Inputs(bias, hier, ratings, K)
    st = State.of(inp)
    res, q = {}, 0
    for b, u in enumerate(inp.users):
        items, yy = inp.history(u)
        targets = inp.t_items[int(inp.t_ptr[b]):int(inp.t_ptr[b + 1])]
        for r in exact(st, items, yy, int(u), targets):
            res[q] = r
            q += 1
    return inp, st, res


def ulps(got, want):
    """|got - want| / want in units of 2^-53 (want: an mpf > 0, or 0 -> got must be 0)"""
    if want == 0:
        return 0.0 if got == 0 else math.inf
    return float(abs(MP.mpf(float(got)) - want) / want / MP.mpf(U53))
