"""-m gpu: two real iterations through the C-ABI on a matrix whose Gamma shapes span 0.3 ... 1e8.

The parity tests run on synthetic data in which 94-99 % of the shapes are below 10 and none is large; a popular item of
a full-size problem takes shapes of 1e6-1e8.  Here a small matrix (200 users x 60 items) reaches that range with
DUPLICATED lines: a user repeats one (user, item) line d times at rating 255, d up to 4e5 (duplicates are legal:
test_duplicate_pairs_count_twice) -- beside users with one rating of 1, users with one large rating (shapes on either
side of 10, where the device digamma switches between its shifted and its direct series), empty users and an empty item.

No oracle: the start state is random and set through hpf_set_state, and the reference is built here from what the
device itself exports after iteration 1.  SHAPE and RATE are exact doubles; from them, with mpmath at 40 digits,
Elog = psi(shape) - log(rate), and from Elog, in long double, the softmax of every unique pair times its multiplicity
and the shapes iteration 2 must produce.  Asserted per case:
  (a) the exported ELOG of every Gamma object is within the digamma bound of test_gpu_special.py,
      u (3 log xs + 16 corr + |psi|), plus u (2 |log rate| + |Elog|)                  (elog_kernel, digamma_pos)
  (b) E == shape / rate bit for bit
  (c) SHAPE after iteration 2 agrees to RTOL = 1e-9, the per-iteration figure of test_gpu_parity.py
      (row_sweep_kernel with psi_parts_rate and exp_neg, the row packing, both phi passes, the combine of long rows)
  (d) no fallback from the packed rows happened where the priors are the default 0.3
  (e) the shapes of a row sum to s_prior K + (sum of the row's ratings) to 1e-12 relative; with bias terms, where a
      share of every rating goes to the other side's bias, the same identity over a whole side and both biases
and that the shapes after iteration 1 do cover [0.3, 0.31], both sides of 10 within +-1, and values above 1e7.
"""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL = 1e-9
U = 2.0 ** -53
N_USERS, N_ITEMS = 200, 60
WL_PLAIN, WL_P59, WL_F64 = 0, 3, 4


def _problem(n=N_USERS, m=N_ITEMS, seed=5, top=400000):
    """-> rowptr, col, val and the unique pairs (user, item, rating, multiplicity).  Item m - 1 is never rated."""
    rng = np.random.default_rng(seed)
    dups = [top] + [30000] * 3 + [1000] * 8 + [30] * 20 + [3] * 30 + [1] * 30
    pairs = []                                            # (user, item, rating, multiplicity)
    u = 0
    for d in dups:                                        # one repeated line at 255 and a few ordinary ratings
        it = rng.choice(m - 1, size=1 + int(rng.integers(0, 6)), replace=False)
        pairs.append((u, int(it[0]), 255, d))
        pairs += [(u, int(i), int(rng.integers(1, 6)), 1) for i in it[1:]]
        u += 1
    for _ in range(40):                                   # rows with one rating of 1
        pairs.append((u, int(rng.integers(m - 1)), 1, 1)); u += 1
    for y in range(9, 9 + 40):                            # rows with one rating of 9 .. 48: shapes around 10
        if u >= n - 8:
            break
        pairs.append((u, int(rng.integers(m - 1)), y, 1)); u += 1
    # the last users stay empty
    pu, pi, py, pm = (np.array(c, dtype=np.int64) for c in zip(*pairs))
    rows_u = np.repeat(pu, pm)
    order = np.argsort(rows_u, kind="stable")
    col = np.repeat(pi, pm)[order].astype(np.uint32)
    val = np.repeat(py, pm)[order].astype(np.uint8)
    rowptr = np.zeros(n + 1, np.int64)
    rowptr[1:] = np.cumsum(np.bincount(rows_u, minlength=n))
    return rowptr, col, val, (pu, pi, py, pm)


def _start_state(n, m, K, hier, bias, s_prior, seed):
    """a random valid state: Elog spread over 12 inside a row -- 30 for hundreds of factors, so that the largest share of a
    softmax stays a good part of the whole -- which is peaked and still far inside what p59 rows hold (a spread of 87)"""
    rng = np.random.default_rng(seed)
    spread = 12.0 if K <= 100 else 30.0
    st = {}
    for name, rows in (("THETA", n), ("BETA", m)):
        st[f"{name}_SHAPE"] = rng.uniform(0.3, 2.0, (rows, K))
        st[f"{name}_E"] = rng.uniform(0.05, 1.5, (rows, K))
        st[f"{name}_ELOG"] = rng.uniform(-spread, 0.0, (rows, K))
    if hier:
        for name, rows in (("XI", n), ("ETA", m)):
            rate = rng.uniform(0.5, 3.0, rows)
            shape = np.full(rows, s_prior + K * s_prior)
            st[f"{name}_SHAPE"], st[f"{name}_RATE"] = shape, rate
            st[f"{name}_E"], st[f"{name}_ELOG"] = shape / rate, rng.uniform(-2.0, 2.0, rows)
    if bias:
        for name, rows in (("UBIAS", n), ("IBIAS", m)):
            st[f"{name}_SHAPE"] = rng.uniform(0.3, 2.0, rows)
            st[f"{name}_E"] = rng.uniform(0.05, 1.5, rows)
            st[f"{name}_ELOG"] = rng.uniform(-12.0, 0.0, rows)
    return st


def _mp_elog(shape, rate):
    """-> psi(shape) - log(rate) as (long double, psi, log xs, corr = log xs - psi) with mpmath at 40 digits"""
    import mpmath as mp
    mp.mp.dps = 40
    shape, rate = np.broadcast_arrays(np.asarray(shape, np.float64), np.asarray(rate, np.float64))
    el = np.empty(shape.shape, np.longdouble)
    psi, logxs, corr = (np.empty(shape.shape) for _ in range(3))
    seen = {}
    for idx in np.ndindex(shape.shape):
        x = float(shape[idx])
        if x not in seen:
            xs = x + 10.0 if x < 10.0 else x
            p, l = mp.digamma(mp.mpf(x)), mp.log(mp.mpf(xs))
            seen[x] = (p, float(p), float(l), float(l - p))
        p, psi[idx], logxs[idx], corr[idx] = seen[x]
        v = p - mp.log(mp.mpf(float(rate[idx])))
        hi = float(v)
        el[idx] = np.longdouble(hi) + np.longdouble(float(v - mp.mpf(hi)))
    mp.mp.dps = 15
    return el, psi, logxs, corr


def _objects(hier, bias):
    o = ["THETA", "BETA"]
    if hier:
        o += ["XI", "ETA"]
    if bias:
        o += ["UBIAS", "IBIAS"]
    return o


# (K, hier, bias, w_storage, s_prior, r_prior, users, items, largest multiplicity, the sweep that must run)
# K = 2 / 21: plain rows; K = 100: p59 rows of G = 8 lanes, built in registers by a sweep group of 16; K = 800: p59 rows of
# G = 64 lanes (the narrower groups hold 544 columns at most, and 48 lines of p59 beat the 50 of plain rows), which the
# sweep builds in LDS -- on a smaller matrix: the reference costs a digamma per element
CASES = [
    pytest.param(2, True, False, 3, 0.3, 0.3, N_USERS, N_ITEMS, 400000, "plain", id="K2-hier-plain"),
    pytest.param(21, True, True, 0, 0.3, 0.3, N_USERS, N_ITEMS, 400000, "plain", id="K21-hier-bias"),
    pytest.param(100, True, False, 0, 0.3, 0.3, N_USERS, N_ITEMS, 400000, "reg-p59", id="K100-hier-regp59"),
    pytest.param(100, False, True, 0, 0.05, 2.0, N_USERS, N_ITEMS, 400000, "reg-p59", id="K100-flat-bias-priors"),
    pytest.param(800, True, False, 0, 0.3, 0.3, 24, 10, 400000, "lds-p59", id="K800-hier-ldsp59"),
]


@pytest.mark.parametrize("K,hier,bias,w_storage,s_prior,r_prior,n,m,top,sweep", CASES)
def test_two_iterations_over_the_whole_shape_range(K, hier, bias, w_storage, s_prior, r_prior, n, m, top, sweep):
    from hgaprec_amd.capi import Hpf
    if (n, m) == (N_USERS, N_ITEMS):
        rowptr, col, val, (pu, pi, py, pm) = _problem()
    else:
        rowptr, col, val, (pu, pi, py, pm) = _small_problem(n, m, top)
    D = Hpf(n, m, K, hier=hier, bias=bias, s_prior=s_prior, r_prior=r_prior, w_storage=w_storage)
    D.upload_csr(rowptr, col, val)
    for name, a in _start_state(n, m, K, hier, bias, s_prior, seed=1000 + K).items():
        D.set_state(name, a)
    wi = D.work_info()
    assert wi["nnz"] == col.size
    if sweep == "plain":
        assert wi["w_layout"] == WL_PLAIN
    else:                      # p59 rows: built in registers where the pass gives a nonzero <= 32 lanes, in LDS for 64
        assert wi["w_layout"] == WL_P59 and (wi["phi_G"] == 64) == (sweep == "lds-p59")

    D.iterate(1)
    objs = _objects(hier, bias)
    S1 = {o: D.get_state(f"{o}_SHAPE") for o in objs}
    R1 = {o: D.get_state(f"{o}_RATE") for o in objs}
    E1 = {o: D.get_state(f"{o}_E") for o in objs}
    L1 = {o: D.get_state(f"{o}_ELOG") for o in objs}

    # the shapes cover the ranges this test is about
    allsh = np.concatenate([S1[o].ravel() for o in objs if o not in ("XI", "ETA")])
    assert np.all(np.isfinite(allsh)) and allsh.min() >= s_prior
    assert np.any((allsh >= s_prior) & (allsh <= s_prior + 0.01))
    assert np.any((allsh >= 9.0) & (allsh < 10.0)) and np.any((allsh >= 10.0) & (allsh <= 11.0))
    assert allsh.max() > 1e7

    # (a), (b)
    ref_elog = {}
    for o in objs:
        rate = R1[o] if R1[o].shape == S1[o].shape else np.broadcast_to(R1[o], S1[o].shape)     # flat: one rate per column
        el, psi, logxs, corr = _mp_elog(S1[o], rate)
        ref_elog[o] = el
        elf = el.astype(np.float64)
        bound = U * (3.0 * logxs + 16.0 * corr + np.abs(psi)) + U * (2.0 * np.abs(np.log(rate)) + np.abs(elf))
        ratio = np.abs((L1[o].astype(np.longdouble) - el).astype(np.float64)) / bound
        print(f"\n{o}_ELOG: max error/bound {ratio.max():.3f} (shapes {S1[o].min():.3g} .. {S1[o].max():.3g})")
        assert np.all(np.isfinite(L1[o])) and ratio.max() <= 1.0, (o, ratio.max())
        assert np.array_equal(E1[o], S1[o] / rate), o

    # (c) the shapes of iteration 2 from the Elog of iteration 1
    x = ref_elog["THETA"][pu] + ref_elog["BETA"][pi]                  # [pairs, K]
    if bias:
        x = np.concatenate([x, ref_elog["UBIAS"][pu, None], ref_elog["IBIAS"][pi, None]], axis=1)
    x = x - x.max(axis=1, keepdims=True)
    e = np.exp(x)
    wgt = (np.where(py > 1, py, 1) * pm).astype(np.longdouble)
    phi = e / e.sum(axis=1, keepdims=True) * wgt[:, None]
    want = {"THETA": np.zeros((n, K), np.longdouble), "BETA": np.zeros((m, K), np.longdouble)}
    np.add.at(want["THETA"], pu, phi[:, :K])
    np.add.at(want["BETA"], pi, phi[:, :K])
    if bias:
        want["UBIAS"], want["IBIAS"] = np.zeros(n, np.longdouble), np.zeros(m, np.longdouble)
        np.add.at(want["UBIAS"], pu, phi[:, K])
        np.add.at(want["IBIAS"], pi, phi[:, K + 1])

    D.iterate(1)
    S2 = {o: D.get_state(f"{o}_SHAPE") for o in want}
    for o, w in want.items():
        ref = (w + np.longdouble(s_prior)).astype(np.float64)
        err = np.abs(S2[o] - ref) / ref
        print(f"{o}_SHAPE after iteration 2: max rel err {err.max():.3e} (shapes {ref.min():.3g} .. {ref.max():.3g})")
        assert err.max() <= RTOL, (o, err.max())

    # (d)
    if s_prior == 0.3 and r_prior == 0.3:
        assert D.work_info()["w_fallbacks"] == 0

    # (e)
    yw = (np.where(py > 1, py, 1) * pm).astype(np.float64)
    for S in (S1, S2):
        if not bias:
            usum = np.array([math.fsum(r) for r in S["THETA"]])
            isum = np.array([math.fsum(r) for r in S["BETA"]])
            uy, iy = np.bincount(pu, yw, minlength=n), np.bincount(pi, yw, minlength=m)
            np.testing.assert_allclose(usum, s_prior * K + uy, rtol=1e-12, atol=0)
            np.testing.assert_allclose(isum, s_prior * K + iy, rtol=1e-12, atol=0)
        else:
            # a rating's K + 2 shares go to the user's row, the user's bias and the item's bias -- or to the item's row
            # and the same two
            biases = math.fsum(np.concatenate([S["UBIAS"], S["IBIAS"]]))
            for o, rows in (("THETA", n), ("BETA", m)):
                total = math.fsum(S[o].ravel()) + biases
                expect = s_prior * (rows * K + n + m) + yw.sum()
                assert abs(total - expect) <= 1e-12 * expect, (o, total, expect)
    D.close()


def _small_problem(n, m, top):
    """the same kinds of rows on a few users, for the case whose reference is expensive per element"""
    rng = np.random.default_rng(9)
    pairs = [(0, 0, 255, top), (0, 3, 4, 1), (1, 1, 255, 30000), (2, 2, 255, 1000), (3, 0, 255, 30), (3, 5, 2, 1),
             (4, 4, 255, 3), (5, 5, 255, 1), (5, 1, 5, 1)]
    u = 6
    for _ in range(4):
        pairs.append((u, int(rng.integers(m - 1)), 1, 1)); u += 1
    for y in (10, 11, 12, 14, 17, 20, 24, 30, 40, 48):
        pairs.append((u, int(rng.integers(m - 1)), y, 1)); u += 1
    assert u <= n - 2                                     # the last users stay empty, item m - 1 is never rated
    pu, pi, py, pm = (np.array(c, dtype=np.int64) for c in zip(*pairs))
    rows_u = np.repeat(pu, pm)
    order = np.argsort(rows_u, kind="stable")
    col = np.repeat(pi, pm)[order].astype(np.uint32)
    val = np.repeat(py, pm)[order].astype(np.uint8)
    rowptr = np.zeros(n + 1, np.int64)
    rowptr[1:] = np.cumsum(np.bincount(rows_u, minlength=n))
    return rowptr, col, val, (pu, pi, py, pm)
