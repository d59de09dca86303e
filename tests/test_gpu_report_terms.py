"""-m gpu: the report kernels -- heldout_ll_kernel, elbo_nnz_kernel, elbo_nnz_w_kernel, rowmax_elog_kernel,
elbo_gamma_kernel -- and the host code around them (hpf_heldout_ll, hpf_heldout_ll_bound, hpf_elbo) held to mpmath term by
term: per pair, per nonzero, per Gamma element, through the test-only entry points of hpf_probe.hip (tests/devprobe.py),
which launch the very __global__ functions of hpf_kernels.hpp on arrays and grids chosen here.

The bound.  Every comparison is |device - exact| <= c u A, u = 2^-53.  `exact` and A -- the sum of the absolute values of
the term's addends -- come from tests/report_ref.py (mpmath, 50 digits, on the doubles handed to the kernel).  c is not a
constant of this file: each test measures c_ref, the largest |plain - exact| / (u A) over ITS OWN inputs, where `plain` is
the reference program's arithmetic in plain doubles (glibc, serial order, log y! as a sum of log i), and holds the device
to c = 4 max(1, c_ref): the device's libm takes a few ulp where glibc takes one, it contracts to fma, and it sums a dot
product as a 16-lane tree -- each changes the rounding of an addend by a small factor, never its magnitude.  Sums of terms
(block partials, totals) get the sum of their terms' bounds plus n u sum |term| for the n additions.  Nothing is skipped or
filtered: an input on which the device misses the bound fails the test.  Every test prints its c_ref and the largest
|device - exact| / (u A) it saw.

Where W enters (elbo_nnz_w_kernel evaluates logsumexp as log(sum Wt Wb) + Mt + Mb):
  * through the probe, W is handed in: the reference takes the same W (nnz_term_w).  Against the Elog reference the W made
    here -- exp(L - M) from mpmath, rounded once, relative error <= u per element, 2 u per product, hence 2 u in the
    logarithm of the sum -- adds y yy 2 u.
  * through hpf_elbo after hpf_set_state(ELOG), W is derive_w_kernel's exp(L - M): the difference rounds within u |L - M|
    and the device exp is taken at one ulp, 2 u, so a row's W carries u (2 + max_c |L_c - M|) and the nonzero gets
    y yy u (4 + spread_t + spread_b), spread = max_c |L_c - M| of a row.
  * through hpf_elbo after an iteration, W is the sweep's own (xs exp_neg(corr) ri, never made from the exported Elog):
    W and the exported Elog each agree with psi(shape) - log(rate) within bound (a) of test_gpu_wide_range.py,
    B = u (3 log xs + 16 corr + |psi|) + u (2 |log rate| + |Elog|), so the nonzero gets y yy 2 (B_t + B_b), B of a row the
    largest over its live columns.

c_ref (CPU, glibc) and the largest |device - exact| / (u A) seen on an MI355X are recorded in each test's docstring.
"""
import math

import numpy as np
import pytest

from tests import devprobe
from tests import report_ref as rr
from tests.test_gpu_wide_range import _mp_elog, _problem, _start_state

pytestmark = pytest.mark.gpu

U = rr.U
NAN = float("nan")


def _hold(name, got, terms, plain, extra=None, c_from=None):
    """every got[k] within c u A_k (+ extra[k]) of terms[k] = (exact, A); c from the plain restatement of the same terms
    (or of c_from = (plain, terms), where the device's terms have no plain counterpart).  -> (c_ref, worst ratio)"""
    c_ref = rr.c_ref(*c_from) if c_from else rr.c_ref(plain, terms)
    c = rr.c_for(c_ref)
    worst, bad = 0.0, []
    for k, (g, (e, A)) in enumerate(zip(got, terms)):
        err = rr.abs_err(float(g), e)
        x = extra[k] if extra is not None else 0.0
        r = err / (U * A) if A > 0 else (0.0 if err == 0 else math.inf)
        worst = max(worst, r)
        if not err <= c * U * A + x:
            bad.append((k, float(g), float(e), r))
    print(f"\n{name}: c_ref {c_ref:.2f} (c = {c:.1f}), largest |device - exact| / (u A) {worst:.2f} over {len(terms)} terms")
    assert not bad, (name, c, bad[:5])
    return c_ref, worst


# ---- held-out pairs, per pair ---------------------------------------------------------------------------------------------
KS_PAIR = [1, 3, 15, 16, 17, 33, 100]
RATINGS = [0, 1, 2, 44, 255, 256, 257, 300, -1, 2 ** 31 - 1]


def _pair_problem(K, bias, targets, seed):
    """one user row and one item row per pair (indices permuted), the user's row -- and the item's bias -- scaled so that the
    pair's score is targets[p] (0: the user row and the item's bias are zero).  Columns past the live ones hold NaN."""
    rng = np.random.default_rng(seed)
    npairs = len(targets)
    ld = K + (2 if bias else 0) + 3
    Et, Eb = rng.uniform(0.1, 1.0, (npairs, ld)), rng.uniform(0.1, 1.0, (npairs, ld))
    Et[:, K:], Eb[:, K:] = NAN, NAN
    ubc, ibc = (K, K + 1) if bias else (-1, -1)
    if bias:
        Et[:, ubc], Eb[:, ibc] = rng.uniform(0.1, 1.0, npairs), rng.uniform(0.1, 1.0, npairs)
    pu, pi = rng.permutation(npairs), rng.permutation(npairs)
    for p, t in enumerate(targets):
        u, i = pu[p], pi[p]
        cur = float(Et[u, :K] @ Eb[i, :K]) + (Et[u, ubc] + Eb[i, ibc] if bias else 0.0)
        f = t / cur
        Et[u, :K] *= f
        if bias:
            Et[u, ubc] *= f
            Eb[i, ibc] *= f
    return Et, Eb, pu.astype(np.uint32), pi.astype(np.uint32), ubc, ibc


def _pair_terms(Et, Eb, pu, pi, y, K, ubc, ibc, binary):
    terms, plain = [], []
    for u, i, yy in zip(pu, pi, y):
        ub, ib = (Et[u, ubc], Eb[i, ibc]) if ubc >= 0 else (None, None)
        terms.append(rr.pair_ll(Et[u, :K], Eb[i, :K], yy, ub, ib, binary))
        plain.append(rr.plain_pair_ll(Et[u, :K], Eb[i, :K], yy, ub, ib, binary))
    return terms, plain


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("K", KS_PAIR)
def test_poisson_pair_likelihood_per_pair(K, bias):
    """heldout_ll_kernel, Poisson form, 200 pairs per (K, bias): scores 1e-40 .. 1e4 (log-uniform), a pair whose rows are
    zero, and scores of 0.5, 0.999, 1.001 and 2 times 1e-30 -- the clamp from both sides; the ratings walk
    {0, 1, 2, 44, 255, 256, 257, 300, -1, 2^31 - 1}, so the wrap y & 0xff and logfact[255] are read.  The table of log y! is
    the library's own (probe_logfact) and must be the serial sum of log i.  A grid that covers the pairs, a grid twice as
    large, and ONE block for the first 37 pairs (16 groups: three trips of the p0 loop, the last with 5 pairs) give the same
    bits.  Seen: c_ref 3.8 .. 6.5 (the serial sum of log i in log y! at y = 255), device 3.8 .. 5.5 (the same table)."""
    rng = np.random.default_rng(100 + K)
    targets = 10.0 ** rng.uniform(-40, 4, 200)
    targets[:5] = [0.0, 0.5e-30, 2e-30, 0.999e-30, 1.001e-30]
    Et, Eb, pu, pi, ubc, ibc = _pair_problem(K, bias, targets, seed=K)
    y = np.array([RATINGS[p % len(RATINGS)] for p in range(200)], np.int64)
    y[:5] = [1, 2, 44, 255, 300]
    lf = devprobe.logfact()
    assert np.array_equal(lf, rr.plain_logfact_table())
    terms, plain = _pair_terms(Et, Eb, pu, pi, y, K, ubc, ibc, False)
    got = devprobe.heldout_ll((200 + 15) // 16, pu, pi, y, Et, Eb, K, ubc, ibc, False, lf)
    _hold(f"Poisson pair K={K} bias={bias}", got, terms, plain)
    assert np.array_equal(devprobe.heldout_ll(26, pu, pi, y, Et, Eb, K, ubc, ibc, False, lf), got)
    one = devprobe.heldout_ll(1, pu[:37], pi[:37], y[:37], Et, Eb, K, ubc, ibc, False, lf)
    assert np.array_equal(one, got[:37])


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("K", [1, 17, 100])
def test_binary_pair_likelihood_per_pair(K, bias):
    """heldout_ll_kernel, binary form.  y = 0 (and 256, which wraps to it): -s, within the bound of the dot product and, for
    K = 1 without bias, where nothing is summed, exactly -(Et Eb).  y >= 1 with s in [1e-12, 700]: log(1 - exp(-s)) within
    the bound, A = 1 / (1 - exp(-s)) + |ll|.  s <= 1e-18, and the clamped s = 1e-30 of a zero row: exp(-s) is 1 in double and
    the value exactly -inf, as the reference's formula gives in double.  The band 1e-17 .. 1e-15, where one ulp of exp(-s)
    decides between -inf and -36.7, is deliberately not sampled: neither outcome there is an error.  One block serves all
    110 pairs (seven trips).  Seen: c_ref 0.8 .. 6.0 (6.0: the serial dot product at K = 100), device 0.8 .. 2.5."""
    rng = np.random.default_rng(200 + K)
    t_zero = 10.0 ** rng.uniform(-12, math.log10(700), 40)
    t_pos = 10.0 ** rng.uniform(-12, math.log10(700), 50)
    t_pos[:2] = [1e-12, 700.0]
    t_inf = 10.0 ** rng.uniform(-40, -18, 20)
    t_inf[:2] = [0.0, 1e-18]
    targets = np.concatenate([t_zero, t_pos, t_inf])
    Et, Eb, pu, pi, ubc, ibc = _pair_problem(K, bias, targets, seed=50 + K)
    y = np.concatenate([np.where(np.arange(40) % 2, 0, 256), np.array([1, 2, 255, 257, -1] * 10), np.ones(20, np.int64)])
    got = devprobe.heldout_ll(1, pu, pi, y, Et, Eb, K, ubc, ibc, True)
    terms, plain = _pair_terms(Et, Eb, pu, pi, y, K, ubc, ibc, True)
    for p in range(40, 90):                                    # the scores are where they were aimed
        s = float(rr._mp_score(Et[pu[p], :K], Eb[pi[p], :K], Et[pu[p], ubc] if bias else None, Eb[pi[p], ibc] if bias else None)[0])
        assert 0.99e-12 <= s <= 701.0, (p, s)
    _hold(f"binary pair K={K} bias={bias}", got[:90], terms[:90], plain[:90])
    if K == 1 and not bias:
        assert np.array_equal(got[:40], -(Et[pu[:40], 0] * Eb[pi[:40], 0]))
    assert np.all(np.isneginf(got[90:])), got[90:]
    assert all(p == -math.inf for p in plain[90:])              # ... as the formula gives in double


# ---- held-out sums through the ABI ----------------------------------------------------------------------------------------
def _serial_sum(v):
    s = 0.0
    for x in v.tolist():
        s += x
    return s


def test_heldout_sums_are_the_serial_sums_of_the_kernel_values():
    """hpf_heldout_ll and hpf_heldout_ll_bound over pairs in a given order equal, bit for bit, the left-to-right sum of
    heldout_ll_kernel's per-pair values (probe) on the exported E: 2^16 + 13 pairs (n = 300, m = 200, K = 5, bias), where a
    bound set takes the copy in eight pipelined pieces, 2^16 - 1 and 37 pairs, where it takes one copy; on the state handed
    in and after an iteration.  (The per-pair values themselves: the tests above.)"""
    from hgaprec_amd.capi import Hpf
    from tests.util import make_problem
    n, m, K = 300, 200, 5
    rowptr, col, val = make_problem(n, m, 3000, seed=11)
    D = Hpf(n, m, K, hier=True, bias=True)
    D.upload_csr(rowptr, col, val)
    for name, a in _start_state(n, m, K, True, True, 0.3, seed=12).items():
        D.set_state(name, a)
    rng = np.random.default_rng(13)
    big = (1 << 16) + 13
    hu, hi = rng.integers(0, n, big).astype(np.uint32), rng.integers(0, m, big).astype(np.uint32)
    hy = rng.choice(np.array(RATINGS + [3, 4, 5], np.int64), big).astype(np.int32)
    lf = devprobe.logfact()
    for step in range(2):
        Et, Eb = np.zeros((n, K + 2)), np.zeros((m, K + 2))
        Et[:, :K], Eb[:, :K] = D.get_state("THETA_E"), D.get_state("BETA_E")
        Et[:, K], Eb[:, K + 1] = D.get_state("UBIAS_E"), D.get_state("IBIAS_E")
        per_pair = devprobe.heldout_ll(4096, hu, hi, hy, Et, Eb, K, K, K + 1, False, lf)
        assert np.all(np.isfinite(per_pair))
        for slot, cnt in enumerate((big, (1 << 16) - 1, 37)):
            want = _serial_sum(per_pair[:cnt])
            got, c = D.heldout_ll(hu[:cnt], hi[:cnt], hy[:cnt])
            assert c == cnt and got == want, (step, cnt, got, want)
            D.heldout_bind(slot, hu[:cnt], hi[:cnt], hy[:cnt])
            assert D.heldout_ll_bound(slot) == (want, cnt), (step, cnt)
        D.iterate(1)
    D.close()


# ---- the nonzero term, per nonzero, both kernels ---------------------------------------------------------------------------
KS_NNZ = [1, 2, 15, 16, 17, 100, 129]
SPREADS = [0.0, 12.0, 87.0, 300.0]


def _elog_rows(rng, K, C, spread, peak, own_slot, other_slot, ld):
    """a row of Elog: the peak column at the row's offset, the others up to `spread` below it, the own bias (C = K + 2) within
    the spread, 0 in the other side's slot, NaN past the live columns"""
    row = np.full(ld, NAN)
    off = rng.uniform(-3.0, 1.0)
    row[:K] = off - rng.uniform(0.0, 1.0, K) * spread
    row[peak] = off
    if K > 1 and spread > 0:
        row[(peak + 1 + rng.integers(K - 1)) % K] = off - spread      # the spread is reached
    if C > K:
        row[own_slot] = off - rng.uniform(0.0, 1.0) * spread
        row[other_slot] = 0.0
    return row


def _w_of(L, K, bias_col, junk_col):
    """-> (W = exp(L - M) from mpmath, rounded once; 0 in the padding; M the maximum of the live columns, the junk slot
    counting as 0)"""
    import mpmath as mp
    live = list(range(K)) + ([bias_col, junk_col] if bias_col >= 0 else [])
    M = np.array([max(max(r[:K]), r[bias_col], 0.0) if bias_col >= 0 else max(r[:K]) for r in L])
    W = np.zeros_like(L)
    with mp.workdps(rr.DPS):
        for r in range(L.shape[0]):
            for c in live:
                W[r, c] = float(mp.exp(mp.mpf(float(L[r, c])) - mp.mpf(float(M[r]))))
    return W, M


def _nnz_state(K, C, spreads, seed, ratings=(0, 1, 2, 255)):
    """row pairs (t, t): for every spread, one pair peaking at the same column and one at different columns; every rating on
    every pair.  -> dict of the arrays and the nonzero list"""
    rng = np.random.default_rng(seed)
    bias = C > K
    ld = C + 3
    ubc, ibc = (K, K + 1) if bias else (-1, -1)
    nrow = 2 * len(spreads)
    Lt, Lb = np.empty((nrow, ld)), np.empty((nrow, ld))
    for t in range(nrow):
        sp, same = spreads[t // 2], t % 2 == 0
        pt = int(rng.integers(K))
        pb = pt if same else (pt + 1 + int(rng.integers(max(K - 1, 1)))) % K
        Lt[t] = _elog_rows(rng, K, C, sp, pt, K, K + 1, ld)
        Lb[t] = _elog_rows(rng, K, C, sp, pb, K + 1, K, ld)
    Et, Eb = rng.uniform(0.05, 1.5, (nrow, ld)), rng.uniform(0.05, 1.5, (nrow, ld))
    Et[:, K:], Eb[:, K:] = NAN, NAN
    if bias:
        Et[:, ubc], Eb[:, ibc] = rng.uniform(0.05, 1.5, nrow), rng.uniform(0.05, 1.5, nrow)
    rows = np.repeat(np.arange(nrow), len(ratings)).astype(np.uint32)
    val = np.tile(np.array(ratings, np.uint8), nrow)
    Wt, Mt = _w_of(Lt, K, ubc, ibc)
    Wb, Mb = _w_of(Lb, K, ibc, ubc)
    return dict(K=K, C=C, ld=ld, ubc=ubc, ibc=ibc, Lt=Lt, Lb=Lb, Et=Et, Eb=Eb, Wt=Wt, Wb=Wb, Mt=Mt, Mb=Mb, rows=rows, cols=rows.copy(),
                val=val)


def _nnz_refs(S, rows, cols, val):
    """-> (Elog-form terms, plain, W-form terms) of the nonzeros (rows[k], cols[k], val[k]); val None: all ones"""
    K, C, ubc, ibc = S["K"], S["C"], S["ubc"], S["ibc"]
    terms, plain, wterms = [], [], []
    for k, (r, c) in enumerate(zip(rows, cols)):
        y = None if val is None else int(val[k])
        ub, ib = (S["Et"][r, ubc], S["Eb"][c, ibc]) if ubc >= 0 else (None, None)
        args = (S["Et"][r, :K], S["Eb"][c, :K], y, ub, ib)
        terms.append(rr.nnz_term(S["Lt"][r, :C], S["Lb"][c, :C], *args))
        plain.append(rr.plain_nnz_term(S["Lt"][r, :C], S["Lb"][c, :C], *args))
        wterms.append(rr.nnz_term_w(S["Wt"][r], S["Wb"][c], S["Mt"][r], S["Mb"][c], *args))
    return terms, plain, wterms


def _yyy(val, n):
    v = np.ones(n) if val is None else np.asarray(val, np.float64)
    return v * np.maximum(v, 1.0)


def _run_both(S, grid, seg, col, val):
    e = devprobe.elbo_nnz(grid, *seg, col, val, S["Lt"], S["Lb"], S["Et"], S["Eb"], S["K"], S["C"], S["ubc"], S["ibc"])
    w = devprobe.elbo_nnz_w(grid, *seg, col, val, S["Wt"], S["Wb"], S["Mt"], S["Mb"], S["Lt"], S["Lb"], S["Et"], S["Eb"], S["K"],
                            S["C"], S["ubc"], S["ibc"])
    return e, w


@pytest.mark.parametrize("with_bias", [False, True], ids=["C=K", "C=K+2"])
@pytest.mark.parametrize("K", KS_NNZ)
def test_nonzero_term_per_nonzero_both_kernels(K, with_bias):
    """elbo_nnz_kernel (from Elog) and elbo_nnz_w_kernel (from W and the row maxima), one nonzero per block -- a segment of
    one nonzero for the block's first wave, three of length 0 for the others -- so that partial[b] is the term of nonzero b.
    K in {1, 2, 15, 16, 17, 100, 129}: fewer columns than the 16 lanes, a ragged last trip, nine trips.  C = K and K + 2 (the
    own bias in its slot, 0 in the other side's, as hpf_create lays the columns out).  Elog spread of a row 0, 12, 87, 300 --
    inside what p59 rows hold, at their edge, far past it -- with the two rows peaking at the same and at different columns
    (at 300 and different peaks the sum of W products is e^-300: still the W route).  Ratings 0, 1, 2, 255, and val = null.
    Past the live columns L and E hold NaN, which must not enter; W holds 0 there, as the kernel assumes.
    rowmax_elog_kernel gives the exact maximum of the live columns, the junk slot counting as 0: bitwise.
    The W kernel is held twice: to the W-form reference on the W handed in, and to the Elog reference plus y yy 2 u (module
    docstring) -- so that the two routes agree with one reference and with each other.
    Seen: c_ref 0.2 (K = 1) .. 17.9 (K = 100: the reference's running logsum and its sum of y phi_k (x_k - log phi_k) over k);
    device, Elog route 0.2 .. 1.8, W route on its own W 0.4 .. 2.5, W route against the Elog reference 0.2 .. 2.2."""
    C = K + 2 if with_bias else K
    S = _nnz_state(K, C, SPREADS, seed=300 + K)
    assert np.array_equal(devprobe.rowmax_elog(S["Lt"], K, S["ubc"], S["ibc"]), S["Mt"])
    assert np.array_equal(devprobe.rowmax_elog(S["Lb"], K, S["ibc"], S["ubc"]), S["Mb"])
    for val in (S["val"], None):
        rows, cols = (S["rows"], S["cols"]) if val is not None else (S["rows"][::4], S["cols"][::4])
        seg = devprobe.one_nonzero_per_block(rows, cols)
        terms, plain, wterms = _nnz_refs(S, rows, cols, val)
        e, w = _run_both(S, rows.size, seg, cols, val)
        tag = f"K={K} C={C} val={'null' if val is None else 'given'}"
        _hold(f"nonzero term, Elog route {tag}", e, terms, plain)
        _hold(f"nonzero term, W route on its own W {tag}", w, wterms, None, c_from=(plain, terms))
        _hold(f"nonzero term, W route against the Elog reference {tag}", w, terms, plain, extra=_yyy(val, rows.size) * 2 * U)


def test_nonzero_term_over_real_segments():
    """the segment walk of both kernels: 11 segments of lengths 1, 3, 4, 5, 63, 64, 65, 0, 1, 3, 5 (not multiples of the four
    nonzeros a wave takes per trip; an empty one), several of one row, on grids of 1 and 2 blocks (4 and 8 waves: a wave
    takes up to three segments).  Every block partial is held to the reference's sum over that block's segments -- wave w
    takes the segments w, w + waves, ...; block b is the waves 4b .. 4b + 3.  Seen: c_ref 11.8; |error| / bound <= 0.008."""
    K, C = 17, 19
    S = _nnz_state(K, C, [12.0, 12.0, 30.0], seed=77)
    rng = np.random.default_rng(78)
    nrow = S["Lt"].shape[0]
    seg_len = np.array([1, 3, 4, 5, 63, 64, 65, 0, 1, 3, 5], np.uint32)
    seg_row = np.array([0, 0, 1, 2, 2, 2, 3, 4, 5, 5, 1], np.uint32)
    seg_start = np.concatenate([[0], np.cumsum(seg_len)[:-1]]).astype(np.int64)
    nnz = int(seg_len.sum())
    col = rng.integers(0, nrow, nnz).astype(np.uint32)
    val = rng.choice(np.array([0, 1, 2, 3, 5, 44, 255], np.uint8), nnz)
    rows = np.repeat(seg_row, seg_len)
    terms, plain, wterms = _nnz_refs(S, rows, col, val)
    c = rr.c_for(rr.c_ref(plain, terms))
    print(f"\nsegments: c_ref {rr.c_ref(plain, terms):.2f}")
    for grid in (1, 2):
        e, w = _run_both(S, grid, (seg_row, seg_start, seg_len), col, val)
        for b in range(grid):
            mine = [k for s in range(seg_len.size) if (s % (4 * grid)) // 4 == b
                    for k in range(int(seg_start[s]), int(seg_start[s] + seg_len[s]))]
            for name, got, tt in (("Elog", e[b], terms), ("W", w[b], wterms)):
                exact, bound = rr.sum_bound([tt[k] for k in mine], c)
                err = rr.abs_err(float(got), exact)
                print(f"\nsegments, {name} route, grid {grid} block {b}: {len(mine)} nonzeros, |error| / bound {err / bound:.3f}")
                assert err <= bound, (name, grid, b, float(got), float(exact), bound)


# ---- the W route's limit ---------------------------------------------------------------------------------------------------
LIMIT_SPREADS = [600.0, 740.0, 760.0, 1400.0]


def _limit_rows(K, S_, with_bias):
    """two rows peaking at different columns whose every product of W is about e^-S_"""
    C = K + 2 if with_bias else K
    ld = C + 3
    lt, lb = np.full(ld, NAN), np.full(ld, NAN)
    lt[:K], lb[:K] = -S_, -S_
    lt[0], lb[1] = -0.25, -0.5
    lt[2], lb[2] = -S_ / 2 - 1.0, -S_ / 2 - 2.0
    if with_bias:
        lt[K], lt[K + 1] = -S_, 0.0
        lb[K], lb[K + 1] = 0.0, -S_
    return lt, lb, C, ld


@pytest.mark.parametrize("with_bias", [False, True], ids=["C=K", "C=K+2"])
def test_w_route_limit_through_the_probe(with_bias):
    """rows peaking at different columns, combined spread 600, 740, 760, 1400: every product Wt Wb is about e^-spread.  At 600
    their sum is a normal double and the W route holds.  At 740 it is subnormal (digits lost), from 760 on it is 0 in double: the
    W form as written gives log 0 = -inf, and 0 * -inf = NaN for a rating of 0.  elbo_nnz_w_kernel
    evaluates such a nonzero -- sum below 2^-960 -- in the Elog form instead, and every value is finite and within the bound
    of the Elog reference (+ y yy 2 u where W was used).  Seen: c_ref 102 .. 422 (the reference's running logsum at these
    spreads), device 0.5 .. 0.7 on both routes.  Without the fallback the W kernel returns -inf at 760 and 1400 (NaN under a
    rating of 0) and misses the bound at 740."""
    K = 5
    rows_l = [_limit_rows(K, s, with_bias) for s in LIMIT_SPREADS]
    C, ld = rows_l[0][2], rows_l[0][3]
    Lt, Lb = np.array([r[0] for r in rows_l]), np.array([r[1] for r in rows_l])
    ubc, ibc = (K, K + 1) if with_bias else (-1, -1)
    rng = np.random.default_rng(5)
    Et, Eb = rng.uniform(0.05, 1.5, Lt.shape), rng.uniform(0.05, 1.5, Lt.shape)
    Et[:, C:], Eb[:, C:] = NAN, NAN
    Wt, Mt = _w_of(Lt, K, ubc, ibc)
    Wb, Mb = _w_of(Lb, K, ibc, ubc)
    S = dict(K=K, C=C, ld=ld, ubc=ubc, ibc=ibc, Lt=Lt, Lb=Lb, Et=Et, Eb=Eb, Wt=Wt, Wb=Wb, Mt=Mt, Mb=Mb)
    ratings = (0, 1, 255)
    rows = np.repeat(np.arange(4), 3).astype(np.uint32)
    val = np.tile(np.array(ratings, np.uint8), 4)
    terms, plain, wterms = _nnz_refs(S, rows, rows, val)
    z = np.einsum("rc,rc->r", Wt, Wb)                              # what the W form as written works on, in double
    assert z[0] > 1e-280 and 0.0 < z[1] < 2.0 ** -1022 and z[2] == 0.0 and z[3] == 0.0, z
    for v in (val, None):
        rr_, tt, pp = (rows, terms, plain) if v is not None else (rows[::3], *_nnz_refs(S, rows[::3], rows[::3], None)[:2])
        e, w = _run_both(S, rr_.size, devprobe.one_nonzero_per_block(rr_, rr_), rr_, v)
        assert np.all(np.isfinite(w)) and np.all(np.isfinite(e)), (e, w)
        _hold(f"limit, Elog route bias={with_bias}", e, tt, pp)
        _hold(f"limit, W route bias={with_bias}", w, tt, pp, extra=_yyy(v, rr_.size) * 2 * U)


def _export(D, hier, bias):
    names = ["THETA", "BETA"] + (["XI", "ETA"] if hier else []) + (["UBIAS", "IBIAS"] if bias else [])
    return {f"{o}_{k}": D.get_state(f"{o}_{k}") for o in names for k in ("SHAPE", "RATE", "E", "ELOG")}


def _elbo_refs(st, used, pairs, K, hier, bias, s_prior, r_prior):
    nnz, gamma = rr.elbo_terms(st, used, pairs, K, hier, bias, s_prior, r_prior)
    c_nnz = rr.c_ref([t[2] for t in nnz], [t[:2] for t in nnz])
    c_gamma = rr.c_ref([t[2] for t in gamma], [t[:2] for t in gamma])
    exact, bound = rr.elbo_bound(nnz, gamma, rr.c_for(c_nnz), rr.c_for(c_gamma))
    return exact, bound, c_nnz, c_gamma, rr.total_A(nnz, gamma)


@pytest.mark.parametrize("spread", LIMIT_SPREADS)
def test_w_route_limit_through_hpf_elbo(spread):
    """hpf_elbo on plain fp64 rows (K = 5: the W route) after hpf_set_state has given one user row and one item row Elog
    peaking at different columns with a combined spread of 600 .. 1400, joined by a nonzero of rating 3 and -- a second user
    with the same row -- by one whose rating wrapped to 0.  The call either fails with an HpfError or returns a finite value
    within the summed bound of the mpmath ELBO of the exported state (W is derive_w_kernel's: y yy u (4 + spread_t +
    spread_b) per nonzero, module docstring); it never hands out inf or NaN as a success.
    Seen: finite at every spread, |error| 0.13 u sum A; c_ref nonzero 91 .. 420 (the reference's running logsum), Gamma 1.7 .. 2.1.
    Without the fallback in elbo_nnz_w_kernel the call returned, as a success, a value off by 0.0148 at 740 (the bound there is
    4.7e-8) and NaN at 760 and 1400."""
    from hgaprec_amd.capi import Hpf, HpfError
    n, m, K = 8, 6, 5
    pairs = [(0, 0, 3, 1), (1, 0, 0, 1), (0, 1, 2, 1), (1, 2, 1, 1), (2, 1, 5, 1), (3, 3, 1, 1), (4, 4, 255, 1), (5, 5, 1, 1),
             (6, 2, 4, 1), (7, 3, 1, 1), (2, 4, 2, 1), (3, 5, 1, 1)]
    pairs.sort()
    rowptr = np.zeros(n + 1, np.int64)
    rowptr[1:] = np.cumsum(np.bincount([p[0] for p in pairs], minlength=n))
    col, val = np.array([p[1] for p in pairs], np.uint32), np.array([p[2] for p in pairs], np.uint8)
    D = Hpf(n, m, K, hier=True, bias=False, w_storage=3)
    D.upload_csr(rowptr, col, val)
    start = _start_state(n, m, K, True, False, 0.3, seed=21)
    for name, a in start.items():
        D.set_state(name, a)
    assert D.work_info()["w_layout"] == 0
    D.iterate(1)
    Lt, Lb = D.get_state("THETA_ELOG"), D.get_state("BETA_ELOG")
    lt, lb, _, _ = _limit_rows(K, spread, False)
    Lt[0], Lt[1], Lb[0] = lt[:K], lt[:K], lb[:K]
    D.set_state("THETA_ELOG", Lt)
    D.set_state("BETA_ELOG", Lb)
    try:
        got = D.elbo()
    except HpfError as e:
        print(f"\nhpf_elbo at spread {spread}: refused ({e})")
        D.close()
        return
    st = _export(D, True, False)
    assert np.array_equal(st["THETA_ELOG"], Lt) and np.array_equal(st["BETA_ELOG"], Lb)
    used = {"XI": (start["XI_E"], start["XI_ELOG"]), "ETA": (start["ETA_E"], start["ETA_ELOG"])}
    exact, bound, c_nnz, c_gamma, sum_A = _elbo_refs(st, used, pairs, K, True, False, 0.3, 0.3)
    sp_t, sp_b = (Lt.max(axis=1)[:, None] - Lt).max(axis=1), (Lb.max(axis=1)[:, None] - Lb).max(axis=1)
    bound += sum(y * max(y, 1) * U * (4 + sp_t[u] + sp_b[i]) for u, i, y, _ in pairs)
    D.close()
    err = rr.abs_err(got, exact)
    print(f"\nhpf_elbo at spread {spread}: {got!r}, c_ref nonzero {c_nnz:.2f} Gamma {c_gamma:.2f}, |error| / (u sum A) "
          f"{err / (U * sum_A):.3f}, |error| / bound {err / bound:.4f}")
    assert math.isfinite(got) and err <= bound, (got, float(exact), bound)


# ---- the Gamma term, per element -------------------------------------------------------------------------------------------
ONE, TWO = 1.0, 2.0
SHAPES = [0.0, -1.0, 1e-3, 0.3, np.nextafter(ONE, 0.0), ONE, np.nextafter(ONE, 2.0), np.nextafter(TWO, 0.0), TWO,
          np.nextafter(TWO, 3.0), 1.4616321449683623, 9.999, 10.0, 1e3, 1e6, 1e8, 2.5e8]
RATES = [1e-2, 1.0, 37.5, 1e6, 0.0]
S0, R0 = 0.3, 0.3


def _ev_el(a, b):
    """E and E[log] of about the size a Gamma(a, b) has (any doubles do: the term is a formula on what it is handed)"""
    a, b = max(a, 1e-30), max(b, 1e-30)
    return a / b, (math.log(a) - 0.5 / a if a > 1 else -1.0 / a - 0.5772) - math.log(b)


def _gamma_mats(shapes, ld=256):
    """one live element per row, at column 0 of a 256-column row: with a grid of as many blocks as rows, block r holds the
    element of row r alone.  The other columns hold NaN and must be skipped."""
    rows = len(shapes)
    S = np.full((rows, ld), NAN)
    S[:, 0] = shapes
    return S, np.full((rows, ld), NAN), np.full((rows, ld), NAN)


@pytest.mark.parametrize("mode", ["flat", "bias-column", "hier", "prior-array"])
def test_gamma_term_per_element(mode):
    """elbo_gamma_kernel, one live element per block.  Shapes: 0 and -1 (the 1e-30 clamp), 1e-3, 0.3, the zeros of lgamma at
    1 and 2 and one ulp on either side of each, lgamma's minimum 1.4616.., 9.999 and 10, 1e3, 1e6, 1e8, 2.5e8; rates 1e-2, 1,
    37.5, 1e6 and 0 (the clamp).
      flat          hier = 0: rate r_prior + colsum_used[0], prior r_prior / log r_prior; one launch per rate
      bias-column   the element sits in bias_col with K = 0: rate r_prior + bias_rate_add, the flat prior
      hier          rate prior_used[row] + colsum_used[0], prior prior_used[row] / prior_elog_used[row]; at column 0 the block
                    also adds the row's prior-array term: held to the sum of the two terms' bounds plus 2 u (|t1| + |t2|)
      prior-array   K = 0, no bias column: the prior-array term of the row alone (hier && c == 0), shape prior_shape
    The columns 1 .. 255 of every row hold NaN and are skipped as padding.
    Seen: c_ref 1.7 (flat, bias-column), 1.2 (prior-array, hier); device 1.4, 1.4, 1.2, and 0.17 of the two-term bound."""
    lg0 = math.lgamma(S0)
    terms, plain, got = [], [], []
    if mode in ("flat", "bias-column"):
        for rate in RATES:
            add = rate - R0
            b = R0 + add                                       # the double the kernel forms
            S, E, L = _gamma_mats(SHAPES)
            for r, a in enumerate(SHAPES):
                E[r, 0], L[r, 0] = _ev_el(a, b)
            cs = np.full(256, NAN)
            if mode == "flat":
                cs[0] = add
                got += list(devprobe.elbo_gamma(len(SHAPES), S, E, L, cs, 1, S0, R0, lg0))
            else:
                got += list(devprobe.elbo_gamma(len(SHAPES), S, E, L, cs, 0, S0, R0, lg0, bias_col=0, bias_rate_add=add))
            for r, a in enumerate(SHAPES):
                args = (float(a), b, E[r, 0], L[r, 0], S0, R0, None)
                terms.append(rr.gamma_term(*args)); plain.append(rr.plain_gamma_term(*args))
        _hold(f"Gamma term, {mode}", got, terms, plain)
        return
    rng = np.random.default_rng(8)
    combos = [(a, rate) for rate in RATES for a in SHAPES]
    rows = len(combos)
    prior_shape = S0 + 5 * S0
    pr_rate = rng.uniform(0.5, 3.0, rows)
    pr_rate[:3] = [1e-2, 1.0, 1e6]
    pr_E, pr_el = prior_shape / pr_rate, rng.uniform(-2.0, 2.0, rows)
    if mode == "prior-array":
        S, E, L = _gamma_mats([1.0] * rows)
        z = np.zeros(rows)
        got = devprobe.elbo_gamma(rows, S, E, L, np.full(256, NAN), 0, S0, R0, lg0, hier=True, prior_used=z, prior_elog_used=z,
                                  prior_E=pr_E, prior_elog=pr_el, prior_rate=pr_rate, prior_shape=prior_shape,
                                  lg_prior_shape=math.lgamma(prior_shape))
        for r in range(rows):
            args = (prior_shape, pr_rate[r], pr_E[r], pr_el[r], S0, R0, None)
            terms.append(rr.gamma_term(*args)); plain.append(rr.plain_gamma_term(*args))
        _hold("Gamma term, prior array", got, terms, plain)
        return
    S, E, L = _gamma_mats([c[0] for c in combos])
    cs = np.full(256, NAN)
    cs[0] = 0.25
    used = np.array([rate - 0.25 if rate > 0 else -0.25 for _, rate in combos])
    used_el = rng.uniform(-2.0, 2.0, rows)
    bs = used + 0.25
    for r, (a, _) in enumerate(combos):
        E[r, 0], L[r, 0] = _ev_el(a, bs[r])
    got = devprobe.elbo_gamma(rows, S, E, L, cs, 1, S0, R0, lg0, hier=True, prior_used=used, prior_elog_used=used_el,
                              prior_E=pr_E, prior_elog=pr_el, prior_rate=pr_rate, prior_shape=prior_shape,
                              lg_prior_shape=math.lgamma(prior_shape))
    both, c_terms, c_plain = [], [], []
    for r, (a, _) in enumerate(combos):
        a1 = (float(a), float(bs[r]), E[r, 0], L[r, 0], S0, float(used[r]), float(used_el[r]))
        a2 = (prior_shape, pr_rate[r], pr_E[r], pr_el[r], S0, R0, None)
        both.append((rr.gamma_term(*a1), rr.gamma_term(*a2)))
        c_terms += list(both[-1]); c_plain += [rr.plain_gamma_term(*a1), rr.plain_gamma_term(*a2)]
    c_ref = rr.c_ref(c_plain, c_terms)
    worst = 0.0
    for r, pair in enumerate(both):
        exact, bound = rr.sum_bound(list(pair), rr.c_for(c_ref))
        err = rr.abs_err(float(got[r]), exact)
        worst = max(worst, err / bound)
        assert err <= bound, (combos[r], float(got[r]), float(exact), bound)
    print(f"\nGamma term, hier (element + prior-array term): c_ref {c_ref:.2f}, largest |error| / bound {worst:.3f}")


def test_gamma_term_grid_stride_second_trip():
    """2700 x 104 elements (K = 100, a bias column, three NaN padding columns; hier) on the 1024 blocks hpf_elbo launches:
    280800 elements on 262144 threads, so the grid-stride loop takes a second trip for the rows from 2520 on.  The total of the
    block partials is held to the summed bound of all 272700 element terms and 2700 prior-array terms.  The mpmath side is a
    table: 40 unique shapes x 12 unique rates, E and E[log] functions of the two.  Seen: c_ref 1.8."""
    rows, K, ld = 2700, 100, 104
    rng = np.random.default_rng(9)
    shapes = np.concatenate([np.array(SHAPES[2:]), 10.0 ** rng.uniform(-1, 7, 40 - len(SHAPES[2:]))])
    pu_vals, cs_vals = np.array([0.4, 1.5, 2.75]), np.array([0.5, 7.0, 300.0, 12345.0])
    used_el_vals = np.array([-0.9, 0.3, 0.95])
    si = rng.integers(0, shapes.size, (rows, K + 1))
    pi_ = rng.integers(0, 3, rows)
    ci = np.arange(K) % 4
    add = 200.0
    S, E, L = np.full((rows, ld), NAN), np.full((rows, ld), NAN), np.full((rows, ld), NAN)
    cs = np.full(ld, NAN)
    cs[:K] = cs_vals[ci]
    table = {}
    prior_shape = S0 + K * S0
    pr_rate_vals, pr_el_vals = np.array([0.7, 1.9, 55.0]), np.array([-1.2, 0.1, 1.7])
    pri = rng.integers(0, 3, rows)

    def term(key, args):
        if key not in table:
            table[key] = rr.gamma_term(*args) + (rr.plain_gamma_term(*args), 0)
        e, A, p, cnt = table[key]
        table[key] = (e, A, p, cnt + 1)

    for r in range(rows):
        for c in range(K + 1):
            a = float(shapes[si[r, c]])
            if c < K:
                b = float(pu_vals[pi_[r]] + cs_vals[ci[c]])
                args = (a, b, *_ev_el(a, b), S0, float(pu_vals[pi_[r]]), float(used_el_vals[pi_[r]]))
                key = ("m", int(si[r, c]), int(pi_[r]), int(ci[c]))
            else:
                b = R0 + add
                args = (a, b, *_ev_el(a, b), S0, R0, None)
                key = ("b", int(si[r, c]))
            S[r, c], E[r, c], L[r, c] = a, args[2], args[3]
            term(key, args)
        b = float(pr_rate_vals[pri[r]])
        term(("p", int(pri[r])), (prior_shape, b, prior_shape / b, float(pr_el_vals[pri[r]]), S0, R0, None))
    got = devprobe.elbo_gamma(1024, S, E, L, cs, K, S0, R0, math.lgamma(S0), bias_col=K, bias_rate_add=add, hier=True,
                              prior_used=pu_vals[pi_], prior_elog_used=used_el_vals[pi_], prior_E=prior_shape / pr_rate_vals[pri],
                              prior_elog=pr_el_vals[pri], prior_rate=pr_rate_vals[pri], prior_shape=prior_shape,
                              lg_prior_shape=math.lgamma(prior_shape))
    uniq = list(table.values())
    c_ref = rr.c_ref([t[2] for t in uniq], [t[:2] for t in uniq])
    exact, bound = rr.elbo_bound([], uniq, 0.0, rr.c_for(c_ref))
    total = math.fsum(got)
    err = rr.abs_err(total, exact)
    print(f"\nGamma term, second trip: {len(uniq)} unique terms, c_ref {c_ref:.2f}, total {total!r}, |error| / bound {err / bound:.3f}, "
          f"bound / |total| {bound / abs(total):.1e}")
    assert sum(t[3] for t in uniq) == rows * (K + 2)
    assert np.all(np.isfinite(got)) and err <= bound


# ---- the whole ELBO at the wide range --------------------------------------------------------------------------------------
WIDE = [
    pytest.param(2, False, 3, id="K2-hier-plain"),
    pytest.param(21, True, 0, id="K21-hier-bias"),
    pytest.param(100, False, 0, id="K100-hier-regp59"),
]


@pytest.mark.parametrize("K,bias,w_storage", WIDE)
def test_whole_elbo_over_the_whole_shape_range(K, bias, w_storage):
    """the problem and start state of test_gpu_wide_range.py -- one popular item with a shape of 1e8, y yy = 65025 on 4e5
    duplicated lines -- after two iterations: hpf_elbo against the mpmath ELBO built from the exported SHAPE, RATE, E and ELOG
    of every object (the nonzero term once per unique pair, times its multiplicity; the prior of theta's and beta's rates is
    the XI / ETA exported BEFORE the second iteration, which is what that iteration's rates were built from), held to the
    summed bound.  K = 2 and 21 keep plain rows and take the W route, on the sweep's own W: y yy 2 (B_t + B_b) per line
    (module docstring); K = 100 packs its rows and takes the Elog route.
    Seen: c_ref nonzero 6.4 / 6.8 / 23.3, Gamma 1.7 / 1.8 / 1.8; |error| = 41 / 14 / 19 u sum A (5.3e5 additions), 3e-5 .. 9e-5
    of the bound, which is 5.5e-11 .. 5.8e-11 |ELBO| -- n u sum |term| for the additions is nearly all of it."""
    from hgaprec_amd.capi import Hpf
    n, m = 200, 60
    rowptr, col, val, (pu, pi, py, pm) = _problem()
    D = Hpf(n, m, K, hier=True, bias=bias, w_storage=w_storage)
    D.upload_csr(rowptr, col, val)
    for name, a in _start_state(n, m, K, True, bias, 0.3, seed=1000 + K).items():
        D.set_state(name, a)
    D.iterate(1)
    used = {o: (D.get_state(f"{o}_E"), D.get_state(f"{o}_ELOG")) for o in ("XI", "ETA")}
    D.iterate(1)
    from_w = D.work_info()["w_layout"] == 0
    assert from_w == (K < 100)
    got = D.elbo()
    st = _export(D, True, bias)
    D.close()
    assert st["THETA_SHAPE"].max() > 1e7 or st["BETA_SHAPE"].max() > 1e7
    pairs = list(zip(pu.tolist(), pi.tolist(), py.tolist(), pm.tolist()))
    exact, bound, c_nnz, c_gamma, sum_A = _elbo_refs(st, used, pairs, K, True, bias, 0.3, 0.3)
    if from_w:
        B = {}
        for o in ["THETA", "BETA"] + (["UBIAS", "IBIAS"] if bias else []):
            S_, R_, L_ = st[f"{o}_SHAPE"], st[f"{o}_RATE"], st[f"{o}_ELOG"]
            el, psi, logxs, corr = _mp_elog(S_, R_)
            b = U * (3.0 * logxs + 16.0 * corr + np.abs(psi)) + U * (2.0 * np.abs(np.log(R_)) + np.abs(el.astype(np.float64)))
            B[o] = b.max(axis=1) if b.ndim == 2 else b
        Bt = np.maximum(B["THETA"], B["UBIAS"]) if bias else B["THETA"]
        Bb = np.maximum(B["BETA"], B["IBIAS"]) if bias else B["BETA"]
        bound += sum(mult * y * max(y, 1) * 2.0 * (Bt[u] + Bb[i]) for u, i, y, mult in pairs)
    err = rr.abs_err(got, exact)
    print(f"\nwhole ELBO K={K} ({'W' if from_w else 'Elog'} route): {got!r}; c_ref nonzero {c_nnz:.2f}, Gamma {c_gamma:.2f}; "
          f"|error| / (u sum A) {err / (U * sum_A):.4f}, |error| / bound {err / bound:.2e}, bound / |ELBO| {bound / abs(got):.1e}")
    assert math.isfinite(got) and err <= bound, (got, float(exact), bound)
