"""-m gpu: the hand-written device arithmetic of hpf_kernels.hpp, function by function, against mpmath.

Every number of an iteration passes through fast_rcp, the two digammas (psi_parts / digamma_pos and the row sweep's
psi_parts_rate), exp_neg and the p59 row codec; the parity tests see them only through whole iterations at 1e-9, where a
slip of 1e-12 relative would pass and then drift into the model over hundreds of sweeps.  Here each function is called
on its own through libhpf_probe.so (hgaprec_amd/csrc/hpf_probe.hip, which calls the very inline functions of the header)
and held against a reference computed with mpmath at 50 digits or more and rounded once to double.

The bounds are a-priori rounding models in u = 2^-53, computed from reference quantities, not fitted to the device:
  fast_rcp   relative error <= 2^-52: the seed's error is squared twice, the last FMA's rounding is what remains
  ri         relative error <= 2^-51: one reciprocal and two roundings (the source's "~2 ulp")
  psi        |psi_dev - psi_ref| <= u (3 log xs + 16 corr_ref + |psi_ref|), corr_ref = log xs - psi_ref: the log is
             1 ulp, the shift and the series cost ~16 roundings of corr, the subtraction one of the result
  W          relative error <= u (16 corr_ref + 10) where W_ref >= 1e-290; below that only W_dev <= 1e-289
  exp_neg    relative error <= 4u where the result is normal, one denormal spacing below, exactly 0 from c = 746 on
Each test prints the measured maximum of error / bound (per band of x where x is the argument) before it asserts; the
header comments above psi_parts, psi_parts_rate and exp_neg quote those figures.
"""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
ROOT_OF_PSI = 1.4616321449683623
BANDS = [(1e-30, 0.3), (0.3, 10.0), (10.0, 1e3), (1e3, math.inf)]     # [lo, hi); the last one is [1e3, 1e300]
BAND_NAMES = ["[1e-30, 0.3)", "[0.3, 10)", "[10, 1e3)", "[1e3, 1e300]"]
TWO_M127 = 2.0 ** -127


def _report(what, x, ratio):
    """the measured maximum of error / bound per band of x"""
    parts = []
    for (lo, hi), name in zip(BANDS, BAND_NAMES):
        m = (x >= lo) & (x < hi)
        parts.append(f"{name}: {ratio[m].max():.3f} (n={int(m.sum())})" if m.any() else f"{name}: -")
    print(f"\n{what}: max error/bound  " + "  ".join(parts))


@pytest.fixture(scope="module")
def probe():
    from tests import devprobe
    devprobe.load()
    return devprobe


@pytest.fixture(scope="module")
def psi_ref():
    """x, rt and the references: psi(x), xs, log xs, corr = log xs - psi(x), W = exp(psi(x)) / rt.  Computed once."""
    import mpmath as mp
    rng = np.random.default_rng(20240611)
    x_log = 10.0 ** rng.uniform(-30.0, 18.0, 4000)
    x_uni = rng.uniform(0.3, 12.0, 6000)
    x_edge = np.array([np.nextafter(10.0, 0.0), 10.0, np.nextafter(10.0, 20.0), 0.3, 1.0, ROOT_OF_PSI,
                       1e-30, 1e30, 1e100, 1e300])                   # the last three: t, p and dp of the shift overflow
    x_floor = rng.uniform(0.3, 100.0, 500)                           # shapes that meet the make_nonzero floor of a rate
    x = np.concatenate([x_log, x_uni, x_edge, x_floor])
    rt = 10.0 ** rng.uniform(-6.0, 12.0, x.size)
    # x >= 1e100: a rate with x / rt finite -- and x * rt, the operand of the sweep's one reciprocal, finite as well
    huge = x >= 1e100
    rt[huge] = 10.0 ** rng.uniform(-6.0, 0.0, int(huge.sum()))
    rt[x.size - x_floor.size:] = 1e-30
    xs = np.where(x < 10.0, x + 10.0, x)

    n = x.size
    psi, logxs, corr, w = np.empty(n), np.empty(n), np.empty(n), np.empty(n)
    for i in range(n):
        # log xs - psi cancels down to 1 / (2 xs): digits for that difference as well
        mp.mp.dps = 50 if xs[i] < 1e20 else 700
        X, XS = mp.mpf(float(x[i])), mp.mpf(float(xs[i]))
        p = mp.digamma(X)
        l = mp.log(XS)
        psi[i], logxs[i], corr[i] = float(p), float(l), float(l - p)
        w[i] = float(mp.exp(p) / mp.mpf(float(rt[i])))
    mp.mp.dps = 15
    for a in (x, rt, xs, psi, logxs, corr, w):
        a.setflags(write=False)
    return dict(x=x, rt=rt, xs=xs, psi=psi, logxs=logxs, corr=corr, w=w)


def test_fast_rcp_is_within_one_ulp(probe):
    import mpmath as mp
    mp.mp.dps = 50
    rng = np.random.default_rng(7)
    x = np.concatenate([10.0 ** rng.uniform(-300.0, 300.0, 20000), rng.uniform(1.0, 2.0, 2000),
                        [1e-300, 1e300, 1.0, 2.0, np.nextafter(2.0, 0.0), np.nextafter(1.0, 2.0), 3.0, 10.0]])
    r = probe.rcp(x)
    assert np.all(np.isfinite(r))
    rel = np.array([float(abs(mp.mpf(float(a)) * mp.mpf(float(b)) - 1)) for a, b in zip(x, r)])
    mp.mp.dps = 15
    print(f"\nfast_rcp: max relative error {rel.max() / U:.3f} u (bound 2 u)")
    assert rel.max() <= 2.0 ** -52


def test_digamma_pos_against_mpmath(probe, psi_ref):
    R = psi_ref
    x = R["x"]
    psi, xs, corr = probe.psi(x)
    assert np.all(np.isfinite(psi)) and np.all(np.isfinite(xs)) and np.all(np.isfinite(corr))
    assert np.array_equal(xs, R["xs"])                   # the shift is by exactly 10, on x < 10 only
    bound = U * (3.0 * R["logxs"] + 16.0 * R["corr"] + np.abs(R["psi"]))
    ratio = np.abs(psi - R["psi"]) / bound
    _report("digamma_pos", x, ratio)
    bad = np.flatnonzero(ratio > 1.0)
    assert bad.size == 0, [(x[i], psi[i], R["psi"][i], ratio[i]) for i in bad[:5]]


def test_sweep_element_against_mpmath(probe, psi_ref):
    import mpmath as mp
    R = psi_ref
    x, rt = R["x"], R["rt"]
    w, ri, corr = probe.sweep_elem(x, rt)
    assert np.all(np.isfinite(w)) and np.all(np.isfinite(ri)) and np.all(np.isfinite(corr))
    # ri = 1 / rt
    mp.mp.dps = 50
    rel = np.array([float(abs(mp.mpf(float(a)) * mp.mpf(float(b)) - 1)) for a, b in zip(rt, ri)])
    mp.mp.dps = 15
    print(f"\npsi_parts_rate ri: max relative error {rel.max() / U:.3f} u (bound 4 u)")
    assert rel.max() <= 2.0 ** -51
    # W = exp(psi(x)) / rt
    big = R["w"] >= 1e-290
    assert np.all(w[~big] <= 1e-289)
    bound = U * (16.0 * R["corr"][big] + 10.0)
    ratio = np.abs(w[big] - R["w"][big]) / R["w"][big] / bound
    _report("sweep element W", x[big], ratio)
    bad = np.flatnonzero(ratio > 1.0)
    assert bad.size == 0, [(x[big][i], rt[big][i], w[big][i], R["w"][big][i], ratio[i]) for i in bad[:5]]


def test_exp_neg_against_mpmath(probe):
    import mpmath as mp
    mp.mp.dps = 50
    rng = np.random.default_rng(11)
    ln2 = math.log(2.0)
    c = np.concatenate([rng.uniform(0.0, 708.0, 20000), 10.0 ** rng.uniform(-20.0, 0.0, 2000), rng.uniform(708.0, 746.0, 500),
                        [0.0, ln2 / 2, ln2, np.nextafter(ln2 / 2, 0.0), np.nextafter(ln2 / 2, 1.0), 745.0, 746.0, 750.0, 760.0, 1e6]])
    got = probe.exp_neg(c)
    assert np.all(np.isfinite(got)) and np.all(got >= 0.0)
    ref_mp = [mp.exp(-mp.mpf(float(v))) for v in c]
    ref = np.array([float(v) for v in ref_mp])
    tiny = np.finfo(np.float64).tiny
    normal = ref >= tiny
    rel = np.array([float(abs(mp.mpf(float(g)) - r) / r) for g, r, nm in zip(got, ref_mp, normal) if nm])
    mp.mp.dps = 15
    print(f"\nexp_neg: max relative error {rel.max() / U:.3f} u over {rel.size} normal results (bound 4 u); "
          f"max |error| below {np.abs(got[~normal] - ref[~normal]).max() / 2.0 ** -1074:.1f} denormal spacings")
    assert rel.max() <= 4.0 * U
    assert np.all(np.abs(got[~normal] - ref[~normal]) <= 2.0 ** -1074)
    assert np.all(got[c >= 746.0] == 0.0)
    assert got[c == 0.0][0] == 1.0


# ---------------------------------------------------------------------------------------------------------------------
# the p59 row codec: both writers against the reader, for every row shape
# ---------------------------------------------------------------------------------------------------------------------
P59_SHAPES = [(L, G) for L in range(1, 9) for G in (8, 64)]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _random_p59_values(rng, n):
    """doubles in [2^-126, 2): every exponent field 897..1023, random 52-bit mantissas"""
    e = rng.integers(897, 1024, n, dtype=np.uint64)
    m = rng.integers(0, 1 << 52, n, dtype=np.uint64)
    return ((e << np.uint64(52)) | m).view(np.float64)


@pytest.mark.parametrize("L,G", P59_SHAPES)
def test_p59_round_trip_is_exact(probe, L, G):
    ld = G * probe.p59_E(L)
    nrows = -(-2000 // ld)
    w = _random_p59_values(np.random.default_rng(100 + L), nrows * ld).reshape(nrows, ld)
    rows = []
    for writer in (0, 1):
        out, flushed, rb = probe.p59(L, G, writer, w)
        assert np.array_equal(_bits(out), _bits(w)), f"writer {writer}"
        assert not flushed.any()
        rows.append(rb)
    assert np.array_equal(rows[0], rows[1])


@pytest.mark.parametrize("L,G", P59_SHAPES)
def test_p59_boundaries(probe, L, G):
    """2^-126 and the largest value below 2 (and 1.0 between them) are stored exactly; what the rows cannot hold --
    the predecessor of 2^-126, a denormal, 2.0, zeros, a negative number, inf, NaN -- reads back as 2^-127, the value of
    the all-zero element, and is reported as flushed unless it is an exact +0.  Every value visits every column."""
    lo = 2.0 ** -126
    exact = [lo, 1.0, np.nextafter(2.0, 0.0)]
    gone = [np.nextafter(lo, 0.0), 2.0, 5e-324, 1e-310, -1.0, -0.0, math.inf, -math.inf, math.nan, 0.0]
    B = np.array(exact + gone)
    ld = G * probe.p59_E(L)
    r, c = np.meshgrid(np.arange(B.size), np.arange(ld), indexing="ij")
    w = B[(r + c) % B.size]
    keep = np.isin(_bits(w), _bits(np.array(exact)))
    plus0 = _bits(w) == 0
    want = np.where(keep, w, TWO_M127)
    rows = []
    for writer in (0, 1):
        out, flushed, rb = probe.p59(L, G, writer, w)
        assert np.array_equal(_bits(out), _bits(want)), f"writer {writer}"
        assert np.array_equal(flushed != 0, ~keep & ~plus0), f"writer {writer}"
        rows.append(rb)
    assert np.array_equal(rows[0], rows[1])


@pytest.mark.parametrize("L,G", P59_SHAPES)
def test_p59_columns_past_the_row_read_as_the_zero_element(probe, L, G):
    ld = G * probe.p59_E(L)
    w = _random_p59_values(np.random.default_rng(200 + L), 3 * ld).reshape(3, ld)
    for ncols in sorted({ld - 1, max(1, ld - G - 3), ld // 2 + 1, 1}):
        rows = []
        for writer in (0, 1):
            out, flushed, rb = probe.p59(L, G, writer, w, ncols=ncols)
            assert np.array_equal(_bits(out[:, :ncols]), _bits(w[:, :ncols])), (writer, ncols)
            assert np.all(out[:, ncols:] == TWO_M127), (writer, ncols)
            assert not flushed.any()
            rows.append(rb)
        assert np.array_equal(rows[0], rows[1]), ncols


@pytest.mark.parametrize("L", range(1, 9))
def test_p59_pos_is_a_permutation_and_the_same_at_run_time(probe, L):
    """the LDS writer computes the dword places at run time from PackedRow (p59_pos), the reader and the register writer at
    compile time (codec_p59<L>::pos): the same table, one-to-one into the lane's 4L dwords (the probe library also
    asserts this at compile time, for both dword orders)"""
    E = probe.p59_E(L)
    S = (27 * E + 31) // 32
    for G in (4, 8, 16, 32, 64):
        rt, ct = probe.p59_pos(L, G)
        assert rt.size == E + S <= 4 * L
        assert np.array_equal(rt, ct)
        assert len(set(ct.tolist())) == ct.size and ct.max() < 4 * L
    if probe.p59_paired():               # low word of element e beside stream dword e, as the header documents
        assert all(ct[k] == 2 * k for k in range(min(E, 2 * L)))
        assert all(ct[E + j] == 2 * j + 1 for j in range(S))
    else:
        assert np.array_equal(ct, np.arange(E + S))
