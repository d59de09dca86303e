"""CPU: pin the oracle (oracle/liborc.so) to everything pinnable here.

 * golden vectors produced by the reference's own GSL-free code (matrix.hh,
   env.hh, log.cc compiled in place -> tests/golden/make_golden.py): bit-exact;
 * published known answers for MT19937 (GSL manual: first default-seed output
   4293858116; C++ standard: 10000th output of seed 5489 is 4123659995) and
   numpy's RandomState (same generator + init_genrand seeding);
 * digamma against mpmath at 50 digits.
The end-to-end path stays "parity unpinned" (the full reference needs GSL).
"""
import hashlib
import json
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

GOLD = Path(__file__).parent / "golden"


def unhex(lst):
    return np.array([float.fromhex(s) for s in lst], dtype=np.float64)


def test_mt19937_published_known_answers(orc):
    r = orc.Rng(0)                      # gsl_rng_default_seed = 0 -> 4357
    assert r.u32() == 4293858116        # value printed in the GSL reference manual
    r = orc.Rng(5489)
    for _ in range(9999):
        r.u32()
    assert r.u32() == 4123659995        # ISO C++ [rand.predef] mt19937 check value


@pytest.mark.parametrize("seed", [4357, 1, 7, 2 ** 31, 2 ** 32 - 1])
def test_mt19937_matches_numpy_randomstate(orc, seed):
    r = orc.Rng(seed)
    got = np.array([r.u32() for _ in range(2000)], dtype=np.uint64)
    rs = np.random.RandomState(seed)
    want = rs.randint(0, 2 ** 32, size=2000, dtype=np.uint64)
    assert np.array_equal(got, want)


def test_uniform_is_u32_over_2_32_and_uniform_int(orc):
    a, b = orc.Rng(7), orc.Rng(7)
    for _ in range(100):
        assert a.uniform() == b.u32() / 4294967296.0
    a, b = orc.Rng(9), orc.Rng(9)
    for n in (1000, 6040, 3):
        scale = 0xFFFFFFFF // n
        k = a.uniform_int(n)
        while True:
            w = b.u32() // scale
            if w < n:
                break
        assert k == w


def test_digamma_against_mpmath(orc):
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    xs = np.concatenate([np.linspace(0.3, 0.32, 50), np.geomspace(1e-30, 1e8, 300),
                         np.array([0.3, 1.0, 1.4616321449683623, 2.0, 10.0, 20.0, 100.0])])
    got = orc.psi(xs)
    for x, g in zip(xs, got):
        w = float(mp.digamma(mp.mpf(float(x))))
        assert abs(g - w) <= 4e-16 * max(1.0, abs(w)), (x, g, w)


def test_softmax_golden_bit_exact(orc):
    d = json.loads((GOLD / "softmax.json").read_text())
    for c in d["cases"]:
        x = unhex(c["x"])
        assert orc.logsum(x) == float.fromhex(c["logsum"])
        phi = orc.lognormalize(x)
        if c["y"] > 1:
            phi = phi * float(c["y"])
        assert np.array_equal(phi, unhex(c["phi"]))


def test_accumulate_golden_bit_exact(orc):
    d = json.loads((GOLD / "accumulate.json").read_text())
    for c in d["cases"]:
        rows, K = c["rows"], c["K"]
        M = np.full((rows, K), 0.3)
        for r in c["recs"]:
            phi = orc.lognormalize(unhex(r["x"]))
            if r["y"] > 1:
                phi = phi * float(r["y"])
            M[r["row"], :] += phi[:K]            # add_slice: first K entries only
        assert np.array_equal(M.ravel(), unhex(c["M"]))


def test_tsv_writers_golden(orc, tmp_path):
    d = json.loads((GOLD / "save.json").read_text())
    for c in d["cases"]:
        A = unhex(c["A"]).reshape(c["rows"], c["cols"])
        v = unhex(c["v"])
        ids = np.array(c["ids"], np.uint32)
        orc.save_matrix(tmp_path / "m.tsv", A, ids)
        orc.save_vector(tmp_path / "v.tsv", v, ids)
        assert (tmp_path / "m.tsv").read_text() == c["matrix_tsv"]
        assert (tmp_path / "v.tsv").read_text() == c["vector_tsv"]


def live_softmax_input():
    """the records of test_oracle_against_live_reference_build and refpart's `softmax` input file holding them"""
    rng = np.random.default_rng(1234)
    recs = [(rng.normal(size=n) * s - 3.0, int(rng.integers(0, 6)))
            for n in (2, 5, 22, 100, 202) for s in (1.0, 20.0)]
    payload = struct.pack("<I", len(recs))
    for x, y in recs:
        payload += struct.pack("<II", x.size, y) + x.astype("<f8").tobytes()
    return recs, payload


def live_rows_inputs():
    """the cases of test_sweep_steps_against_live_reference_build: (mode, sn, ev, u, v) and refpart's `rows` input file"""
    rng = np.random.default_rng(99)
    out = []
    for mode, rows, k in ((0, 11, 22), (1, 5, 22), (2, 13, 1), (3, 13, 1)):
        sn = 0.3 + rng.gamma(0.5, 3.0, size=(rows, k))
        ev, u, v = rng.gamma(2.0, 0.2, size=rows), rng.gamma(1.0, 30.0, size=rows if mode == 2 else k), 6.3
        payload = (struct.pack("<IIIddd", mode, rows, k, 0.3, 0.3, v) + sn.astype("<f8").tobytes()
                   + ev.astype("<f8").tobytes() + u.astype("<f8").tobytes())
        out.append(((mode, sn, ev, u, v), payload))
    return out


def live_key(cmd, payload):
    return f"{cmd}:{hashlib.sha256(payload).hexdigest()[:16]}"


def refpart_output(orc, cmd, payload, tmp_path):
    """refpart's output for this input: run live where oracle/_ref/refpart is built (and then equal to the stored copy),
    elsewhere the copy tests/golden/live.json keeps of the same input (tests/golden/make_golden.py live)"""
    stored = json.loads((GOLD / "live.json").read_text())["runs"].get(live_key(cmd, payload))
    if orc.REFPART.exists():
        fin, fout = tmp_path / "i.bin", tmp_path / "o.bin"
        fin.write_bytes(payload)
        r = subprocess.run([str(orc.REFPART), cmd, str(fin), str(fout)])
        if r.returncode == 0:
            raw = np.fromfile(fout, "<f8")
            assert stored is None or np.array_equal(raw, unhex(stored)), f"refpart {cmd} disagrees with its stored output"
            return raw
        assert r.returncode == 2 and stored is not None, f"refpart {cmd} failed (rc {r.returncode})"   # 2: predates `cmd`
    assert stored is not None, f"no stored refpart output for {live_key(cmd, payload)}: tests/golden/make_golden.py live"
    return unhex(stored)


def test_oracle_against_live_reference_build(orc, tmp_path):
    """fresh random vectors through oracle/_ref/refpart (where it is built; elsewhere its stored output for the same
    vectors, tests/golden/live.json)"""
    recs, payload = live_softmax_input()
    raw, pos = refpart_output(orc, "softmax", payload, tmp_path), 0
    for x, y in recs:
        phi = orc.lognormalize(x)
        if y > 1:
            phi = phi * float(y)
        assert orc.logsum(x) == raw[pos]
        assert np.array_equal(phi, raw[pos + 1: pos + 1 + x.size])
        pos += 1 + x.size


def test_initialize_draw_order_and_counts(orc):
    """the number of MT19937 words consumed by HGAPRec::initialize"""
    n, m, K = 13, 7, 4
    for hier, bias, want in (
        (True, False, n + m + (m * K + K + m * K) + (n * K + K + n * K)),
        (True, True, n + m + (m * K + K + m * K) + (n * K + K + n * K) + n + m),
        (False, False, (m * K + K) + (n * K + K) + m * K + n * K),
        (False, True, (m * K + K) + (n * K + K) + m * K + n * K + n + m),
    ):
        M = orc.Model(n, m, K, hier, bias, False)
        M.initialize(7)
        r = orc.Rng(7)
        for _ in range(want):
            r.u32()
        assert M.rng_u32() == r.u32()


def test_initialize_values_follow_the_stream(orc):
    n, m, K = 5, 3, 2
    M = orc.Model(n, m, K, True, False, False)
    M.initialize(0)
    r = orc.Rng(0)
    xi_shape = np.array([0.3 + 0.01 * r.uniform() for _ in range(n)])
    eta_shape = np.array([0.3 + 0.01 * r.uniform() for _ in range(m)])
    beta_shape = np.array([0.3 + 0.01 * r.uniform() for _ in range(m * K)]).reshape(m, K)
    for _ in range(K):
        r.uniform()
    brate = np.array([0.3 + 0.1 * r.uniform() for _ in range(m * K)]).reshape(m, K)
    assert np.array_equal(M.state("XI_SHAPE"), xi_shape)
    assert np.array_equal(M.state("ETA_SHAPE"), eta_shape)
    assert np.array_equal(M.state("XI_RATE"), np.full(n, 0.3 + K))
    assert np.array_equal(M.state("BETA_SHAPE"), beta_shape)
    assert np.array_equal(M.state("BETA_E"), beta_shape / brate)
    assert np.allclose(M.state("BETA_ELOG"), orc.psi(beta_shape.ravel()).reshape(m, K) - np.log(brate),
                       rtol=0, atol=1e-15)


def test_sum_set_elements_zero_golden_bit_exact(orc):
    """D1Array::sum is a plain left-to-right sum from 0.0 -- what GPMatrix::sum_rows / sum_cols
    (gpbase.hh:264-280) are made of; the oracle's row / column sums go through the same loop
    (also with a stride, as sum_rows walks a column).  set_elements / zero carry no arithmetic."""
    d = json.loads((GOLD / "arrays.json").read_text())
    for c in d["cases"]:
        x = unhex(c["x"])
        assert orc.seq_sum(x) == float.fromhex(c["sum"])
        assert orc.seq_sum(x[: c["maxn"]]) == float.fromhex(c["sum_maxn"])
        wide = np.zeros((x.size, 3)); wide[:, 0] = x               # the same numbers, 3 apart
        assert orc.seq_sum(wide.ravel(), stride=3) == float.fromhex(c["sum"])
        assert np.all(unhex(c["set_elements"]) == float.fromhex(c["fill"])) and len(c["set_elements"]) == 3 * x.size
        assert np.all(unhex(c["zero"]) == 0.0)


def test_sweep_steps_golden_bit_exact(orc):
    """the rest of the pinnable set: D2Array::set_elements(row, v), add_slice of one vector on every row,
    D1Array::operator+=, swap + set_elements(prior) -- the reference's own containers, called in gpbase.hh's order by
    oracle/ref_harness.cc -- against the very functions the oracle's iteration runs (orc_test_sweep_steps), bit for bit.
    What this does NOT pin is that gpbase.hh calls them in that order: that translation unit needs GSL."""
    d = json.loads((GOLD / "rows.json").read_text())
    modes = set()
    for c in d["cases"]:
        rows, k, mode = c["rows"], c["k"], c["mode"]
        sn = unhex(c["snext_in"]).reshape(rows, k)
        got = orc.sweep_steps(mode, sn, unhex(c["ev"]), unhex(c["u"]), float.fromhex(c["v"]))
        for g, nm in zip(got, ("scurr", "rcurr", "snext", "rnext")):
            assert np.array_equal(g, unhex(c[nm])), (mode, rows, k, nm)
        # and what the values ARE: the rate row is E[xi_row] + colsum (the 0.3 it held is overwritten, gpbase.hh:168)
        if mode == 0:
            assert np.array_equal(unhex(c["rcurr"]).reshape(rows, k), unhex(c["ev"])[:, None] + unhex(c["u"])[None, :])
        if mode == 1:
            assert np.array_equal(unhex(c["rcurr"]), 0.3 + unhex(c["u"]))
        if mode == 2:
            assert np.array_equal(unhex(c["scurr"]), sn.ravel() + float.fromhex(c["v"]))
            assert np.array_equal(unhex(c["rcurr"]), 0.3 + unhex(c["u"]))
        if mode == 3:
            assert np.array_equal(unhex(c["rcurr"]), np.full(rows, 0.3) + float.fromhex(c["v"]))
        assert np.all(unhex(c["snext"]) == 0.3) and np.all(unhex(c["rnext"]) == 0.3)
        modes.add(mode)
    assert modes == {0, 1, 2, 3}


def test_sweep_steps_against_live_reference_build(orc, tmp_path):
    """fresh random arrays through oracle/_ref/refpart rows (where it is built; elsewhere its stored output for the same
    arrays, tests/golden/live.json)"""
    for (mode, sn, ev, u, v), payload in live_rows_inputs():
        rows, k = sn.shape
        raw = refpart_output(orc, "rows", payload, tmp_path)
        ns, nr = rows * k, (k if mode == 1 else rows * k)
        got = orc.sweep_steps(mode, sn, ev, u, v)
        want = (raw[:ns], raw[ns:ns + nr], raw[ns + nr:2 * ns + nr], raw[2 * ns + nr:])
        for g, w in zip(got, want):
            assert np.array_equal(g, w)


def test_model_rate_sums_are_the_pinned_loop(orc):
    """the column sums inside the oracle's sweep (sum_rows, gpbase.hh:264-271) are, per column,
    the left-to-right loop pinned above: without -hier the theta rate after one iteration is
    0.3 + sum_i E[beta_ik] (gpbase.hh:558-562), bit for bit"""
    from tests.util import make_problem
    n, m, K = 40, 30, 7
    rowptr, col, val = make_problem(n, m, 300, 3)
    M = orc.Model(n, m, K, False, False, False)
    M.set_csr(rowptr, col, val)
    M.initialize(11)
    be = M.state("BETA_E").copy()
    M.iterate(1)
    tr = M.state("THETA_RATE")
    for k in range(K):
        assert tr[k] == 0.3 + orc.seq_sum(be.ravel()[k:], stride=K, n=m)


def test_vb_bias_novb_branch_by_construction(orc):
    """vb_bias() with -novb (hgaprec.cc:1276-1297): theta.update_rate_next(betasum), then
    _theta.sum_rows() -- still the OLD expectations, nothing is swapped yet -- feeds
    beta.update_rate_next; the default branch (1250-1272) swaps theta first.  The K-vector
    rates after one iteration say which sums went in."""
    from tests.util import make_problem
    n, m, K = 120, 90, 4
    rowptr, col, val = make_problem(n, m, 1500, 8)
    runs = {}
    for novb in (False, True):
        M = orc.Model(n, m, K, False, True, False, novb=novb)
        M.set_csr(rowptr, col, val)
        M.initialize(8)
        start_t, start_b = M.state("THETA_E").copy(), M.state("BETA_E").copy()
        M.iterate(1)
        runs[novb] = {w: M.state(w).copy() for w in ("THETA_RATE", "BETA_RATE", "THETA_E", "BETA_E", "UBIAS_RATE", "IBIAS_RATE")}
    for novb in (False, True):
        assert np.allclose(runs[novb]["THETA_RATE"], 0.3 + start_b.sum(0), rtol=1e-14)     # both: old sum_i E[beta]
        assert np.allclose(runs[novb]["UBIAS_RATE"], 0.3 + m) and np.allclose(runs[novb]["IBIAS_RATE"], 0.3 + n)
    assert np.allclose(runs[True]["BETA_RATE"], 0.3 + start_t.sum(0), rtol=1e-14)          # -novb: OLD sum_u E[theta]
    assert np.allclose(runs[False]["BETA_RATE"], 0.3 + runs[False]["THETA_E"].sum(0), rtol=1e-14)   # default: the new one
    assert np.array_equal(runs[True]["THETA_E"], runs[False]["THETA_E"])                   # theta's update is the same
    # without -bias the flag is never read (vb(), hgaprec.cc:919-980)
    outs = []
    for novb in (False, True):
        M = orc.Model(n, m, K, False, False, False, novb=novb)
        M.set_csr(rowptr, col, val); M.initialize(8); M.iterate(2)
        outs.append(M.state("BETA_E").copy())
    assert np.array_equal(outs[0], outs[1])
