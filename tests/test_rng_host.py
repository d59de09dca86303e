"""CPU: hgaprec_amd/csrc/hpf_rng.hpp -- the generator and the Gamma sampler of hpf_sample_state / hpf_recommend_thompson -- as
host/rng_selftest.cpp compiles it with g++ (`make -C hgaprec_amd/csrc rng`), the lines gamma_rows_kernel compiles for the
device.  Philox4x32-10 against the Random123 known answers; Philox, the element counters and the uniforms bit for bit against
tests/thompson_ref.py; the Gamma variates against it within the bound the GPU test uses, the decisions (accepted attempt)
equal; a NaN shape and a shape of 0 return; the launch shape of gamma_rows_kernel (hpf_plan::sample_plan).  The same program
under ASan + UBSan (`make rng_asan`) walks the same lines."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import thompson_ref as ref

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "hgaprec_amd" / "csrc"

# Random123's kat_vectors for philox4x32 10 (recomputed with the plain-integer Philox of thompson_ref.philox_int)
KNOWN = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]


@pytest.fixture(scope="module", params=["rng", "rng_asan"])
def exe(request):
    r = subprocess.run(["make", "-C", str(CSRC), request.param], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return str(ROOT / "hgaprec_amd" / ("rng_selftest" if request.param == "rng" else "rng_selftest_asan"))


def run(exe, lines, ok=True):
    r = subprocess.run([exe], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, timeout=120)
    assert (r.returncode == 0) == ok, (r.returncode, r.stderr[-3000:])
    out = r.stdout.splitlines()
    assert not ok or len(out) == len(lines)
    return out if ok else r


def f64(hexes):
    return np.array([int(h, 16) for h in hexes], dtype=np.uint64).view(np.float64)


def test_known_answers(exe):
    out = run(exe, ["philox %x %x %x %x %x %x" % (c + k) for c, k, _ in KNOWN])
    assert out == ["philox " + w for _, _, w in KNOWN]
    for c, k, w in KNOWN:
        assert " ".join("%08x" % x for x in ref.philox_int(c, k)) == w
        assert " ".join("%08x" % int(x) for x in ref.philox(*c, *k)) == w


def test_philox_counters_and_uniforms_equal_the_reference_bit_for_bit(exe):
    rng = np.random.default_rng(1)
    N = 300
    c = rng.integers(0, 2 ** 32, (N, 4), dtype=np.uint64)
    k = rng.integers(0, 2 ** 32, (N, 2), dtype=np.uint64)
    c[:4] = [[0, 0, 0, 0], [2 ** 32 - 1] * 4, [1, 0, 0, 0], [0, 0, 0, 1]]
    out = run(exe, ["philox %x %x %x %x %x %x" % (*map(int, c[i]), *map(int, k[i])) for i in range(N)])
    w = ref.philox(c[:, 0], c[:, 1], c[:, 2], c[:, 3], k[:, 0], k[:, 1])
    assert out == ["philox %08x %08x %08x %08x" % tuple(int(x[i]) for x in w) for i in range(N)]
    # the counter of block b of attempt j of an element: (column, row, draw, object | b << 4 | j << 8), key (seed low, seed high)
    seed = rng.integers(0, 2 ** 64, N, dtype=np.uint64)
    draw, row = rng.integers(0, 2 ** 32, N, dtype=np.uint64), rng.integers(0, 2 ** 32, N, dtype=np.uint64)
    col, obj, b, j = rng.integers(0, 1024, N), rng.integers(0, 2, N), rng.integers(0, 2, N), rng.integers(0, 32, N)
    out = run(exe, ["block %x %x %x %x %x %x %x" % (int(seed[i]), int(draw[i]), obj[i], int(row[i]), col[i], b[i], j[i]) for i in range(N)])
    for i in range(N):
        want = ref.philox_int((int(col[i]), int(row[i]), int(draw[i]), int(obj[i]) | (int(b[i]) << 4) | (int(j[i]) << 8)),
                              (int(seed[i]) & 0xffffffff, int(seed[i]) >> 32))
        assert out[i] == "block %08x %08x %08x %08x" % want, i
        assert tuple(int(x) for x in ref.element_block(int(seed[i]), draw[i], obj[i], row[i], col[i], b[i], j[i])) == want, i
    # uniforms: 52 bits, (n + 0.5) 2^-52, strictly inside (0, 1), symmetric
    x, y = c[:, 0].copy(), c[:, 1].copy()
    x[:2], y[:2] = [0, 2 ** 32 - 1], [0, 2 ** 32 - 1]
    out = run(exe, ["uniform %x %x" % (int(x[i]), int(y[i])) for i in range(N)])
    u = f64([ln.split()[1] for ln in out])
    assert np.array_equal(u.view(np.uint64), ref.bits(ref.uniform(x, y)))
    assert u[0] == 2.0 ** -53 and u[1] == 1.0 - 2.0 ** -53 and np.all((u > 0) & (u < 1))
    assert np.array_equal(ref.uniform(~x & ref.MASK32, ~y & ref.MASK32), 1.0 - u)


def test_gamma_variates_within_the_bound_of_the_reference(exe):
    rng = np.random.default_rng(2)
    N = 4000
    a = np.exp(rng.uniform(np.log(0.05), np.log(1e8), N))
    a[:6] = [0.05, 0.3, np.nextafter(1.0, 0.0), 1.0, np.nextafter(1.0, 2.0), 1e8]
    row, col, obj = rng.integers(0, 2 ** 32, N, dtype=np.uint64), rng.integers(0, 1024, N).astype(np.uint64), 1
    out = run(exe, ["gamma %x 0 %x %x %x %016x" % (ref.SEED, obj, int(row[i]), int(col[i]), int(ref.bits(a)[i])) for i in range(N)])
    f = [ln.split() for ln in out]
    g, attempt, t, q = f64([x[1] for x in f]), np.array([int(x[2]) for x in f]), f64([x[3] for x in f]), f64([x[4] for x in f])
    want, tr = ref.gamma_unit(ref.SEED, 0, obj, row, col, a)
    assert tr["ratio"].min() >= ref.MARGIN_MIN and np.abs(tr["t"]).min() >= ref.T_MIN        # no decision near its edge: they agree
    assert np.array_equal(attempt, tr["attempt"]) and attempt.min() >= 0 and 1 <= attempt.max() < 8
    assert np.array_equal(ref.bits(t), ref.bits(tr["t"])) or np.abs(t - tr["t"]).max() <= 8 * ref.U
    rel = np.abs(g - want) / want
    b = ref.bound(tr, a)
    print(f"largest error / bound {np.max(rel / b):.4f}, largest error {rel.max() / ref.U:.2f} x 2^-52, bit-equal share {np.mean(g == want):.4f}")
    assert np.all(rel <= b) and np.all(np.abs(q - tr["q"]) <= 4 * ref.U * np.abs(tr["q"]))
    assert np.all(np.isfinite(g)) and np.all(g > 0)
    # the sample of an element: g * (E / a); E = +0.0 gives +0.0
    E = rng.random(N) * 3.0
    E[:3] = 0.0
    out = run(exe, ["sample %x 0 %x %x %x %016x %016x" % (ref.SEED, obj, int(row[i]), int(col[i]), int(ref.bits(E)[i]), int(ref.bits(a)[i]))
                    for i in range(N)])
    x = f64([ln.split()[1] for ln in out])
    assert np.array_equal(ref.bits(x), ref.bits(g * (E / a))) and np.all(ref.bits(x[:3]) == 0)


def test_a_nan_shape_and_a_shape_of_zero_return(exe):
    out = run(exe, ["gamma 5 0 0 1 2 %016x" % int(ref.bits(np.nan)[0]), "gamma 5 0 0 1 2 %016x" % 0, "gamma 5 0 0 1 2 %016x" % int(ref.bits(-1.0)[0]),
                    "gamma 5 0 0 1 2 %016x" % int(ref.bits(np.inf)[0])])
    g = f64([ln.split()[1] for ln in out])
    attempt = [int(ln.split()[2]) for ln in out]
    assert np.isnan(g[0]) and attempt[0] == -1                      # every attempt refused, the loop's bound ends it
    assert ref.bits(g[1])[0] == 0 and attempt[1] >= 0               # u4^(1 / 0) = +0.0
    want, tr = ref.gamma_unit(5, 0, 0, np.array([1, 1]), np.array([2, 2]), np.array([np.nan, 0.0]))
    assert np.isnan(want[0]) and want[1] == 0.0 and list(tr["attempt"]) == attempt[:2] and tr["tries"][0] == ref.ATTEMPTS
    assert len(out) == 4                                            # a negative and an infinite shape return too


def test_launch_shape_and_malformed_input(exe):
    assert run(exe, ["plan"]) == ["plan ok: 2600 points"]
    r = run(exe, ["gamma 1 2 3"], ok=False)
    assert r.returncode == 2 and "cannot read the line" in r.stderr
