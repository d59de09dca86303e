// hpf_rng.hpp -- a counter-based generator and a Gamma sampler, host and device.
//
// One posterior draw of the model (hpf_sample_state, hpf_recommend_thompson) needs a Gamma(shape, rate) variate for every
// element of both sides, the same bits whatever the batches, the grid, the selection or the order of the calls.  So a
// variate is a pure function of (seed, draw, side, row, column): Philox4x32-10 keyed by the seed, counted by the element.
// Nothing here needs a HIP header: a CPU build (host/rng_selftest.cpp) compiles the same lines, the high halves of the
// products from a 64-bit product where the device takes __umulhi.  tests/thompson_ref.py states the same algorithm in numpy.
//
//   key      (seed low 32 bits, seed high 32 bits)
//   counter  (column c, row r, draw t, object | b << 4 | j << 8): block b of attempt j; object 0 = user side, 1 = item side;
//            r the row's index on its side (the LOCAL user index), c the column in the handle's row layout
//   uniform  from two words x, y: n = (x >> 6) * 2^26 + (y >> 6) (52 bits), u = (n + 0.5) * 2^-52: exact in fp64, strictly
//            inside (0, 1), symmetric.  Block 0: u1 (words 0, 1), u2 (words 2, 3); block 1: u3, u4
//   gamma    Marsaglia-Tsang for Gamma(a, 1), the acceptance test in the form log u3 < z^2 / 2 + d (3 log1p(w) - w (3 + w (3 + w))),
//            in which nothing cancels at large shapes (d - v d + d log v with v = (1 + w)^3 loses everything there); a < 1 by
//            the boost g(a + 1) u4^(1 / a).  Every line is one fp64 operation or one libm / ocml call, nothing is contracted.
#ifndef HPF_RNG_HPP
#define HPF_RNG_HPP

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define HPF_RNG_HD __host__ __device__ __forceinline__
#else
#define HPF_RNG_HD inline
#endif

namespace hpf_rng {

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;   // the multipliers
constexpr uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;   // the key increments
constexpr int      GAMMA_ATTEMPTS = 32;                                // the loop's bound (8 bits of the counter word hold it)
constexpr double   TWO_PI = 6.283185307179586476925286766559;          // the double nearest 2 pi

struct Block { uint32_t w[4]; };

HPF_RNG_HD uint32_t mulhi32(uint32_t a, uint32_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
  return __umulhi(a, b);
#else
  return (uint32_t)(((uint64_t)a * b) >> 32);
#endif
}

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw 2011): ten rounds, the key bumped between them
HPF_RNG_HD Block philox4x32(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = mulhi32(PHILOX_M0, c0), lo0 = PHILOX_M0 * c0;
    const uint32_t hi1 = mulhi32(PHILOX_M1, c2), lo1 = PHILOX_M1 * c2;
    c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    k0 += PHILOX_W0; k1 += PHILOX_W1;
  }
  Block b;
  b.w[0] = c0; b.w[1] = c1; b.w[2] = c2; b.w[3] = c3;
  return b;
}

// block b of attempt j of element (object, row, col) of draw `draw`
HPF_RNG_HD Block element_block(uint64_t seed, uint32_t draw, uint32_t object, uint32_t row, uint32_t col, uint32_t b, uint32_t j)
{
  return philox4x32(col, row, draw, object | (b << 4) | (j << 8), (uint32_t)seed, (uint32_t)(seed >> 32));
}

// u = (n + 0.5) 2^-52 of the 52 bits n = (x >> 6) 2^26 + (y >> 6): both operations exact
HPF_RNG_HD double uniform52(uint32_t x, uint32_t y)
{
  const uint64_t n = ((uint64_t)(x >> 6) << 26) + (uint64_t)(y >> 6);
  const double h = (double)n + 0.5;
  return h * 0x1p-52;
}

// what the sampler decided for one element, for tests/thompson_ref.py to be compared with
struct GammaTrace {
  int    attempt = -1;     // the accepted attempt, -1: none of GAMMA_ATTEMPTS was (never on the domain)
  double t = 0.0;          // 1 + w of the accepted attempt
  double q = 0.0;          // log(u4) / a where a < 1, else 0.0
  double u[4] = {0.0, 0.0, 0.0, 0.0};   // the uniforms of the accepted attempt (of the last one tried where none was)
};

// One Gamma(a, 1) variate of element (seed, draw, object, row, col).  Domain: a finite and > 0.  A NaN shape rejects every
// attempt and returns NaN after GAMMA_ATTEMPTS of them; a = 0 returns 0.
HPF_RNG_HD double gamma_unit(uint64_t seed, uint32_t draw, uint32_t object, uint32_t row, uint32_t col, double a, GammaTrace *tr)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const bool   small = a < 1.0;
  const double ap = small ? a + 1.0 : a;
  const double d = ap - 1.0 / 3.0;
  const double d9 = 9.0 * d;
  const double sd = sqrt(d9);
  const double cc = 1.0 / sd;
  double g = ap, u4 = 1.0;
  for (uint32_t j = 0; j < (uint32_t)GAMMA_ATTEMPTS; ++j) {
    const Block b0 = element_block(seed, draw, object, row, col, 0, j);
    const double u1 = uniform52(b0.w[0], b0.w[1]), u2 = uniform52(b0.w[2], b0.w[3]);
    const double l1 = log(u1);
    const double m2 = -2.0 * l1;
    const double rad = sqrt(m2);
    const double ang = TWO_PI * u2;
    const double cs = cos(ang);
    const double z = rad * cs;
    const double w = cc * z;
    if (tr) { tr->u[0] = u1; tr->u[1] = u2; }
    if (!(w > -1.0)) continue;
    const Block b1 = element_block(seed, draw, object, row, col, 1, j);
    const double u3 = uniform52(b1.w[0], b1.w[1]);
    const double lp = log1p(w);
    const double l = 3.0 * lp;
    const double p1 = 3.0 + w;
    const double p2 = w * p1;
    const double p3 = 3.0 + p2;
    const double p = w * p3;
    const double h = l - p;
    const double l3 = log(u3);
    const double hz = 0.5 * z;
    const double zz = hz * z;
    const double dh = d * h;
    const double rhs = zz + dh;
    if (tr) { tr->u[2] = u3; tr->u[3] = uniform52(b1.w[2], b1.w[3]); }
    if (l3 < rhs) {
      const double t = 1.0 + w;
      const double t2 = t * t;
      const double t3 = t2 * t;
      g = d * t3;
      u4 = uniform52(b1.w[2], b1.w[3]);
      if (tr) { tr->attempt = (int)j; tr->t = t; }
      break;
    }
  }
  if (small) {
    const double l4 = log(u4);
    const double q = l4 / a;
    const double e = exp(q);
    g = g * e;
    if (tr) tr->q = q;
  }
  return g;
}

// The sample of an element with expectation e and shape a: Gamma(a, rate) = Gamma(a, 1) / rate and 1 / rate = e / a, so the
// rate is never read.  e = +0.0 gives +0.0.
HPF_RNG_HD double gamma_sample(uint64_t seed, uint32_t draw, uint32_t object, uint32_t row, uint32_t col, double e, double a, GammaTrace *tr)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double g = gamma_unit(seed, draw, object, row, col, a, tr);
  const double scale = e / a;
  return g * scale;
}

}  // namespace hpf_rng

#endif  // HPF_RNG_HPP
