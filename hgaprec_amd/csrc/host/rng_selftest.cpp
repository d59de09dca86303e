// rng_selftest.cpp -- hpf_rng.hpp on a CPU, and the launch shape of gamma_rows_kernel (hpf_plan::sample_plan).
// tests/test_rng_host.py builds and runs it; nothing links it.  The lines of the generator and of the sampler compiled here
// are the ones gamma_rows_kernel compiles for the device (-ffp-contract=off stands in for the pragma g++ does not know).
//
// It reads commands from stdin, one per line, and answers each with one line; numbers are hexadecimal, a double is its 64
// bits (16 digits):
//   philox c0 c1 c2 c3 k0 k1              -> philox w0 w1 w2 w3              one Philox4x32-10 block
//   uniform x y                           -> uniform U                       the uniform of two words
//   block seed draw object row col b j    -> block w0 w1 w2 w3               block b of attempt j of an element
//   gamma seed draw object row col A      -> gamma G attempt T Q U1 U2 U3 U4 one Gamma(A, 1) variate with its trace: the
//                                            accepted attempt (decimal, -1: none), 1 + w, log(u4) / a, the four uniforms
//   sample seed draw object row col E A   -> sample X                        the sample of an element: g * (E / A)
//   plan                                  -> plan ok: <points> points        walks sample_plan and sample_piece_rows
// An unknown command or a malformed line ends the run with status 2.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../hpf_plan.hpp"
#include "../hpf_rng.hpp"

using namespace hpf_rng;

static int g_fail = 0;
#define CHECK(cond, ...)                                                                     \
  do { if (!(cond)) { if (++g_fail <= 20) { fprintf(stderr, "FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } } } while (0)

static uint64_t bits_of(double x) { uint64_t b; memcpy(&b, &x, 8); return b; }
static double double_of(uint64_t b) { double x; memcpy(&x, &b, 8); return x; }

// sample_plan: 1 <= grid <= SAMPLE_BLOCKS_MAX, every element has a thread below the cap, no idle workgroup; a piece of
// hpf_sample_state has at least one row, no more rows than are selected, and fits SAMPLE_PIECE_BYTES where one row does
static unsigned walk_plan()
{
  using namespace hpf_plan;
  uint64_t rng = 20261021u;
  unsigned points = 0;
  for (uint32_t ld = 2; ld <= HPF_MAX_COLUMNS + 4; ld += (ld < 40 ? 1 : 37))
    for (int i = 0; i < 40; ++i, ++points) {
      rng = rng * 6364136223846793005ull + 1442695040888963407ull;
      const uint64_t rows = i == 0 ? 0u : i == 1 ? 1u : i == 2 ? 0xffffffffu : (uint32_t)(rng >> 32) >> ((rng >> 16) % 31);
      const SamplePlan p = sample_plan(rows, ld);
      CHECK(p.elements == rows * ld, "rows=%" PRIu64 " ld=%u elements", rows, ld);
      CHECK(p.grid >= 1 && p.grid <= SAMPLE_BLOCKS_MAX, "rows=%" PRIu64 " ld=%u grid=%u", rows, ld, p.grid);
      CHECK(p.grid == SAMPLE_BLOCKS_MAX || (uint64_t)p.grid * 256 >= p.elements, "rows=%" PRIu64 " ld=%u grid=%u: elements without a thread", rows, ld, p.grid);
      CHECK(rows == 0 || (uint64_t)(p.grid - 1) * 256 < p.elements, "rows=%" PRIu64 " ld=%u grid=%u: an idle workgroup", rows, ld, p.grid);
      const uint32_t n_sel = (uint32_t)rows ? (uint32_t)rows : 1u, piece = sample_piece_rows(n_sel, ld);
      CHECK(piece >= 1 && piece <= n_sel, "n_sel=%u ld=%u piece=%u", n_sel, ld, piece);
      CHECK(piece == 1 || (uint64_t)piece * ld * 8 <= SAMPLE_PIECE_BYTES, "n_sel=%u ld=%u piece=%u: beyond the piece", n_sel, ld, piece);
      CHECK(piece == n_sel || (uint64_t)(piece + 1) * ld * 8 > SAMPLE_PIECE_BYTES, "n_sel=%u ld=%u piece=%u: a piece could be longer", n_sel, ld, piece);
    }
  return points;
}

int main()
{
  char line[512];
  while (fgets(line, sizeof line, stdin)) {
    char cmd[16] = "";
    uint64_t v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int got = sscanf(line, "%15s %" SCNx64 " %" SCNx64 " %" SCNx64 " %" SCNx64 " %" SCNx64 " %" SCNx64 " %" SCNx64, cmd, &v[0], &v[1], &v[2],
                           &v[3], &v[4], &v[5], &v[6]);
    if (got < 1) continue;
    const int nargs = got - 1;
    if (!strcmp(cmd, "philox") && nargs == 6) {
      const Block b = philox4x32((uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3], (uint32_t)v[4], (uint32_t)v[5]);
      printf("philox %08x %08x %08x %08x\n", b.w[0], b.w[1], b.w[2], b.w[3]);
    } else if (!strcmp(cmd, "uniform") && nargs == 2) {
      printf("uniform %016" PRIx64 "\n", bits_of(uniform52((uint32_t)v[0], (uint32_t)v[1])));
    } else if (!strcmp(cmd, "block") && nargs == 7) {
      const Block b = element_block(v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3], (uint32_t)v[4], (uint32_t)v[5], (uint32_t)v[6]);
      printf("block %08x %08x %08x %08x\n", b.w[0], b.w[1], b.w[2], b.w[3]);
    } else if (!strcmp(cmd, "gamma") && nargs == 6) {
      GammaTrace tr;
      const double g = gamma_unit(v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3], (uint32_t)v[4], double_of(v[5]), &tr);
      printf("gamma %016" PRIx64 " %d %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", bits_of(g), tr.attempt,
             bits_of(tr.t), bits_of(tr.q), bits_of(tr.u[0]), bits_of(tr.u[1]), bits_of(tr.u[2]), bits_of(tr.u[3]));
    } else if (!strcmp(cmd, "sample") && nargs == 7) {
      const double x = gamma_sample(v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3], (uint32_t)v[4], double_of(v[5]), double_of(v[6]), nullptr);
      printf("sample %016" PRIx64 "\n", bits_of(x));
    } else if (!strcmp(cmd, "plan") && nargs == 0) {
      const unsigned points = walk_plan();
      if (g_fail) { fprintf(stderr, "rng_selftest: %d checks failed\n", g_fail); return 1; }
      printf("plan ok: %u points\n", points);
    } else {
      fprintf(stderr, "rng_selftest: cannot read the line: %s", line);
      return 2;
    }
  }
  return 0;
}
