// because_selftest.cpp -- CPU check of hpf_plan::because_plan, the shape of hpf_because's two kernels
// (tests/test_because_plan.py builds and runs it; nothing links it).  A sweep over K = 1..HPF_MAX_COLUMNS with and
// without bias and a seeded list of user and pair counts checks
//   ld >= K + 2 * bias, ld a multiple of 16 (whole 128-byte lines), ld == fold_plan's (the gathered copy is the fold-in's)
//   R * 64 >= ld > (R - 1) * 64, a kernel instance for R        the columns lie across the 64 lanes, R per lane
//   1 <= grid_users(n), grid_pairs(nt) <= BECAUSE_BLOCKS_MAX, nobody without a wave below the cap, no idle workgroup
// stdout: for a fixed list of cases a line
//   bp K bias ld R grid_users(1) grid_users(40) grid_users(16384) grid_pairs(1) grid_pairs(4099) grid_pairs(1638400)
// which the test compares with tests/data/because_plan_table.txt, then `because_selftest ok: <points> points`.
#include "../hpf_plan.hpp"

using namespace hpf_plan;

static int g_fail = 0;
#define CHECK(cond, ...)                                                                     \
  do { if (!(cond)) { if (++g_fail <= 20) { fprintf(stderr, "FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } } } while (0)

static_assert(BECAUSE_MAX == HPF_BECAUSE_MAX && BECAUSE_MAX <= 64, "a lane per returned entry");

static void check_because(uint32_t K, bool bias, uint64_t &rng)
{
  const uint32_t C = K + (bias ? 2u : 0u);
  const BecausePlan p = because_plan(K, bias);
  if (C > HPF_MAX_COLUMNS) { CHECK(!p.ok, "K=%u bias=%d: a plan beyond HPF_MAX_COLUMNS", K, (int)bias); return; }
  CHECK(p.ok, "K=%u bias=%d: no plan", K, (int)bias);
  CHECK(p.ld >= C && p.ld % 16 == 0 && p.ld < C + 16 && p.ld == fold_plan(K, bias).ld, "K=%u bias=%d ld=%u", K, (int)bias, p.ld);
  CHECK(p.R * 64 >= p.ld && (p.R - 1) * 64 < p.ld && has_because((int)p.R), "K=%u bias=%d ld=%u R=%u", K, (int)bias, p.ld, p.R);
  const uint64_t per = BecausePlan::pairs_per_block();
  CHECK(per == (uint64_t)BECAUSE_WAVES * BECAUSE_RUN, "pairs per workgroup %llu", (unsigned long long)per);
  for (int i = 0; i < 8; ++i) {
    rng = rng * 6364136223846793005ull + 1442695040888963407ull;
    const uint64_t nt = i == 0 ? 1u : i == 1 ? (1ull << 40) : (rng >> 24) >> ((rng >> 8) % 39);
    const uint32_t g = p.grid_pairs(nt);
    CHECK(g >= 1 && g <= BECAUSE_BLOCKS_MAX, "K=%u nt=%llu grid=%u", K, (unsigned long long)nt, g);
    CHECK(nt == 0 || g == BECAUSE_BLOCKS_MAX || (uint64_t)g * per >= nt, "K=%u nt=%llu grid=%u: pairs without a wave", K, (unsigned long long)nt, g);
    CHECK(nt == 0 || (uint64_t)(g - 1) * per < nt, "K=%u nt=%llu grid=%u: an idle workgroup", K, (unsigned long long)nt, g);
    const uint32_t n = i == 0 ? 1u : i == 1 ? 0xffffffffu : (uint32_t)(rng >> 32) >> ((rng >> 16) % 31);
    const uint32_t gu = p.grid_users(n);
    CHECK(gu >= 1 && gu <= BECAUSE_BLOCKS_MAX, "K=%u n=%u grid=%u", K, n, gu);
    CHECK(n == 0 || gu == BECAUSE_BLOCKS_MAX || (uint64_t)gu * BECAUSE_WAVES >= n, "K=%u n=%u grid=%u: users without a wave", K, n, gu);
    CHECK(n == 0 || (uint64_t)(gu - 1) * BECAUSE_WAVES < n, "K=%u n=%u grid=%u: an idle workgroup", K, n, gu);
  }
}

int main()
{
  uint64_t rng = 20261021u;
  unsigned points = 0;
  for (uint32_t K = 1; K <= HPF_MAX_COLUMNS; ++K)
    for (int bias = 0; bias < 2; ++bias) { check_because(K, bias != 0, rng); ++points; }
  CHECK(!because_plan(0, false).ok, "K=0 has a plan");
  const uint32_t cases[] = {1, 3, 5, 14, 16, 17, 50, 62, 63, 64, 65, 100, 126, 128, 129, 130, 190, 192, 256, 512, 768, 1000, 1022, 1024};
  for (uint32_t K : cases)
    for (int bias = 0; bias < 2; ++bias) {
      const BecausePlan p = because_plan(K, bias != 0);
      if (!p.ok) { printf("bp %u %d none\n", K, bias); continue; }
      printf("bp %u %d %u %u %u %u %u %u %u %u\n", K, bias, p.ld, p.R, p.grid_users(1), p.grid_users(40), p.grid_users(16384),
             p.grid_pairs(1), p.grid_pairs(4099), p.grid_pairs(1638400));
    }
  if (g_fail) { fprintf(stderr, "because_selftest: %d checks failed\n", g_fail); return 1; }
  printf("because_selftest ok: %u points\n", points);
  return 0;
}
