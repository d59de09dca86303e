// fold_selftest.cpp -- CPU check of hpf_plan::fold_plan, the shape of hpf_fold_in's kernel (tests/test_fold_plan.py builds and
// runs it; nothing links it).  A seeded sweep over K = 1..HPF_MAX_COLUMNS with and without bias and over user counts checks
//   R * 64 >= ld >= K + 2 * bias, a kernel instance for R          the row's columns lie across the 64 lanes, R per lane
//   LDS per workgroup <= the 64 KiB a launch may ask for            and three workgroups fit a CU's 160 KiB
//   1 <= rows_held <= 64 and rows_held * ld * 8 <= the wave's slice
//   grid(n) >= 1 for n >= 1, never more waves than FOLD_BLOCKS_MAX workgroups hold
// stdout: for a fixed list of cases a line
//   fp K bias ld R lds_wave_bytes rows_held grid(1) grid(5) grid(100000) grid(4000000)
// which the test compares with tests/data/fold_plan_table.txt, then `fold_selftest ok: <points> points`.
#include "../hpf_plan.hpp"

using namespace hpf_plan;

static int g_fail = 0;
#define CHECK(cond, ...)                                                                     \
  do { if (!(cond)) { if (++g_fail <= 20) { fprintf(stderr, "FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } } } while (0)

static void check_fold(uint32_t K, bool bias, uint64_t &rng)
{
  const uint32_t C = K + (bias ? 2u : 0u);
  const FoldPlan p = fold_plan(K, bias);
  if (C > HPF_MAX_COLUMNS) { CHECK(!p.ok, "K=%u bias=%d: a plan beyond HPF_MAX_COLUMNS", K, (int)bias); return; }
  CHECK(p.ok, "K=%u bias=%d: no plan", K, (int)bias);
  CHECK(p.ld >= C && p.ld % 16 == 0 && p.ld < C + 16, "K=%u bias=%d ld=%u", K, (int)bias, p.ld);
  CHECK(p.R * 64 >= p.ld && (p.R - 1) * 64 < p.ld && has_fold((int)p.R), "K=%u bias=%d ld=%u R=%u", K, (int)bias, p.ld, p.R);
  CHECK(p.lds_block_bytes() == FOLD_WAVES * p.lds_wave_bytes && p.lds_block_bytes() <= FOLD_LDS_LIMIT && 3 * p.lds_block_bytes() <= 160u * 1024u,
        "K=%u bias=%d lds=%u", K, (int)bias, p.lds_block_bytes());
  CHECK(p.rows_held >= 1 && p.rows_held <= 64 && (uint64_t)p.rows_held * p.ld * 8 <= p.lds_wave_bytes, "K=%u bias=%d rows_held=%u", K, (int)bias, p.rows_held);
  CHECK(p.rows_held == 64 || (uint64_t)(p.rows_held + 1) * p.ld * 8 > p.lds_wave_bytes, "K=%u bias=%d rows_held=%u: room for one more", K, (int)bias, p.rows_held);
  for (int i = 0; i < 8; ++i) {
    rng = rng * 6364136223846793005ull + 1442695040888963407ull;
    const uint32_t n = i == 0 ? 1u : i == 1 ? 0xffffffffu : (uint32_t)(rng >> 32) >> ((rng >> 8) % 31);
    const uint32_t g = p.grid(n);
    CHECK(g >= 1 && g <= FOLD_BLOCKS_MAX, "K=%u n=%u grid=%u", K, n, g);
    CHECK(n == 0 || g == FOLD_BLOCKS_MAX || (uint64_t)g * FOLD_WAVES >= n, "K=%u n=%u grid=%u: users without a wave", K, n, g);
    CHECK(n == 0 || (uint64_t)(g - 1) * FOLD_WAVES < n, "K=%u n=%u grid=%u: an idle workgroup", K, n, g);
  }
}

int main()
{
  uint64_t rng = 20260101u;
  unsigned points = 0;
  for (uint32_t K = 1; K <= HPF_MAX_COLUMNS; ++K)
    for (int bias = 0; bias < 2; ++bias) { check_fold(K, bias != 0, rng); ++points; }
  CHECK(!fold_plan(0, false).ok, "K=0 has a plan");
  const uint32_t cases[] = {1, 3, 7, 14, 16, 17, 20, 50, 62, 64, 65, 100, 126, 128, 129, 190, 192, 256, 300, 512, 760, 768, 1000, 1022, 1024};
  for (uint32_t K : cases)
    for (int bias = 0; bias < 2; ++bias) {
      const FoldPlan p = fold_plan(K, bias != 0);
      if (!p.ok) { printf("fp %u %d none\n", K, bias); continue; }
      printf("fp %u %d %u %u %u %u %u %u %u %u\n", K, bias, p.ld, p.R, p.lds_wave_bytes, p.rows_held, p.grid(1), p.grid(5), p.grid(100000), p.grid(4000000));
    }
  if (g_fail) { fprintf(stderr, "fold_selftest: %d checks failed\n", g_fail); return 1; }
  printf("fold_selftest ok: %u points\n", points);
  return 0;
}
