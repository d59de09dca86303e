// moments_selftest.cpp -- CPU check of hpf_plan::moments_plan, the shape of hpf_score_moments' and hpf_recommend_ucb's
// kernels (tests/test_moments_plan.py builds and runs it; nothing links it).  A sweep over K = 1..HPF_MAX_COLUMNS with and
// without bias and a seeded list of pair, row, item and user counts checks
//   C == 2 K + 2 * bias <= HPF_MAX_COLUMNS, no plan beyond (K <= 511 with bias, K <= 512 without)
//   ldx >= C, ldx % 4 == 0, ldx < C + 4              the derived rows end on a whole MFMA step, rows of 32-byte multiples
//   mean_cols >= K, mean_cols % 4 == 0, mean_cols < K + 4, mean_steps == (K + 3) / 4, var_steps == (C + 3) / 4
//                                                    the two chains are those hpf_scores issues for K and for C columns
//   C, ldx, mean_cols even                           a 16-byte piece of the staged concatenation lies in one part
//   x_rows == topn_batch_users(...)                  X is built for exactly the users of a batch of the top-N sweep
//   1 <= grid_pairs, grid_rows <= MOMENTS_BLOCKS_MAX, nobody without a wave or thread below the cap, no idle workgroup
// stdout: for a fixed list of cases a line
//   mp K bias C ldx mean_cols mean_steps var_steps grid_pairs(1) grid_pairs(4099) grid_pairs(1638400) grid_rows(70) x_rows(700, 70, 64, 32)
// which the test compares with tests/data/moments_plan_table.txt, then `moments_selftest ok: <points> points`.
#include "../hpf_plan.hpp"

using namespace hpf_plan;

static int g_fail = 0;
#define CHECK(cond, ...)                                                                     \
  do { if (!(cond)) { if (++g_fail <= 20) { fprintf(stderr, "FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } } } while (0)

static void check_moments(uint32_t K, bool bias, uint64_t &rng)
{
  const uint32_t C = 2 * K + (bias ? 2u : 0u);
  const MomentsPlan p = moments_plan(K, bias);
  if (C > HPF_MAX_COLUMNS) { CHECK(!p.ok, "K=%u bias=%d: a plan beyond HPF_MAX_COLUMNS", K, (int)bias); return; }
  CHECK(p.ok, "K=%u bias=%d: no plan", K, (int)bias);
  CHECK(p.C == C, "K=%u bias=%d C=%u", K, (int)bias, p.C);
  CHECK(p.ldx >= C && p.ldx % 4 == 0 && p.ldx < C + 4, "K=%u bias=%d ldx=%u", K, (int)bias, p.ldx);
  CHECK(p.mean_cols >= K && p.mean_cols % 4 == 0 && p.mean_cols < K + 4, "K=%u mean_cols=%u", K, p.mean_cols);
  CHECK(p.mean_steps == (K + 3) / 4 && p.var_steps == (C + 3) / 4 && 4 * p.mean_steps == p.mean_cols && 4 * p.var_steps == p.ldx,
        "K=%u bias=%d steps %u %u", K, (int)bias, p.mean_steps, p.var_steps);
  CHECK(p.C % 2 == 0 && p.ldx % 2 == 0 && p.mean_cols % 2 == 0, "K=%u bias=%d: a piece across two parts", K, (int)bias);
  const uint64_t per = MomentsPlan::pairs_per_block();
  CHECK(per == (uint64_t)MOMENTS_WAVES * MOMENTS_PAIRS && MOMENTS_PAIRS == 16, "pairs per workgroup %llu", (unsigned long long)per);
  for (int i = 0; i < 8; ++i) {
    rng = rng * 6364136223846793005ull + 1442695040888963407ull;
    const uint64_t cnt = i == 0 ? 1u : i == 1 ? (1ull << 40) : (rng >> 24) >> ((rng >> 8) % 39);
    const uint32_t g = p.grid_pairs(cnt);
    CHECK(g >= 1 && g <= MOMENTS_BLOCKS_MAX, "K=%u cnt=%llu grid=%u", K, (unsigned long long)cnt, g);
    CHECK(cnt == 0 || g == MOMENTS_BLOCKS_MAX || (uint64_t)g * per >= cnt, "K=%u cnt=%llu grid=%u: pairs without a wave", K, (unsigned long long)cnt, g);
    CHECK(cnt == 0 || (uint64_t)(g - 1) * per < cnt, "K=%u cnt=%llu grid=%u: an idle workgroup", K, (unsigned long long)cnt, g);
    const uint32_t rows = i == 0 ? 1u : i == 1 ? 0xffffffffu : (uint32_t)(rng >> 32) >> ((rng >> 16) % 31);
    const uint32_t gr = p.grid_rows(rows);
    CHECK(gr >= 1 && gr <= MOMENTS_BLOCKS_MAX, "K=%u rows=%u grid=%u", K, rows, gr);
    CHECK(rows == 0 || gr == MOMENTS_BLOCKS_MAX || (uint64_t)gr * 256 >= (uint64_t)rows * p.ldx, "K=%u rows=%u grid=%u: elements without a thread", K, rows, gr);
    CHECK(rows == 0 || (uint64_t)(gr - 1) * 256 < (uint64_t)rows * p.ldx, "K=%u rows=%u grid=%u: an idle workgroup", K, rows, gr);
    const uint32_t m = 1u + (uint32_t)(rng >> 40) % 200000u, n_sel = 1u + (uint32_t)(rng >> 20) % 100000u, topn = 1u + (uint32_t)(rng >> 12) % TOPN_FUSED_MAX;
    const long long knob = (i & 1) ? (long long)(1 + (rng >> 50) % 200) : 0;
    const uint32_t x = p.x_rows(m, n_sel, topn, knob);
    CHECK(x == topn_batch_users(m, n_sel, topn_cap(topn), knob) && x >= 16 && x % 16 == 0, "K=%u m=%u n_sel=%u topn=%u: x_rows %u", K, m, n_sel, topn, x);
    CHECK(p.derived_bytes(m, x) == ((uint64_t)m + x) * p.ldx * 8, "K=%u: derived bytes", K);
  }
}

int main()
{
  uint64_t rng = 20261021u;
  unsigned points = 0;
  for (uint32_t K = 1; K <= HPF_MAX_COLUMNS; ++K)
    for (int bias = 0; bias < 2; ++bias) { check_moments(K, bias != 0, rng); ++points; }
  CHECK(!moments_plan(0, false).ok, "K=0 has a plan");
  CHECK(moments_plan(511, true).ok && moments_plan(512, false).ok && !moments_plan(512, true).ok && !moments_plan(513, false).ok, "the limit");
  const uint32_t cases[] = {1, 2, 3, 5, 14, 16, 17, 50, 63, 64, 65, 100, 127, 128, 129, 255, 256, 510, 511, 512, 513, 1024};
  for (uint32_t K : cases)
    for (int bias = 0; bias < 2; ++bias) {
      const MomentsPlan p = moments_plan(K, bias != 0);
      if (!p.ok) { printf("mp %u %d none\n", K, bias); continue; }
      printf("mp %u %d %u %u %u %u %u %u %u %u %u %u\n", K, bias, p.C, p.ldx, p.mean_cols, p.mean_steps, p.var_steps,
             p.grid_pairs(1), p.grid_pairs(4099), p.grid_pairs(1638400), p.grid_rows(70), p.x_rows(700, 70, 64, 32));
    }
  if (g_fail) { fprintf(stderr, "moments_selftest: %d checks failed\n", g_fail); return 1; }
  printf("moments_selftest ok: %u points\n", points);
  return 0;
}
