// explain_selftest.cpp -- CPU check of hpf_plan::explain_plan, the shape of hpf_explain's kernel, and of
// hpf_plan::factor_top_batch (tests/test_explain_plan.py builds and runs it; nothing links it).  A seeded sweep over
// K = 1..HPF_MAX_COLUMNS with and without bias and over pair counts checks
//   terms == K + 2 * bias, R * 64 >= terms > (R - 1) * 64, a kernel instance for R     the terms lie across the 64 lanes, R per lane
//   1 <= grid(cnt) <= EXPLAIN_BLOCKS_MAX, no pair without a wave below the cap, no idle workgroup
//   pairs_per_trip(cnt) == grid(cnt) * EXPLAIN_WAVES * EXPLAIN_RUN
//   factor_top_batch: 1 <= batch <= K, batch * rows * 8 <= 512 MB unless batch == 1, never above the knob
// stdout: for a fixed list of cases a line
//   ep K bias terms R grid(1) grid(5) grid(4099) grid(10000000) pairs_per_trip(10000000)
// and for a fixed list of (rows, K, knob) a line
//   ft rows K knob batch
// which the test compares with tests/data/explain_plan_table.txt, then `explain_selftest ok: <points> points`.
#include "../hpf_plan.hpp"

using namespace hpf_plan;

static int g_fail = 0;
#define CHECK(cond, ...)                                                                     \
  do { if (!(cond)) { if (++g_fail <= 20) { fprintf(stderr, "FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } } } while (0)

static_assert(EXPLAIN_MAX == HPF_EXPLAIN_MAX && EXPLAIN_MAX <= 64, "a lane per returned term");
static_assert(FACTOR_TOP_MAX == 1024, "hpf_rank_topn's limit");

static void check_explain(uint32_t K, bool bias, uint64_t &rng)
{
  const uint32_t C = K + (bias ? 2u : 0u);
  const ExplainPlan p = explain_plan(K, bias);
  if (C > HPF_MAX_COLUMNS) { CHECK(!p.ok, "K=%u bias=%d: a plan beyond HPF_MAX_COLUMNS", K, (int)bias); return; }
  CHECK(p.ok, "K=%u bias=%d: no plan", K, (int)bias);
  CHECK(p.terms == C, "K=%u bias=%d terms=%u", K, (int)bias, p.terms);
  CHECK(p.R * 64 >= p.terms && (p.R - 1) * 64 < p.terms && has_explain((int)p.R), "K=%u bias=%d terms=%u R=%u", K, (int)bias, p.terms, p.R);
  const uint64_t per = ExplainPlan::pairs_per_block();
  CHECK(per == (uint64_t)EXPLAIN_WAVES * EXPLAIN_RUN, "pairs per workgroup %llu", (unsigned long long)per);
  for (int i = 0; i < 8; ++i) {
    rng = rng * 6364136223846793005ull + 1442695040888963407ull;
    const uint64_t cnt = i == 0 ? 1u : i == 1 ? (1ull << 40) : (rng >> 24) >> ((rng >> 8) % 39);
    const uint32_t g = p.grid(cnt);
    CHECK(g >= 1 && g <= EXPLAIN_BLOCKS_MAX, "K=%u cnt=%llu grid=%u", K, (unsigned long long)cnt, g);
    CHECK(cnt == 0 || g == EXPLAIN_BLOCKS_MAX || (uint64_t)g * per >= cnt, "K=%u cnt=%llu grid=%u: pairs without a wave", K, (unsigned long long)cnt, g);
    CHECK(cnt == 0 || (uint64_t)(g - 1) * per < cnt, "K=%u cnt=%llu grid=%u: an idle workgroup", K, (unsigned long long)cnt, g);
    CHECK(p.pairs_per_trip(cnt) == (uint64_t)g * per, "K=%u cnt=%llu trip=%llu", K, (unsigned long long)cnt, (unsigned long long)p.pairs_per_trip(cnt));
    // the columns of hpf_factor_top for a side of `rows` rows
    const uint32_t rows = i == 0 ? 0u : i == 1 ? 0xffffffffu : (uint32_t)(rng >> 32) >> ((rng >> 16) % 31);
    const long long knob = (i & 1) ? (long long)((rng >> 40) % 9) : 0;
    const uint32_t b = factor_top_batch(rows, K, knob);
    CHECK(b >= 1 && b <= K, "rows=%u K=%u batch=%u", rows, K, b);
    CHECK(b == 1 || (uint64_t)b * rows * 8 <= FACTOR_TOP_BYTES, "rows=%u K=%u batch=%u: above 512 MB", rows, K, b);
    CHECK(knob <= 0 || b <= (uint64_t)knob, "rows=%u K=%u knob=%lld batch=%u", rows, K, knob, b);
    CHECK(knob > 0 || b == K || (uint64_t)(b + 1) * rows * 8 > FACTOR_TOP_BYTES, "rows=%u K=%u batch=%u: room for one more", rows, K, b);
  }
}

int main()
{
  uint64_t rng = 20261020u;
  unsigned points = 0;
  for (uint32_t K = 1; K <= HPF_MAX_COLUMNS; ++K)
    for (int bias = 0; bias < 2; ++bias) { check_explain(K, bias != 0, rng); ++points; }
  CHECK(!explain_plan(0, false).ok, "K=0 has a plan");
  const uint32_t cases[] = {1, 3, 7, 14, 16, 17, 20, 50, 62, 63, 64, 65, 100, 126, 128, 129, 190, 192, 256, 300, 512, 760, 768, 1000, 1022, 1024};
  for (uint32_t K : cases)
    for (int bias = 0; bias < 2; ++bias) {
      const ExplainPlan p = explain_plan(K, bias != 0);
      if (!p.ok) { printf("ep %u %d none\n", K, bias); continue; }
      printf("ep %u %d %u %u %u %u %u %u %llu\n", K, bias, p.terms, p.R, p.grid(1), p.grid(5), p.grid(4099), p.grid(10000000),
             (unsigned long long)p.pairs_per_trip(10000000));
    }
  const struct { uint32_t rows, K; long long knob; } ft[] = {
    {1, 1, 0}, {5000, 100, 0}, {5000, 129, 7}, {257, 100, 32}, {100000, 100, 0}, {1000000, 100, 0}, {10000000, 100, 0},
    {10000000, 1024, 0}, {100000000, 100, 0}, {0, 20, 0}, {5000, 100, -3}};
  for (const auto &c : ft) printf("ft %u %u %lld %u\n", c.rows, c.K, c.knob, factor_top_batch(c.rows, c.K, c.knob));
  if (g_fail) { fprintf(stderr, "explain_selftest: %d checks failed\n", g_fail); return 1; }
  printf("explain_selftest ok: %u points\n", points);
  return 0;
}
