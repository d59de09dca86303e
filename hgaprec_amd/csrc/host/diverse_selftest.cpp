// diverse_selftest.cpp -- CPU check of hpf_plan::diverse_plan, the shape of hpf_recommend_diverse's mmr_kernel
// (tests/test_diverse_plan.py builds and runs it; nothing links it).  A sweep over pool = 1..HPF_DIVERSE_POOL_MAX, a list
// of K and a seeded list of user counts and compute-unit counts checks
//   Pp >= pool, Pp a multiple of 16, Pp < pool + 16, side = Pp / 16, tiles = side^2, steps * 4 >= K > (steps - 1) * 4
//   the strips dealt round-robin to the waves cover every tile exactly once, and tiles_per_wave is the largest share
//   slab_bytes = Pp^2 * 8 <= 512 KB; 1 <= workgroups <= users; workgroups * slab_bytes <= 256 MB;
//   workgroups <= CUs * DIVERSE_WGS_PER_CU; no cap is left unused (one more workgroup would break one of them)
//   lds_bytes holds the kernel's arrays and stays far below what a launch may ask for
//   no plan for pool = 0, pool > HPF_DIVERSE_POOL_MAX, K = 0 or nobody selected
// stdout: for a fixed list of cases a line
//   dp pool K Pp side tiles steps strips tiles_per_wave slab_bytes lds_bytes wg(1 user) wg(100 users) wg(100000 users)
// (256 compute units), which the test compares with tests/data/diverse_plan_table.txt, then
// `diverse_selftest ok: <points> points`.
#include <vector>

#include "../hpf_plan.hpp"
#include "../../../include/hpf.h"

using namespace hpf_plan;

static int g_fail = 0;
#define CHECK(cond, ...)                                                                     \
  do { if (!(cond)) { if (++g_fail <= 20) { fprintf(stderr, "FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } } } while (0)

static_assert(DIVERSE_POOL_MAX == HPF_DIVERSE_POOL_MAX && DIVERSE_POOL_MAX == DIVERSE_WAVES * 64, "a thread per pool entry");

static void check_diverse(uint32_t pool, uint32_t K, uint64_t &rng)
{
  for (int i = 0; i < 8; ++i) {
    rng = rng * 6364136223846793005ull + 1442695040888963407ull;
    const uint32_t n = i == 0 ? 1u : i == 1 ? 0xffffffffu : std::max(1u, (uint32_t)(rng >> 32) >> ((rng >> 16) % 31));
    const uint32_t cus = i < 2 ? 256u : 1u + (uint32_t)((rng >> 8) % 400);
    const DiversePlan p = diverse_plan(pool, n, K, cus);
    CHECK(p.ok, "pool=%u K=%u n=%u: no plan", pool, K, n);
    if (!p.ok) return;
    CHECK(p.Pp >= pool && p.Pp % 16 == 0 && p.Pp < pool + 16, "pool=%u Pp=%u", pool, p.Pp);
    CHECK(p.side == p.Pp / 16 && p.tiles == p.side * p.side, "pool=%u side=%u tiles=%u", pool, p.side, p.tiles);
    CHECK(p.steps * 4 >= K && (p.steps - 1) * 4 < K, "K=%u steps=%u", K, p.steps);
    // the kernel's walk: wave w takes strips w, w + DIVERSE_WAVES, ...
    CHECK(p.strips == diverse_strips(p.side) && p.strips == p.side * ((p.side + DIVERSE_STRIP - 1) / DIVERSE_STRIP), "pool=%u strips=%u", pool, p.strips);
    std::vector<uint32_t> seen(p.tiles, 0);
    uint32_t most = 0;
    for (uint32_t w = 0; w < DIVERSE_WAVES; ++w) {
      uint32_t mine = 0;
      for (uint32_t s = w; s < p.strips; s += DIVERSE_WAVES) {
        const uint32_t ti = diverse_strip(s, p.side).ti, tj0 = diverse_strip(s, p.side).tj0;   // the function mmr_kernel walks with
        for (uint32_t t = 0; t < DIVERSE_STRIP; ++t)
          if (tj0 + t < p.side) { ++seen[ti * p.side + tj0 + t]; ++mine; }
      }
      most = std::max(most, mine);
    }
    bool once = true;
    for (uint32_t v : seen) once = once && v == 1;
    CHECK(once, "pool=%u: a tile not computed exactly once", pool);
    CHECK(p.tiles_per_wave == most, "pool=%u tiles_per_wave=%u, the walk gives %u", pool, p.tiles_per_wave, most);
    CHECK(p.slab_bytes == (uint64_t)p.Pp * p.Pp * 8 && p.slab_bytes <= (512u << 10), "pool=%u slab=%llu", pool, (unsigned long long)p.slab_bytes);
    CHECK(p.workgroups >= 1 && p.workgroups <= n, "pool=%u n=%u workgroups=%u", pool, n, p.workgroups);
    CHECK((uint64_t)p.workgroups * p.slab_bytes <= DIVERSE_SLABS_BYTES, "pool=%u n=%u workgroups=%u: slabs beyond 256 MB", pool, n, p.workgroups);
    CHECK(p.workgroups <= (uint64_t)cus * DIVERSE_WGS_PER_CU, "pool=%u cus=%u workgroups=%u", pool, cus, p.workgroups);
    const uint64_t more = (uint64_t)p.workgroups + 1;
    CHECK(more > n || more * p.slab_bytes > DIVERSE_SLABS_BYTES || more > (uint64_t)cus * DIVERSE_WGS_PER_CU,
          "pool=%u n=%u cus=%u workgroups=%u: a cap left unused", pool, n, cus, p.workgroups);
    CHECK(p.lds_bytes >= DIVERSE_POOL_MAX * 4 + 4 + 8 + 2 * DIVERSE_WAVES * 12 && p.lds_bytes <= 4096, "lds=%u", p.lds_bytes);
  }
}

int main()
{
  uint64_t rng = 20261021u;
  unsigned points = 0;
  const uint32_t Ks[] = {1, 3, 4, 5, 100, 129, 1024};
  for (uint32_t pool = 1; pool <= HPF_DIVERSE_POOL_MAX; ++pool)
    for (uint32_t K : Ks) { check_diverse(pool, K, rng); ++points; }
  CHECK(!diverse_plan(0, 1, 100, 256).ok, "pool=0 has a plan");
  CHECK(!diverse_plan(HPF_DIVERSE_POOL_MAX + 1, 1, 100, 256).ok, "pool=257 has a plan");
  CHECK(!diverse_plan(16, 1, 0, 256).ok, "K=0 has a plan");
  CHECK(!diverse_plan(16, 0, 100, 256).ok, "nobody selected has a plan");
  CHECK(diverse_plan(16, 5, 100, 0).workgroups == 5, "no compute unit count: one is assumed");
  const uint32_t cases[] = {1, 15, 16, 17, 32, 33, 64, 65, 100, 127, 128, 129, 200, 255, 256};
  const uint32_t Kc[] = {1, 3, 100, 129};
  for (uint32_t pool : cases)
    for (uint32_t K : Kc) {
      const DiversePlan p = diverse_plan(pool, 1, K, 256);
      printf("dp %u %u %u %u %u %u %u %u %llu %u %u %u %u\n", pool, K, p.Pp, p.side, p.tiles, p.steps, p.strips, p.tiles_per_wave,
             (unsigned long long)p.slab_bytes, p.lds_bytes, p.workgroups, diverse_plan(pool, 100, K, 256).workgroups,
             diverse_plan(pool, 100000, K, 256).workgroups);
    }
  if (g_fail) { fprintf(stderr, "diverse_selftest: %d checks failed\n", g_fail); return 1; }
  printf("diverse_selftest ok: %u points\n", points);
  return 0;
}
