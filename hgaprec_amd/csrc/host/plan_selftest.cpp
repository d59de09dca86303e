// plan_selftest.cpp -- CPU check of hpf_plan.hpp (tests/test_plan.py builds it under ASan/UBSan and runs it).
// Every column count C = 1..HPF_MAX_COLUMNS x w_storage 0..3 x HPF_W_PACK off/on: the planned shapes are consistent, a kernel
// instance exists for each of them (the has_* predicates the dispatcher of hpf_capi.hip is generated from), and a p59 plan
// turned into plain doubles IS the w_storage = 3 plan.  Then the shapes the tests force through HPF_PHI_CFG / HPF_SWEEP_CFG.
// stdout: the mapping as runs of equal shapes, one line each --
//   w_storage pack C_first C_last w_layout phi_G phi_R phi_V sweep_G sweep_R ld       (the fields hpf_get_work_info exports)
// -- which tests/test_plan.py compares with tests/data/plan_table.txt, recorded from the library on a GPU.
#include "../hpf_plan.hpp"

#include <string>

using namespace hpf_plan;

static int g_fail = 0;
#define CHECK(cond, ...)                                                                     \
  do { if (!(cond)) { if (++g_fail <= 20) { fprintf(stderr, "FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } } } while (0)

static bool same_row(const Row &a, const Row &b) { return a.G == b.G && a.E == b.E && a.L == b.L && a.row_bytes == b.row_bytes && a.lgG == b.lgG; }
static bool same_plan(const Plan &a, const Plan &b)
{
  return a.ld == b.ld && a.w32 == b.w32 && a.wl == b.wl && same_row(a.pk, b.pk) && same_row(a.pks, b.pks) && a.phiG == b.phiG &&
         a.phiR == b.phiR && a.phiV == b.phiV && a.swG == b.swG && a.swR == b.swR && a.sw_mode == b.sw_mode;
}

// what must hold of any plan for C live columns
static void check_plan(const Plan &p, uint32_t C, const char *what)
{
  CHECK(p.ld >= C, "%s C=%u ld=%u", what, C, p.ld);
  if (p.wl != WL_PLAIN) {
    CHECK(p.wl == WL_P59 || p.wl == WL_F48 || p.wl == WL_F64, "%s C=%u wl=%d", what, C, p.wl);
    CHECK(!p.w32 && p.phiV == 0 && p.phiG == (int)p.pk.G && p.phiR == (int)p.pk.L, "%s C=%u", what, C);
    // G*E == ld; plain doubles sit two to a piece, so an odd count per lane is rounded up by one (those slots hold zeros)
    CHECK(p.ld % p.pk.G == 0 && p.pk.E == (p.wl == WL_F64 ? (p.ld / p.pk.G + 1) / 2 * 2 : p.ld / p.pk.G), "%s C=%u G=%u E=%u ld=%u", what, C, p.pk.G, p.pk.E, p.ld);
    CHECK(p.pk.row_bytes == 16u * p.pk.G * p.pk.L && (1u << p.pk.lgG) == p.pk.G, "%s C=%u", what, C);
    CHECK(has_phi_packed(p.wl, p.phiG, p.phiR), "%s C=%u wl=%d G=%d L=%d", what, C, p.wl, p.phiG, p.phiR);
    CHECK((uint32_t)(p.swG * p.swR) >= p.ld, "%s C=%u sweep %dx%d", what, C, p.swG, p.swR);
    CHECK(p.sw_mode == (p.wl == WL_F48 ? SW_LDS_F48 : p.wl == WL_F64 ? SW_F64 : p.phiG <= 32 ? SW_REG_P59 : SW_LDS_P59), "%s C=%u mode %d", what, C, p.sw_mode);
    if (p.wl == WL_P59) {                    // the plain-doubles row it can fall back to holds the same columns in the same lanes
      CHECK(p.pks.G == p.pk.G && p.pks.lgG == p.pk.lgG && p.pks.E >= p.pk.E && p.pks.E == 2 * p.pks.L && p.pks.row_bytes == 16u * p.pks.G * p.pks.L, "%s C=%u", what, C);
    }
  } else {
    CHECK((uint32_t)(p.phiG * p.phiR * p.phiV) == p.ld, "%s C=%u phi %d,%d,%d ld=%u", what, C, p.phiG, p.phiR, p.phiV, p.ld);
    CHECK((uint32_t)(p.swG * p.swR) == p.ld, "%s C=%u sweep %dx%d ld=%u", what, C, p.swG, p.swR, p.ld);
    CHECK(has_phi(p.w32, p.phiG, p.phiR, p.phiV), "%s C=%u phi %d,%d,%d", what, C, p.phiG, p.phiR, p.phiV);
    CHECK(p.sw_mode == SW_PLAIN, "%s C=%u mode %d", what, C, p.sw_mode);
  }
  CHECK(has_sweep(p.sw_mode, p.swG, p.swR), "%s C=%u sweep mode %d %dx%d", what, C, p.sw_mode, p.swG, p.swR);
  if (!p.w32 && (p.wl != WL_PLAIN || p.phiV == 2))          // the layouts hpf_gather_only accepts
    CHECK(has_gather_only(p.phiG, p.phiR), "%s C=%u gather-only %d,%d", what, C, p.phiG, p.phiR);
}

static std::string shape_of(int rc, const Plan &p)
{
  if (rc) return "unsupported";
  char b[96];
  snprintf(b, sizeof b, "%d %d %d %d %d %d %u", p.wl, p.phiG, p.phiR, p.phiV, p.swG, p.swR, p.ld);
  return b;
}

int main()
{
  unsigned points = 0, runs = 0;
  for (uint32_t ws = 0; ws <= 3; ++ws)
    for (int pack = 0; pack <= 1; ++pack) {
      Knobs kn; kn.w_pack = pack != 0;
      std::string run; uint32_t first = 0;
      for (uint32_t C = 1; C <= HPF_MAX_COLUMNS + 1; ++C) {
        Plan p;
        const int rc = C <= HPF_MAX_COLUMNS ? plan_shapes(C, ws, kn, &p) : HPF_ERR_INVALID /* ends the last run */;
        if (C <= HPF_MAX_COLUMNS) {
          ++points;
          CHECK(rc == HPF_OK || rc == HPF_ERR_UNSUPPORTED, "ws=%u pack=%d C=%u rc=%d", ws, pack, C, rc);
          if (rc == HPF_OK) {
            check_plan(p, C, "plan");
            CHECK(p.w32 == (ws == 1), "ws=%u C=%u", ws, C);
            if (p.wl == WL_P59) {
              const Plan d = p.as_plain_doubles();
              check_plan(d, C, "as_plain_doubles");
              CHECK(ws == 0, "ws=%u C=%u: p59 rows", ws, C);
              Plan q;
              CHECK(plan_shapes(C, 3, kn, &q) == HPF_OK && same_plan(d, q), "C=%u pack=%d: fall-back differs from w_storage 3", C, pack);
            }
          }
        }
        const std::string s = C <= HPF_MAX_COLUMNS ? shape_of(rc, p) : std::string();
        if (s != run) {
          if (!run.empty()) { printf("%u %d %u %u %s\n", ws, pack, first, C - 1, run.c_str()); ++runs; }
          run = s; first = C;
        }
      }
    }
  // out of range: no plan
  { Plan p; Knobs kn; CHECK(plan_shapes(0, 0, kn, &p) == HPF_ERR_UNSUPPORTED && plan_shapes(HPF_MAX_COLUMNS + 1, 0, kn, &p) == HPF_ERR_UNSUPPORTED &&
                            plan_shapes(8, 4, kn, &p) == HPF_ERR_UNSUPPORTED, "out of range"); }
  // HPF_PHI_CFG as tests/test_gpu_parity.py builds it ("8,R,2" up to 128 columns, "16,R,2" above): that plain shape, no packing
  for (uint32_t C = 1; C <= 256; ++C) {
    Knobs kn;
    kn.phi_cfg[0] = C <= 128 ? 8 : 16; kn.phi_cfg[1] = (int)((C + (C <= 128 ? 15 : 31)) / (C <= 128 ? 16 : 32)); kn.phi_cfg[2] = 2;
    Plan p;
    CHECK(plan_shapes(C, 0, kn, &p) == HPF_OK, "phi_cfg C=%u", C);
    check_plan(p, C, "phi_cfg");
    CHECK(p.wl == WL_PLAIN && p.phiG == kn.phi_cfg[0] && p.phiR == kn.phi_cfg[1] && p.phiV == 2, "phi_cfg C=%u: %d,%d,%d wl=%d", C, p.phiG, p.phiR, p.phiV, p.wl);
    kn.w_pack = true;                        // ... even with the packing forced (w_storage 2 still packs)
    CHECK(plan_shapes(C, 0, kn, &p) == HPF_OK && p.wl == WL_PLAIN, "phi_cfg + w_pack C=%u", C);
    CHECK(plan_shapes(C, 2, kn, &p) == HPF_OK && p.wl == WL_F48, "phi_cfg, f48 C=%u", C);
    check_plan(p, C, "phi_cfg f48");
  }
  {                                          // "16,1,2" (tests/test_gpu_handover.py); a shape too small for C or none at all is ignored
    Knobs kn, none; Plan p, q;
    kn.phi_cfg[0] = 16; kn.phi_cfg[1] = 1; kn.phi_cfg[2] = 2;
    CHECK(plan_shapes(20, 0, kn, &p) == HPF_OK && p.wl == WL_PLAIN && p.ld == 32 && p.phiG == 16 && p.phiR == 1 && p.phiV == 2, "16,1,2");
    for (int bad = 0; bad < 4; ++bad) {
      Knobs kb;
      const int cfgs[4][3] = {{16, 1, 2} /* 32 < 40 */, {12, 2, 2}, {16, 9, 2}, {16, 2, 4} /* doubles: V = 1 | 2 */};
      std::copy(cfgs[bad], cfgs[bad] + 3, kb.phi_cfg);
      CHECK(plan_shapes(40, 0, kb, &p) == HPF_OK && plan_shapes(40, 0, none, &q) == HPF_OK && same_plan(p, q), "phi_cfg %d ignored", bad);
    }
  }
  // HPF_SWEEP_CFG: any (G,R) with G*R == ld that has a plain sweep is taken on plain rows, and only there
  for (uint32_t C = 1; C <= HPF_MAX_COLUMNS; ++C)
    for (uint32_t ws : {1u, 3u, 0u}) {
      Knobs none; Plan base;
      if (plan_shapes(C, ws, none, &base) != HPF_OK) continue;
      for (int g : {4, 8, 16, 32, 64, 12})
        for (int r = 0; r <= 17; ++r) {
          Knobs kn; kn.sweep_cfg[0] = g; kn.sweep_cfg[1] = r;
          Plan p;
          CHECK(plan_shapes(C, ws, kn, &p) == HPF_OK, "sweep_cfg C=%u", C);
          check_plan(p, C, "sweep_cfg");
          const bool taken = base.wl == WL_PLAIN && has_sweep(SW_PLAIN, g, r) && (uint32_t)(g * r) == base.ld;
          Plan want = base; if (taken) { want.swG = g; want.swR = r; }
          CHECK(same_plan(p, want), "sweep_cfg C=%u ws=%u %d,%d", C, ws, g, r);
        }
    }
  // ---- the fused rank kernels (hpf_loo_ranks, hpf_rank_queries): users per batch, launch grid, chunks in registers
  CHECK(rank_batch_users(100000, 1000000, 0) == 21440, "batch at m = 10^5: %u", rank_batch_users(100000, 1000000, 0));
  {                                          // HPF_LOO_BATCH=16 as the batch-boundary tests set it: 37 users go as 16, 16, 5
    const uint32_t b = rank_batch_users(70, 37, 16);
    CHECK(b == 16 && 37 - 2 * b == 5, "batch of 37 users under the knob 16: %u", b);
    CHECK(rank_batch_users(70, 37, 17) == 32 && rank_batch_users(70, 37, 1) == 16, "the knob is rounded up to 16 users");
  }
  for (long long knob : {0ll, -1ll, -16ll, (long long)INT64_MIN})
    CHECK(rank_batch_users(100000, 1000000, knob) == 21440 && rank_batch_users(70, 37, knob) == 48, "knob %lld is ignored", knob);
  CHECK(rank_batch_users(1, UINT32_MAX, 0) >= 64 && rank_batch_users(1, UINT32_MAX, 0) % 64 == 0, "m = 1: %u", rank_batch_users(1, UINT32_MAX, 0));
  CHECK(rank_batch_users(UINT32_MAX, UINT32_MAX, 0) == 64, "the widest bit rows: a workgroup's 64 users, %u", rank_batch_users(UINT32_MAX, UINT32_MAX, 0));
  CHECK(rank_batch_users(1, 5, 0) == 16 && rank_batch_users(1, 16, 0) == 16 && rank_batch_users(1, 17, 0) == 32, "n_sel rounded up to 16");
  {
    const struct { uint32_t rows, ntiles, blocks, tps, splits; } pins[] = {
      {150, 391, 3, 2, 196},                 // test_a_workgroup_sweeps_several_tiles
      {70000, 2, 1094, 2, 1},                // test_more_than_1024_blocks_of_rows_and_one_split
      {1, 1, 1, 1, 1}};
    for (const auto &p : pins) {
      const RankGrid g = rank_grid(p.rows, p.ntiles);
      CHECK(g.blocks == p.blocks && g.tiles_per_split == p.tps && g.splits == p.splits, "grid of %u rows x %u tiles: %u blocks, %u tiles per split, %u splits",
            p.rows, p.ntiles, g.blocks, g.tiles_per_split, g.splits);
    }
    for (uint32_t rows = 1; rows <= 4200; rows += (rows < 200 ? 1 : 97))
      for (uint32_t ntiles = 1; ntiles <= 3000; ntiles += (ntiles < 70 ? 1 : 53)) {
        const RankGrid g = rank_grid(rows, ntiles);
        CHECK(g.blocks == (rows + 63) / 64 && g.splits >= 1 && g.tiles_per_split >= 1, "grid %u x %u", rows, ntiles);
        CHECK((uint64_t)g.splits * g.tiles_per_split >= ntiles, "grid %u x %u: tiles left out", rows, ntiles);            // every tile swept
        CHECK((uint64_t)(g.splits - 1) * g.tiles_per_split < ntiles, "grid %u x %u: an empty split", rows, ntiles);       // no workgroup without one
      }
  }
  {
    const uint32_t Ks[] = {1, 32, 33, 64, 65, 128, 129, HPF_MAX_COLUMNS};
    const int want[] = {1, 1, 2, 2, 4, 4, 0, 0};
    for (int i = 0; i < 8; ++i) CHECK(rank_chunks(Ks[i]) == want[i], "K=%u: %d chunks", Ks[i], rank_chunks(Ks[i]));
    bool returned[8] = {false, false, false, false, false, false, false, false};
    for (uint32_t K = 1; K <= HPF_MAX_COLUMNS; ++K) {
      const int nch = rank_chunks(K);
      CHECK(nch >= 0 && nch < 8 && has_rank_chunks(nch), "K=%u: no instance for %d chunks", K, nch);
      CHECK(nch == 0 || 32u * (uint32_t)nch >= K, "K=%u does not fit %d chunks of 32 columns", K, nch);
      if (nch >= 0 && nch < 8) returned[nch] = true;
    }
    for (int nch = -1; nch <= 8; ++nch) CHECK(has_rank_chunks(nch) == (nch >= 0 && nch < 8 && returned[nch]), "has_rank_chunks(%d)", nch);
  }
  if (g_fail) { fprintf(stderr, "plan_selftest: %d checks failed\n", g_fail); return 1; }
  printf("# plan_selftest ok: %u points, %u runs\n", points, runs);
  return 0;
}
