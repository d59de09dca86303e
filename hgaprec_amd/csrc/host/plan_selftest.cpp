// plan_selftest.cpp -- CPU check of hpf_plan.hpp (tests/test_plan.py builds it under ASan/UBSan and runs it).
// Every column count C = 1..HPF_MAX_COLUMNS x w_storage 0..3 x HPF_W_PACK off/on: the planned shapes are consistent, a kernel
// instance exists for each of them (the has_* predicates the dispatcher of hpf_capi.hip is generated from), and a p59 plan
// turned into plain doubles IS the w_storage = 3 plan.  Then the shapes the tests force through HPF_PHI_CFG / HPF_SWEEP_CFG.
// stdout: the mapping as runs of equal shapes, one line each --
//   w_storage pack C_first C_last w_layout phi_G phi_R phi_V sweep_G sweep_R ld       (the fields hpf_get_work_info exports)
// -- which tests/test_plan.py compares with tests/data/plan_table.txt, recorded from the library on a GPU.
// Then the tiled pass: the policy's pins from DESIGN.md section 5, the invariants of plan_tile_queues over a seeded sweep,
// and for a fixed list of cases a line
//   tq case-id chunks chunk_segs fnv64-of-the-list
// -- printed when the program is run as `plan_selftest_asan tile-queues` (then only the tiled pass is checked, and stdout
// holds nothing else) -- which tests/test_plan.py compares with tests/data/tile_queue_table.txt, recorded from the queue arithmetic as it stood
// inside hpf_capi.hip's build_tiled_side before it moved into the header.
// Then top-N for every user (hpf_recommend): the invariants of topn_cap, topn_grid and topn_batch_users over a seeded sweep and,
// run as `plan_selftest_asan topn-grid`, for a fixed list of cases a line
//   tg case-id m n_sel topn fused cap batch blocks splits tiles_per_split candidate-bytes
// which tests/test_plan_topn.py compares with tests/data/topn_grid_table.txt.
// Then the fused sweep epilogue (fused_checks) and, run as `plan_selftest_asan fused-sweep`, a line per pinned column count
//   fs C w_layout phi_G phi_R fused_user fused_item fused_user_under_knob_2
// which tests/test_fused_sweep_plan.py compares with its own list.
// Then the call order of an iteration's steps (phase_checks): every (phase, step) pair of next_phase.
#include "../hpf_plan.hpp"

#include <string>
#include <vector>

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

// ---- the tiled pass ------------------------------------------------------------------------------------------------------
struct Lcg { uint64_t s; uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); } };

// A tiled side's first-segment table: key 0 (the row-major rest) holds rest_segs segments, tile k base + [0, spread) of them,
// every absent_every-th tile none and every big_every-th one `big` more
struct TqShape { uint64_t seed; uint32_t tiles, rest_segs, base, spread, absent_every, big_every, big; };
static std::vector<uint32_t> make_fs(const TqShape &c, uint32_t *nseg)
{
  Lcg g = {c.seed};
  std::vector<uint32_t> fs(c.tiles + 1, TILE_NO_SEG);
  uint32_t at = 0;
  if (c.rest_segs) { fs[0] = 0; at = c.rest_segs; }
  for (uint32_t k = 1; k <= c.tiles; ++k) {
    uint32_t n = c.base + (c.spread ? g.next() % c.spread : 0);
    if (c.big_every && k % c.big_every == 1) n += c.big;
    if (c.absent_every && k % c.absent_every == 0) n = 0;
    if (n) { fs[k] = at; at += n; }
  }
  *nseg = at;
  return fs;
}

// what must hold of any queue plan: every segment in exactly one chunk, no chunk across two keys, each queue's chunks in
// front of its padding, and no more workgroups than a launch holds
static void check_queues(const TileQueuePlan &qp, const std::vector<uint32_t> &fs, uint32_t nseg, size_t max_wgs, const char *what, unsigned id)
{
  CHECK(qp.ok == (nseg != 0), "%s %u: ok=%d with %u segments", what, id, (int)qp.ok, nseg);
  if (!qp.ok) return;
  CHECK(qp.chunks.size() % 8 == 0 && qp.chunks.size() <= 8 * max_wgs, "%s %u: %zu chunks, %zu workgroups fit", what, id, qp.chunks.size(), max_wgs);
  std::vector<uint32_t> key_of(nseg, 0);
  for (uint32_t k = 0; k < (uint32_t)fs.size(); ++k)
    if (fs[k] != TILE_NO_SEG) for (uint32_t p = fs[k]; p < tile_key_end(fs, nseg, k); ++p) key_of[p] = k;
  std::vector<uint8_t> seen(nseg, 0);
  bool padded[8] = {false, false, false, false, false, false, false, false};
  for (size_t j = 0; j < qp.chunks.size(); ++j) {
    const TileChunk c = qp.chunks[j];
    if (c.x == c.y) { CHECK(c.x == 0, "%s %u: padding {%u,%u}", what, id, c.x, c.y); padded[j % 8] = true; continue; }
    CHECK(!padded[j % 8], "%s %u: a chunk behind the padding of queue %zu", what, id, j % 8);
    CHECK(c.x < c.y && c.y <= nseg, "%s %u: chunk {%u,%u} of %u segments", what, id, c.x, c.y, nseg);
    if (!(c.x < c.y && c.y <= nseg)) continue;
    CHECK(key_of[c.x] == key_of[c.y - 1], "%s %u: chunk {%u,%u} spans keys %u and %u", what, id, c.x, c.y, key_of[c.x], key_of[c.y - 1]);
    for (uint32_t p = c.x; p < c.y; ++p) { CHECK(!seen[p], "%s %u: segment %u twice", what, id, p); seen[p] = 1; }
  }
  for (uint32_t p = 0; p < nseg; ++p) CHECK(seen[p], "%s %u: segment %u in no chunk", what, id, p);
}

static uint64_t fnv64(const std::vector<TileChunk> &v)
{
  uint64_t hsh = 14695981039346656037ull;
  for (const TileChunk &c : v)
    for (uint32_t w : {c.x, c.y}) for (int b = 0; b < 4; ++b) { hsh ^= (w >> (8 * b)) & 0xffu; hsh *= 1099511628211ull; }
  return hsh;
}

static void tile_checks(bool print_cases)
{
  // ---- policy, default knobs
  const Knobs def;
  {
    const TilePolicy c2 = tile_policy(1000000, 768, 100000000, 100000, 8, true, def, 0);           // C2's item side gathers 10^6 users' rows
    CHECK(c2.tile && c2.tiles == 184 && c2.T == 5461 && c2.min_run == 12 && c2.light_below == 184u * 12u, "C2 items: %u tiles of %u rows, bar %llu", c2.tiles, c2.T, (unsigned long long)c2.light_below);
    const TilePolicy c4u = tile_policy(17770, 1536, 100480507, 480189, 4, false, def, 0), c4i = tile_policy(480189, 1536, 100480507, 17770, 4, true, def, 0);
    CHECK(c4u.tile && c4u.tiles == 7 && c4u.light_below == 7u * 12u * 4u, "C4 users: %u tiles, bar %llu", c4u.tiles, (unsigned long long)c4u.light_below);   // x 4 below 8 tiles
    CHECK(c4i.tile && c4i.tiles == 176 && c4i.light_below == 176u * 12u, "C4 items: %u tiles, bar %llu", c4i.tiles, (unsigned long long)c4i.light_below);
    const TilePolicy k50 = tile_policy(1000000, 256, 100000000, 100000, 16, true, def, 0);         // a batch of sixteen nonzeros: runs of 32
    CHECK(k50.tile && k50.min_run == 32 && k50.light_below == (uint64_t)k50.tiles * 32u, "16 per batch: run %u, bar %llu", k50.min_run, (unsigned long long)k50.light_below);
    for (uint32_t tiles = 2; tiles <= 9; ++tiles) {                                                // x 4 below 8 tiles, x 1 from 8 on
      Knobs kn; kn.tile_bytes = 4096; kn.tile_mode = 1;
      const TilePolicy forced = tile_policy(tiles * 4, 1024, 1000, 100, 8, false, kn, 0);
      CHECK(forced.tile && forced.tiles == tiles && forced.T == 4 && forced.light_below == 0, "forced, %u tiles", tiles);
      kn.tile_mode = 2;
      const TilePolicy autop = tile_policy(tiles * 4, 1024, 1000, 100, 8, false, kn, 0);
      CHECK(autop.tile == (tiles >= 3) && (!autop.tile || autop.light_below == (uint64_t)tiles * 12u * (tiles < 8 ? 4u : 1u)), "auto, %u tiles: bar %llu", tiles, (unsigned long long)autop.light_below);
    }
    Knobs kn;
    CHECK(!tile_policy(1000000, 768, 100000000, 100000, 8, true, def, 1).tile, "hpf_config.tiling = 1");
    CHECK(!tile_policy(1000000, 768, 0, 100000, 8, true, def, 0).tile && !tile_policy(1000000, 768, 5, 0, 8, true, def, 0).tile, "nothing to tile");
    CHECK(!tile_policy(5461, 768, 1000, 100, 8, true, def, 0).tile, "one tile");
    CHECK(!tile_policy(13652, 768, 1000, 100, 8, true, def, 0).tile && tile_policy(13654, 768, 1000, 100, 8, true, def, 0).tile, "auto: 2.5 tiles");
    kn.tile_bytes = 1024; CHECK(!tile_policy(65535, 1024, 1000, 100, 8, true, kn, 0).tile && tile_policy(65534, 1024, 1000, 100, 8, true, kn, 0).tiles == 65534, "at most 65 534 tiles");
    kn = Knobs(); kn.tile_sides = 1; CHECK(!tile_policy(1000000, 768, 1000, 100, 8, true, kn, 0).tile && tile_policy(1000000, 768, 1000, 100, 8, false, kn, 0).tile, "HPF_TILE_SIDES");
    kn = Knobs(); kn.tile_min_run = 2; CHECK(tile_policy(1000000, 768, 1000, 100, 16, true, kn, 0).min_run == 2, "HPF_TILE_RUN");
    // the memory rule: a job of C4's size (some 23 GB with the temporaries) fits a device of 288 GB and not one of 8 GB
    CHECK(tiling_fits(896, 480189, 17770, 100480507, true, (size_t)288 << 30) && !tiling_fits(896, 480189, 17770, 100480507, true, (size_t)8 << 30), "tiling_fits");
  }
  // ---- invariants of the queue plan over a seeded sweep
  Lcg g = {20240521};
  unsigned grown = 0;
  for (unsigned t = 0; t < 4000; ++t) {
    TqShape c;
    c.seed = g.next(); c.tiles = 2 + g.next() % 199;
    c.rest_segs = g.next() % 3 ? 1 + g.next() % 3000 : 0;
    c.base = g.next() % 4 ? 1 + g.next() % 40 : 0; c.spread = 1 + g.next() % 60;          // base 0: tiles without a segment of their own accord
    c.absent_every = g.next() % 3 ? 0 : 2 + g.next() % 9;
    c.big_every = g.next() % 4 ? 0 : 1 + g.next() % 50; c.big = 1000 + g.next() % 9000;
    uint32_t nseg = 0;
    const std::vector<uint32_t> fs = make_fs(c, &nseg);
    Knobs kn;
    kn.tile_order = (int)(g.next() % 3); kn.tile_split_below = g.next() % 64; kn.tile_chunk = g.next() % 10;
    const uint32_t wg = 64u << (g.next() % 3);
    // a launch that holds few workgroups makes the chunks grow; never fewer than a chunk per range of a queue (each of
    // the tiles and as many pieces of the rest), which is as far as growing goes
    const size_t max_wgs = g.next() % 2 ? ((size_t)1 << 28) / wg : 8 * (size_t)(2 * (c.tiles + 8) + 2) + g.next() % 512;
    const uint64_t rest_nnz = c.rest_segs ? (uint64_t)c.rest_segs * (1 + g.next() % 300) : 12345;
    const TileQueuePlan qp = plan_tile_queues(fs, nseg, c.tiles, rest_nnz, wg, max_wgs, kn);
    check_queues(qp, fs, nseg, max_wgs, "sweep case", t);
    const uint32_t ch0 = kn.tile_chunk ? kn.tile_chunk : 2 * (wg / 64);
    CHECK(qp.chunk_segs >= ch0 && qp.chunk_segs % ch0 == 0, "sweep case %u: chunks of %u segments from %u", t, qp.chunk_segs, ch0);
    grown += qp.chunk_segs > ch0;
  }
  CHECK(grown >= 100, "the sweep reached the growing chunks %u times", grown);
  // ---- the recorded cases: what the GPU tests force, one per tile_order, one where the chunks grow
  const size_t W = (size_t)1 << 28;
  const struct { const char *id; TqShape c; uint32_t wg, chunk; int order; uint32_t split_below; size_t max_wgs; uint32_t nnz_per_rest_seg; } cases[] = {
    {"default",       {1, 12, 40, 3, 9, 0, 0, 0},        64,  0, 1, 8, W / 64,  37},
    {"wg256_chunk8",  {1, 12, 40, 3, 9, 0, 0, 0},        256, 8, 1, 8, W / 256, 37},
    {"wg128_chunk3",  {1, 12, 40, 3, 9, 0, 0, 0},        128, 3, 1, 8, W / 128, 37},
    {"wg64_chunk1",   {1, 12, 40, 3, 9, 0, 0, 0},        64,  1, 1, 8, W / 64,  37},
    {"tiles5",        {2, 5, 700, 20, 30, 0, 0, 0},      64,  0, 1, 8, W / 64,  12},
    {"tiles7",        {3, 7, 2100, 150, 100, 0, 0, 0},   64,  0, 1, 8, W / 64,  60},
    {"tiles8",        {4, 8, 300, 10, 25, 0, 0, 0},      64,  0, 1, 8, W / 64,  45},
    {"tiles9",        {5, 9, 300, 10, 25, 0, 0, 0},      64,  0, 1, 8, W / 64,  45},
    {"tiles12",       {6, 12, 300, 10, 25, 5, 0, 0},     64,  0, 1, 8, W / 64,  45},
    {"tiles184",      {7, 184, 5000, 30, 90, 0, 23, 400}, 64, 0, 1, 8, W / 64,  500},
    {"tiles184_norest", {8, 184, 0, 30, 90, 7, 0, 0},    64,  0, 1, 8, W / 64,  0},
    {"order0",        {9, 22, 900, 15, 40, 0, 0, 0},     64,  0, 0, 8, W / 64,  30},
    {"order1",        {9, 22, 900, 15, 40, 0, 0, 0},     64,  0, 1, 8, W / 64,  30},
    {"order2",        {9, 22, 900, 15, 40, 0, 0, 0},     64,  0, 2, 8, W / 64,  30},
    {"split_below32", {9, 22, 900, 15, 40, 0, 0, 0},     256, 8, 0, 32, W / 256, 30},
    {"grow",          {10, 20, 4000, 50, 200, 0, 6, 5000}, 64, 0, 1, 8, 8 * 64, 20},
  };
  for (const auto &k : cases) {
    uint32_t nseg = 0;
    const std::vector<uint32_t> fs = make_fs(k.c, &nseg);
    Knobs kn; kn.tile_order = k.order; kn.tile_split_below = k.split_below; kn.tile_chunk = k.chunk;
    const uint64_t rest_nnz = k.c.rest_segs ? (uint64_t)k.c.rest_segs * k.nnz_per_rest_seg : 987654;
    const TileQueuePlan qp = plan_tile_queues(fs, nseg, k.c.tiles, rest_nnz, k.wg, k.max_wgs, kn);
    check_queues(qp, fs, nseg, k.max_wgs, k.id, 0);
    if (print_cases) printf("tq %s %zu %u %016llx\n", k.id, qp.chunks.size(), qp.chunk_segs, (unsigned long long)fnv64(qp.chunks));
  }
}

// ---- top-N for every user (hpf_recommend) ----------------------------------------------------------------------------------
static void topn_checks(bool print_cases)
{
  CHECK(TOPN_MAX == 1024 && TOPN_FUSED_MAX == 256 && !topn_fused(0) && topn_fused(1) && topn_fused(256) && !topn_fused(257), "the fused range");
  for (uint32_t topn = 1; topn <= TOPN_MAX; ++topn) {
    const uint32_t np = topn_np(topn), cap = topn_cap(topn);
    CHECK(np >= 64 && np >= topn && (np & (np - 1)) == 0 && (np == 64 || np / 2 < topn) && cap == 2 * np, "topn=%u: np=%u cap=%u", topn, np, cap);
    CHECK(cap >= topn + 64, "topn=%u: a compacted buffer of %u has no room for a tile", topn, cap);
    CHECK(!topn_fused(topn) || cap * TOPN_ENTRY_BYTES <= 6144, "topn=%u: %u entries do not fit a wave's 6 KB of LDS", topn, cap);
  }
  // C2 at topn = 100: 21 440 users x 4 splits x 256 entries x 12 B = 263 MB
  {
    const uint32_t cap = topn_cap(100), batch = topn_batch_users(100000, 1000000, cap, 0);
    const RankGrid g = topn_grid(batch, 1563, cap);
    CHECK(cap == 256 && batch == 21440 && g.blocks == 335 && g.splits == 4 && g.tiles_per_split == 391, "C2: cap %u, %u users, %u x %u of %u tiles", cap, batch, g.blocks, g.splits, g.tiles_per_split);
    CHECK(topn_batch_bytes(batch, 1563, cap) == 21440ull * 4 * 256 * 12 && topn_batch_bytes(batch, 1563, cap) / 1000000 == 263, "C2: %llu bytes", (unsigned long long)topn_batch_bytes(batch, 1563, cap));
  }
  // test_gpu_recommend's compaction case: 150 users x 391 tiles are 3 blocks with splits of 8, 16 and 32 tiles
  for (uint32_t topn : {1u, 100u, 256u}) {
    const RankGrid g = topn_grid(150, 391, topn_cap(topn));
    CHECK(g.blocks == 3 && g.tiles_per_split == topn_cap(topn) / 16 && g.tiles_per_split > topn_cap(topn) / 64, "topn=%u: %u blocks, %u tiles per split", topn, g.blocks, g.tiles_per_split);
  }
  Lcg r = {20260107};
  unsigned reduced = 0, ruled = 0;
  for (unsigned t = 0; t < 6000; ++t) {
    const uint32_t topn = 1 + r.next() % TOPN_FUSED_MAX, cap = topn_cap(topn);
    const uint32_t m = t % 5 == 0 ? 1 + r.next() % 300 : t % 5 == 1 ? 1 + r.next() % 4000000 : 1 + r.next() % 200000;
    const uint32_t n_sel = t % 3 == 0 ? 1 + r.next() % 200 : 1 + r.next() % 3000000;
    const long long knob = t % 4 == 0 ? 1 + (long long)(r.next() % 5000) : 0;
    const uint32_t ntiles = (m + 63) / 64;
    const uint32_t batch = topn_batch_users(m, n_sel, cap, knob), base = rank_batch_users(m, n_sel, knob);
    CHECK(batch >= 16 && batch <= base && batch % 16 == 0, "case %u: batch %u of %u", t, batch, base);
    CHECK(batch == base || batch % 64 == 0, "case %u: a reduced batch of %u users", t, batch);
    if (!knob) CHECK(batch % 64 == 0 || batch == ((n_sel + 15) & ~15u), "case %u: batch %u, n_sel %u", t, batch, n_sel);
    CHECK(topn_batch_bytes(batch, ntiles, cap) <= TOPN_BATCH_BYTES, "case %u: %llu bytes of candidates", t, (unsigned long long)topn_batch_bytes(batch, ntiles, cap));
    reduced += batch < base;
    for (uint32_t rows : {batch, 1u + r.next() % batch}) {
      const RankGrid g = topn_grid(rows, ntiles, cap), g0 = rank_grid(rows, ntiles);
      CHECK(g.blocks == (rows + 63) / 64 && g.splits >= 1 && g.splits <= g0.splits && g.tiles_per_split >= g0.tiles_per_split, "case %u: grid %u x %u", t, rows, ntiles);
      CHECK((uint64_t)g.splits * g.tiles_per_split >= ntiles, "case %u: tiles left out", t);
      CHECK((uint64_t)(g.splits - 1) * g.tiles_per_split < ntiles, "case %u: an empty split", t);
      CHECK(g.tiles_per_split >= cap / 16 || g.splits == 1, "case %u: %u splits of %u tiles, cap %u", t, g.splits, g.tiles_per_split, cap);
      ruled += g.splits < g0.splits;
    }
  }
  CHECK(reduced >= 50 && ruled >= 500, "the sweep reduced %u batches and regrouped %u grids", reduced, ruled);
  const struct { const char *id; uint32_t m, n_sel, topn; long long knob; } cases[] = {
    {"c2_top10", 100000, 1000000, 10, 0},     {"c2_top100", 100000, 1000000, 100, 0},   {"c2_top256", 100000, 1000000, 256, 0},
    {"c2_16k_top100", 100000, 16384, 100, 0}, {"c2_top257", 100000, 1000000, 257, 0},   {"c2_top1024", 100000, 1000000, 1024, 0},
    {"edges_top1", 25000, 150, 1, 0},         {"edges_top100", 25000, 150, 100, 0},     {"edges_top256", 25000, 150, 256, 0},
    {"m200_top100", 200, 37, 100, 0},         {"m64_top256", 64, 37, 256, 0},           {"m1000_knob16", 1000, 37, 64, 16},
    {"one_user", 100000, 1, 100, 0},          {"m4e6_top256", 4000000, 3000000, 256, 0}, {"m1e4_many", 10000, 3000000, 256, 0},
    {"m64_many", 64, 3000000, 256, 0},
  };
  for (const auto &k : cases) {
    const uint32_t cap = topn_cap(k.topn), ntiles = (k.m + 63) / 64, batch = topn_batch_users(k.m, k.n_sel, cap, k.knob);
    const RankGrid g = topn_grid(batch, ntiles, cap);
    if (print_cases)
      printf("tg %s %u %u %u %d %u %u %u %u %u %llu\n", k.id, k.m, k.n_sel, k.topn, (int)topn_fused(k.topn), cap, batch, g.blocks, g.splits, g.tiles_per_split,
             (unsigned long long)topn_batch_bytes(batch, ntiles, cap));
  }
}

// The fused sweep epilogue (fused_sweep, has_phi_fused, has_sums): which (side, layout, shape) runs it.  Over every column count:
// only the user side of p59 rows, only with the knob on, only a shape of the list whose build keeps three waves per SIMD
// without scratch -- by default only the one measured to pay -- always with a sums kernel for the sweep's shape, never after
// the fall-back to plain doubles.  With
// print_cases a line per pinned column count:   fs C w_layout phi_G phi_R fused_user fused_item fused_user_under_knob_2
static void fused_checks(bool print_cases)
{
  Knobs on, off, all; off.fused_sweep = 0; all.fused_sweep = 2;
  CHECK(on.fused_sweep == 1, "the knob's default");
  for (uint32_t ws = 0; ws <= 3; ++ws)
    for (uint32_t C = 1; C <= HPF_MAX_COLUMNS; ++C) {
      Plan p;
      if (plan_shapes(C, ws, on, &p) != HPF_OK) continue;
      const bool fu = fused_sweep(p, on, false);
      CHECK(!fused_sweep(p, on, true), "ws=%u C=%u: the item side fused", ws, C);
      CHECK(!fused_sweep(p, off, false) && !fused_sweep(p, off, true), "ws=%u C=%u: fused with the knob off", ws, C);
      CHECK(!fu || (ws == 0 && p.wl == WL_P59), "ws=%u C=%u wl=%d: fused rows that are not p59", ws, C, p.wl);
      const bool fa = fused_sweep(p, all, false);                         // HPF_FUSED_SWEEP=2: wherever an instance exists
      CHECK(!fused_sweep(p, all, true), "ws=%u C=%u: the item side fused under the knob 2", ws, C);
      CHECK(fa == (p.wl == WL_P59 && has_phi_fused(p.wl, p.phiG, p.phiR) && has_sums(p.sw_mode, p.swG, p.swR)), "ws=%u C=%u", ws, C);
      CHECK(fu == (fa && fused_pays(p.phiG, p.phiR)) && (!fu || (C >= 81 && C <= 104)), "ws=%u C=%u: the default fuses what was measured to pay", ws, C);
      if (fa) {
        CHECK(has_phi_packed(p.wl, p.phiG, p.phiR) && has_sweep(p.sw_mode, p.swG, p.swR), "ws=%u C=%u: no unfused instance beside the fused one", ws, C);
        CHECK(p.pk.row_bytes <= 1536u, "ws=%u C=%u: a staged row of %u bytes", ws, C, p.pk.row_bytes);
        CHECK(!fused_sweep(p.as_plain_doubles(), all, false), "ws=%u C=%u: fused after the fall-back", ws, C);
      }
    }
  // the instance list itself: G <= 8 up to six pieces, then 16 x 3, 32 x 2, 64 x 1; nothing for another layout
  for (int g : {2, 4, 8, 16, 32, 64, 128})
    for (int l = 0; l <= 10; ++l) {
      const bool want = (g == 4 || g == 8) ? (l >= 1 && l <= 6) : g == 16 ? (l >= 1 && l <= 3) : g == 32 ? (l >= 1 && l <= 2) : g == 64 ? l == 1 : false;
      CHECK(has_phi_fused(WL_P59, g, l) == want, "has_phi_fused(p59, %d, %d)", g, l);
      CHECK(!has_phi_fused(WL_F64, g, l) && !has_phi_fused(WL_F48, g, l) && !has_phi_fused(WL_PLAIN, g, l), "has_phi_fused(other, %d, %d)", g, l);
    }
  for (int m : {SW_PLAIN, SW_LDS_F48, SW_F64}) for (int g : {4, 8, 16, 32, 64}) for (int r = 1; r <= 16; ++r) CHECK(!has_sums(m, g, r), "has_sums(%d, %d, %d)", m, g, r);
  // the shapes of the benchmark's configurations and of the tests: K = 20, 50, 100, 200, plain and with the two bias columns
  const uint32_t pins[] = {20, 22, 50, 52, 100, 102, 200, 202, 800};
  for (uint32_t C : pins) {
    Plan p;
    CHECK(plan_shapes(C, 0, on, &p) == HPF_OK, "C=%u", C);
    if (print_cases) printf("fs %u %d %d %d %d %d %d\n", C, p.wl, p.phiG, p.phiR, (int)fused_sweep(p, on, false), (int)fused_sweep(p, on, true), (int)fused_sweep(p, all, false));
  }
  { Plan p; CHECK(plan_shapes(100, 0, on, &p) == HPF_OK && p.phiG == 8 && p.phiR == 6 && fused_sweep(p, on, false), "K = 100: (8, 6), fused"); }
  { Plan p; CHECK(plan_shapes(200, 0, on, &p) == HPF_OK && p.phiG == 16 && p.phiR == 6 && !fused_sweep(p, all, false), "K = 200: (16, 6) spills, unfused"); }
  { Plan p; CHECK(plan_shapes(50, 0, on, &p) == HPF_OK && p.phiG == 4 && p.phiR == 6 && !fused_sweep(p, on, false) && fused_sweep(p, all, false), "K = 50: (4, 6) loses, unfused by default"); }
}

// The call order of an iteration's steps (next_phase): every (phase, step) pair against the rule the header states -- the
// items pass from anywhere, every other step after its predecessor only -- and the three cuts of an iteration the exported
// calls compose, each from idle back to idle.
static void phase_checks()
{
  for (int phase = -2; phase <= 6; ++phase)
    for (int s = -1; s <= 4; ++s) {
      const bool in_range = phase >= 0 && phase <= 3 && s >= 0 && s <= 3;
      const int want = !in_range ? -1 : s == ITEMS_PASS ? 1 : s == phase ? (phase + 1) % 4 : -1;
      CHECK(next_phase(phase, (Step)s) == want, "next_phase(%d, %d) = %d, not %d", phase, s, next_phase(phase, (Step)s), want);
    }
  // the exported calls as the steps they compose, and a sequence of calls walked from a phase (-1 once a call is refused)
  using Call = std::vector<Step>;
  const Call items = {ITEMS_PASS}, phi = {ITEMS_PASS, USERS_PASS}, sweep = {USERS_SWEEP}, users = {USERS_PASS, USERS_SWEEP},
             local = {ITEMS_PASS, USERS_PASS, USERS_SWEEP}, global = {ITEMS_SWEEP};
  const auto walk = [](int phase, std::initializer_list<Call> calls) {
    for (const Call &call : calls) for (Step s : call) if (phase >= 0) phase = next_phase(phase, s);
    return phase;
  };
  CHECK(walk(0, {items, users, global}) == 0 && walk(0, {phi, sweep, global}) == 0 && walk(0, {local, global}) == 0, "the three cuts of an iteration");
  CHECK(walk(0, {items}) == 1 && walk(0, {phi}) == 2 && walk(0, {items, users}) == 3 && walk(0, {local}) == 3, "the phases on the way");
  // what tests/test_gpu_parity.py::test_iteration_pieces_and_their_call_order expects to be refused
  CHECK(walk(0, {global}) == -1 && walk(0, {users}) == -1 && walk(0, {sweep}) == -1, "an iteration begins with its items pass");
  CHECK(walk(0, {items, sweep}) == -1 && walk(0, {items, users, users}) == -1 && walk(0, {items, global}) == -1 &&
        walk(0, {phi, global}) == -1 && walk(0, {phi, users}) == -1 && walk(0, {local, sweep}) == -1, "a step out of turn");
  for (int phase = 0; phase <= 3; ++phase) CHECK(walk(phase, {local, global}) == 0, "an iteration begun again in phase %d", phase);
}

int main(int argc, char **argv)
{
  if (argc > 1 && !strcmp(argv[1], "fused-sweep")) {
    fused_checks(true);
    if (g_fail) { fprintf(stderr, "plan_selftest: %d checks failed\n", g_fail); return 1; }
    return 0;
  }
  if (argc > 1 && !strcmp(argv[1], "topn-grid")) {
    topn_checks(true);
    if (g_fail) { fprintf(stderr, "plan_selftest: %d checks failed\n", g_fail); return 1; }
    return 0;
  }
  if (argc > 1 && !strcmp(argv[1], "tile-queues")) {
    tile_checks(true);
    if (g_fail) { fprintf(stderr, "plan_selftest: %d checks failed\n", g_fail); return 1; }
    return 0;
  }
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
  tile_checks(false);
  topn_checks(false);
  fused_checks(false);
  phase_checks();
  if (g_fail) { fprintf(stderr, "plan_selftest: %d checks failed\n", g_fail); return 1; }
  printf("# plan_selftest ok: %u points, %u runs\n", points, runs);
  return 0;
}
