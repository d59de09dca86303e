// hpf_plan.hpp -- what the GPU will run, decided on the host: the experimental knobs, the shapes of the phi pass, of the rows
// of W and of the row sweep for a column count (plan_shapes), which kernel instances exist for them (has_*), and the batches
// and launch grid of the fused rank kernels (rank_batch_users, rank_grid, rank_chunks), the score batch of the unfused ones
// (score_batch_rows), the fused range, candidate buffers, grid and batches of hpf_recommend (topn_fused, topn_cap, topn_grid,
// topn_batch_users), and the tiled pass: whether a side is tiled and with which tiles (tile_policy, tiling_fits) and which
// XCD queue and chunk every segment runs in (plan_tile_queues); and the call order of an iteration's steps (next_phase).
// Plain C++17 without a HIP header: hpf_capi.hip builds its handle and its dispatcher from it, host/plan_selftest.cpp
// walks every column count on a CPU, pins the tile policy, checks the invariants of the queue plan over a seeded sweep and
// prints the plan of a fixed list of cases (tests/data/tile_queue_table.txt, recorded before the arithmetic moved here).
#pragma once
#include "../../include/hpf.h"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

namespace hpf_plan {

// The codes of hpf_kernels.hpp in plain int (hpf_capi.hip pins each with a static_assert): layout of the rows of W
// (hpf_work_info.w_layout) and how the sweep writes them (row_sweep_kernel MODE)
enum { WL_PLAIN = 0, WL_F48 = 2, WL_P59 = 3, WL_F64 = 4 };
enum { SW_PLAIN = 0, SW_LDS_F48 = 2, SW_LDS_P59 = 3, SW_F64 = 4, SW_REG_P59 = 5 };

// Tuning knobs, read from the environment ONLY under HPF_EXPERIMENTAL=1 (tests, tools/): a stray variable must not change
// the layout or the summation order of a production run.  The values here are the defaults.
struct Knobs {
  int xfer_mode = 1;               // HPF_H2D=plain|staged|register: 0 plain, 1 staged, 2 hipHostRegister
  unsigned xfer_threads = 4;       // HPF_H2D_THREADS
  int phi_cfg[3] = {0, 0, 0};      // HPF_PHI_CFG "G,R,V": an explicit plain shape of the phi pass (zeros: none given)
  bool w_pack = false;             // HPF_W_PACK=1: pack whenever a shape exists
  int sweep_cfg[2] = {0, 0};       // HPF_SWEEP_CFG "G,R" with G*R == ld (plain rows)
  uint32_t sweep_blocks_max = 2048;     // 8 waves per SIMD (HPF_SWEEP_BLOCKS); 1024 -> 2048: C2 user sweep 0.587 -> 0.544 ms
  int graph_mode = -1;                  // HPF_GRAPH: -1 auto, 0 off, 1 on
  uint32_t seg_max = 512;               // HPF_SEG_MAX
  uint32_t huge_slots = 256, group_slots = 64;  // two-level combine above huge_slots segments (HPF_HUGE_SLOTS)
  // tiled pass: 2 auto, 0 never, 1 forced with every row regrouped (HPF_TILE); bytes of gathered rows per tile
  // (HPF_TILE_BYTES), segments per workgroup (HPF_TILE_CHUNK), the mean run a heavy row must reach in a
  // tile (HPF_TILE_RUN), the share of the nonzeros the heavy rows must hold (HPF_TILE_SHARE, per cent)
  // order of an XCD's queue (HPF_TILE_ORDER): 1 = the row-major rest in front on the even XCDs and behind on the
  // odd ones, so that half the chip pulls over the fabric while the other half runs from its L2 (C2 item pass
  // 4.39 ms; 0 = in front everywhere 4.75; 2 = dealt between the tiles 4.58)
  int tile_order = 1;
  uint32_t tile_split_below = 8;       // with fewer tiles than this EVERY tile is cut eight ways, a piece per XCD queue (round 4: below 32 tiles; C4's seven tiles of
                                       // items are 2 % faster that way than levelled); from here on whole tiles are dealt eight at a time and the remainder levels
                                       // the queues (plan_tile_queues)
  int tile_sides = 3;                   // HPF_TILE_SIDES: bit 0 the user pass, bit 1 the item pass (experiments)
  int tile_mode = 2; uint64_t tile_bytes = 4u << 20; uint32_t tile_chunk = 0 /* 0: two segments per wave of the workgroup */, tile_min_run = 0; double tile_min_share = 0.15;
  uint32_t phi_blocks = 65536;      // ~one wave per few segments; the dispatcher balances (HPF_PHI_BLOCKS)
  // Threads per workgroup of a packed phi pass.  0 (default): 256 -- four waves, grid-stride -- for a ROW-MAJOR side, 64 -- one
  // wave, a chunk of two segments -- for a TILED side (round 5).  A workgroup's wave slots come back one SIMD at a time but a
  // new workgroup needs one on each of the four SIMDs at once: with the uneven runs of a tiled list a third of the slots stood
  // empty (SQ_WAVE_CYCLES: ~2 of 3 waves per SIMD resident on average) -- which a pass that lives on its L2 hits and on issue
  // pays for (C4 18.65 -> 17.45 ms, a C5 shard 44.8 -> 41.5; experiments.md) and a pass bound by the fabric does not (C2's
  // user pass, a C3 shard: unchanged).  Same segments, same order inside each: the same bits.  HPF_PHI_WG forces 64 | 128 | 256.
  uint32_t phi_wg = 0;
  long long loo_batch = 0;          // HPF_LOO_BATCH: at most so many users per batch of the fused rank calls (<= 0: no limit of its own)
  long long ftop_batch = 0;         // HPF_FACTOR_TOP_BATCH: at most so many columns per transposed batch of hpf_factor_top (<= 0: no limit of its own)
  int fold_route = 0;               // HPF_FOLD_ROUTE=sweeps: hpf_fold_in / hpf_fold_in_items through the training kernels (1), for A/B runs; never chosen by the library
  // HPF_FOLD_LONG_MIN: hpf_fold_in_items gives an item with at least so many ratings to a workgroup (fold_in_long_kernel), the
  // others to a wave.  Inside the gate: the route changes the order of a row's sums.  >= 2^32 - 1: every row to the wave
  // kernel; 1: every non-empty row to the workgroup kernel (tests).  0 = the plan's FOLD_LONG_MIN
  uint32_t fold_long_min = 0;
  // HPF_FUSED_SWEEP=0|1|2: the user pass writes W of its single-segment rows in its segment epilogue and the user sweep only
  // takes their sums (fused_sweep below).  0: never (the A/B switch), 1: where it was measured to pay (fused_pays), 2: wherever
  // an instance exists (tests, A/B runs of the other shapes).  Every route gives the same bits in every array, so the variable
  // is read outside the gate.
  int fused_sweep = 1;
};

// the one place that reads the knobs from the environment
inline Knobs read_knobs()
{
  Knobs k;
  if (const char *e = getenv("HPF_LOO_BATCH")) k.loo_batch = atoll(e);      // outside the gate: the batch size cannot change a result
  if (const char *e = getenv("HPF_FUSED_SWEEP")) { int v = atoi(e); if (v >= 0 && v <= 2) k.fused_sweep = v; }   // likewise: which kernel writes a row of W cannot
  const char *x = getenv("HPF_EXPERIMENTAL");
  if (!x || atoi(x) != 1) return k;
  if (const char *e = getenv("HPF_H2D")) k.xfer_mode = !strcmp(e, "plain") ? 0 : !strcmp(e, "register") ? 2 : 1;
  if (const char *e = getenv("HPF_H2D_THREADS")) { int v = atoi(e); if (v >= 1 && v <= 64) k.xfer_threads = (unsigned)v; }
  if (const char *e = getenv("HPF_PHI_CFG")) { int c[3] = {0, 0, 0}; if (sscanf(e, "%d,%d,%d", &c[0], &c[1], &c[2]) == 3) std::copy(c, c + 3, k.phi_cfg); }
  if (const char *e = getenv("HPF_W_PACK")) k.w_pack = atoi(e) == 1;
  if (const char *e = getenv("HPF_SWEEP_CFG")) { int c[2] = {0, 0}; if (sscanf(e, "%d,%d", &c[0], &c[1]) == 2) std::copy(c, c + 2, k.sweep_cfg); }
  if (const char *e = getenv("HPF_SWEEP_BLOCKS")) { int v = atoi(e); if (v >= 1 && v <= 65536) k.sweep_blocks_max = (uint32_t)v; }
  if (const char *e = getenv("HPF_GRAPH")) k.graph_mode = atoi(e) != 0;
  if (const char *e = getenv("HPF_SEG_MAX")) { int v = atoi(e); if (v >= 16) k.seg_max = (uint32_t)v; }
  if (const char *e = getenv("HPF_HUGE_SLOTS")) { int v = atoi(e); if (v >= 2) { k.huge_slots = (uint32_t)v; k.group_slots = std::max<uint32_t>(2, std::min<uint32_t>(64, (uint32_t)v / 2)); } }
  if (const char *e = getenv("HPF_TILE")) { int v = atoi(e); if (v >= 0 && v <= 2) k.tile_mode = v; }
  if (const char *e = getenv("HPF_TILE_SIDES")) { int v = atoi(e); if (v >= 0 && v <= 3) k.tile_sides = v; }
  if (const char *e = getenv("HPF_TILE_SPLIT_BELOW")) { int v = atoi(e); if (v >= 0) k.tile_split_below = (uint32_t)v; }
  if (const char *e = getenv("HPF_TILE_ORDER")) { int v = atoi(e); if (v >= 0 && v <= 2) k.tile_order = v; }
  if (const char *e = getenv("HPF_TILE_BYTES")) { long long v = atoll(e); if (v >= 1024) k.tile_bytes = (uint64_t)v; }
  if (const char *e = getenv("HPF_TILE_CHUNK")) { int v = atoi(e); if (v >= 1) k.tile_chunk = (uint32_t)v; }       // default: two per wave of the workgroup
  if (const char *e = getenv("HPF_TILE_RUN")) { int v = atoi(e); if (v >= 1) k.tile_min_run = (uint32_t)v; }
  if (const char *e = getenv("HPF_TILE_SHARE")) { int v = atoi(e); if (v >= 0 && v <= 100) k.tile_min_share = v / 100.0; }
  if (const char *e = getenv("HPF_PHI_BLOCKS")) { int v = atoi(e); if (v >= 1) k.phi_blocks = (uint32_t)v; }
  if (const char *e = getenv("HPF_FACTOR_TOP_BATCH")) k.ftop_batch = atoll(e);
  if (const char *e = getenv("HPF_FOLD_ROUTE")) k.fold_route = !strcmp(e, "sweeps") ? 1 : 0;
  if (const char *e = getenv("HPF_FOLD_LONG_MIN")) { unsigned long long v = strtoull(e, nullptr, 10); if (v >= 1) k.fold_long_min = (uint32_t)std::min<unsigned long long>(v, 0xffffffffull); }
  if (const char *e = getenv("HPF_PHI_WG")) { int v = atoi(e); if (v == 64 || v == 128 || v == 256) k.phi_wg = (uint32_t)v; }
  return k;
}

// ---- which kernel instances exist: the dispatcher of hpf_capi.hip instantiates exactly these ---------------------------
constexpr bool is_group(int G) { return G == 4 || G == 8 || G == 16 || G == 32 || G == 64; }   // lanes per nonzero / per row

// phi_pass_kernel: plain rows, R loads of V elements per lane -- V = 1 or 2 doubles, 2 or 4 floats (8- or 16-byte accesses)
constexpr bool has_phi(bool w32, int G, int R, int V) { return is_group(G) && R >= 1 && R <= 8 && (w32 ? V == 2 || V == 4 : V == 1 || V == 2); }
// phi_pass_packed_kernel: G lanes per nonzero, L 16-byte pieces per lane; nine pieces of plain doubles stand in for p59
// rows of 17 elements
constexpr bool has_phi_packed(int wl, int G, int L) { return (wl == WL_P59 || wl == WL_F48 || wl == WL_F64) && is_group(G) && L >= 1 && (L <= 8 || (wl == WL_F64 && L == 9)); }
// phi_pass_fused_kernel (the packed pass with the sweep epilogue): the p59 shapes whose build keeps the pass's three waves per SIMD
// (<= 168 VGPRs) WITHOUT scratch and without SGPRs spilled into VGPR lanes -- the compiler's figures decide
// (-Rpass-analysis=kernel-resource-usage; profiles/r10/experiments.md 1 lists every candidate).  The shapes left out spill
// (K = 200's (16, 6): 40 bytes per lane) or lose the LDS promotion of their gather registers to the staged row ((16, 4),
// (32, 4): 80 bytes of scratch inside the batch loop).  A row per wave of the workgroup is staged in LDS: <= 6 KiB, + the
// column sums: the pass keeps its twelve waves per CU.
constexpr bool has_phi_fused(int wl, int G, int L)
{
  return wl == WL_P59 && has_phi_packed(wl, G, L) &&
         ((G <= 8 && L <= 6) || (G == 16 && L <= 3) || (G == 32 && L <= 2) || (G == 64 && L == 1));
}
// gather_only_kernel: the loads of a pass over rows of 16-byte pieces (plain rows of doubles read in pairs are such rows)
constexpr bool has_gather_only(int G, int L) { return is_group(G) && L >= 1 && L <= 9; }
// row_sweep_kernel: G lanes per row with R columns each
constexpr bool has_sweep(int mode, int G, int R)
{
  if (!is_group(G) || R < 1) return false;
  switch (mode) {
    case SW_REG_P59: return G >= 8 && R <= 9 && R != 6;     // the slot counts p59 shapes have (p59_of_slots): 6 is none; G = 2 x the pass's lanes <= 64
    case SW_LDS_P59: return G == 64 && R <= 16;             // narrower groups build in registers
    case SW_F64:     if (R == 9) return true;               // otherwise the shapes of plain rows
                     [[fallthrough]];
    case SW_LDS_F48:
    case SW_PLAIN:   return R <= (G == 64 ? 16 : 8);        // G = 64 up to R = 16: 513..1024 columns
  }
  return false;
}

// row_sums_kernel: the sweep that follows such a pass -- the modes that write p59 rows
constexpr bool has_sums(int mode, int G, int R) { return (mode == SW_REG_P59 || mode == SW_LDS_P59) && has_sweep(mode, G, R); }

// loo_rank_kernel / rank_queries_kernel: NCH chunks of 32 columns of the A fragments in registers, 0 = re-read per step
constexpr bool has_rank_chunks(int NCH) { return NCH == 0 || NCH == 1 || NCH == 2 || NCH == 4; }
constexpr int rank_chunks(uint32_t K) { return K <= 32 ? 1 : K <= 64 ? 2 : K <= 128 ? 4 : 0; }

// ---- the fused rank calls (hpf_loo_ranks, hpf_rank_queries) -----------------------------------------------------------
// Users per batch: the bit rows of a batch (one bit per item, 64-bit words) stay under 256 MB, a multiple of the 64 users of
// a workgroup; HPF_LOO_BATCH (rounded up to the 16 users of a wave's block; a TEST knob, so that a handful of users crosses
// a batch boundary) makes it smaller; never more than the selected users need.
inline uint32_t rank_batch_users(uint32_t m, uint32_t n_sel, long long knob)
{
  const uint64_t words = std::max<uint64_t>(((uint64_t)m + 63) / 64, 1);
  uint64_t batch = std::max<uint64_t>(64, (((uint64_t)256 << 20) / (words * 8)) & ~63ull);
  if (knob > 0) batch = std::min<uint64_t>(batch, ((uint64_t)knob + 15) & ~15ull);
  return (uint32_t)std::min<uint64_t>(batch, ((uint64_t)n_sel + 15) & ~15ull);
}

// Launch grid over `rows` users or rows and `ntiles` 64-item tiles: a block per 64 rows.  Few blocks: the item range is
// cut so that some 1024 workgroups exist; many: one sweep per block.  No split is empty.
struct RankGrid { uint32_t blocks, splits, tiles_per_split; };
inline RankGrid rank_grid(uint32_t rows, uint32_t ntiles)
{
  RankGrid g;
  g.blocks = (rows + 63) / 64;
  g.splits = std::max<uint32_t>(1, std::min<uint32_t>(ntiles, (1024 + g.blocks - 1) / g.blocks));
  g.tiles_per_split = (ntiles + g.splits - 1) / g.splits;
  g.splits = (ntiles + g.tiles_per_split - 1) / g.tiles_per_split;
  return g;
}

// Rows of scores the unfused ranking calls (hpf_scores, hpf_rank_topn, hpf_item_ranks) keep at once: <= 1 GiB of rows of
// m doubles, a multiple of 16, at least 16; never more than the selected users need
inline uint32_t score_batch_rows(uint32_t m, uint32_t n_sel)
{
  uint64_t bmax = ((1ull << 30) / (8ull * std::max<uint32_t>(m, 1))) & ~15ull;
  bmax = std::max<uint64_t>(bmax, 16);
  return (uint32_t)std::min<uint64_t>(bmax, ((uint64_t)n_sel + 15) & ~15ull);
}

// ---- top-N for every user (hpf_recommend) ---------------------------------------------------------
// hpf_similar plans with the same functions, m = the rows of the side it ranks
// Up to TOPN_FUSED_MAX the call is fused (topn_sweep_kernel + topn_merge_kernel); above it, up to TOPN_MAX, it runs the
// materialising route of hpf_rank_topn.  hgaprec_amd/capi.py mirrors the cut as RECOMMEND_FUSED_MAX.
constexpr uint32_t TOPN_MAX = 1024, TOPN_FUSED_MAX = 256;
constexpr bool topn_fused(uint32_t topn) { return topn >= 1 && topn <= TOPN_FUSED_MAX; }
// Entries of the candidate buffer of one (user, split): twice the power of two >= max(topn, 64).  A tile adds at most 64
// and a compacted buffer holds topn, so cap >= topn + 64 leaves room for a tile after every compaction.
constexpr uint32_t pow2_ceil(uint32_t x, uint32_t least = 1) { while (least < x) least <<= 1; return least; }   // `least` a power of two
constexpr uint32_t log2_of(uint32_t pow2) { uint32_t lg = 0; while ((1u << lg) < pow2) ++lg; return lg; }
constexpr uint32_t topn_np(uint32_t topn) { return pow2_ceil(topn, 64); }
constexpr uint32_t topn_cap(uint32_t topn) { return 2 * topn_np(topn); }
constexpr uint64_t TOPN_ENTRY_BYTES = 12, TOPN_BATCH_BYTES = (uint64_t)512 << 20;    // a key and an item; candidate memory of a batch

// rank_grid's policy with one more rule: a split covers at least four buffers' worth of items (cap / 16 tiles) unless the
// whole range is shorter -- with the one or two tiles per split that rank_grid gives a handful of users nothing would be
// filtered and the merge would do all the work.  No split is empty.
inline RankGrid topn_grid(uint32_t rows, uint32_t ntiles, uint32_t cap)
{
  RankGrid g = rank_grid(rows, ntiles);
  const uint32_t least = std::max<uint32_t>(1, std::min<uint32_t>(ntiles, cap / 16));
  if (g.tiles_per_split < least) {
    g.tiles_per_split = least;
    g.splits = std::max<uint32_t>(1, (ntiles + least - 1) / least);
  }
  return g;
}
// candidate memory of a batch of `rows` users
inline uint64_t topn_batch_bytes(uint32_t rows, uint32_t ntiles, uint32_t cap)
{
  return (uint64_t)((rows + 15) & ~15u) * topn_grid(rows, ntiles, cap).splits * cap * TOPN_ENTRY_BYTES;
}
// Users per batch: rank_batch_users (the bit rows; HPF_LOO_BATCH), reduced -- staying a multiple of 64 -- until the
// candidate buffers of a batch are <= 512 MB.  64 users always fit: 1024 + 1 splits at most, 64 x 1025 x 512 x 12 B = 403 MB.
inline uint32_t topn_batch_users(uint32_t m, uint32_t n_sel, uint32_t cap, long long knob)
{
  const uint32_t ntiles = (uint32_t)(((uint64_t)m + 63) / 64);
  uint32_t batch = rank_batch_users(m, n_sel, knob);
  while (batch > 64 && topn_batch_bytes(batch, ntiles, cap) > TOPN_BATCH_BYTES) batch = (batch - 1) & ~63u;
  return batch;
}

// ---- fold-in of new users (hpf_fold_in) ------------------------------------------------------------
// fold_in_kernel<R>: a wave per user, lane l holds the columns l + 64 t, t < R.  The item rows it gathers are a plain fp64
// copy of its own stride ld: the live columns K + 2 * bias padded to whole 128-byte lines (independent of how the handle
// stores W).  Workgroups of FOLD_WAVES waves; every wave owns a slice of LDS in which the gathered rows of its user stay
// between iterations when all of them fit: rows_held of them, at most the 64 whose ratings one register per lane holds.
// Three workgroups' slices fit a CU's 160 KiB.  hgaprec_amd/capi.py mirrors the arithmetic (fold_plan).
constexpr uint32_t FOLD_WAVES = 4, FOLD_SLICE_BYTES = 12288, FOLD_LDS_LIMIT = 65536, FOLD_BLOCKS_MAX = 65536;
constexpr bool has_fold(int R) { return R >= 1 && R <= 16; }
struct FoldPlan {
  uint32_t ld = 0, R = 0;               // row stride of the gathered copy, columns; columns per lane
  uint32_t lds_wave_bytes = 0;          // a wave's slice of LDS
  uint32_t rows_held = 0;               // gathered rows a slice holds
  bool ok = false;                      // false: no kernel instance for this column count
  uint32_t lds_block_bytes() const { return FOLD_WAVES * lds_wave_bytes; }
  // workgroups for n users: one wave per user until the grid is FOLD_BLOCKS_MAX workgroups, which then stride
  uint32_t grid(uint32_t n) const { return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(((uint64_t)n + FOLD_WAVES - 1) / FOLD_WAVES, FOLD_BLOCKS_MAX)); }
};
inline FoldPlan fold_plan(uint32_t K, bool bias)
{
  FoldPlan p;
  const uint32_t C = K + (bias ? 2u : 0u);
  if (K < 1 || C > HPF_MAX_COLUMNS) return p;
  p.ld = (C + 15u) & ~15u;
  p.R = (p.ld + 63u) / 64u;
  p.lds_wave_bytes = FOLD_SLICE_BYTES;
  p.rows_held = std::min<uint32_t>(64u, p.lds_wave_bytes / (p.ld * 8u));
  p.ok = has_fold((int)p.R) && p.rows_held >= 1;
  return p;
}

// ---- fold-in of new items (hpf_fold_in_items) ------------------------------------------------------
// Two kernels share the rows: fold_in_kernel<R> (a wave per row, as above) takes the rows with fewer than long_min
// nonzeros, fold_in_long_kernel<R, WAVES> (a WORKGROUP per row) the others.  WAVES per R is the largest of {8, 4} whose
// build uses no scratch: launch_bounds(512) leaves a wave 256 registers (VGPR + AGPR), launch_bounds(256) the whole SIMD's
// 512 (the compiler's figures: DESIGN.md section 4g).  The workgroup's LDS: WAVES partial rows of R * 64 doubles and the
// shared stop word.  At most FOLD_LONG_BLOCKS_MAX workgroups, which then stride over the list of long rows.
// hgaprec_amd/capi.py mirrors the arithmetic (fold_items_plan).
constexpr uint32_t FOLD_LONG_MIN = 256, FOLD_LONG_BLOCKS_MAX = 4096;   // 256: the best of {128 .. 2048} measured
constexpr int fold_long_waves(int R) { return R <= 8 ? 8 : 4; }     // <9, 8> spills 96 bytes per lane
constexpr bool has_fold_long(int R, int WAVES) { return has_fold(R) && WAVES == fold_long_waves(R); }
// the nonzeros [begin, end) of a row of len that wave w of `waves` walks: the row's 64-blocks dealt in contiguous runs of
// ceil(blocks / waves); a function of len and waves only.  Empty (begin == end) for the waves beyond the last block.
struct FoldPart { uint32_t begin, end; };
constexpr FoldPart fold_part(uint32_t len, uint32_t waves, uint32_t w)
{
  const uint64_t blocks = ((uint64_t)len + 63u) / 64u, per = (blocks + waves - 1) / waves;
  const uint64_t lo = (uint64_t)w * per < blocks ? (uint64_t)w * per : blocks, hi = (uint64_t)(w + 1) * per < blocks ? (uint64_t)(w + 1) * per : blocks;
  return {(uint32_t)(lo * 64u < len ? lo * 64u : len), (uint32_t)(hi * 64u < len ? hi * 64u : len)};
}
struct FoldItemsPlan {
  FoldPlan wave;                        // fold_in_kernel's shape (the gathered copy, R and the LDS slices are shared)
  uint32_t waves = 0;                   // waves of a workgroup of fold_in_long_kernel
  uint32_t long_min = FOLD_LONG_MIN;    // a row with at least so many nonzeros is the workgroup kernel's
  bool ok = false;
  uint32_t lds_long_bytes() const { return waves * wave.R * 64u * 8u + 16u; }
  // workgroups for n_long long rows (0: no launch)
  uint32_t grid_long(uint32_t n_long) const { return std::min<uint32_t>(n_long, FOLD_LONG_BLOCKS_MAX); }
};
inline FoldItemsPlan fold_items_plan(uint32_t K, bool bias, uint32_t long_min = FOLD_LONG_MIN)
{
  FoldItemsPlan p;
  p.wave = fold_plan(K, bias);
  if (!p.wave.ok) return p;
  p.waves = (uint32_t)fold_long_waves((int)p.wave.R);
  p.long_min = long_min;
  p.ok = has_fold_long((int)p.wave.R, (int)p.waves) && p.lds_long_bytes() <= FOLD_LDS_LIMIT;
  return p;
}

// ---- why a score is what it is (hpf_explain, hpf_factor_top) --------------------------------------
// explain_kernel<R>: a wave per pair, lane l holds the terms l + 64 t, t < R, of the pair's score -- the K products and,
// with bias, the two bias terms K and K + 1 -- read straight from the handle's E (whatever its row stride; no copy).
// Workgroups of EXPLAIN_WAVES waves; a wave takes EXPLAIN_RUN consecutive pairs per trip, so that the run of pairs a
// recommend list makes keeps its user's row in registers; at most EXPLAIN_BLOCKS_MAX workgroups (eight per CU), which then
// stride.  hgaprec_amd/capi.py mirrors the arithmetic (explain_plan).
constexpr uint32_t EXPLAIN_MAX = 32;      // HPF_EXPLAIN_MAX of hpf.h (pinned there by hpf_capi.hip): a lane per returned term
constexpr uint32_t EXPLAIN_WAVES = 4, EXPLAIN_RUN = 8, EXPLAIN_BLOCKS_MAX = 2048;
constexpr bool has_explain(int R) { return R >= 1 && R <= 16; }
struct ExplainPlan {
  uint32_t terms = 0, R = 0;            // terms of a score: K + 2 * bias; terms per lane
  bool ok = false;                      // false: no kernel instance for this column count
  static constexpr uint32_t pairs_per_block() { return EXPLAIN_WAVES * EXPLAIN_RUN; }
  // workgroups for cnt pairs: a run per wave until the grid is EXPLAIN_BLOCKS_MAX workgroups
  uint32_t grid(uint64_t cnt) const { return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((cnt + pairs_per_block() - 1) / pairs_per_block(), EXPLAIN_BLOCKS_MAX)); }
  // pairs one trip of that grid covers: above it the waves stride
  uint64_t pairs_per_trip(uint64_t cnt) const { return (uint64_t)grid(cnt) * pairs_per_block(); }
};
inline ExplainPlan explain_plan(uint32_t K, bool bias)
{
  ExplainPlan p;
  const uint32_t C = K + (bias ? 2u : 0u);
  if (K < 1 || C > HPF_MAX_COLUMNS) return p;
  p.terms = C;
  p.R = (C + 63u) / 64u;
  p.ok = has_explain((int)p.R);
  return p;
}

// hpf_factor_top: columns transposed at once into the temporary [batch x rows] the selection reads, <= 512 MB of it (one
// column where a single one is longer); `knob` (HPF_FACTOR_TOP_BATCH, a TEST knob) makes the batch smaller
constexpr uint32_t FACTOR_TOP_MAX = TOPN_MAX, FACTOR_TOP_TILE = 32;
constexpr uint64_t FACTOR_TOP_BYTES = (uint64_t)512 << 20;
inline uint32_t factor_top_batch(uint32_t rows, uint32_t K, long long knob)
{
  uint64_t b = std::max<uint64_t>(1, FACTOR_TOP_BYTES / (8ull * std::max<uint32_t>(rows, 1)));
  if (knob > 0) b = std::min<uint64_t>(b, (uint64_t)knob);
  return (uint32_t)std::min<uint64_t>(b, std::max<uint32_t>(K, 1));
}

// ---- because you rated (hpf_because) ----------------------------------------------------------------
// because_shape_kernel<R>: a wave per selected user; because_kernel<R>: a wave per target pair, BECAUSE_RUN consecutive
// pairs per trip (the targets of one user are consecutive: its row is set up once per run).  Lane l holds the columns
// l + 64 t, t < R.  The item rows are the fold-in's gathered copy (fold_plan's stride: the live columns K + 2 * bias padded
// to whole 128-byte lines).  Workgroups of BECAUSE_WAVES waves, at most BECAUSE_BLOCKS_MAX of them, which then stride.
// hgaprec_amd/capi.py mirrors the arithmetic (because_plan).
constexpr uint32_t BECAUSE_MAX = 32;      // HPF_BECAUSE_MAX of hpf.h (pinned there by hpf_capi.hip): a lane per returned entry
constexpr uint32_t BECAUSE_WAVES = 4, BECAUSE_RUN = 4, BECAUSE_BLOCKS_MAX = 4096;
constexpr bool has_because(int R) { return R >= 1 && R <= 16; }
struct BecausePlan {
  uint32_t ld = 0, R = 0;               // row stride of the gathered copy and of D, columns; columns per lane
  bool ok = false;                      // false: no kernel instance for this column count
  static constexpr uint32_t pairs_per_block() { return BECAUSE_WAVES * BECAUSE_RUN; }
  // workgroups for n selected users: a wave per user
  uint32_t grid_users(uint32_t n) const { return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(((uint64_t)n + BECAUSE_WAVES - 1) / BECAUSE_WAVES, BECAUSE_BLOCKS_MAX)); }
  // workgroups for nt target pairs: a run per wave
  uint32_t grid_pairs(uint64_t nt) const { return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((nt + pairs_per_block() - 1) / pairs_per_block(), BECAUSE_BLOCKS_MAX)); }
};
inline BecausePlan because_plan(uint32_t K, bool bias)
{
  BecausePlan p;
  const FoldPlan f = fold_plan(K, bias);
  if (f.ld == 0) return p;
  p.ld = f.ld;
  p.R = f.R;
  p.ok = has_because((int)p.R);
  return p;
}

// ---- posterior moments of a score (hpf_score_moments, hpf_recommend_ucb) ----------------------------
// var(u, i) = X_u . Y_i over C = 2 K + 2 * bias derived columns (moment_rows_kernel).  ucb_sweep_kernel sweeps the
// concatenation [the K columns of E padded to whole MFMA steps | the C derived columns] with the A rows read per step: the
// mean chain ends after mean_steps MFMAs, the variance chain takes the other var_steps.  The derived rows have the stride
// ldx: C padded to a whole MFMA step (32-byte rows, the padding zero).  X is built for the selected users of one batch
// (topn_batch_users: the batches are hpf_recommend's), Y once for every item.  pair_moments_kernel: a wave per MOMENTS_PAIRS
// pairs, workgroups of MOMENTS_WAVES waves, at most MOMENTS_BLOCKS_MAX of them, which then stride; moment_rows_kernel: a
// thread per element, the same cap.  hgaprec_amd/capi.py mirrors the arithmetic (moments_plan).
constexpr uint32_t MOMENTS_WAVES = 4, MOMENTS_PAIRS = 16, MOMENTS_BLOCKS_MAX = 4096;
struct MomentsPlan {
  uint32_t C = 0, ldx = 0;              // columns and row stride of the derived rows
  uint32_t mean_cols = 0;               // K padded to a whole MFMA step: where the derived columns begin in the concatenation
  uint32_t mean_steps = 0, var_steps = 0;   // MFMAs of the two chains of one output: those hpf_scores issues for K and for C columns
  bool ok = false;                      // false: C does not fit HPF_MAX_COLUMNS
  static constexpr uint32_t pairs_per_block() { return MOMENTS_WAVES * MOMENTS_PAIRS; }
  // selected users whose X rows are built at once: the users of a batch of the top-N sweep
  uint32_t x_rows(uint32_t m, uint32_t n_sel, uint32_t topn, long long knob) const { return topn_batch_users(m, n_sel, topn_cap(topn), knob); }
  // bytes of the call's derived rows: Y of every item and X of a batch
  uint64_t derived_bytes(uint32_t m, uint32_t x_rows_) const { return ((uint64_t)m + x_rows_) * ldx * 8; }
  // workgroups of pair_moments_kernel for cnt pairs
  uint32_t grid_pairs(uint64_t cnt) const { return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((cnt + pairs_per_block() - 1) / pairs_per_block(), MOMENTS_BLOCKS_MAX)); }
  // workgroups of moment_rows_kernel for `rows` derived rows
  uint32_t grid_rows(uint32_t rows) const { return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(((uint64_t)rows * ldx + 255) / 256, MOMENTS_BLOCKS_MAX)); }
};
inline MomentsPlan moments_plan(uint32_t K, bool bias)
{
  MomentsPlan p;
  const uint64_t C = 2ull * K + (bias ? 2u : 0u);
  if (K < 1 || C > HPF_MAX_COLUMNS) return p;
  p.C = (uint32_t)C;
  p.ldx = (p.C + 3u) & ~3u;
  p.mean_cols = (K + 3u) & ~3u;
  p.mean_steps = p.mean_cols / 4;
  p.var_steps = p.ldx / 4;
  p.ok = true;
  return p;
}

// ---- one posterior draw of a side's rows (hpf_sample_state, hpf_recommend_thompson) -----------------
// gamma_rows_kernel: a thread per element of rows x ld output doubles (the padding columns are written too, as zeros), 256
// threads a workgroup, at most SAMPLE_BLOCKS_MAX workgroups, which then stride -- MomentsPlan::grid_rows' cap.
// hpf_recommend_thompson keeps the item side's draw (n_items x ld doubles) for the call and the user side's per batch of
// the top-N sweep (topn_batch_users: the batches are hpf_recommend's); hpf_sample_state works through its rows in pieces
// of at most SAMPLE_PIECE_BYTES of sampled rows.
constexpr uint32_t SAMPLE_BLOCKS_MAX = MOMENTS_BLOCKS_MAX;
constexpr uint64_t SAMPLE_PIECE_BYTES = 256ull << 20;
struct SamplePlan {
  uint64_t elements = 0;                // rows x ld
  uint32_t grid = 1;                    // workgroups of gamma_rows_kernel
};
inline SamplePlan sample_plan(uint64_t rows, uint32_t ld)
{
  SamplePlan p;
  p.elements = rows * ld;
  p.grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((p.elements + 255) / 256, SAMPLE_BLOCKS_MAX));
  return p;
}
// rows of one piece of hpf_sample_state
inline uint32_t sample_piece_rows(uint32_t n_sel, uint32_t ld)
{
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(n_sel, SAMPLE_PIECE_BYTES / ((uint64_t)std::max(ld, 1u) * 8)));
}

// ---- diversified top-N (hpf_recommend_diverse) -------------------------------------------------------
// mmr_kernel: a workgroup of DIVERSE_WAVES waves per selected user, a persistent grid that strides over the users of a
// launch.  The pool of a user (at most `pool` entries) is padded to Pp, whole 16 x 16 MFMA tiles; its Gram matrix has
// side^2 tiles of `steps` MFMAs each (K columns, four a step, the tail padded by zeros).  A wave takes strips of up to
// DIVERSE_STRIP tiles of one tile row (one A fragment, DIVERSE_STRIP accumulators), the strips dealt round-robin to the
// waves.  Every workgroup owns a slab of Pp x Pp doubles in device memory for the matrix; the slabs of one launch total at
// most DIVERSE_SLABS_BYTES, which caps the grid beside DIVERSE_WGS_PER_CU workgroups a CU and the users of the launch.
// LDS: the pool's item ids, the prefix length and two buffers of the waves' arg-max (key, position).
constexpr uint32_t DIVERSE_POOL_MAX = 256;      // HPF_DIVERSE_POOL_MAX of hpf.h (pinned there by hpf_capi.hip): a thread per pool entry
constexpr uint32_t DIVERSE_WAVES = 4, DIVERSE_STRIP = 4, DIVERSE_WGS_PER_CU = 8;
constexpr uint64_t DIVERSE_SLABS_BYTES = 256ull << 20;
constexpr uint32_t DIVERSE_LDS_BYTES = DIVERSE_POOL_MAX * 4 + 16 + 2 * DIVERSE_WAVES * (8 + 4);   // ids, P and r_0, two arg-max buffers
// Strip s of a Gram matrix of `side` tiles a side: its tile row and its first tile column.  Strips 0 .. side - 1 are the
// first DIVERSE_STRIP tile columns of every tile row, the next `side` strips the next columns, ...: the short strips of a
// ragged side come last.  Wave w of a workgroup takes strips w, w + DIVERSE_WAVES, ...  mmr_kernel walks with this very
// function, so what the selftest checks of the walk is the kernel's walk.
struct DiverseStrip { uint32_t ti, tj0; };
constexpr DiverseStrip diverse_strip(uint32_t s, uint32_t side) { return DiverseStrip{s % side, (s / side) * DIVERSE_STRIP}; }
constexpr uint32_t diverse_strips(uint32_t side) { return side * ((side + DIVERSE_STRIP - 1) / DIVERSE_STRIP); }
// tiles, steps, strips, tiles_per_wave and lds_bytes are not launch parameters (the kernel derives its walk from each
// user's own P through diverse_strip, and its LDS is static): they describe the work for DESIGN.md's estimates and let the
// selftest hold the walk and the kernel's static LDS (a static_assert in hpf_kernels.hpp) to the committed table.
struct DiversePlan {
  uint32_t Pp = 0;                      // the pool padded to whole tiles; also the slab's row stride, doubles
  uint32_t side = 0, tiles = 0;         // tiles along one side of the Gram matrix; side^2
  uint32_t steps = 0;                   // MFMAs of one tile: those hpf_scores issues for K columns
  uint32_t strips = 0;                  // side x ceil(side / DIVERSE_STRIP)
  uint32_t tiles_per_wave = 0;          // the most tiles a wave computes: its strips' tiles, those past the side left out
  uint64_t slab_bytes = 0;              // Pp x Pp doubles: at most 512 KB
  uint32_t workgroups = 0;              // the grid of one launch
  uint32_t lds_bytes = 0;
  bool ok = false;                      // false: pool outside 1 .. DIVERSE_POOL_MAX, K = 0 or nobody selected
};
inline DiversePlan diverse_plan(uint32_t pool, uint32_t n_sel, uint32_t K, uint32_t CUs)
{
  DiversePlan p;
  if (pool < 1 || pool > DIVERSE_POOL_MAX || K < 1 || n_sel < 1) return p;
  p.Pp = (pool + 15u) & ~15u;
  p.side = p.Pp / 16;
  p.tiles = p.side * p.side;
  p.steps = (K + 3u) / 4;
  p.strips = diverse_strips(p.side);
  for (uint32_t w = 0; w < DIVERSE_WAVES; ++w) {
    uint32_t t = 0;
    for (uint32_t s = w; s < p.strips; s += DIVERSE_WAVES) t += std::min(DIVERSE_STRIP, p.side - diverse_strip(s, p.side).tj0);
    p.tiles_per_wave = std::max(p.tiles_per_wave, t);
  }
  p.slab_bytes = (uint64_t)p.Pp * p.Pp * 8;
  const uint64_t by_mem = DIVERSE_SLABS_BYTES / p.slab_bytes, by_cus = (uint64_t)std::max(CUs, 1u) * DIVERSE_WGS_PER_CU;
  p.workgroups = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(n_sel, std::min(by_mem, by_cus)));
  p.lds_bytes = DIVERSE_LDS_BYTES;
  p.ok = true;
  return p;
}

// ---- the tiled phi pass: what is tiled, and where its segments run --------------------------------
// Policy of one side, decided before anything is allocated.  The gathered matrix (rows_oth rows of row_bytes) is cut into
// tiles of T consecutive rows; owner rows with at least light_below nonzeros are heavy (their nonzeros are regrouped by
// tile), the rest stay row-major.  Auto mode (tile_mode 2): the gathered matrix must be larger than 2.5 tiles.  Forced
// (tile_mode 1, an experimental knob): every row is regrouped whenever there are two tiles.  tile == false: not worth tiling.
struct TilePolicy { bool tile = false; uint32_t T = 0, tiles = 0, min_run = 0; uint64_t light_below = 0; };
inline TilePolicy tile_policy(uint32_t rows_oth, size_t row_bytes, uint64_t nnz, uint32_t rows, uint32_t nz_per_batch, bool item_side,
                              const Knobs &kn, uint32_t cfg_tiling)
{
  TilePolicy p;
  if (!((kn.tile_sides >> (item_side ? 1 : 0)) & 1)) return p;
  if (kn.tile_mode == 0 || cfg_tiling == 1 || nnz == 0 || rows == 0) return p;      // (>= 2^32 nonzeros: positions are 64-bit throughout;
                                                                                    //  segments and partial slots must number < 2^31, checked by the builder)
  p.T = (uint32_t)std::max<uint64_t>(kn.tile_bytes / row_bytes, 1);
  p.tiles = (rows_oth + p.T - 1) / p.T;
  if (p.tiles < 2 || p.tiles > 65534) return p;
  if (kn.tile_mode == 2 && (uint64_t)rows_oth * row_bytes < 2 * kn.tile_bytes + kn.tile_bytes / 2) return p;
  // a gathered matrix of a few tiles is already served largely from L2 when the ratings are skewed (the popular
  // rows stay resident): regrouping then pays only for rows that meet a tile many times (size sweep, m = 20 000:
  // four tiles, user pass 3.19 ms row-major, 3.64 ms with runs of 16)
  // ... and a run is worth its fixed work from two batches on: a batch is 64 / G nonzeros (K = 50: G = 4, sixteen
  // per batch -- with runs of 16 its ten-tile user side went 2.31 -> 2.68 ms)
  // Round 5: with one wave per workgroup on a tiled side (Knobs::phi_wg) a run costs less, and the bar of 16 came down
  // to 12 where a batch holds eight nonzeros or fewer (C2 8.42 -> 8.34 ms, a C3 shard 24.3 -> 23.9; 10 is better still at C2
  // and worse on the shard; C4 is flat from 10 to 16; K = 50's two batches of sixteen stay: 24 loses 1 %; experiments.md)
  p.min_run = kn.tile_min_run ? kn.tile_min_run                    // HPF_TILE_RUN: as given
                              : (nz_per_batch >= 16u ? 2u * nz_per_batch : 12u);
  p.light_below = (uint64_t)p.tiles * p.min_run * (p.tiles < 8 ? 4u : 1u);
  if (kn.tile_mode == 1) p.light_below = 0;                         // forced: every row is regrouped
  p.tile = true;
  return p;
}

// Room for the temporaries of the tiling (26 bytes per nonzero)?  Decided from what the handle holds and the size of the
// device (tot: its TOTAL bytes), not from the free memory of the moment: tiling changes the order of a row's
// sum, and whether a side is tiled must be a function of the job, not of what else happens to be allocated.
inline bool tiling_fits(uint32_t ld, uint32_t n_users, uint32_t n_items, uint64_t nnz, bool with_val, size_t tot)
{
  const double by = with_val ? 1.0 : 0.0;
  const double resident = 5.0 * 8.0 * (double)ld * ((double)n_users + (double)n_items)        // S, E, L, W + vectors of both sides
                        + (double)nnz * (3.0 * (4.0 + by));                                  // CSR, CSC and the other side's tiled copy
  return !(resident + (double)nnz * (26.0 + 4.0 + by) + (double)(1ull << 30) > 0.9 * (double)tot);
}

// A tiled side's segments are sorted by key: key 0 the row-major rest, key t the tile t - 1.  fs[k] = the first segment of
// key k, TILE_NO_SEG where it has none; a key ends where the next one that is present begins
constexpr uint32_t TILE_NO_SEG = 0xffffffffu;
inline uint32_t tile_key_end(const std::vector<uint32_t> &fs, uint32_t nseg, uint32_t k)
{
  for (uint32_t j = k + 1; j < (uint32_t)fs.size(); ++j) if (fs[j] != TILE_NO_SEG) return fs[j];
  return nseg;
}
// end of the row-major rest: the first tiled segment (nseg where there is none); 0 without a rest
inline uint32_t tile_rest_end(const std::vector<uint32_t> &fs, uint32_t nseg) { return fs[0] != TILE_NO_SEG ? tile_key_end(fs, nseg, 0) : 0u; }

struct TileChunk { uint32_t x, y; };          // segments [x, y) of one workgroup: the uint2 the pass reads; {0, 0} = none
struct TileQueuePlan {
  std::vector<TileChunk> chunks;              // chunks[j * 8 + x]: the j-th workgroup of XCD x's queue
  uint32_t chunk_segs = 0;                    // segments per chunk of a tile (hpf_work_info.tile_chunk_*)
  bool ok = false;                            // false: no list (no segment at all, or too long for a launch even so)
};

// Where every segment of a tiled pass runs.
//   fs, nseg   the first segment per key (tiles + 1 keys) and the number of segments
//   rest_nnz   nonzeros in front of the first tiled segment (its Seg::start; all of them where nothing is tiled)
//   wg         threads per workgroup of the pass; max_wgs the workgroups a launch holds (2^28 / wg)
// Chunks: eight queues, one per XCD (workgroup b runs on XCD b % 8).  The first 8 * floor(t / 8) of the t tiles
// that hold segments go WHOLE to the queue with the least work so far (a tile's segments stay together and in order:
// its rows are fetched into one L2, once); the remaining t mod 8 tiles level the queues: their segments are poured, in
// order, into the queues up to the common fill mark, so that a levelling tile is shared by two or three XCDs instead of
// all eight and every queue ends at the same count (round 5; until round 4 EVERY tile was cut eight ways below 32
// tiles, so that each XCD fetched every tile: an eighth of C4 -- 22 tiles of users -- ran its item pass in 1.36 ms,
// now 1.10; 9 and 12 tiles: -4 %; from 32 tiles on nothing changes).  Below tile_split_below = 8 tiles the old rule
// stays (HPF_TILE_SPLIT_BELOW=N: for fewer than N tiles).  The row-major rest (key 0) is cut eight ways.
inline TileQueuePlan plan_tile_queues(const std::vector<uint32_t> &fs, uint32_t nseg, uint32_t tiles, uint64_t rest_nnz, uint32_t wg,
                                      size_t max_wgs, const Knobs &kn)
{
  TileQueuePlan out;
  const uint32_t nkeys = tiles + 1;
  std::vector<std::pair<uint32_t, uint32_t>> q[8], qt[8];
  uint64_t load[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  auto key_end = [&](uint32_t k) { return tile_key_end(fs, nseg, k); };
  uint64_t tiled_segs = 0;
  uint32_t tiles_present = 0;
  for (uint32_t k = 1; k < nkeys; ++k) if (fs[k] != TILE_NO_SEG) { tiles_present++; tiled_segs += key_end(k) - fs[k]; }
  const bool old_rule = tiles < kn.tile_split_below;
  const uint32_t whole_tiles = old_rule ? 0u : (tiles_present / 8u) * 8u;
  uint32_t seen = 0;
  int fill = 0;                                                  // the queue the levelling tiles are being poured into
  const uint64_t mark = (tiled_segs + 7) / 8;                    // the common fill mark
  for (uint32_t k = 1; k < nkeys; ++k) {
    if (fs[k] == TILE_NO_SEG) continue;
    const uint32_t a0 = fs[k], a1 = key_end(k);
    if (seen++ < whole_tiles) {
      int best = 0;
      for (int x = 1; x < 8; ++x) if (load[x] < load[best]) best = x;
      qt[best].push_back({a0, a1}); load[best] += a1 - a0;
      continue;
    }
    if (old_rule) {
      const uint64_t n = a1 - a0;
      for (int x = 0; x < 8; ++x) {
        const uint32_t lo = a0 + (uint32_t)(n * x / 8), hi = a0 + (uint32_t)(n * (x + 1) / 8);
        if (hi > lo) { qt[x].push_back({lo, hi}); load[x] += hi - lo; }
      }
      continue;
    }
    for (uint32_t p0 = a0; p0 < a1;) {
      while (fill < 7 && load[fill] >= mark) ++fill;
      const uint64_t room = fill < 7 ? mark - load[fill] : (uint64_t)(a1 - p0);
      const uint32_t take = (uint32_t)std::min<uint64_t>(room, a1 - p0);
      qt[fill].push_back({p0, p0 + take}); load[fill] += take;
      p0 += take;
    }
  }
  // the row-major rest: an eighth per queue.  tile_order 0: in front of the tiles; 1: in front on the even
  // XCDs, behind on the odd ones (half the chip pulls over the fabric while the other half runs from L2);
  // 2: dealt between the tiles in equal pieces
  const uint32_t c0 = fs[0] != TILE_NO_SEG ? fs[0] : 0u, c1 = fs[0] != TILE_NO_SEG ? key_end(0) : 0u;
  for (int x = 0; x < 8; ++x) {
    const uint64_t n = c1 - c0;
    const uint32_t lo = c0 + (uint32_t)(n * x / 8), hi = c0 + (uint32_t)(n * (x + 1) / 8);
    const bool front = kn.tile_order == 0 || (kn.tile_order == 1 && (x & 1) == 0);
    if (kn.tile_order == 2 && !qt[x].empty()) {
      const uint64_t nt = qt[x].size(), nc = hi - lo;
      for (uint64_t t = 0; t < nt; ++t) {
        const uint32_t l2 = lo + (uint32_t)(nc * t / nt), h2 = lo + (uint32_t)(nc * (t + 1) / nt);
        if (h2 > l2) q[x].push_back({l2, h2});
        q[x].push_back(qt[x][t]);
      }
      continue;
    }
    if (front && hi > lo) q[x].push_back({lo, hi});
    for (auto &rg : qt[x]) q[x].push_back(rg);
    if (!front && hi > lo) q[x].push_back({lo, hi});
  }
  // a launch holds fewer than 2^32 work-items (the AQL packet counts them in 32 bits): at most 2^28 / wg workgroups
  // (2^20 of four waves, 2^22 of one -- round 5 kept 2^20 for the one-wave groups as well, and the longest lists, whole
  // C3 or C5 on one GPU, got chunks of 8-16 segments instead of two), so a list too long for chunks of
  // tile_chunk segments gets longer chunks; hpf_work_info.tile_chunk_user / _item say what was used
  uint32_t CH = kn.tile_chunk ? kn.tile_chunk : 2 * (wg / 64);      // two segments per wave
  // the row-major segments of a side with short rows (users: a few batches each) come in chunks of ~4096 nonzeros:
  // a workgroup that lives for two 40-nonzero rows costs more to dispatch than to run (K = 50, 10^6 light users
  // in chunks of 8: user pass 2.27 -> 2.54 ms)
  uint32_t CHc = CH;
  if (c1 > c0) {
    const uint64_t avg = std::max<uint64_t>(rest_nnz / (c1 - c0), 1);
    CHc = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(4096ull * wg / 256 / avg, CH), 512);
  }
  auto chunk_of = [&](const std::pair<uint32_t, uint32_t> &rg, uint32_t ch, uint32_t chc) { return (rg.first >= c0 && rg.second <= c1) ? chc : ch; };
  for (;; CH *= 2, CHc *= 2) {
    size_t worst = 0;
    for (int x = 0; x < 8; ++x) {
      size_t c = 0;
      for (auto &rg : q[x]) { const uint32_t ch = chunk_of(rg, CH, CHc); c += (rg.second - rg.first + ch - 1) / ch; }
      worst = std::max(worst, c);
    }
    if (worst * 8 <= max_wgs || CH >= (1u << 30)) break;
  }
  std::vector<TileChunk> qc[8];
  size_t longest = 0;
  for (int x = 0; x < 8; ++x) {
    for (auto &rg : q[x]) {
      const uint32_t ch = chunk_of(rg, CH, CHc);
      for (uint32_t p0 = rg.first; p0 < rg.second; p0 += std::min(ch, rg.second - p0)) qc[x].push_back({p0, p0 + std::min(ch, rg.second - p0)});
    }
    longest = std::max(longest, qc[x].size());
  }
  out.chunk_segs = CH;
  if (longest == 0 || longest * 8 > max_wgs) return out;
  out.chunks.assign(longest * 8, TileChunk{0u, 0u});
  for (int x = 0; x < 8; ++x) for (size_t j = 0; j < qc[x].size(); ++j) out.chunks[j * 8 + x] = qc[x][j];
  out.ok = true;
  return out;
}

// ---- the plan ---------------------------------------------------------------------------------------------------------
struct Row { uint32_t G, E, L, row_bytes, lgG; };     // PackedRow of hpf_kernels.hpp: G lanes x L 16-byte pieces, E elements per lane

struct Plan {
  uint32_t ld = 0;                      // row stride of every device matrix, columns
  bool w32 = false;                     // W stored as float (hpf_config.w_storage = 1)
  int wl = WL_PLAIN;                    // layout of W rows: plain, WL_P59 (lossless packing, default where it shortens
                                        // the row), WL_F48 (w_storage = 2) or WL_F64 (w_storage = 3, or after a fall-back); rows in pieces: phiR = 16-byte pieces per lane
  Row pk = {0, 0, 0, 0, 0};
  Row pks = {0, 0, 0, 0, 0};            // plain-fp64 rows in pieces for the same columns (codec_f64): what the rows become when p59
                                        // cannot hold a state (recover_flush)
  int phiG = 0, phiR = 0, phiV = 0, swG = 0, swR = 0;
  int sw_mode = SW_PLAIN;               // how the sweep writes W (row_sweep_kernel MODE)

  // p59 rows -> plain doubles in the same shape (codec_f64): what a handle falls back to, and what w_storage = 3 asks for
  Plan as_plain_doubles() const { Plan p = *this; p.wl = WL_F64; p.pk = pks; p.phiR = (int)pks.L; p.sw_mode = SW_F64; return p; }
};

// pick (G,R) with G*R*V >= ld, R <= 8.  Cost = padded row length, +20 % when a lane
// group spans less than one 128-byte line per load although the row is at least two
// lines long (K=50: (4,7,2) loses to the wider, more padded (8,4,2): user pass 2.58
// vs 2.29 ms).  Ties (row lengths that several shapes cover exactly, e.g. K = 64,
// 128) are decided by what the K sweep on MI355X showed: keep
// 2..7 loads per lane in flight (R = 1 has no ILP: K=64 user pass 3.30 ms vs 2.35 ms
// at R = 4; R = 8 costs registers), span a line, and among equals be narrow (more
// nonzeros per wave).
inline bool choose_cfg(uint32_t ld, int V, int *G, int *R, long *cost)
{
  int bestG = 0, bestR = 0; long bestc = -1; int bestp = 0;
  for (int g : {4, 8, 16, 32, 64}) {
    const int r = (int)((ld + (uint32_t)(g * V) - 1) / (uint32_t)(g * V));
    if (r < 1 || r > 8) continue;
    const bool narrow = g * V * 8 < 128;
    const long c = (long)g * r * V * ((narrow && ld * 8 >= 256) ? 12 : 10);
    const int p = (r == 1 ? 3 : 0) + (r > 7 ? 2 : 0) + (narrow ? 1 : 0);
    if (bestc < 0 || c < bestc || (c == bestc && p < bestp)) { bestc = c; bestG = g; bestR = r; bestp = p; }
  }
  if (bestc < 0) return false;
  *G = bestG; *R = bestR; *cost = bestc;
  return true;
}

// Kernel shape and row stride for C = K + 2*bias live columns.  The phi pass gives G lanes to a nonzero, each with R loads
// of V elements; the row stride of every device matrix is EXACTLY ld = G*R*V elements
// (round 3): the live columns K + 2*bias are padded with zero columns, so the kernels carry
// no column test (K=100: 800-byte rows become 896 = seven whole 128-byte lines, the
// number of lines a gather of an unaligned 800-byte row touched anyway).
inline int plan_shapes(uint32_t C, uint32_t w_storage, const Knobs &kn, Plan *out)
{
  if (C < 1 || C > HPF_MAX_COLUMNS || w_storage > 3) return HPF_ERR_UNSUPPORTED;
  Plan p;
  p.w32 = w_storage == 1;          // only ever chosen by the caller's hpf_config
  // 16-byte loads when they pad no worse than 8-byte ones (measured: C2
  // phi_user 4.36 ms vs 4.52 ms).  Elements per load: doubles 1|2, floats 2|4.
  bool phi_cfg_forced = false;
  const int Vs = p.w32 ? 2 : 1, Vl = 2 * Vs;
  int g1 = 0, r1 = 0, g2 = 0, r2 = 0;
  long w1 = 1L << 40, w2 = 1L << 40;            // stay so where no shape exists
  const bool ok1 = choose_cfg(C, Vs, &g1, &r1, &w1), ok2 = choose_cfg(C, Vl, &g2, &r2, &w2);
  if (!ok1 && !ok2) return HPF_ERR_UNSUPPORTED;
  if (w2 <= w1) { p.phiG = g2; p.phiR = r2; p.phiV = Vl; }
  else { p.phiG = g1; p.phiR = r1; p.phiV = Vs; }
  if (p.w32) {
    // f32 rows are half as long: measured at C2 (K=100) the passes want 256
    // contiguous bytes per nonzero-group -- (G,R,V) = (16,2,4): 3.7 + 3.4 ms
    // against 5.0 + 3.8 ms for (8,4,4) and 9.8 + 5.3 ms for the least-padding (4,7,4)
    const int g = C > 512 ? 32 : C > 32 ? 16 : C > 16 ? 8 : 4;
    p.phiG = g; p.phiV = 4; p.phiR = (int)((C + (uint32_t)(4 * g) - 1) / (uint32_t)(4 * g));
  }
  {
    const int g = kn.phi_cfg[0], r = kn.phi_cfg[1], v = kn.phi_cfg[2];          // "G,R,V"
    if (has_phi(p.w32, g, r, v) && (uint32_t)(g * r * v) >= C && g * r * v <= 2048) {
      p.phiG = g; p.phiR = r; p.phiV = v;
      phi_cfg_forced = true;                             // an explicit plain shape: no packing
    }
  }
  p.ld = (uint32_t)(p.phiG * p.phiR * p.phiV);
  // Packed rows: G lanes x L 16-byte pieces, E elements per lane (p59: 128L/59, f48: 8L/3); fewest
  // row bytes G*L*16 with G*E >= C.  w_storage 0 takes the lossless p59 packing when it saves
  // at least one 128-byte line per row against the plain fp64 row (K = 100: 6 instead of 7,
  // K = 50: 3 instead of 4 -- measured on a C5 shard: 65.6 -> 51.7 ms); 2 asks for f48; 3 keeps
  // plain rows.  HPF_W_PACK=1 (experimental) packs whenever a shape exists.
  // w_storage 3 asks for plain doubles: where the default would pack, the rows keep the packed SHAPE (lanes per nonzero,
  // columns, row stride of S) and hold plain doubles in its pieces (WL_F64) -- the layout a packed handle falls back to
  // when a state turns up that p59 cannot hold, so that the two give the same bits
  const int want = w_storage == 2 ? WL_F48 : w_storage == 1 ? WL_PLAIN : WL_P59;
  if (want != WL_PLAIN && !(phi_cfg_forced && want == WL_P59)) {
    auto per_lane = [&](int l) { return want == WL_F48 ? (8 * l) / 3 : (128 * l) / 59; };
    long bestb = -1; int bg = 0, bl = 0;
    for (int g : {8, 16, 32, 64, 4})
      for (int l = 1; l <= 8; ++l) {
        if ((uint32_t)(g * per_lane(l)) < C) continue;
        const long b = (long)g * l * 16;
        if (bestb < 0 || b < bestb) { bestb = b; bg = g; bl = l; }
        break;                                                                   // larger l only adds bytes
      }
    const long plain_lines = ((long)p.ld * 8 + 127) / 128, packed_lines = (bestb + 127) / 128;
    bool take = bestb > 0 && (want == WL_F48 || kn.w_pack || packed_lines < plain_lines);
    if (want == WL_F48 && bestb < 0) return HPF_ERR_UNSUPPORTED;
    const int e = per_lane(bl);
    // the sweep must have a shape for the packed stride too
    if (take) {
      const uint32_t pld = (uint32_t)(bg * e);
      bool fits = false;
      if (want == WL_F48) for (int g : {64, 32, 16, 8, 4}) { const uint32_t r = (pld + (uint32_t)g - 1) / (uint32_t)g; fits |= r >= 1 && r <= (g == 64 ? 16u : 8u); }
      else fits = bg <= 32 || e <= 16;      // p59: groups of twice the pass's lanes (<= 9 slots), or 64 lanes with a slot per element
      if (!fits && want == WL_F48) return HPF_ERR_UNSUPPORTED;
      if (!fits) take = false;                         // e.g. 961..1024 columns: 1088 packed columns have none; rows stay plain
    }
    if (take) {
      p.wl = want;
      p.phiG = bg; p.phiR = bl; p.phiV = 0;
      p.pk.G = (uint32_t)bg; p.pk.L = (uint32_t)bl; p.pk.E = (uint32_t)e; p.pk.row_bytes = (uint32_t)(bg * bl) * 16u;
      p.pk.lgG = 0; while ((1u << p.pk.lgG) < (uint32_t)bg) ++p.pk.lgG;
      p.ld = (uint32_t)(bg * e);
      if (want == WL_P59) {
        const uint32_t ls = ((uint32_t)e + 1u) / 2u;
        p.pks = p.pk; p.pks.L = ls; p.pks.E = 2u * ls; p.pks.row_bytes = (uint32_t)bg * ls * 16u;
      }
    }
  }
  // The row sweep gives G' lanes to a row with R' columns each.  Plain rows: G'*R' == ld exactly.  p59 rows (and the plain
  // doubles in their shape): G' is TWICE the pass's lanes -- the two lanes that share a packed lane swap their halves and
  // build the row in registers (row_sweep_kernel, SW_REG_P59) -- or the pass's 64.  48-bit rows: G'*R' >= ld, built in LDS.
  if (p.wl == WL_P59) {
    const uint32_t ep = p.ld / (uint32_t)p.phiG;                 // elements per lane of the p59 shape
    if (p.phiG <= 32) { p.swG = 2 * p.phiG; p.swR = (int)((ep + 1) / 2); p.sw_mode = SW_REG_P59; }
    else { p.swG = 64; p.swR = (int)ep; p.sw_mode = SW_LDS_P59; }
    if (w_storage == 3) p = p.as_plain_doubles();
  } else {
    p.sw_mode = p.wl == WL_F48 ? SW_LDS_F48 : SW_PLAIN;
    int best = 1 << 30;
    for (int g : {64, 32, 16, 8, 4}) {
      if (p.wl == WL_PLAIN && p.ld % (uint32_t)g) continue;
      const int r = (int)((p.ld + (uint32_t)g - 1) / (uint32_t)g);
      if (r < 1 || r > (g == 64 ? 16 : 8)) continue;
      const int pen = (r == 1 ? 3 : 0) + (r > 7 ? 2 : 0) + (g * 8 < 128 ? 1 : 0);   // same preferences as round 1's K sweep
      if (pen < best || (pen == best && g < p.swG)) { best = pen; p.swG = g; p.swR = r; }
    }
    if (!p.swG) return HPF_ERR_UNSUPPORTED;
    const int g = kn.sweep_cfg[0], r = kn.sweep_cfg[1];
    if (p.wl == WL_PLAIN && has_sweep(SW_PLAIN, g, r) && (uint32_t)(g * r) == p.ld) { p.swG = g; p.swR = r; }
  }
  *out = p;
  return HPF_OK;
}

// ---- the fused sweep epilogue: which (side, layout, shape) runs it --------------------------------------------------------
// The USER side of a handle whose rows are p59 (a handle that has fallen back to plain doubles, or was created with them,
// runs the two kernels apart: the W-only repeat of recover_flush and w_storage = 3 must stay one arithmetic).  The item side
// stays unfused: its single-segment rows are worth at most 0.05 ms of C2's 8.2 and its pass is the one at the HBM limit.
// Among the shapes with an instance the library takes the fused route only where it was measured against the unfused build
// (profiles/r10/experiments.md 3): (8, 6) -- 81..104 columns, K = 100 -- gains 0.12-0.15 ms of C2's 8.2 and is level on a C3
// shard; (4, 6) -- K = 50, a C5 shard -- LOSES 3.7 % (its pass already carries unhidden arithmetic: the epilogue's ~90 fp64
// instructions per element weigh twice as much against rows half as long) and stays unfused; the other shapes have not been
// measured and stay unfused until they are.
constexpr bool fused_pays(int G, int L) { return G == 8 && L == 6; }
inline bool fused_sweep(const Plan &p, const Knobs &kn, bool item_side)
{
  return kn.fused_sweep != 0 && !item_side && has_phi_fused(p.wl, p.phiG, p.phiR) && has_sums(p.sw_mode, p.swG, p.swR) &&
         (kn.fused_sweep == 2 || fused_pays(p.phiG, p.phiR));
}

// ---- the call order of an iteration's steps ------------------------------------------------------------------------------
// An iteration is four steps on one stream; the exported calls are compositions of them:
//   hpf_iterate_local_items  ITEMS_PASS                     hpf_iterate_local_sweep  USERS_SWEEP
//   hpf_iterate_local_phi    ITEMS_PASS USERS_PASS          hpf_iterate_local_users  USERS_PASS USERS_SWEEP
//   hpf_iterate_local        ITEMS_PASS USERS_PASS USERS_SWEEP                       hpf_iterate_global  ITEMS_SWEEP
// so an iteration is local_items | local_users | global, local_phi | local_sweep | global or local | global.
// phase: 0 idle | 1 items pass done | 2 users pass done | 3 user sweep done.  Every other step follows its predecessor only;
// the items pass may be called in any phase (an iteration that was begun and not finished is begun again).
enum Step : int { ITEMS_PASS = 0, USERS_PASS = 1, USERS_SWEEP = 2, ITEMS_SWEEP = 3 };
// the phase after `step` is on the stream, -1: a call-order error
constexpr int next_phase(int phase, Step step)
{
  constexpr int next[4][4] = {          // [phase][step]
    {1, -1, -1, -1},
    {1, 2, -1, -1},
    {1, -1, 3, -1},
    {1, -1, -1, 0}};
  return phase < 0 || phase > 3 || step < ITEMS_PASS || step > ITEMS_SWEEP ? -1 : next[phase][step];
}

}  // namespace hpf_plan
