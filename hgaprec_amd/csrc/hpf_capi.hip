// hpf_capi.hip -- implementation of include/hpf.h (libhpf_hip.so).
// Host orchestration of the gfx950 kernels in hpf_kernels.hpp: device state,
// CSR -> (CSR, CSC, segment lists), the per-iteration launch sequence, the
// exchange buffer for the multi-GPU all-reduce, hipEvent timing.
//
// Device layout (all fp64; row stride ld = G*R*V of the phi kernel shape >= K + 2*bias,
// the columns beyond the live ones hold zeros):
//   user side  theta: S,E,L,W [n x ld]   column K   = user bias (thetabias)
//                                         column K+1 = 0 ("junk": Elog 0)
//   item side  beta : S,E,L,W [m x ld]   column K   = junk, column K+1 = item bias
//   xi/eta     prior_E[rows] (+ prior_used, prior_rate for export)
//   exchange   [m x ld | ld]: item S rows followed by sum_u E[theta_u,:]
#include "../../include/hpf.h"
#include "hpf_kernels.hpp"
#include "hpf_build.hpp"
#include "hpf_plan.hpp"
#include "hpf_lazy.hpp"

#include <dlfcn.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <utility>
#include <vector>

using namespace hpf;
using hpf_plan::Knobs;
using hpf_plan::Plan;

// hpf_plan.hpp spells the layout codes, the sweep modes and the packed row on its own (it includes no HIP header)
static_assert(hpf_plan::WL_PLAIN == WL_PLAIN && hpf_plan::WL_F48 == WL_F48 && hpf_plan::WL_P59 == WL_P59 && hpf_plan::WL_F64 == WL_F64, "layout codes");
static_assert(hpf_plan::SW_PLAIN == SW_PLAIN && hpf_plan::SW_LDS_F48 == SW_LDS_F48 && hpf_plan::SW_LDS_P59 == SW_LDS_P59 &&
              hpf_plan::SW_F64 == SW_F64 && hpf_plan::SW_REG_P59 == SW_REG_P59, "sweep modes");
static_assert(sizeof(hpf_plan::Row) == sizeof(PackedRow) && offsetof(hpf_plan::Row, G) == offsetof(PackedRow, G) && offsetof(hpf_plan::Row, E) == offsetof(PackedRow, E) &&
              offsetof(hpf_plan::Row, L) == offsetof(PackedRow, L) && offsetof(hpf_plan::Row, row_bytes) == offsetof(PackedRow, row_bytes) && offsetof(hpf_plan::Row, lgG) == offsetof(PackedRow, lgG), "packed row");

namespace {

PackedRow packed_row(const hpf_plan::Row &r) { return {r.G, r.E, r.L, r.row_bytes, r.lgG}; }

struct Side {
  uint32_t rows = 0;
  double *S = nullptr, *E = nullptr, *L = nullptr;
  void *W = nullptr;                   // [rows x ld] double, or float in the f32-storage mode; rows of pieces: [rows x pk.row_bytes]
  double *prior_E = nullptr, *prior_used = nullptr, *prior_rate = nullptr;
  double *prior_elog = nullptr, *prior_elog_used = nullptr;   // Elog xi/eta now / as used by the last rate
  double *colsum = nullptr;       // [ld] sum over this side's rows of E
  double *colsum_used = nullptr;  // [ld] other side's colsum used in the last rate
  double *colsum_part = nullptr;  // [sweep_blocks x ld]
  double *rate_set = nullptr;     // rate handed in by hpf_set_state (export before iter 0)
  size_t  rate_set_count = 0;
  double *prior_shape_set = nullptr, *prior_elog_set = nullptr;  // xi/eta extras
  // phi pass work list: segments of <= seg_max nonzeros of one row; rows of several
  // segments ("long") have their segment sums combined by a second kernel
  Seg *segs = nullptr; uint32_t nseg = 0;
  LongRow *longrows = nullptr; uint32_t nlong = 0;
  uint32_t nlong_wave = 0;             // the first nlong_wave of them: a wave each; the rest (a tiled side's rows with more than 64 partials) a workgroup each
  double *partial = nullptr; uint32_t npartial = 0;
  // rows with more than HUGE_SLOTS segments are combined in two levels so that
  // no wave walks a chain of thousands of partials: groups of GROUP_SLOTS
  // consecutive partials are summed into partial2 (grouprows), then the group
  // sums into S (hugerows, reading partial2)
  LongRow *grouprows = nullptr; uint32_t ngroup = 0;
  LongRow *hugerows = nullptr; uint32_t nhuge = 0;
  double *partial2 = nullptr; uint32_t npartial2 = 0;
  uint32_t *idx = nullptr; uint8_t *val = nullptr;
  // tiled pass (hpf_build.hpp): the nonzeros regrouped by (tile of the gathered row, owner row); segs then
  // index p_idx / p_val, and workgroup b takes the segments chunks[b]
  uint32_t *p_idx = nullptr; uint8_t *p_val = nullptr;
  uint2 *chunks = nullptr; uint32_t nchunk_blocks = 0;
  uint32_t tiles = 0, tile_rows = 0, chunk_segs = 0; uint64_t tiled_nnz = 0, light_below = 0;
  const uint32_t *pass_idx() const { return p_idx ? p_idx : idx; }
  const uint8_t *pass_val() const { return p_idx ? p_val : val; }
  int32_t bias_col = -1, junk_col = -1;
  double bias_rate_add = 0.0;
  uint32_t sweep_blocks = 0;
  // fused sweep epilogue (hpf_plan::fused_sweep): this side's pass writes W of the rows that are one segment -- a bit per row in
  // row_done, set with the work lists -- and its sweep is row_sums_kernel
  bool fused = false;
  uint32_t *row_done = nullptr;
};

}  // namespace

// the shapes (ld, wl, pk, phiG ...) are the Plan, the tuning values (seg_max, tile_mode ...) the Knobs: hpf_plan.hpp
struct hpf_handle : Plan, Knobs {
  hpf_config cfg;
  uint32_t K = 0, C = 0;
  uint32_t fallbacks = 0;               // automatic moves from p59 rows to plain fp64 rows so far
  uint32_t notes = 0;                   // hpf_work_info.notes
  uint64_t iters_counted = 0;           // iterations launched since the device counter flags[1] was last reset
  bool in_recovery = false;
  uint32_t *flags = nullptr;            // device words: [0] bit 0 = a softmax denominator underflowed, bit 1 = p59 flushed an entry,
                                        // bit 2 = passes and sweeps are skipping; [1] = iterations begun (PhiArgs::flags)
  hipStream_t stream = nullptr;
  bool own_stream = false;
  Side u, it;
  hpf_lazy::State lz;                   // what is pending on S, E, Elog, W and the start sums: hpf_lazy.hpp
  int side_of(const Side &s) const { return &s == &it ? hpf_lazy::ITEMS : hpf_lazy::USERS; }
  double *exch = nullptr; size_t exch_count = 0; bool exch_external = false;
  // -novb with -bias and without -hier (vb_bias()'s else-branch, hgaprec.cc:1276-1297): the
  // item rate is built from the sum_u E[theta] of BEFORE this iteration's user sweep
  bool jacobi = false;
  double *u_colsum_prev = nullptr;      // [ld]
  double *logfact = nullptr;
  int64_t *rowptr_dev = nullptr;   // user CSR row pointers (ranking mask, CSC build)
  int64_t *colptr_dev = nullptr;   // item-major (CSC) column pointers, built on device
  uint64_t nnz = 0;
  // pinned double buffer for host <-> device hand-over (hpf_upload_csr, hpf_set_state,
  // hpf_get_state): pageable hipMemcpy runs at ~4 GB/s, the staged pipeline at the
  // host memcpy rate.  HPF_H2D=plain|staged|register picks the carrier.
  void *stage[2] = {nullptr, nullptr};
  hipEvent_t stage_ev[2] = {nullptr, nullptr};
  size_t stage_bytes = 0;
  bool have_csr = false;
  uint32_t iterations = 0;
  uint32_t wg_of(bool tiled) const { return wl == WL_PLAIN ? 256u : phi_wg ? phi_wg : (tiled ? 64u : 256u); }   // (plain rows: phi_pass_kernel, always 256)
  uint32_t nz_per_batch() const { return phiG > 0 ? 64u / (uint32_t)phiG : 8u; }
  static constexpr uint32_t RING = 64;          // timed iterations kept
  hipEvent_t evr[RING][8] = {};
  hipEvent_t *ev = evr[0];                      // events of the iteration in flight
  uint32_t ev_count = 0;                        // iterations recorded so far
  void *comm = nullptr;                 // ncclComm_t once hpf_comm_init succeeded
  // the item part of the exchange buffer is reduced on its own stream so that
  // the user-side half of the iteration overlaps it (hpf_allreduce_items_begin)
  hipStream_t comm_stream = nullptr;
  hipEvent_t ev_ready = nullptr, ev_reduced = nullptr;
  bool items_reduce_pending = false;
  // hipGraph replay of one whole iteration for launch-bound problems (hpf_iterate,
  // n_ranks == 1).  HPF_GRAPH=0/1 forces it off/on; default: on when the phi passes
  // are short enough that the ~10 launches per iteration dominate (nnz <= graph_nnz_max).
  uint64_t graph_nnz_max = 4u << 20;
  hipGraphExec_t graph_exec = nullptr;
  // the same for a rank of several (round 6): the iteration is cut by its two collectives, so it is THREE graphs -- the item
  // pass | the user pass + the user sweep | the item sweep -- replayed by hpf_iterate_local_items, hpf_iterate_local_users and
  // hpf_iterate_global (and so by hpf_iterate with a communicator) around whatever exchange the caller or the library runs
  hipGraphExec_t split_exec[3] = {nullptr, nullptr, nullptr};
  int phase = 0;                        // 0 idle | 1 items pass done | 2 users pass done | 3 user sweep done (hpf_plan::next_phase)
  bool replaying = false;               // the iteration in flight runs its pieces as graph replays: set by its item step, cleared by its item sweep
  bool ring_graphed[RING] = {};         // slot was a graph replay: only events 0 and 6 exist
  // held-out sets bound once (hpf_heldout_bind): indices and ratings on the device, the per-pair values in a kept
  // page-locked buffer the DMA writes directly
  struct HeldSet { uint32_t *du = nullptr, *di = nullptr; int32_t *dy = nullptr; double *dout = nullptr, *hout = nullptr; size_t cnt = 0; bool bound = false; };
  HeldSet held[HPF_HELDOUT_SLOTS];
  hipEvent_t held_ev[8] = {};
  std::string err;
};

// ---- RCCL, loaded at run time (one process per GPU; the library must not
// depend on librccl at link time: single-GPU users never load it) -------------
namespace {
struct IdByValue { char internal[HPF_COMM_ID_BYTES]; };   // layout of ncclUniqueId (rccl.h:43)
struct RcclApi {
  void *lib = nullptr;
  int (*GetUniqueId)(void *) = nullptr;
  int (*CommInitRank)(void **, int, IdByValue /* ncclUniqueId by value */, int) = nullptr;
  int (*AllReduce)(const void *, void *, size_t, int, int, void *, void *) = nullptr;
  int (*CommDestroy)(void *) = nullptr;
  int (*CommGetAsyncError)(void *, int *) = nullptr;
  const char *(*GetErrorString)(int) = nullptr;
};
RcclApi g_rccl;

const char *load_rccl()
{
  if (g_rccl.lib) return nullptr;
  // candidates, in order: HPF_RCCL_LIB (a full path: the operator's word wins), the soname as the loader finds it,
  // $TORCH_LIB_DIR/librccl.so (a box whose only copy ships inside a torch wheel: the C++ CLI has no torch to have
  // mapped it already), $ROCM_PATH/lib, /opt/rocm/lib
  std::vector<std::string> names;
  if (const char *e = getenv("HPF_RCCL_LIB")) if (*e) names.push_back(e);
  names.push_back("librccl.so.1");
  names.push_back("librccl.so");
  if (const char *e = getenv("TORCH_LIB_DIR")) if (*e) { names.push_back(std::string(e) + "/librccl.so.1"); names.push_back(std::string(e) + "/librccl.so"); }
  if (const char *e = getenv("ROCM_PATH")) if (*e) { names.push_back(std::string(e) + "/lib/librccl.so.1"); names.push_back(std::string(e) + "/lib/librccl.so"); }
  names.push_back("/opt/rocm/lib/librccl.so.1");
  names.push_back("/opt/rocm/lib/librccl.so");
  void *lib = nullptr;
  // a copy this process has already mapped (a host application's, torch's) is THE copy:
  // two RCCL builds in one process do not survive each other's teardown
  for (const std::string &n : names) if ((lib = dlopen(n.c_str(), RTLD_NOW | RTLD_GLOBAL | RTLD_NOLOAD))) break;
  if (!lib) for (const std::string &n : names) if ((lib = dlopen(n.c_str(), RTLD_NOW | RTLD_GLOBAL))) break;
  if (!lib) {
    static std::string why;
    const char *de = dlerror();
    why = std::string("cannot dlopen librccl.so (set HPF_RCCL_LIB to its full path, or TORCH_LIB_DIR to a torch/lib that holds it)") +
          (de ? std::string(": ") + de : std::string());
    return why.c_str();
  }
  RcclApi a; a.lib = lib;
  a.GetUniqueId = (int (*)(void *))dlsym(lib, "ncclGetUniqueId");
  a.CommInitRank = (int (*)(void **, int, IdByValue, int))dlsym(lib, "ncclCommInitRank");
  a.AllReduce = (int (*)(const void *, void *, size_t, int, int, void *, void *))dlsym(lib, "ncclAllReduce");
  a.CommDestroy = (int (*)(void *))dlsym(lib, "ncclCommDestroy");
  a.GetErrorString = (const char *(*)(int))dlsym(lib, "ncclGetErrorString");
  a.CommGetAsyncError = (int (*)(void *, int *))dlsym(lib, "ncclCommGetAsyncError");   // optional
  if (!a.GetUniqueId || !a.CommInitRank || !a.AllReduce || !a.CommDestroy || !a.GetErrorString)
    return "librccl.so lacks an expected symbol";
  g_rccl = a;
  return nullptr;
}
}  // namespace

namespace {

// an asynchronous RCCL failure (a peer died, a link error) surfaces here, once
// per iteration, instead of as a hang in a later collective
int check_comm_async(hpf_handle *h);

#define HIPCHK(h, expr)                                                        \
  do {                                                                         \
    hipError_t e_ = (expr);                                                    \
    if (e_ != hipSuccess) {                                                    \
      (h)->err = std::string(#expr) + ": " + hipGetErrorString(e_);            \
      return (e_ == hipErrorOutOfMemory) ? HPF_ERR_OOM : HPF_ERR_HIP;          \
    }                                                                          \
  } while (0)

template <typename T>
int dalloc(hpf_handle *h, T **p, size_t n)
{
  if (n == 0) n = 1;
  HIPCHK(h, hipMalloc((void **)p, n * sizeof(T)));
  HIPCHK(h, hipMemsetAsync(*p, 0, n * sizeof(T), h->stream));
  return HPF_OK;
}

void dfree(void *p) { if (p) (void)hipFree(p); }

void free_held(hpf_handle::HeldSet &hs)
{
  dfree(hs.du); dfree(hs.di); dfree(hs.dy); dfree(hs.dout);
  if (hs.hout) (void)hipHostFree(hs.hout);
  hs = hpf_handle::HeldSet();
}

void free_side(Side &s, bool S_external)
{
  if (!S_external) dfree(s.S);
  dfree(s.E); dfree(s.L); dfree(s.W);
  dfree(s.prior_E); dfree(s.prior_used); dfree(s.prior_rate);
  dfree(s.prior_elog); dfree(s.prior_elog_used);
  dfree(s.colsum_used); dfree(s.colsum_part);
  dfree(s.rate_set); dfree(s.prior_shape_set); dfree(s.prior_elog_set);
  dfree(s.segs); dfree(s.longrows); dfree(s.grouprows); dfree(s.hugerows);
  dfree(s.partial); dfree(s.partial2); dfree(s.idx); dfree(s.val);
  dfree(s.p_idx); dfree(s.p_val); dfree(s.chunks); dfree(s.row_done);
  s = Side();
}

// bytes of a side's W: plain rows of ld doubles (floats use half), or rows of 16-byte pieces; never less than one whole
// row (the packed passes read row 0 of the gathered side even for a segment without nonzeros)
size_t w_bytes(const hpf_handle *h, uint32_t rows)
{
  const size_t row = std::max<size_t>((size_t)h->ld * 8, h->wl != WL_PLAIN ? (size_t)h->pk.row_bytes : 0);
  return (size_t)std::max<uint32_t>(rows, 1u) * row;
}

// ---- kernel dispatch over the template grid -------------------------------
// The instances that exist are the ones hpf_plan.hpp's has_* predicates name: a shape they reject instantiates nothing
// and launches nothing (false), a shape they accept cannot be left out.
// pick: calls f(std::integral_constant<int, v>()) for the v among Vs that equals x; false where none does
template <int... Vs, typename F>
bool pick(int x, std::integer_sequence<int, Vs...>, F &&f) { return ((x == Vs && f(std::integral_constant<int, Vs>())) || ...); }
using Groups = std::integer_sequence<int, 4, 8, 16, 32, 64>;
using Counts = std::integer_sequence<int, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16>;
#define PICKED(x) decltype(x)::value

// how a phi pass is launched: workgroups x threads (256 = four waves that share a chunk of segments, 64 = one wave: a
// tiled side) on a stream -- handed down explicitly (until round 5 the thread count travelled in a thread_local)
struct PhiLaunch { uint32_t blocks, wg; hipStream_t st; };

// plain rows: G lanes per nonzero, R loads of V elements per lane (phi_pass_kernel, always 256 threads)
bool launch_phi(bool w32, int G, int R, int V, int side, const PhiArgs &a, const PhiLaunch &pl)
{
  return pick(w32, std::integer_sequence<int, 0, 1>(), [&](auto f32) { return pick(V, std::integer_sequence<int, 1, 2, 4>(), [&](auto v) {
    return pick(G, Groups(), [&](auto g) { return pick(R, Counts(), [&](auto r) { return pick(side & 1, std::integer_sequence<int, 0, 1>(), [&](auto sd) {
      if constexpr (hpf_plan::has_phi(PICKED(f32), PICKED(g), PICKED(r), PICKED(v))) {
        using WT = std::conditional_t<PICKED(f32) != 0, float, double>;
        hipLaunchKernelGGL((phi_pass_kernel<WT, PICKED(g), PICKED(r), PICKED(v), PICKED(sd)>), dim3(pl.blocks), dim3(256), 0, pl.st, a);
        return true;
      } else return false;
    }); }); }); }); });
}

// packed W rows: G lanes per nonzero, L 16-byte pieces per lane (phi_pass_packed_kernel)
template <template <int> class C, int WL>
bool launch_phipk(int G, int L, int side, const PhiArgs &a, const PhiLaunch &pl)
{
  return pick(G, Groups(), [&](auto g) { return pick(L, Counts(), [&](auto l) { return pick(side & 1, std::integer_sequence<int, 0, 1>(), [&](auto sd) {
    if constexpr (hpf_plan::has_phi_packed(WL, PICKED(g), PICKED(l))) {
      hipLaunchKernelGGL((phi_pass_packed_kernel<C, PICKED(g), PICKED(l), PICKED(sd)>), dim3(pl.blocks), dim3(pl.wg), 0, pl.st, a);
      return true;
    } else return false;
  }); }); });
}
// the user pass with the fused sweep epilogue (hpf_plan::fused_sweep): p59 rows, side 0
bool launch_phi_fused(int G, int L, const PhiArgs &a, const PhiLaunch &pl)
{
  return pick(G, Groups(), [&](auto g) { return pick(L, Counts(), [&](auto l) {
    if constexpr (hpf_plan::has_phi_fused(WL_P59, PICKED(g), PICKED(l))) {
      hipLaunchKernelGGL((phi_pass_fused_kernel<PICKED(g), PICKED(l), 0>), dim3(pl.blocks), dim3(pl.wg), 0, pl.st, a);
      return true;
    } else return false;
  }); });
}
bool launch_phi_packed(int wl, int G, int L, int side, const PhiArgs &a, const PhiLaunch &pl)
{
  switch (wl) {
    case WL_P59: return launch_phipk<codec_p59, WL_P59>(G, L, side, a, pl);
    case WL_F48: return launch_phipk<codec_f48, WL_F48>(G, L, side, a, pl);
    case WL_F64: return launch_phipk<codec_f64, WL_F64>(G, L, side, a, pl);
  }
  return false;
}

bool launch_gather_only(int G, int L, const PhiArgs &a, uint32_t *sink, const PhiLaunch &pl)
{
  return pick(G, Groups(), [&](auto g) { return pick(L, Counts(), [&](auto l) {
    if constexpr (hpf_plan::has_gather_only(PICKED(g), PICKED(l))) {
      hipLaunchKernelGGL((gather_only_kernel<PICKED(g), PICKED(l)>), dim3(pl.blocks), dim3(pl.wg), 0, pl.st, a, sink);
      return true;
    } else return false;
  }); });
}

// The ladders this replaced also compiled sweeps behind tests that were never true (R = 9..16 below 64 lanes, the slot counts
// p59 has no shape for): nothing launches them, they stay only so that the library's kernels are the ones it had
constexpr bool unreachable_sweep(int mode, int G, int R) { return mode != SW_LDS_P59 && (mode != SW_REG_P59 || G >= 8) && !hpf_plan::has_sweep(mode, G, R); }
bool launch_sweep(int mode, int G, int R, const SweepArgs &a, uint32_t blocks, hipStream_t st)
{
  return pick(mode, std::integer_sequence<int, SW_PLAIN, SW_LDS_F48, SW_LDS_P59, SW_F64, SW_REG_P59>(), [&](auto m) {
    return pick(G, Groups(), [&](auto g) { return pick(R, Counts(), [&](auto r) {
      if constexpr (hpf_plan::has_sweep(PICKED(m), PICKED(g), PICKED(r))) {
        hipLaunchKernelGGL((row_sweep_kernel<PICKED(g), PICKED(r), PICKED(m)>), dim3(blocks), dim3(256), 0, st, a);
        return true;
      } else if constexpr (unreachable_sweep(PICKED(m), PICKED(g), PICKED(r))) (void)&row_sweep_kernel<PICKED(g), PICKED(r), PICKED(m)>;
      return false;
    }); }); });
}
// row_sums_kernel: the sweep after a pass with the fused epilogue
bool launch_sums(int mode, int G, int R, const SweepArgs &a, uint32_t blocks, hipStream_t st)
{
  return pick(mode, std::integer_sequence<int, SW_LDS_P59, SW_REG_P59>(), [&](auto m) {
    return pick(G, Groups(), [&](auto g) { return pick(R, Counts(), [&](auto r) {
      if constexpr (hpf_plan::has_sums(PICKED(m), PICKED(g), PICKED(r))) {
        hipLaunchKernelGGL((row_sums_kernel<PICKED(g), PICKED(r), PICKED(m)>), dim3(blocks), dim3(256), 0, st, a);
        return true;
      } else return false;
    }); }); });
}
// fold_in_kernel: R columns per lane (hpf_plan::fold_plan), four waves and their slices of LDS per workgroup
bool launch_fold(int R, const FoldArgs &a, uint32_t blocks, uint32_t lds_bytes, hipStream_t st)
{
  return pick(R, Counts(), [&](auto r) {
    if constexpr (hpf_plan::has_fold(PICKED(r))) {
      hipLaunchKernelGGL((fold_in_kernel<PICKED(r)>), dim3(blocks), dim3(64 * hpf_plan::FOLD_WAVES), lds_bytes, st, a);
      return true;
    } else return false;
  });
}
// fold_in_long_kernel: R columns per lane, hpf_plan::fold_long_waves(R) waves per workgroup and their partial rows in LDS
bool launch_fold_long(int R, const FoldArgs &a, uint32_t blocks, uint32_t lds_bytes, hipStream_t st)
{
  return pick(R, Counts(), [&](auto r) {
    constexpr int WAVES = hpf_plan::fold_long_waves(PICKED(r));
    if constexpr (hpf_plan::has_fold_long(PICKED(r), WAVES)) {
      hipLaunchKernelGGL((fold_in_long_kernel<PICKED(r), WAVES>), dim3(blocks), dim3(64 * WAVES), lds_bytes, st, a);
      return true;
    } else return false;
  });
}
// explain_kernel: R terms per lane (hpf_plan::explain_plan), four waves per workgroup
bool launch_explain(int R, const ExplainArgs &a, uint32_t blocks, hipStream_t st)
{
  return pick(R, Counts(), [&](auto r) {
    if constexpr (hpf_plan::has_explain(PICKED(r))) {
      hipLaunchKernelGGL((explain_kernel<PICKED(r)>), dim3(blocks), dim3(64 * hpf_plan::EXPLAIN_WAVES), 0, st, a);
      return true;
    } else return false;
  });
}
// because_shape_kernel / because_kernel: R columns per lane (hpf_plan::because_plan), four waves per workgroup
bool launch_because(int R, bool pairs, const BecauseArgs &a, uint32_t blocks, hipStream_t st)
{
  return pick(R, Counts(), [&](auto r) {
    if constexpr (hpf_plan::has_because(PICKED(r))) {
      if (pairs) hipLaunchKernelGGL((because_kernel<PICKED(r)>), dim3(blocks), dim3(64 * hpf_plan::BECAUSE_WAVES), 0, st, a);
      else hipLaunchKernelGGL((because_shape_kernel<PICKED(r)>), dim3(blocks), dim3(64 * hpf_plan::BECAUSE_WAVES), 0, st, a);
      return true;
    } else return false;
  });
}
int check_launch(hpf_handle *h, const char *what);
// the fused rank kernels, by the chunks of A a column count keeps in registers (hpf_plan::rank_chunks); launch(nch) names
// the kernel template: loo_rank_kernel<nch>, rank_queries_kernel<nch> or topn_sweep_kernel<nch>.  Fails where the column
// count has no instance of `kernel`; what was launched is checked under `what` (the kernel's name unless given).
template <typename F>
int launch_rank(hpf_handle *h, const char *kernel, F &&launch, const char *what = nullptr)
{
  const bool launched = pick(hpf_plan::rank_chunks(h->K), std::integer_sequence<int, 0, 1, 2, 4>(), [&](auto nch) {
    if constexpr (hpf_plan::has_rank_chunks(PICKED(nch))) { launch(nch); return true; } else return false;
  });
  if (!launched) { h->err = std::string(kernel) + ": no instance for this column count"; return HPF_ERR_UNSUPPORTED; }
  return check_launch(h, what ? what : kernel);
}
#undef PICKED

int recover_flush(hpf_handle *h, uint32_t fl0, uint32_t begun);

// A sweep (or derive_w) met an element the p59 rows cannot hold: move the handle to plain fp64 rows and repeat
// whatever the passes skipped since (recover_flush).  Synchronises the stream.  Every consumer outside the hot
// loop comes through here before it touches S, E or W (hpf_lazy::RECOVER, first in the list ready() runs).
int recover_if_flushed(hpf_handle *h)
{
  if (h->in_recovery) return HPF_OK;
  uint32_t f[2] = {0, 0};
  HIPCHK(h, hipMemcpyAsync(f, h->flags, 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (!(f[0] & 2u)) return HPF_OK;
  return recover_flush(h, f[0], f[1]);
}

// surfaces a numerical breakdown the kernels flagged (synchronises the stream; hpf_lazy::REPORT)
int check_flags(hpf_handle *h)
{
  uint32_t f = 0;
  HIPCHK(h, hipMemcpyAsync(&f, h->flags, 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (f & 1u) {
    h->err = h->w32 ? "a softmax denominator underflowed to zero: the Elog spread is too wide for f32-stored W; use w_storage = 0"
                    : "a softmax denominator underflowed to zero (Elog spread > ~700): the state is not a valid HPF state";
    return HPF_ERR_STATE;
  }
  return HPF_OK;
}

int check_launch(hpf_handle *h, const char *what)
{
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    h->err = std::string(what) + ": " + hipGetErrorString(e);
    return HPF_ERR_HIP;
  }
  return HPF_OK;
}

int check_comm_async(hpf_handle *h)
{
  if (!h->comm || !g_rccl.CommGetAsyncError) return HPF_OK;
  int st = 0;
  const int rc = g_rccl.CommGetAsyncError(h->comm, &st);
  if (rc != 0 || (st != 0 && st != 7 /* ncclInProgress */)) {
    h->err = std::string("RCCL asynchronous error: ") + g_rccl.GetErrorString(rc != 0 ? rc : st);
    return HPF_ERR_HIP;
  }
  return HPF_OK;
}

// ---- host <-> device hand-over ----------------------------------------------
// Pageable hipMemcpy is staged by the runtime at ~4 GB/s; here the bytes go
// through two pinned buffers filled / drained by a few host threads while the
// other buffer is on the wire (HPF_H2D=staged, default), or the caller's pages
// are pinned for the duration of the copy (HPF_H2D=register), or it is left to
// the runtime (HPF_H2D=plain).
constexpr size_t STAGE_BYTES = 64u << 20;

int ensure_stage(hpf_handle *h)
{
  if (h->stage[0]) return HPF_OK;
  for (int k = 0; k < 2; ++k) {
    HIPCHK(h, hipHostMalloc(&h->stage[k], STAGE_BYTES, hipHostMallocDefault));
    HIPCHK(h, hipEventCreateWithFlags(&h->stage_ev[k], hipEventDisableTiming));
  }
  h->stage_bytes = STAGE_BYTES;
  return HPF_OK;
}

void par_memcpy(void *dst, const void *src, size_t bytes, unsigned T)
{
  if (T <= 1 || bytes < (8u << 20)) { memcpy(dst, src, bytes); return; }
  const size_t per = ((bytes + T - 1) / T + 4095) & ~(size_t)4095;
  std::vector<std::thread> th;
  for (unsigned t = 0; t < T; ++t) {
    const size_t o = (size_t)t * per;
    if (o >= bytes) break;
    const size_t len = std::min(per, bytes - o);
    th.emplace_back([=] { memcpy((char *)dst + o, (const char *)src + o, len); });
  }
  for (auto &x : th) x.join();
}

// is this host pointer page-locked memory HIP knows (hpf_host_alloc, hipHostMalloc, hipHostRegister)?  Then it is the
// DMA's own source / target: no staging, no host copy
bool host_is_pinned(const void *p)
{
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
  return at.type == hipMemoryTypeHost;
}

// contiguous host -> device; returns after the bytes have left `src`
int h2d(hpf_handle *h, void *dst, const void *src, size_t bytes)
{
  if (!bytes) return HPF_OK;
  if (bytes >= (1u << 20) && host_is_pinned(src) && host_is_pinned((const char *)src + bytes - 1)) {
    HIPCHK(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return HPF_OK;
  }
  if (h->xfer_mode == 2 && bytes >= (1u << 20)) {
    if (hipHostRegister(const_cast<void *>(src), bytes, hipHostRegisterDefault) == hipSuccess) {
      hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, h->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
      (void)hipHostUnregister(const_cast<void *>(src));
      if (e != hipSuccess) { h->err = std::string("h2d: ") + hipGetErrorString(e); return HPF_ERR_HIP; }
      return HPF_OK;
    }
    (void)hipGetLastError();             // not registrable (e.g. read-only mapping): stage it
  }
  if (h->xfer_mode == 0 || bytes < (1u << 20)) {
    HIPCHK(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return HPF_OK;
  }
  int rc;
  if ((rc = ensure_stage(h))) return rc;
  size_t off = 0; int k = 0;
  bool used[2] = {false, false};
  while (off < bytes) {
    const size_t len = std::min(h->stage_bytes, bytes - off);
    if (used[k]) HIPCHK(h, hipEventSynchronize(h->stage_ev[k]));
    par_memcpy(h->stage[k], (const char *)src + off, len, h->xfer_threads);
    HIPCHK(h, hipMemcpyAsync((char *)dst + off, h->stage[k], len, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipEventRecord(h->stage_ev[k], h->stream));
    used[k] = true; k ^= 1; off += len;
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return HPF_OK;
}

// contiguous device -> host (synchronous)
int d2h(hpf_handle *h, void *dst, const void *src, size_t bytes)
{
  if (!bytes) return HPF_OK;
  if (bytes >= (1u << 20) && host_is_pinned(dst) && host_is_pinned((char *)dst + bytes - 1)) {
    HIPCHK(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return HPF_OK;
  }
  if (h->xfer_mode == 2 && bytes >= (1u << 20)) {
    if (hipHostRegister(dst, bytes, hipHostRegisterDefault) == hipSuccess) {
      hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
      (void)hipHostUnregister(dst);
      if (e != hipSuccess) { h->err = std::string("d2h: ") + hipGetErrorString(e); return HPF_ERR_HIP; }
      return HPF_OK;
    }
    (void)hipGetLastError();
  }
  if (h->xfer_mode == 0 || bytes < (1u << 20)) {
    HIPCHK(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return HPF_OK;
  }
  int rc;
  if ((rc = ensure_stage(h))) return rc;
  // chunk c is copied out of its pinned buffer while chunk c+1 is on the wire
  size_t off = 0, prev_off = 0, prev_len = 0; int k = 0;
  bool have_prev = false;
  while (off < bytes || have_prev) {
    size_t len = 0;
    if (off < bytes) {
      len = std::min(h->stage_bytes, bytes - off);
      HIPCHK(h, hipMemcpyAsync(h->stage[k], (const char *)src + off, len, hipMemcpyDeviceToHost, h->stream));
      HIPCHK(h, hipEventRecord(h->stage_ev[k], h->stream));
    }
    if (have_prev) {
      HIPCHK(h, hipEventSynchronize(h->stage_ev[k ^ 1]));
      par_memcpy((char *)dst + prev_off, h->stage[k ^ 1], prev_len, h->xfer_threads);
    }
    have_prev = len > 0; prev_off = off; prev_len = len; off += len; k ^= 1;
  }
  return HPF_OK;
}

// Owner of the device temporaries of one call: what alloc() hands out is freed when the owner goes out of scope, once the
// stream is idle (after an error something launched may still read it) -- unless it was released earlier or kept
struct Scratch {
  hpf_handle *h;
  std::vector<void *> owned;
  explicit Scratch(hpf_handle *h_) : h(h_) {}
  Scratch(const Scratch &) = delete;
  Scratch &operator=(const Scratch &) = delete;
  ~Scratch() { (void)hipStreamSynchronize(h->stream); for (void *p : owned) dfree(p); }

  // n zeroed elements, or a copy of src[0 .. n)
  template <typename T>
  int alloc(T **p, size_t n, const T *src = nullptr)
  {
    const int rc = dalloc(h, p, n);
    if (*p) owned.push_back(*p);                                 // also when only dalloc's memset failed
    return rc || !src ? rc : h2d(h, *p, src, n * sizeof(T));
  }
  // free this one now (a temporary of O(nnz) must not wait for the end of the call)
  template <typename T>
  void release(T *&p) { dfree(keep(p)); }
  // give up ownership: the handle takes the pointer over
  template <typename T>
  T *keep(T *&p)
  {
    owned.erase(std::remove(owned.begin(), owned.end(), (void *)p), owned.end());
    T *r = p; p = nullptr;
    return r;
  }
};

// Device side of a ranking call: the selected users and the mask list (upload) and, for the fused calls (hpf_loo_ranks,
// hpf_rank_queries, hpf_recommend, hpf_audience), the bit rows of one batch of selected rows (bit_rows; hpf_plan::rank_batch_users)
struct FusedCtx : Scratch {
  uint32_t *d_users = nullptr, *d_mitems = nullptr; uint64_t *d_mptr = nullptr, *d_bits = nullptr;
  uint32_t words = 0, batch = 0;       // 64-bit words of a bit row; users per batch
  using Scratch::Scratch;

  int upload(const uint32_t *users, uint32_t n_sel, const uint64_t *mask_ptr, const uint32_t *mask_items)
  {
    int rc;
    if ((rc = alloc(&d_users, n_sel, users)) || !mask_ptr) return rc;
    if ((rc = alloc(&d_mptr, (size_t)n_sel + 1, mask_ptr))) return rc;
    return alloc(&d_mitems, (size_t)mask_ptr[n_sel], mask_ptr[n_sel] ? mask_items : nullptr);
  }
  // the bit rows of a batch over the `swept` rows the call ranks: the items for the calls that select users, the users for
  // hpf_audience
  int bit_rows(uint32_t n_sel, uint32_t swept)
  {
    words = (swept + 63) / 64;
    batch = hpf_plan::rank_batch_users(swept, n_sel, h->loo_batch);
    return alloc(&d_bits, (size_t)batch * words);
  }
  // the bit rows of the selected rows [b0, b0 + rows): cleared (alloc left them zero for the first batch) and set from the
  // view whose rows the selected ids name -- (rowptr_dev, u.idx, u.val) for users, (colptr_dev, it.idx, it.val) for items
  using MaskKernel = void (*)(const uint32_t *, uint32_t, const int64_t *, const uint32_t *, const uint8_t *, const uint64_t *,
                              const uint32_t *, uint32_t *, uint32_t);
  int mask_batch(uint32_t b0, uint32_t rows, const int64_t *ptr, const uint32_t *idx, const uint8_t *val,
                 MaskKernel kernel = loo_mask_kernel)
  {
    if (b0) HIPCHK(h, hipMemsetAsync(d_bits, 0, (size_t)rows * words * 8, h->stream));
    hipLaunchKernelGGL(kernel, dim3(std::min<uint32_t>((rows + 3) / 4, 4096)), dim3(256), 0, h->stream,
                       d_users + b0, rows, ptr, idx, val, d_mptr ? d_mptr + b0 : nullptr, d_mitems,
                       (uint32_t *)d_bits, words);
    return HPF_OK;
  }
};

uint32_t grid_for(uint64_t n) { return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((n + 255) / 256, 1), 16384); }

// dense [rows x cols] host <-> columns [col0, col0+cols) of the padded device
// matrix.  Full-width blocks (cols == ld) move straight; anything else goes
// through a contiguous device chunk and a repack kernel.
int copy_in(hpf_handle *h, double *dev, uint32_t ld, uint32_t col0, const double *host,
            uint32_t rows, uint32_t cols)
{
  if (!rows || !cols) return HPF_OK;
  if (cols == ld && col0 == 0) return h2d(h, dev, host, (size_t)rows * cols * 8);
  const uint64_t rows_per = std::max<uint64_t>(1, (256u << 20) / ((uint64_t)cols * 8));
  Scratch sc(h);
  double *tmp = nullptr; int rc;
  if ((rc = sc.alloc(&tmp, (size_t)std::min<uint64_t>(rows, rows_per) * cols))) return rc;
  for (uint64_t r0 = 0; r0 < rows; r0 += rows_per) {
    const uint64_t nr = std::min<uint64_t>(rows_per, rows - r0);
    if ((rc = h2d(h, tmp, host + r0 * cols, (size_t)nr * cols * 8))) return rc;
    hipLaunchKernelGGL(repack_in_kernel, dim3(grid_for(nr * cols)), dim3(256), 0, h->stream, tmp,
                       dev + r0 * ld, nr, cols, ld, col0);
    if ((rc = check_launch(h, "repack_in_kernel"))) return rc;
  }
  if (hipStreamSynchronize(h->stream) != hipSuccess) { h->err = "copy_in: stream error"; return HPF_ERR_HIP; }
  return HPF_OK;
}
int copy_out(hpf_handle *h, const double *dev, uint32_t ld, uint32_t col0, double *host,
             uint32_t rows, uint32_t cols)
{
  if (!rows || !cols) return HPF_OK;
  if (cols == ld && col0 == 0) return d2h(h, host, dev, (size_t)rows * cols * 8);
  const uint64_t rows_per = std::max<uint64_t>(1, (256u << 20) / ((uint64_t)cols * 8));
  Scratch sc(h);
  double *tmp = nullptr; int rc;
  if ((rc = sc.alloc(&tmp, (size_t)std::min<uint64_t>(rows, rows_per) * cols))) return rc;
  for (uint64_t r0 = 0; r0 < rows; r0 += rows_per) {
    const uint64_t nr = std::min<uint64_t>(rows_per, rows - r0);
    hipLaunchKernelGGL(repack_out_kernel, dim3(grid_for(nr * cols)), dim3(256), 0, h->stream,
                       dev + r0 * ld, tmp, nr, cols, ld, col0);
    if ((rc = check_launch(h, "repack_out_kernel"))) return rc;
    if ((rc = d2h(h, host + r0 * cols, tmp, (size_t)nr * cols * 8))) return rc;
  }
  return HPF_OK;
}
// the same for a caller's DEVICE buffer (hpf_set_state_device / hpf_get_state_device)
int copy_in_dev(hpf_handle *h, double *dev, uint32_t ld, uint32_t col0, const double *src,
                uint32_t rows, uint32_t cols)
{
  if (!rows || !cols) return HPF_OK;
  if (cols == ld && col0 == 0)
    HIPCHK(h, hipMemcpyAsync(dev, src, (size_t)rows * cols * 8, hipMemcpyDeviceToDevice, h->stream));
  else {
    hipLaunchKernelGGL(repack_in_kernel, dim3(grid_for((uint64_t)rows * cols)), dim3(256), 0, h->stream, src,
                       dev, (uint64_t)rows, cols, ld, col0);
    int rc = check_launch(h, "repack_in_kernel");
    if (rc) return rc;
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return HPF_OK;
}
int copy_out_dev(hpf_handle *h, const double *dev, uint32_t ld, uint32_t col0, double *dst,
                 uint32_t rows, uint32_t cols)
{
  if (!rows || !cols) return HPF_OK;
  if (cols == ld && col0 == 0)
    HIPCHK(h, hipMemcpyAsync(dst, dev, (size_t)rows * cols * 8, hipMemcpyDeviceToDevice, h->stream));
  else {
    hipLaunchKernelGGL(repack_out_kernel, dim3(grid_for((uint64_t)rows * cols)), dim3(256), 0, h->stream, dev,
                       dst, (uint64_t)rows, cols, ld, col0);
    int rc = check_launch(h, "repack_out_kernel");
    if (rc) return rc;
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return HPF_OK;
}

// exclusive scan of n counters (uint32 or uint64) into uint64 out[0..n) (+ out[n] = total)
template <typename IN>
int device_scan(hpf_handle *h, const IN *in, uint64_t n, uint64_t *out, bool write_total)
{
  if (n == 0) {
    if (write_total) HIPCHK(h, hipMemsetAsync(out, 0, 8, h->stream));
    return HPF_OK;
  }
  const uint64_t nb = (n + SCAN_CHUNK - 1) / SCAN_CHUNK;
  Scratch sc(h);
  uint64_t *bsum = nullptr; int rc;
  if ((rc = sc.alloc(&bsum, (size_t)nb))) return rc;
  hipLaunchKernelGGL((scan_reduce_kernel<IN>), dim3((uint32_t)nb), dim3(256), 0, h->stream, in, n, bsum);
  hipLaunchKernelGGL(scan_spine_kernel, dim3(1), dim3(256), 0, h->stream, bsum, nb);
  hipLaunchKernelGGL((scan_apply_kernel<IN>), dim3((uint32_t)nb), dim3(256), 0, h->stream, in, n, bsum, out,
                     write_total ? 1 : 0);
  rc = check_launch(h, "device_scan");
  const hipError_t e = hipStreamSynchronize(h->stream);
  if (!rc && e != hipSuccess) { h->err = std::string("device_scan: ") + hipGetErrorString(e); rc = HPF_ERR_HIP; }
  return rc;
}

// Work lists of one side cut on the device from its row pointers (dptr, in HBM): nothing of
// size O(rows) or O(nnz) crosses PCIe.
int device_side_work(hpf_handle *h, Side &s, const int64_t *dptr, uint32_t rows)
{
  dfree(s.segs); dfree(s.longrows); dfree(s.grouprows); dfree(s.hugerows);
  s.segs = nullptr; s.longrows = s.grouprows = s.hugerows = nullptr;
  s.nseg = s.nlong = s.nlong_wave = s.ngroup = s.nhuge = 0;
  dfree(s.partial); dfree(s.partial2);
  s.partial = nullptr; s.partial2 = nullptr;
  s.npartial = 0; s.npartial2 = 0;
  dfree(s.p_idx); dfree(s.p_val); dfree(s.chunks);
  s.p_idx = nullptr; s.p_val = nullptr; s.chunks = nullptr;
  s.nchunk_blocks = 0; s.tiles = 0; s.tile_rows = 0; s.chunk_segs = 0; s.tiled_nnz = 0; s.light_below = 0;
  if (rows == 0) return HPF_OK;
  int rc;
  Scratch sc(h);
  uint64_t *cnt[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  uint32_t *bad = nullptr;
  for (int k = 0; k < 5; ++k) if ((rc = sc.alloc(&cnt[k], (size_t)rows + 1))) return rc;
  if ((rc = sc.alloc(&bad, 1))) return rc;
  SegPlan pl = {cnt[0], cnt[1], cnt[2], cnt[3], cnt[4]};
  hipLaunchKernelGGL(seg_plan_kernel, dim3(grid_for(rows)), dim3(256), 0, h->stream, dptr, rows, h->seg_max,
                     h->huge_slots, h->group_slots, pl, bad);
  if ((rc = check_launch(h, "seg_plan_kernel"))) return rc;
  for (int k = 0; k < 5; ++k) if ((rc = device_scan<uint64_t>(h, cnt[k], rows, cnt[k], true))) return rc;
  uint64_t tot[5]; uint32_t hb = 0;
  hipError_t e = hipSuccess;
  for (int k = 0; k < 5 && e == hipSuccess; ++k)
    e = hipMemcpyAsync(&tot[k], cnt[k] + rows, 8, hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(&hb, bad, 4, hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) { h->err = std::string("seg_plan_kernel: ") + hipGetErrorString(e); return HPF_ERR_HIP; }
  if (hb) { h->err = "row pointers must start at 0 and be monotone"; return HPF_ERR_INVALID; }
  if (tot[0] > 0xffffffffull || tot[1] > 0x7fffffffull) { h->err = "too many segments for 32-bit work lists"; return HPF_ERR_UNSUPPORTED; }
  s.nseg = (uint32_t)tot[0]; s.npartial = (uint32_t)tot[1]; s.nlong = s.nlong_wave = (uint32_t)tot[2];
  s.nhuge = (uint32_t)tot[3]; s.ngroup = s.npartial2 = (uint32_t)tot[4];
  if ((rc = dalloc(h, &s.segs, s.nseg)) || (rc = dalloc(h, &s.longrows, s.nlong))) return rc;
  if (s.ngroup && ((rc = dalloc(h, &s.grouprows, s.ngroup)) || (rc = dalloc(h, &s.hugerows, s.nhuge)))) return rc;
  hipLaunchKernelGGL(seg_fill_kernel, dim3(grid_for(rows)), dim3(256), 0, h->stream, dptr, rows, h->seg_max,
                     h->huge_slots, h->group_slots, pl, s.segs, s.longrows, s.hugerows, s.grouprows);
  if ((rc = check_launch(h, "seg_fill_kernel"))) return rc;
  if ((rc = dalloc(h, &s.partial, (size_t)s.npartial * h->ld))) return rc;
  if (s.npartial2 && (rc = dalloc(h, &s.partial2, (size_t)s.npartial2 * h->ld))) return rc;
  if (hipStreamSynchronize(h->stream) != hipSuccess) { h->err = "work-list build failed on the device"; return HPF_ERR_HIP; }
  return HPF_OK;
}

// ---- stable LSD radix sort of n records on the low `bits` bits of a 32-bit key, carrying a 32-bit
// payload u (NULL at the start: the row of the record, by bisection in rowptr), an optional second
// one x, and an optional byte v.  Buffers: the pass p writes set p & 1 of (K, U, X, V); *res = the
// set that holds the result.  in_* are only read.
struct SortSets { uint32_t *K[2], *U[2], *X[2]; uint8_t *V[2]; };
int radix_sort_records(hpf_handle *h, uint64_t n, uint32_t bits, const uint32_t *in_k, const uint32_t *in_u,
                       const uint32_t *in_x, const uint8_t *in_v, const int64_t *rowptr, uint32_t n_rows,
                       const SortSets &b, int *res)
{
  const uint32_t P = std::max<uint32_t>(1, (bits + RADIX_BITS - 1) / RADIX_BITS);
  const uint64_t ntiles = (n + RADIX_TILE - 1) / RADIX_TILE;
  const uint32_t nblk = (uint32_t)((ntiles + 3) / 4);
  Scratch sc(h);
  uint64_t *counts = nullptr; uint32_t *bad = nullptr; int rc;
  *res = (int)((P - 1) & 1);
  if ((rc = sc.alloc(&counts, (size_t)ntiles * RADIX_DIGITS)) || (rc = sc.alloc(&bad, 1))) return rc;
  for (uint32_t p = 0; p < P; ++p) {
    const int o = (int)(p & 1), i = o ^ 1;
    RadixArgs a;
    a.keys_in = p == 0 ? in_k : b.K[i];
    a.users_in = p == 0 ? in_u : b.U[i];
    a.extra_in = p == 0 ? in_x : b.X[i];
    a.vals_in = p == 0 ? in_v : (in_v ? b.V[i] : nullptr);
    a.rowptr = rowptr; a.n_rows = n_rows;
    a.keys_out = b.K[o]; a.users_out = b.U[o];
    a.extra_out = in_x ? b.X[o] : nullptr;
    a.vals_out = in_v ? b.V[o] : nullptr;
    a.offsets = counts; a.nnz = n; a.ntiles = ntiles; a.shift = p * RADIX_BITS;
    hipLaunchKernelGGL(radix_count_kernel, dim3(nblk), dim3(256), 0, h->stream, a.keys_in, n, a.shift, ntiles, counts,
                       0xffffffffu, bad);
    if ((rc = check_launch(h, "radix_count_kernel"))) return rc;
    if ((rc = device_scan<uint64_t>(h, counts, ntiles * RADIX_DIGITS, counts, false))) return rc;
    hipLaunchKernelGGL(radix_scatter_kernel, dim3(nblk), dim3(256), 0, h->stream, a);
    if ((rc = check_launch(h, "radix_scatter_kernel"))) return rc;
  }
  if (hipStreamSynchronize(h->stream) != hipSuccess) { h->err = "record sort failed on the device"; return HPF_ERR_HIP; }
  return HPF_OK;
}

uint32_t bits_for(uint64_t count) { uint32_t b = 0; while (b < 32 && ((uint64_t)1 << b) < count) ++b; return std::max<uint32_t>(b, 1); }

// ---- Tiled work list of one side (hpf_build.hpp "Tiled phi pass"), stage by stage.  What a stage
// allocates belongs to the caller's Scratch; what the next stage no longer reads is released at once (the temporaries are
// 26 bytes per nonzero).

// the side's nonzeros sorted by (tile of the gathered row | 0 for a light owner row), stable: key, owner row, index, rating
struct TiledRecords { uint32_t *key = nullptr, *row = nullptr, *idx = nullptr; uint8_t *val = nullptr; };
int tile_sort_records(hpf_handle *h, Scratch &sc, const Side &s, const int64_t *ptr, uint32_t rows_oth, uint64_t nnz,
                      const hpf_plan::TilePolicy &tp, TiledRecords *out)
{
  int rc;
  uint32_t *tilemap = nullptr, *key0 = nullptr, *row0 = nullptr;
  if ((rc = sc.alloc(&tilemap, rows_oth)) || (rc = sc.alloc(&key0, (size_t)nnz)) || (rc = sc.alloc(&row0, (size_t)nnz))) return rc;
  hipLaunchKernelGGL(tile_map_kernel, dim3(grid_for(rows_oth)), dim3(256), 0, h->stream, tilemap, rows_oth, tp.T);
  const uint32_t wblk = (uint32_t)(((nnz + RADIX_TILE - 1) / RADIX_TILE + 3) / 4);
  hipLaunchKernelGGL(tile_key_kernel, dim3(wblk), dim3(256), 0, h->stream, ptr, s.rows, s.idx, nnz, tilemap, tp.light_below,
                     key0, row0);
  if ((rc = check_launch(h, "tile_key_kernel"))) return rc;
  const uint32_t kbits = bits_for(tp.tiles + 1), KP = (kbits + RADIX_BITS - 1) / RADIX_BITS;
  SortSets b = {{nullptr, nullptr}, {nullptr, nullptr}, {nullptr, nullptr}, {nullptr, nullptr}};
  for (int k = 0; k < (KP > 1 ? 2 : 1); ++k) {
    if ((rc = sc.alloc(&b.K[k], (size_t)nnz)) || (rc = sc.alloc(&b.U[k], (size_t)nnz)) || (rc = sc.alloc(&b.X[k], (size_t)nnz))) return rc;
    if (s.val && (rc = sc.alloc(&b.V[k], (size_t)nnz))) return rc;
  }
  int r = 0;
  if ((rc = radix_sort_records(h, nnz, kbits, key0, row0, s.idx, s.val, nullptr, 0, b, &r))) return rc;
  sc.release(key0); sc.release(row0); sc.release(tilemap);
  sc.release(b.K[r ^ 1]); sc.release(b.U[r ^ 1]); sc.release(b.X[r ^ 1]); sc.release(b.V[r ^ 1]);      // the set that lost
  *out = {b.K[r], b.U[r], b.X[r], b.V[r]};
  return HPF_OK;
}

// the segments of the sorted records (<= seg_max nonzeros of one owner row and one key), each one's owner row, and the
// first segment of every key on the host; rec.key and rec.row are released.  nseg == 0: no list the pass can index
struct TiledSegs { Seg *segs = nullptr; uint32_t *seg_row = nullptr; uint32_t nseg = 0; std::vector<uint32_t> fs; };
int tile_segments(hpf_handle *h, Scratch &sc, uint64_t nnz, uint32_t nkeys, TiledRecords &rec, TiledSegs *out)
{
  int rc;
  const uint64_t nwt = (nnz + RADIX_TILE - 1) / RADIX_TILE;
  const uint32_t wblk = (uint32_t)((nwt + 3) / 4);
  uint64_t *cnt = nullptr; uint32_t *seg_key = nullptr, *first_seg = nullptr;
  if ((rc = sc.alloc(&cnt, (size_t)nwt + 1))) return rc;
  hipLaunchKernelGGL(seg_count_kernel, dim3(wblk), dim3(256), 0, h->stream, rec.key, rec.row, nnz, h->seg_max, cnt);
  if ((rc = check_launch(h, "seg_count_kernel"))) return rc;
  if ((rc = device_scan<uint64_t>(h, cnt, nwt, cnt, true))) return rc;
  uint64_t nseg64 = 0;
  HIPCHK(h, hipMemcpyAsync(&nseg64, cnt + nwt, 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (nseg64 == 0 || nseg64 > 0x7fffffffull) return HPF_OK;
  const uint32_t nseg = (uint32_t)nseg64;
  if ((rc = sc.alloc(&out->segs, nseg)) || (rc = sc.alloc(&out->seg_row, nseg)) || (rc = sc.alloc(&seg_key, nseg)) ||
      (rc = sc.alloc(&first_seg, nkeys))) return rc;
  HIPCHK(h, hipMemsetAsync(first_seg, 0xff, (size_t)nkeys * 4, h->stream));
  hipLaunchKernelGGL(seg_emit_kernel, dim3(wblk), dim3(256), 0, h->stream, rec.key, rec.row, nnz, h->seg_max, cnt, out->segs, out->seg_row, seg_key);
  hipLaunchKernelGGL(seg_len_kernel, dim3(grid_for(nseg)), dim3(256), 0, h->stream, out->segs, nseg, nnz, seg_key, first_seg);
  if ((rc = check_launch(h, "seg_emit_kernel"))) return rc;
  out->fs.resize(nkeys);
  HIPCHK(h, hipMemcpyAsync(out->fs.data(), first_seg, (size_t)nkeys * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  sc.release(rec.key); sc.release(rec.row);
  sc.release(cnt); sc.release(seg_key); sc.release(first_seg);
  out->nseg = nseg;
  return HPF_OK;
}

// per owner row: its segments in key order -> partial slots and combine lists (the segments get their slots).
// fits == false: more partial slots than the work lists index
struct TiledSlots {
  LongRow *longs = nullptr, *huges = nullptr, *groups = nullptr; double *partial = nullptr, *partial2 = nullptr;
  uint32_t npartial = 0, nlong = 0, nlong_wave = 0, nhuge = 0, ngroup = 0; bool fits = false;
};
int tile_slots(hpf_handle *h, Scratch &sc, uint32_t rows, const TiledSegs &sg, TiledSlots *out)
{
  int rc;
  const uint32_t nseg = sg.nseg;
  uint32_t *iota = nullptr; int64_t *segptr = nullptr; uint64_t *pl[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  SortSets sb = {{nullptr, nullptr}, {nullptr, nullptr}, {nullptr, nullptr}, {nullptr, nullptr}};
  if ((rc = sc.alloc(&iota, nseg))) return rc;
  hipLaunchKernelGGL(iota_kernel, dim3(grid_for(nseg)), dim3(256), 0, h->stream, iota, nseg);
  for (int k = 0; k < 2; ++k) if ((rc = sc.alloc(&sb.K[k], nseg)) || (rc = sc.alloc(&sb.U[k], nseg))) return rc;
  int sr = 0;
  if ((rc = radix_sort_records(h, nseg, bits_for(rows), sg.seg_row, iota, nullptr, nullptr, nullptr, 0, sb, &sr))) return rc;
  if ((rc = sc.alloc(&segptr, (size_t)rows + 1))) return rc;
  hipLaunchKernelGGL(colptr_from_sorted_kernel, dim3(grid_for(nseg)), dim3(256), 0, h->stream, sb.K[sr], (uint64_t)nseg, rows, segptr);
  for (int k = 0; k < 5; ++k) if ((rc = sc.alloc(&pl[k], (size_t)rows + 1))) return rc;
  SegPlan plan = {pl[0], pl[1], pl[2], pl[3], pl[4]};
  hipLaunchKernelGGL(slot_plan_kernel, dim3(grid_for(rows)), dim3(256), 0, h->stream, segptr, rows, h->huge_slots,
                     h->group_slots, plan);
  if ((rc = check_launch(h, "slot_plan_kernel"))) return rc;
  for (int k = 0; k < 5; ++k) if ((rc = device_scan<uint64_t>(h, pl[k], rows, pl[k], true))) return rc;
  uint64_t tot[5];
  for (int k = 0; k < 5; ++k) HIPCHK(h, hipMemcpyAsync(&tot[k], pl[k] + rows, 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (tot[1] > 0x7fffffffull) return HPF_OK;
  TiledSlots &o = *out;
  o.npartial = (uint32_t)tot[1]; o.nlong = (uint32_t)tot[2]; o.nhuge = (uint32_t)tot[3]; o.ngroup = (uint32_t)tot[4];
  if ((rc = sc.alloc(&o.longs, o.nlong))) return rc;
  if (o.ngroup && ((rc = sc.alloc(&o.groups, o.ngroup)) || (rc = sc.alloc(&o.huges, o.nhuge)))) return rc;
  hipLaunchKernelGGL(slot_fill_kernel, dim3(grid_for(rows)), dim3(256), 0, h->stream, segptr, rows, h->huge_slots,
                     h->group_slots, plan, sb.U[sr], sg.segs, o.longs, o.huges, o.groups);
  if ((rc = check_launch(h, "slot_fill_kernel"))) return rc;
  if ((rc = sc.alloc(&o.partial, (size_t)o.npartial * h->ld))) return rc;
  if (o.ngroup && (rc = sc.alloc(&o.partial2, (size_t)o.ngroup * h->ld))) return rc;
  // the combine gives the rows with more than COMBINE_SPLIT partials a workgroup each: they go behind the others (a stable
  // partition of the row-ordered list: a function of the matrix alone)
  // (the rows WITHOUT any nonzero stay in the wave kernel's part: taking them out -- cleared once, and again only after
  // an export or a hand-over had written S -- was built in round 5 and bought nothing measurable: C2's 48 000 of them
  // are 40 MB of zeros, ~10 us of a 45 us launch that the multi-segment light rows' chains set; experiments.md)
  o.nlong_wave = o.nlong;
  if (o.nlong) {
    std::vector<LongRow> lr(o.nlong), big;
    HIPCHK(h, hipMemcpyAsync(lr.data(), o.longs, (size_t)o.nlong * sizeof(LongRow), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    size_t w = 0;
    for (const LongRow &x : lr) { if (x.nslots > COMBINE_SPLIT) big.push_back(x); else lr[w++] = x; }
    if (!big.empty()) {
      std::copy(big.begin(), big.end(), lr.begin() + (ptrdiff_t)w);
      o.nlong_wave = (uint32_t)w;
      HIPCHK(h, hipMemcpyAsync(o.longs, lr.data(), (size_t)o.nlong * sizeof(LongRow), hipMemcpyHostToDevice, h->stream));
      HIPCHK(h, hipStreamSynchronize(h->stream));
    }
  }
  o.fits = true;
  return HPF_OK;
}

// the queues and chunks of the segments (hpf_plan::plan_tile_queues) on the device; *chunks stays null where there is no list
int tile_chunks(hpf_handle *h, Scratch &sc, const TiledSegs &sg, uint32_t tiles, uint64_t nnz, uint2 **chunks, uint32_t *nchunks, uint32_t *chunk_segs)
{
  uint64_t rest_nnz = nnz;
  const uint32_t rest_end = hpf_plan::tile_rest_end(sg.fs, sg.nseg);
  if (rest_end && rest_end < sg.nseg) {
    Seg first_tiled;
    HIPCHK(h, hipMemcpy(&first_tiled, sg.segs + rest_end, sizeof(Seg), hipMemcpyDeviceToHost));
    rest_nnz = (uint64_t)first_tiled.start;
  }
  const uint32_t wg = h->wg_of(true);
  const hpf_plan::TileQueuePlan qp = hpf_plan::plan_tile_queues(sg.fs, sg.nseg, tiles, rest_nnz, wg, ((size_t)1 << 28) / wg, *h);
  if (!qp.ok) return HPF_OK;
  static_assert(sizeof(hpf_plan::TileChunk) == sizeof(uint2) && offsetof(hpf_plan::TileChunk, x) == offsetof(uint2, x) &&
                offsetof(hpf_plan::TileChunk, y) == offsetof(uint2, y), "chunk");
  int rc;
  if ((rc = sc.alloc(chunks, qp.chunks.size()))) return rc;
  HIPCHK(h, hipMemcpyAsync(*chunks, qp.chunks.data(), qp.chunks.size() * sizeof(uint2), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  *nchunks = (uint32_t)qp.chunks.size(); *chunk_segs = qp.chunk_segs;
  return HPF_OK;
}

// Replaces the side's plain work list by the tiled one -- once the new one is complete; until then the side is not touched
int tile_side(hpf_handle *h, Side &s, const int64_t *ptr, uint32_t rows_oth, uint64_t nnz, const hpf_plan::TilePolicy &tp, uint64_t heavy_nnz)
{
  int rc;
  Scratch sc(h);
  TiledRecords rec; TiledSegs sg; TiledSlots sl;
  uint2 *chunks = nullptr; uint32_t nchunks = 0, chunk_segs = 0;
  if ((rc = tile_sort_records(h, sc, s, ptr, rows_oth, nnz, tp, &rec))) return rc;
  if ((rc = tile_segments(h, sc, nnz, tp.tiles + 1, rec, &sg)) || !sg.nseg) return rc;
  if ((rc = tile_slots(h, sc, s.rows, sg, &sl)) || !sl.fits) return rc;
  if ((rc = tile_chunks(h, sc, sg, tp.tiles, nnz, &chunks, &nchunks, &chunk_segs)) || !chunks) return rc;
  dfree(s.segs); dfree(s.longrows); dfree(s.grouprows); dfree(s.hugerows); dfree(s.partial); dfree(s.partial2);
  s.segs = sc.keep(sg.segs); s.nseg = sg.nseg;
  s.longrows = sc.keep(sl.longs); s.nlong = sl.nlong; s.nlong_wave = sl.nlong_wave;
  s.grouprows = sc.keep(sl.groups); s.ngroup = sl.ngroup;
  s.hugerows = sc.keep(sl.huges); s.nhuge = sl.nhuge;
  s.partial = sc.keep(sl.partial); s.npartial = sl.npartial;
  s.partial2 = sc.keep(sl.partial2); s.npartial2 = sl.ngroup;
  s.p_idx = sc.keep(rec.idx); s.p_val = sc.keep(rec.val);
  s.chunks = sc.keep(chunks); s.nchunk_blocks = nchunks;
  s.tiles = tp.tiles; s.tile_rows = tp.T; s.tiled_nnz = heavy_nnz; s.light_below = tp.light_below; s.chunk_segs = chunk_segs;
  return HPF_OK;
}

// Called after device_side_work: when the policy (hpf_plan::tile_policy) finds the side worth tiling, the plain work list
// is replaced.
//   ptr       the side's own row pointers (rows + 1), s.idx / s.val its nonzeros in row order
//   rows_oth  rows of the gathered side, row_bytes bytes each
// Auto mode takes the "ranges" policy when the heavy rows hold >= 15 % (tile_min_share) of the nonzeros.
int build_tiled_side(hpf_handle *h, Side &s, const int64_t *ptr, uint32_t rows_oth, uint64_t nnz, size_t row_bytes)
{
  const bool item_side = &s == &h->it;
  const hpf_plan::TilePolicy tp = hpf_plan::tile_policy(rows_oth, row_bytes, nnz, s.rows, h->nz_per_batch(), item_side, *h, h->cfg.tiling);
  if (!tp.tile) return HPF_OK;
  int rc;
  uint64_t heavy_nnz = nnz;
  if (tp.light_below) {
    Scratch sc(h);
    unsigned long long *stat = nullptr;
    if ((rc = sc.alloc(&stat, 2))) return rc;
    hipLaunchKernelGGL(deg_ge_kernel, dim3(grid_for(s.rows)), dim3(256), 0, h->stream, ptr, s.rows, tp.light_below, stat);
    unsigned long long hv[2] = {0, 0};       // heavy rows, their nonzeros
    hipError_t e = hipMemcpyAsync(hv, stat, 16, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) { h->err = std::string("deg_ge_kernel: ") + hipGetErrorString(e); return HPF_ERR_HIP; }
    heavy_nnz = hv[1];
    if ((double)heavy_nnz < h->tile_min_share * (double)nnz) return HPF_OK;
  }
  // if the allocations fail although the rule finds room, the side stays row-major and hpf_work_info.notes says so
  size_t fr = 0, tot = 0;
  if (hipMemGetInfo(&fr, &tot) == hipSuccess && !hpf_plan::tiling_fits(h->ld, h->u.rows, h->it.rows, nnz, h->u.val != nullptr, tot)) {
    h->notes |= (item_side ? 2u : 1u);
    return HPF_OK;
  }
  rc = tile_side(h, s, ptr, rows_oth, nnz, tp, heavy_nnz);
  if (rc == HPF_ERR_OOM) {       // tiling is optional: without the room for it the side stays row-major -- and says so
    (void)hipGetLastError();
    h->err.clear();
    h->notes |= (item_side ? 8u : 4u);
    rc = HPF_OK;
  }
  return rc;
}

// Which side runs the fused sweep epilogue (hpf_plan::fused_sweep) and, for it, the rows whose W the pass writes: those that
// are ONE segment of the final work list, row-major or tiled.  Rows cut into several segments and rows without any keep the
// full sweep body (row_sums_kernel).  Called whenever the lists or the layout of the rows have changed.
int mark_fused_rows(hpf_handle *h)
{
  Side *sides[2] = {&h->u, &h->it};
  for (Side *s : sides) {
    dfree(s->row_done); s->row_done = nullptr;
    s->fused = hpf_plan::fused_sweep(*h, *h, s == &h->it) && s->rows > 0 && s->nseg > 0;
    if (!s->fused) continue;
    int rc;
    if ((rc = dalloc(h, &s->row_done, ((size_t)s->rows + 31) / 32))) return rc;      // zeroed
    hipLaunchKernelGGL(mark_done_rows_kernel, dim3(grid_for(s->nseg)), dim3(256), 0, h->stream, s->segs, s->nseg, s->row_done);
    if ((rc = check_launch(h, "mark_done_rows_kernel"))) return rc;
  }
  if (hipStreamSynchronize(h->stream) != hipSuccess) { h->err = "work-list build failed on the device"; return HPF_ERR_HIP; }
  return HPF_OK;
}

// the tiled lists of both sides (after device_side_work); a tile is 4 MiB of the rows the pass gathers
int build_work_lists_tiled(hpf_handle *h, uint64_t nnz)
{
  const uint32_t n = h->u.rows, m = h->it.rows;
  int rc;
  const size_t rowb = h->wl != WL_PLAIN ? (size_t)h->pk.row_bytes : (size_t)h->ld * (h->w32 ? 4 : 8);
  h->notes &= ~15u;
  if ((rc = build_tiled_side(h, h->u, h->rowptr_dev, m, nnz, rowb))) return rc;     // the user pass gathers item rows
  if ((rc = build_tiled_side(h, h->it, h->colptr_dev, n, nnz, rowb))) return rc;
  return mark_fused_rows(h);
}

// Item-major view of the ratings, built in HBM: h->u.idx / h->u.val (CSR order)
// and h->rowptr_dev are in place; fills h->colptr_dev, h->it.idx, h->it.val.
// Stable LSD radix sort on the item id => users ascending inside an item.
int build_csc_device(hpf_handle *h, uint32_t n, uint32_t m, uint64_t nnz)
{
  int rc;
  Scratch sc(h);
  uint32_t *bad = nullptr;
  uint32_t *kbuf[2] = {nullptr, nullptr}, *ut = nullptr; uint8_t *vt = nullptr; uint64_t *counts = nullptr;
  unsigned char *pool = nullptr;
  dfree(h->colptr_dev); h->colptr_dev = nullptr;
  dfree(h->it.idx); dfree(h->it.val); h->it.idx = nullptr; h->it.val = nullptr;
  if ((rc = dalloc(h, &h->colptr_dev, (size_t)m + 1))) return rc;          // zeroed: the answer for nnz == 0
  if ((rc = dalloc(h, &h->it.idx, (size_t)nnz))) return rc;
  if (h->u.val && (rc = dalloc(h, &h->it.val, (size_t)nnz))) return rc;
  if (nnz == 0) return HPF_OK;
  if ((rc = sc.alloc(&bad, 1))) return rc;
  uint32_t bits = 0;
  while (bits < 32 && ((uint64_t)1 << bits) < (uint64_t)m) ++bits;
  const uint32_t P = std::max<uint32_t>(1, (bits + RADIX_BITS - 1) / RADIX_BITS);
  const uint64_t ntiles = (nnz + RADIX_TILE - 1) / RADIX_TILE;
  const uint32_t nblk = (uint32_t)((ntiles + 3) / 4);
  // one allocation for every temporary of the sort (mapping ~100 GB piecewise was most of
  // whole C5's upload time): [counts | keys A | keys B | users | ratings], 256-byte aligned parts
  {
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t b_counts = up((size_t)ntiles * RADIX_DIGITS * 8), b_k = up((size_t)nnz * 4);
    const size_t b_k1 = P >= 2 ? b_k : 0, b_ut = P >= 2 ? b_k : 0, b_vt = (P >= 2 && h->u.val) ? up((size_t)nnz) : 0;
    if ((rc = sc.alloc(&pool, b_counts + b_k + b_k1 + b_ut + b_vt))) return rc;
    char *q = (char *)pool;
    counts = (uint64_t *)q; q += b_counts;
    kbuf[0] = (uint32_t *)q; q += b_k;
    if (b_k1) { kbuf[1] = (uint32_t *)q; q += b_k1; }
    if (b_ut) { ut = (uint32_t *)q; q += b_ut; }
    if (b_vt) { vt = (uint8_t *)q; q += b_vt; }
  }
  for (uint32_t p = 0; p < P; ++p) {
    RadixArgs a;
    a.keys_in = p == 0 ? h->u.idx : kbuf[(p - 1) & 1];
    const bool out_final = ((P - 1 - p) & 1u) == 0;      // the last pass lands in it.idx / it.val
    a.users_in = p == 0 ? nullptr : (out_final ? ut : h->it.idx);
    a.vals_in = !h->u.val ? nullptr : p == 0 ? h->u.val : (out_final ? vt : h->it.val);
    a.rowptr = h->rowptr_dev; a.n_rows = n;
    a.extra_in = nullptr; a.extra_out = nullptr;
    a.keys_out = kbuf[p & 1];
    a.users_out = out_final ? h->it.idx : ut;
    a.vals_out = !h->u.val ? nullptr : (out_final ? h->it.val : vt);
    a.offsets = counts; a.nnz = nnz; a.ntiles = ntiles; a.shift = p * RADIX_BITS;
    hipLaunchKernelGGL(radix_count_kernel, dim3(nblk), dim3(256), 0, h->stream, a.keys_in, nnz, a.shift, ntiles, counts,
                       m, bad);
    if ((rc = check_launch(h, "radix_count_kernel"))) return rc;
    if (p == 0) {                                        // every item id was range-checked on the way
      uint32_t hb = 0;
      hipError_t e = hipMemcpyAsync(&hb, bad, 4, hipMemcpyDeviceToHost, h->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
      if (e != hipSuccess) { h->err = std::string("radix_count_kernel: ") + hipGetErrorString(e); return HPF_ERR_HIP; }
      if (hb) { h->err = "item index out of range"; return HPF_ERR_INVALID; }
    }
    if ((rc = device_scan<uint64_t>(h, counts, ntiles * RADIX_DIGITS, counts, false))) return rc;
    hipLaunchKernelGGL(radix_scatter_kernel, dim3(nblk), dim3(256), 0, h->stream, a);
    if ((rc = check_launch(h, "radix_scatter_kernel"))) return rc;
  }
  hipLaunchKernelGGL(colptr_from_sorted_kernel, dim3(grid_for(nnz)), dim3(256), 0, h->stream, kbuf[(P - 1) & 1], nnz, m,
                     h->colptr_dev);
  if ((rc = check_launch(h, "colptr_from_sorted_kernel"))) return rc;
  if (hipStreamSynchronize(h->stream) != hipSuccess) { h->err = "CSC build failed on the device"; return HPF_ERR_HIP; }
  return HPF_OK;
}

// host digamma for the xi/eta Elog export (same series as the device one)
double host_digamma(double x)
{
  double acc = 0.0;
  while (x < 10.0) { acc -= 1.0 / x; x += 1.0; }
  const double xi = 1.0 / x, x2 = xi * xi;
  double s = x2 * (1.0 / 12 - x2 * (1.0 / 120 - x2 * (1.0 / 252 - x2 * (1.0 / 240 -
             x2 * (1.0 / 132 - x2 * (691.0 / 32760 - x2 * (1.0 / 12)))))));
  return acc + std::log(x) - 0.5 * xi - s;
}

// shape (prior added, in place) and E from the raw sums and the rate the last
// sweep used; needed by every consumer outside the hot loop (hpf_lazy::ES_*)
int refresh_es(hpf_handle *h, Side &s)
{
  if (s.rows) {
    const size_t ne = (size_t)s.rows * h->ld;
    const uint32_t blocks = (uint32_t)std::min<size_t>((ne + 255) / 256, 8192);
    hipLaunchKernelGGL(materialize_es_kernel, dim3(blocks), dim3(256), 0, h->stream, s.S, s.E, s.prior_used,
                       s.colsum_used, s.rows, h->ld, h->K, s.bias_col, s.bias_rate_add, h->cfg.s_prior,
                       h->cfg.r_prior, h->cfg.hier);
    if (int rc = check_launch(h, "materialize_es_kernel")) return rc;
  }
  h->lz.refreshed(h->side_of(s) ? hpf_lazy::ES_ITEMS : hpf_lazy::ES_USERS);
  return HPF_OK;
}

// rebuild Elog from shape and the rate the last sweep used (export only; hpf_lazy::ELOG_*)
int refresh_elog(hpf_handle *h, Side &s)
{
  if (s.rows) {
    const size_t ne = (size_t)s.rows * h->ld;
    const uint32_t blocks = (uint32_t)std::min<size_t>((ne + 255) / 256, 8192);
    hipLaunchKernelGGL(elog_kernel, dim3(blocks), dim3(256), 0, h->stream, s.S, s.prior_used,
                       s.colsum_used, s.L, s.rows, h->ld, h->K, s.bias_col, s.bias_rate_add,
                       h->cfg.r_prior, h->cfg.hier);
    if (int rc = check_launch(h, "elog_kernel")) return rc;
  }
  h->lz.refreshed(h->side_of(s) ? hpf_lazy::ELOG_ITEMS : hpf_lazy::ELOG_USERS);
  return HPF_OK;
}

// ---- what the report-step endpoints share -------------------------------------------------------------------------------
// the fields every scoring kernel's argument struct has
template <class Args>
void factor_args(const hpf_handle *h, Args &a)
{
  a.Et = h->u.E; a.Eb = h->it.E; a.ld = h->ld; a.K = h->K;
  a.ubias_col = h->cfg.bias ? h->u.bias_col : -1;
  a.ibias_col = h->cfg.bias ? h->it.bias_col : -1;
}
// the tail of a call: its outputs back to the host (a null dst is one the caller did not ask for), the stream idle
struct HostOut { void *dst; const void *src; size_t bytes; };
int copy_back(hpf_handle *h, std::initializer_list<HostOut> outs)
{
  hipError_t e = hipSuccess;
  for (const HostOut &o : outs) if (e == hipSuccess && o.dst) e = hipMemcpyAsync(o.dst, o.src, o.bytes, hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) { h->err = hipGetErrorString(e); return HPF_ERR_HIP; }
  return HPF_OK;
}

// What hpf_recommend and hpf_similar share: a streaming selection behind a sweep over the m rows of Eb (`sweep(nch, grid, a)`
// launches the caller's kernel) and a merge of each row's splits (topn_merge_kernel) -- per batch the candidate buffers
// (hpf_plan::topn_batch_users), nothing of n_sel x m.  `a` comes with the factor pointers, the bias columns and the bit rows
// of the caller; batch(b0, rows) readies the bit rows of a batch.  A list has `real` entries; the rest is padding.
// lists_dev: where a caller that goes on with the lists on the device (hpf_recommend_ucb) finds the items; c owns them.
// scores_dev: the same for the scores (hpf_recommend_diverse).
template <typename Batch, typename Sweep>
int topn_run(FusedCtx &c, TopnArgs a, uint32_t m, uint32_t n_sel, uint32_t topn, uint32_t real, const char *kernel,
             Batch &&batch, Sweep &&sweep, uint32_t *out_items, double *out_scores, uint32_t **lists_dev = nullptr,
             double **scores_dev = nullptr)
{
  hpf_handle *h = c.h; int rc;
  const uint32_t ntiles = (m + 63) / 64, cap = hpf_plan::topn_cap(topn), NP = hpf_plan::pow2_ceil(topn);
  static_assert(hpf_plan::topn_cap(hpf_plan::TOPN_FUSED_MAX) == TOPN_CAP_MAX, "a wave's LDS scratch holds the largest candidate buffer");
  c.batch = hpf_plan::topn_batch_users(m, n_sel, cap, h->loo_batch);      // <= the users the bit rows were sized for
  // segments (row, split) of a batch: a full batch's; a shorter last batch takes its own grid where that needs no more
  const hpf_plan::RankGrid gfull = hpf_plan::topn_grid(std::min(c.batch, n_sel), ntiles, cap);
  const size_t nseg = (size_t)c.batch * gfull.splits;
  uint32_t *d_items = nullptr; double *d_sc = nullptr;
  if ((rc = c.alloc(&a.ckey, nseg * cap)) || (rc = c.alloc(&a.citem, nseg * cap)) || (rc = c.alloc(&a.ccount, nseg)) ||
      (rc = c.alloc(&d_items, (size_t)n_sel * topn)) || (rc = c.alloc(&d_sc, (size_t)n_sel * topn))) return rc;
  if (lists_dev) *lists_dev = d_items;
  if (scores_dev) *scores_dev = d_sc;
  a.m = m; a.topn = topn; a.cap = cap; a.lg_cap = hpf_plan::log2_of(cap);
  const std::string what = std::string(kernel) + "/topn_merge_kernel";
  for (uint32_t b0 = 0; b0 < n_sel; b0 += c.batch) {
    const uint32_t rows = std::min(n_sel - b0, c.batch);
    if ((rc = batch(b0, rows))) return rc;
    hpf_plan::RankGrid g = hpf_plan::topn_grid(rows, ntiles, cap);
    if ((size_t)rows * g.splits > nseg) { g.splits = gfull.splits; g.tiles_per_split = gfull.tiles_per_split; }
    a.users = c.d_users + b0; a.out_items = d_items + (size_t)b0 * topn; a.out_scores = d_sc + (size_t)b0 * topn;
    a.n_sel = rows; a.tiles_per_split = g.tiles_per_split; a.splits = g.splits;
    if ((rc = launch_rank(h, kernel, [&](auto nch) {
          sweep(nch, dim3(g.blocks, g.splits), a);
          hipLaunchKernelGGL(topn_merge_kernel, dim3(rows), dim3(256), (size_t)NP * 12, h->stream, a, NP, real);
        }, what.c_str()))) return rc;
  }
  return copy_back(h, {{out_items, d_items, (size_t)n_sel * topn * 4}, {out_scores, d_sc, (size_t)n_sel * topn * 8}});
}

// W of the sides that follow a handed-in Elog (hpf_lazy::DERIVE_W)
int prepare_derived(hpf_handle *h)
{
  Side *sides[2] = {&h->u, &h->it};
  for (int attempt = 0; attempt < 2; ++attempt) {
    bool derived = false;
    for (Side *s : sides) {
      if (!h->lz.w_due(h->side_of(*s))) continue;
      h->lz.w_derived(h->side_of(*s));
      derived = true;
      const uint32_t blocks = std::min<uint32_t>((s->rows + 3) / 4, 4096);
      hipLaunchKernelGGL(derive_w_kernel, dim3(blocks), dim3(256), 0, h->stream, s->L, s->W,
                         h->wl != WL_PLAIN ? (uint32_t)h->wl : (uint32_t)h->w32,
                         s->rows, h->ld, h->K, s->bias_col, s->junk_col, packed_row(h->pk), h->flags);
    }
    if (!derived || h->wl != WL_P59) break;
    // an Elog spread above 88 inside a row: p59 cannot hold the state -- plain rows then, derived again (recover_flush)
    uint32_t f[2] = {0, 0};
    HIPCHK(h, hipMemcpyAsync(f, h->flags, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (!(f[0] & 2u)) break;
    { int rc0 = recover_flush(h, f[0], f[1]); if (rc0) return rc0; }
  }
  return HPF_OK;
}

// c[k] = sum_i E[beta_ik], consumed by the first user sweep; jacobi: sum_u E[theta] of the start state, which the first
// item rate uses (hpf_lazy::COLUMN_SUMS)
void start_column_sums(hpf_handle *h)
{
  for (Side *s : {&h->it, &h->u}) {
    if (s == &h->u && !h->jacobi) break;
    hipLaunchKernelGGL(colsum_partial_kernel, dim3(s->sweep_blocks), dim3(256), 0, h->stream, s->E, s->rows,
                       h->ld, h->K, s->colsum_part);
    hipLaunchKernelGGL(colsum_finalize_kernel, dim3(h->ld), dim3(256), 0, h->stream,
                       s->colsum_part, s->sweep_blocks, h->ld, s->colsum, h->flags);
  }
}

// hpf_lazy::EXCHANGE_START_SUMS
int exchange_start_sums(hpf_handle *h)
{
  if (h->comm) {                        // the library owns the exchange: the [ld] tail, in place, on the kernels' stream
    const size_t items = (size_t)h->it.rows * h->ld;
    const int rc2 = g_rccl.AllReduce(h->exch + items, h->exch + items, h->exch_count - items, 8, 0, h->comm, (void *)h->stream);
    if (rc2 != 0) { h->err = std::string("ncclAllReduce: ") + g_rccl.GetErrorString(rc2); return HPF_ERR_HIP; }
    if (int rc = check_comm_async(h)) return rc;
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));     // the caller's all-reduce may run on another stream
  h->lz.start_sums_handed(h->comm != nullptr);
  return HPF_OK;
}

// The one prologue of a call: what it names is current when this returns HPF_OK.  hpf_lazy::State::ask decides -- the
// error the call returns, or the deferred jobs and their order --, `validate` (the call's own argument checks) runs between
// the two, so that which error a bad call gets does not depend on the device, and each job has one executor here.
template <typename Validate>
int ready(hpf_handle *h, hpf_lazy::Need need, int side, int kind, Validate &&validate)
{
  const hpf_lazy::Todo todo = h->lz.ask(need, {h->phase, h->iterations, h->wl == WL_P59, h->comm != nullptr}, side, kind);
  if (todo.status) { h->err = todo.error; return todo.status; }
  int rc = validate();
  for (int j = 0; j < todo.n && !rc; ++j)
    switch (todo.job[j]) {
      case hpf_lazy::RECOVER: rc = recover_if_flushed(h); break;
      case hpf_lazy::REPORT: rc = check_flags(h); break;
      case hpf_lazy::ES_USERS: rc = refresh_es(h, h->u); break;
      case hpf_lazy::ES_ITEMS: rc = refresh_es(h, h->it); break;
      case hpf_lazy::ELOG_USERS: rc = refresh_elog(h, h->u); break;
      case hpf_lazy::ELOG_ITEMS: rc = refresh_elog(h, h->it); break;
      case hpf_lazy::DERIVE_W: rc = prepare_derived(h); break;
      case hpf_lazy::COLUMN_SUMS: start_column_sums(h); break;
      case hpf_lazy::DERIVED_DONE: if (!(rc = check_launch(h, "prepare_derived"))) h->lz.derived(); break;
      case hpf_lazy::EXCHANGE_START_SUMS: rc = exchange_start_sums(h); break;
      case hpf_lazy::N_JOBS: break;
    }
  return rc;
}
int ready(hpf_handle *h, hpf_lazy::Need need, int side = -1, int kind = -1) { return ready(h, need, side, kind, [] { return (int)HPF_OK; }); }

// rows of W in 16-byte pieces?
bool rows_in_pieces(const hpf_handle *h) { return h->wl != WL_PLAIN; }
// the arguments of a pass over own's segments and its workgroups (run_phi; hpf_gather_only, which sums nothing)
PhiLaunch phi_setup(const hpf_handle *h, const Side &own, const Side &oth, bool sums, PhiArgs &a)
{
  a.segs = own.segs; a.nseg = own.nseg; a.idx = own.pass_idx(); a.val = own.pass_val();
  a.W_own = own.W; a.W_oth = oth.W; a.S_own = sums ? own.S : nullptr; a.partial = sums ? own.partial : nullptr; a.flags = h->flags;
  a.chunks = own.chunks; a.ld = h->ld;
  a.epi = PhiArgs::Epi();
  if (sums && own.fused) {       // what this side's sweep reads (sweep_args; the user sweep's column sums are the item side's)
    a.epi.W_out = own.W; a.epi.prior_E = own.prior_E; a.epi.colsum_oth = oth.colsum;
    a.epi.s_prior = h->cfg.s_prior; a.epi.r_prior = h->cfg.r_prior; a.epi.rate_bias = h->cfg.r_prior + own.bias_rate_add;
    a.epi.K = h->K; a.epi.hier = h->cfg.hier; a.epi.bias_col = own.bias_col; a.epi.junk_col = own.junk_col;
  }
  const uint32_t wpb = rows_in_pieces(h) ? h->wg_of(own.chunks != nullptr) / 64 : 4;      // waves per workgroup
  const uint32_t blocks = own.chunks ? own.nchunk_blocks : std::min<uint32_t>((a.nseg + wpb - 1) / wpb, h->phi_blocks * (4 / wpb));
  return {blocks, wpb * 64, h->stream};
}
// after_kernel: recorded between the pass and its combines; null = not recorded (under capture, fold_sweeps)
int run_phi(hpf_handle *h, const Side &own, const Side &oth, hipEvent_t after_kernel)
{
  const int side = &own == &h->it ? 1 : 0;
  hipStream_t st = h->stream;
  PhiArgs a;
  const PhiLaunch pl = phi_setup(h, own, oth, true, a);
  if (a.nseg) {
    const bool ok = own.fused ? launch_phi_fused(h->phiG, h->phiR, a, pl)
                  : rows_in_pieces(h) ? launch_phi_packed(h->wl, h->phiG, h->phiR, side, a, pl)
                                      : launch_phi(h->w32, h->phiG, h->phiR, h->phiV, side, a, pl);
    if (!ok) { h->err = "no phi kernel for this configuration"; return HPF_ERR_UNSUPPORTED; }
  } else if (side == 1) {
    // the item-major pass opens an iteration (phi_pass_skips keeps the books of the fallback protocol): an empty one still does
    PhiArgs e = a; e.segs = nullptr; e.nseg = 0; e.chunks = nullptr;
    hipLaunchKernelGGL(phi_open_kernel, dim3(1), dim3(64), 0, st, e);
  }
  // the event separates the phi kernel from the combine that follows it
  if (after_kernel) HIPCHK(h, hipEventRecord(after_kernel, st));
  auto combine = [&](const LongRow *rows, uint32_t nrows, const double *src, double *dst) {
    hipLaunchKernelGGL(combine_partials_kernel, dim3(std::min<uint32_t>((nrows + 3) / 4, 16384)), dim3(256), 0, st,
                       rows, nrows, src, dst, h->ld, h->flags);
  };
  if (own.ngroup) combine(own.grouprows, own.ngroup, own.partial, own.partial2);     // level 1 of the very long rows: partial -> partial2
  if (own.nlong_wave) combine(own.longrows, own.nlong_wave, own.partial, own.S);
  if (own.nlong > own.nlong_wave)          // a tiled side's heavy rows (a partial per tile they meet): a workgroup each
    hipLaunchKernelGGL(combine_partials_wg_kernel, dim3(std::min<uint32_t>(own.nlong - own.nlong_wave, 65536)), dim3(256), (size_t)4 * h->ld * 8,
                       st, own.longrows + own.nlong_wave, own.nlong - own.nlong_wave, own.partial, own.S, h->ld, h->flags);
  if (own.nhuge) combine(own.hugerows, own.nhuge, own.partial2, own.S);              // level 2: partial2 -> S
  return check_launch(h, "phi pass");
}

// how the sweep of this handle writes W, and the arguments that do not change from launch to launch
void sweep_args(const hpf_handle *h, const Side &s, SweepArgs &a)
{
  a.S = s.S; a.W = s.W; a.w32 = h->w32;
  a.pk = packed_row(h->pk); a.flags = h->flags;
  a.prior_E = s.prior_E; a.prior_rate = s.prior_rate;
  a.psi_prior_shape = host_digamma(h->cfg.s_prior + (double)h->K * h->cfg.s_prior);
  a.colsum_part = s.colsum_part; a.colsum_used = s.colsum_used;
  a.rows = s.rows; a.ld = h->ld; a.K = h->K;
  a.bias_col = s.bias_col; a.junk_col = s.junk_col; a.bias_rate_add = s.bias_rate_add;
  a.s_prior = h->cfg.s_prior; a.r_prior = h->cfg.r_prior; a.hier = h->cfg.hier;
  a.row_done = s.row_done;
}

int run_sweep(hpf_handle *h, const Side &s, const double *colsum_oth, double *colsum_out)
{
  hipStream_t st = h->stream;
  SweepArgs a;
  sweep_args(h, s, a);
  a.colsum_oth = colsum_oth;                 // the kernel also copies it to colsum_used: what the rate was built from (export of *_rate.tsv)
  // after a pass with the fused epilogue: the sums of the rows it wrote, the full body for the rest
  if (!(s.fused ? launch_sums(h->sw_mode, h->swG, h->swR, a, s.sweep_blocks, st)
                : launch_sweep(h->sw_mode, h->swG, h->swR, a, s.sweep_blocks, st))) {
    h->err = "no sweep kernel for this configuration"; return HPF_ERR_UNSUPPORTED;
  }
  if (h->cfg.hier && s.rows)                // xi / eta: E and Elog from the rate the sweep just wrote
    hipLaunchKernelGGL(prior_update_kernel, dim3(std::min<uint32_t>((s.rows + 255) / 256, 4096)), dim3(256), 0, st,
                       s.prior_E, s.prior_used, s.prior_rate, s.prior_elog, s.prior_elog_used, s.rows,
                       h->cfg.s_prior + (double)h->K * h->cfg.s_prior, a.psi_prior_shape, h->flags);
  hipLaunchKernelGGL(colsum_finalize_kernel, dim3(h->ld), dim3(256), 0, st,
                     s.colsum_part, s.sweep_blocks, h->ld, colsum_out, h->flags);
  return check_launch(h, "row sweep");
}

// ---- one iteration: four steps, launched, captured and replayed alike ----------------------------------------------------
// The steps (hpf_plan::Step) in stream order, and the events of the ring slot each of them records (event 0, the start of
// the iteration, is begin_iteration's):
//   ITEMS_PASS   step A, item-major: beta shape sums, straight into the exchange buffer.  The two gather passes over the
//                same W_theta / W_beta are independent; this one runs first so that, with several ranks, its all-reduce
//                can overlap the whole user-side half of the iteration.      1 phi_item kernel done | 2 its combine done
//   USERS_PASS   step A, user-major: theta shape sums.                       3 phi_user kernel done | 4 its combine done
//   USERS_SWEEP  steps B (+D user, E): the theta rate uses c = sum_i E[beta]; emits d = sum_u E[theta] into the tail of
//                the exchange buffer.  Does not touch the item part of the exchange buffer, so its all-reduce may already
//                be running.  Carries the -novb copy of the old column sums.                               5 user sweep
//   ITEMS_SWEEP  steps C (+D item, F): the beta rate uses d (all-reduced when n_ranks > 1).
//                7 start of the replicated half (after whatever exchange the stream waited for) | 6 item sweep
// enqueue_step puts a step's kernels on the stream and writes no field of the handle or of a Side, so one body serves the
// eager launch and the capture.  step_done keeps the books of a step that IS on the stream, however it got there -- never
// under capture.  run_steps checks the call order (hpf_plan::next_phase) and does both for consecutive steps; handed an
// executable it replays that instead of launching, and the events inside the replayed piece coincide (a piece's time then
// sits in its first field).  A whole-iteration replay (replay_iteration) has events 0 and 6 only: ring_graphed.
using hpf_plan::Step;
void drop_graph(hpf_handle *h);

// events: the ring slot to record into, null under capture
int enqueue_step(hpf_handle *h, Step step, hipEvent_t *ev)
{
  int rc;
  hipStream_t st = h->stream;
  switch (step) {
    case Step::ITEMS_PASS:
      if ((rc = run_phi(h, h->it, h->u, ev ? ev[1] : nullptr))) return rc;
      if (ev) HIPCHK(h, hipEventRecord(ev[2], st));
      break;
    case Step::USERS_PASS:
      if ((rc = run_phi(h, h->u, h->it, ev ? ev[3] : nullptr))) return rc;
      if (ev) HIPCHK(h, hipEventRecord(ev[4], st));
      break;
    case Step::USERS_SWEEP:
      if (h->jacobi)      // keep what _theta.sum_rows() still returns before _theta.swap() (hgaprec.cc:1281-1282)
        HIPCHK(h, hipMemcpyAsync(h->u_colsum_prev, h->u.colsum, (size_t)h->ld * 8, hipMemcpyDeviceToDevice, st));
      if ((rc = run_sweep(h, h->u, h->it.colsum, h->u.colsum))) return rc;
      if (ev) HIPCHK(h, hipEventRecord(ev[5], st));
      break;
    case Step::ITEMS_SWEEP:
      if (ev) HIPCHK(h, hipEventRecord(ev[7], st));
      if ((rc = run_sweep(h, h->it, h->jacobi ? h->u_colsum_prev : h->u.colsum, h->it.colsum))) return rc;
      if (ev) HIPCHK(h, hipEventRecord(ev[6], st));
      break;
  }
  return HPF_OK;
}

void step_done(hpf_handle *h, Step step)
{
  h->phase = hpf_plan::next_phase(h->phase, step);
  if (step == Step::USERS_SWEEP) h->lz.swept(hpf_lazy::USERS);
  if (step != Step::ITEMS_SWEEP) return;
  h->lz.swept(hpf_lazy::ITEMS);
  h->replaying = false;
  h->ev_count++;
  h->iterations++;
  h->iters_counted++;
}

// The steps first..last captured into an executable (the kernels' arguments stay fixed until the CSR, the rows' layout or
// the exchange buffer change: drop_graph there).  A failure leaves the handle as it was, without graphs.
int capture_steps(hpf_handle *h, Step first, Step last, hipGraphExec_t *exec)
{
  hipGraph_t g = nullptr;
  HIPCHK(h, hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
  int rc = HPF_OK;
  for (int s = first; s <= last && !rc; ++s) rc = enqueue_step(h, (Step)s, nullptr);
  hipError_t e = hipStreamEndCapture(h->stream, &g);
  if (!rc && e != hipSuccess) { h->err = std::string("hipStreamEndCapture: ") + hipGetErrorString(e); rc = HPF_ERR_HIP; }
  if (!rc && (e = hipGraphInstantiate(exec, g, nullptr, nullptr, 0)) != hipSuccess) {
    *exec = nullptr; h->err = std::string("hipGraphInstantiate: ") + hipGetErrorString(e); rc = HPF_ERR_HIP;
  }
  if (g) (void)hipGraphDestroy(g);
  if (rc) drop_graph(h);
  return rc;
}

// The consecutive steps first..last: call order, stream, books.  exec: a graph of exactly these steps to replay in their
// place, or null.
int run_steps(hpf_handle *h, Step first, Step last, hipGraphExec_t exec)
{
  int rc, ph = h->phase;
  for (int s = first; s <= last; ++s)
    if ((ph = hpf_plan::next_phase(ph, (Step)s)) < 0) { h->err = "call order: items pass, users pass, user sweep, iterate_global"; return HPF_ERR_STATE; }
  if (!exec) {
    for (int s = first; s <= last; ++s) {
      if ((rc = enqueue_step(h, (Step)s, h->ev))) return rc;
      step_done(h, (Step)s);
    }
    return HPF_OK;
  }
  if (first == Step::ITEMS_SWEEP) HIPCHK(h, hipEventRecord(h->ev[7], h->stream));
  HIPCHK(h, hipGraphLaunch(exec, h->stream));
  static const int first_event[4] = {1, 3, 5, 6}, last_event[4] = {2, 4, 5, 6};
  for (int j = first_event[first]; j <= last_event[last]; ++j) HIPCHK(h, hipEventRecord(h->ev[j], h->stream));
  for (int s = first; s <= last; ++s) step_done(h, (Step)s);
  return HPF_OK;
}

// The cut the piece graphs are captured along: items pass | users pass + user sweep | item sweep.
// OPT-IN (HPF_GRAPH=1 under HPF_EXPERIMENTAL), never chosen by the library: measured on MI355X (profiles/r06/experiments.md 4)
// the three replays buy nothing where the pieces are long -- an eighth of C4, 2.50 ms eager against 2.51 -- and LOSE where they
// are short -- C1 through the pieces: 0.101 ms eager, 0.127 replayed: a replay costs the host 10-16 us, three of them more than
// the eleven eager launches they stand for, which the host issues ahead of the device anyway.  (One graph for a whole
// iteration -- one rank -- does pay: 0.085 ms.)
bool split_graph_on(const hpf_handle *h) { return !h->in_recovery && h->graph_mode == 1; }

constexpr Step PIECE[3][2] = {{Step::ITEMS_PASS, Step::ITEMS_PASS}, {Step::USERS_PASS, Step::USERS_SWEEP}, {Step::ITEMS_SWEEP, Step::ITEMS_SWEEP}};
hipGraphExec_t piece_graph(const hpf_handle *h, int k) { return h->replaying ? h->split_exec[k] : nullptr; }   // null once dropped: the piece then runs eagerly

// How the iteration about to begin wants to run.  PIECES: the caller goes on with hpf_iterate_local_users and
// hpf_iterate_global (granted where split_graph_on).  WHOLE: hpf_iterate on one rank (want_graph).
enum Replay { EAGER, PIECES, WHOLE };

// What precedes the first step of an iteration: the state the kernels read is in place, the graphs the iteration will
// replay exist, its ring slot is chosen and event 0 recorded.
int begin_iteration(hpf_handle *h, Replay want)
{
  int rc;
  if (!h->have_csr) { h->err = "hpf_upload_csr has not been called"; return HPF_ERR_STATE; }
  if ((rc = ready(h, hpf_lazy::ITERATION))) return rc;
  if (want == PIECES && !split_graph_on(h)) want = EAGER;
  for (int k = 0; want == PIECES && k < 3; ++k)
    if (!h->split_exec[k] && (rc = capture_steps(h, PIECE[k][0], PIECE[k][1], &h->split_exec[k]))) return rc;
  if (want == WHOLE && !h->graph_exec && (rc = capture_steps(h, Step::ITEMS_PASS, Step::ITEMS_SWEEP, &h->graph_exec))) return rc;
  const uint32_t slot = h->ev_count % hpf_handle::RING;
  h->lz.iteration_begun();
  h->ev = h->evr[slot];
  h->ring_graphed[slot] = want == WHOLE;
  h->replaying = want == PIECES;
  HIPCHK(h, hipEventRecord(h->ev[0], h->stream));
  return HPF_OK;
}

int items_pass(hpf_handle *h, Replay want)
{
  const int rc = begin_iteration(h, want);
  return rc ? rc : run_steps(h, Step::ITEMS_PASS, Step::ITEMS_PASS, piece_graph(h, 0));
}
int iterate_local_users(hpf_handle *h) { return run_steps(h, Step::USERS_PASS, Step::USERS_SWEEP, piece_graph(h, 1)); }
int iterate_global(hpf_handle *h) { return run_steps(h, Step::ITEMS_SWEEP, Step::ITEMS_SWEEP, piece_graph(h, 2)); }
int iterate_local(hpf_handle *h)
{
  const int rc = items_pass(h, EAGER);
  return rc ? rc : run_steps(h, Step::USERS_PASS, Step::USERS_SWEEP, nullptr);
}
// one launch for the whole iteration: only its start and its end are timed
int replay_iteration(hpf_handle *h)
{
  int rc;
  if ((rc = begin_iteration(h, WHOLE))) return rc;
  HIPCHK(h, hipGraphLaunch(h->graph_exec, h->stream));
  HIPCHK(h, hipEventRecord(h->ev[6], h->stream));
  for (int s = Step::ITEMS_PASS; s <= Step::ITEMS_SWEEP; ++s) step_done(h, (Step)s);
  return HPF_OK;
}

// p59 rows -> plain doubles in the same shape (codec_f64): W reallocated, the work lists cut again
// for the new row size -- exactly what a handle created with w_storage = 3 holds
int set_rows_f64(hpf_handle *h)
{
  int rc;
  drop_graph(h);
  static_cast<Plan &>(*h) = h->as_plain_doubles();
  Side *sides[2] = {&h->u, &h->it};
  for (Side *s : sides) {
    dfree(s->W); s->W = nullptr;
    unsigned char *w = nullptr;
    if ((rc = dalloc(h, &w, w_bytes(h, s->rows)))) return rc;
    s->W = w;
  }
  if (h->have_csr) {
    if ((rc = device_side_work(h, h->u, h->rowptr_dev, h->u.rows))) return rc;
    if ((rc = device_side_work(h, h->it, h->colptr_dev, h->it.rows))) return rc;
    if ((rc = build_work_lists_tiled(h, h->nnz))) return rc;
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return HPF_OK;
}

// recover_flush between setting and clearing hpf_handle::in_recovery; redo: the iterations the passes skipped
int redo_in_plain_rows(hpf_handle *h, uint32_t fl0, uint64_t redo)
{
  int rc;
  if ((rc = set_rows_f64(h))) return rc;
  const uint32_t clear[2] = {fl0 & 1u, 0u};
  if (hipMemcpyAsync(h->flags, clear, 8, hipMemcpyHostToDevice, h->stream) != hipSuccess) { h->err = "recover_flush: cannot reset the flags"; return HPF_ERR_HIP; }
  h->iters_counted = 0;
  Side *sides[2] = {&h->u, &h->it};
  for (Side *s : sides) {
    const hpf_lazy::Repair how = h->lz.fell_back(h->side_of(*s));
    if (how == hpf_lazy::REPAIR_NOTHING || how == hpf_lazy::REPAIR_FROM_ELOG) continue;      // from Elog: the next DERIVE_W
    SweepArgs a;
    sweep_args(h, *s, a);
    a.prior_E = s->prior_used; a.colsum_oth = s->colsum_used; a.colsum_used = nullptr;             // what that sweep read
    if (how == hpf_lazy::REPAIR_REPEAT_ON_SHAPE) a.s_prior = 0.0;      // S is the shape (prior added, in place) already
    if (!launch_sweep(h->sw_mode, h->swG, h->swR, a, s->sweep_blocks, h->stream)) { h->err = "no sweep kernel for this configuration"; return HPF_ERR_UNSUPPORTED; }
  }
  if ((rc = check_launch(h, "repeat of the sweeps in plain rows"))) return rc;
  h->fallbacks++;
  if (redo) {
    if (h->cfg.n_ranks != 1) { h->err = "internal: iterations were skipped on a rank of several"; return HPF_ERR_STATE; }
    h->iterations -= (uint32_t)std::min<uint64_t>(redo, h->iterations);
    for (uint64_t t = 0; t < redo; ++t) if ((rc = iterate_local(h)) || (rc = iterate_global(h))) return rc;
  }
  if (hipStreamSynchronize(h->stream) != hipSuccess) { h->err = "recover_flush: stream error"; return HPF_ERR_HIP; }
  return HPF_OK;
}

// Flag bit 1: an element of W fell below 2^-126 of its row maximum (an Elog spread above 88 inside a row) and the p59
// rows cannot hold it.  The layout is lossless by contract, and the library holds everything it takes to go on without
// it: the rows become plain doubles, W is written again -- by a W-ONLY repeat of the side's last sweep (same S, the prior
// and the column sums that sweep used: the same arithmetic, so the same bits a w_storage = 3 handle has) or by derive_w
// where W came from a handed-in Elog -- and the iterations the passes skipped in the meantime are run.
// fl0 / begun: the device's flag word and its count of iterations begun; the stream is synchronised.
int recover_flush(hpf_handle *h, uint32_t fl0, uint32_t begun)
{
  if (h->wl != WL_P59) { h->err = "internal: an entry of W was reported flushed, but the rows are not packed"; return HPF_ERR_STATE; }
  const uint64_t redo = h->iters_counted > (uint64_t)begun ? h->iters_counted - (uint64_t)begun : 0;   // several ranks: none (the host looks every iteration)
  h->in_recovery = true;
  const int rc = redo_in_plain_rows(h, fl0, redo);
  h->in_recovery = false;
  return rc;
}

void drop_graph(hpf_handle *h)
{
  if (h->graph_exec) { (void)hipGraphExecDestroy(h->graph_exec); h->graph_exec = nullptr; }
  for (int k = 0; k < 3; ++k) if (h->split_exec[k]) { (void)hipGraphExecDestroy(h->split_exec[k]); h->split_exec[k] = nullptr; }
}

bool want_graph(const hpf_handle *h)
{
  if (h->graph_mode >= 0) return h->graph_mode == 1;
  return h->nnz <= h->graph_nnz_max;
}

}  // namespace

// ---------------------------------------------------------------------------
extern "C" {

int hpf_abi_version(void) { return HPF_ABI_VERSION; }

const char *hpf_strerror(int st)
{
  switch (st) {
    case HPF_OK: return "ok";
    case HPF_ERR_INVALID: return "invalid argument or call order";
    case HPF_ERR_NO_DEVICE: return "no usable HIP device";
    case HPF_ERR_OOM: return "out of memory";
    case HPF_ERR_HIP: return "HIP runtime error";
    case HPF_ERR_UNSUPPORTED: return "unsupported configuration";
    case HPF_ERR_STATE: return "model state not initialised";
  }
  return "unknown status";
}

const char *hpf_last_error(const hpf_handle *h) { return h ? h->err.c_str() : "null handle"; }

int hpf_create(const hpf_config *cfg, hpf_handle **out)
{
  if (!cfg || !out) return HPF_ERR_INVALID;
  *out = nullptr;
  if (cfg->struct_size != sizeof(hpf_config)) return HPF_ERR_INVALID;
  if (cfg->K == 0 || cfg->n_items == 0) return HPF_ERR_INVALID;
  if (cfg->n_ranks == 0 || cfg->rank >= cfg->n_ranks) return HPF_ERR_INVALID;
  const bool jacobi = cfg->novb && cfg->bias && !cfg->hier;       // the only place the reference reads Env::vb
  const uint32_t C = cfg->K + (cfg->bias ? 2u : 0u);
  if (C > HPF_MAX_COLUMNS) return HPF_ERR_UNSUPPORTED;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return HPF_ERR_NO_DEVICE;
  if (cfg->device < 0 || cfg->device >= ndev) return HPF_ERR_NO_DEVICE;
  if (hipSetDevice(cfg->device) != hipSuccess) return HPF_ERR_NO_DEVICE;

  if (cfg->w_storage > 3 || cfg->tiling > 1) return HPF_ERR_INVALID;
  const Knobs knobs = hpf_plan::read_knobs();
  Plan plan;
  if (int rc = hpf_plan::plan_shapes(C, cfg->w_storage, knobs, &plan)) return rc;

  hpf_handle *h = new (std::nothrow) hpf_handle();
  if (!h) return HPF_ERR_OOM;
  static_cast<Plan &>(*h) = plan;
  static_cast<Knobs &>(*h) = knobs;
  h->cfg = *cfg;
  if (h->cfg.n_users_total == 0) h->cfg.n_users_total = cfg->n_users;
  if (h->cfg.s_prior <= 0) h->cfg.s_prior = 0.3;
  if (h->cfg.r_prior <= 0) h->cfg.r_prior = 0.3;
  h->K = cfg->K; h->C = C;

  auto fail = [&](int rc) { hpf_destroy(h); return rc; };
  if (cfg->stream) h->stream = (hipStream_t)cfg->stream;
  else {
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) return fail(HPF_ERR_HIP);
    h->own_stream = true;
  }
  for (uint32_t r = 0; r < hpf_handle::RING; ++r)
    for (int e = 0; e < 8; ++e)
      if (hipEventCreate(&h->evr[r][e]) != hipSuccess) return fail(HPF_ERR_HIP);

  const uint32_t n = cfg->n_users, m = cfg->n_items, ld = h->ld;
  h->u.rows = n; h->it.rows = m;
  if (cfg->bias) {
    h->u.bias_col = (int32_t)h->K;      h->u.junk_col = (int32_t)h->K + 1;
    h->it.bias_col = (int32_t)h->K + 1; h->it.junk_col = (int32_t)h->K;
    h->u.bias_rate_add = (double)m;                       // hgaprec.cc:1389 (0.3 + m)
    h->it.bias_rate_add = (double)h->cfg.n_users_total;   // hgaprec.cc:1393 (0.3 + n)
  }
  int rc;
  Side *sides[2] = {&h->u, &h->it};
  for (Side *s : sides) {
    const size_t ne = (size_t)s->rows * ld;
    const uint32_t gpb = 256u / (uint32_t)h->swG;         // groups (rows) per block
    s->sweep_blocks = std::max<uint32_t>(1, std::min<uint32_t>((s->rows + gpb - 1) / gpb, h->sweep_blocks_max));
    if (s == &h->u) { if ((rc = dalloc(h, &s->S, ne))) return fail(rc); }
    if ((rc = dalloc(h, &s->E, ne))) return fail(rc);
    if ((rc = dalloc(h, &s->L, ne))) return fail(rc);
    { unsigned char *w = nullptr; if ((rc = dalloc(h, &w, w_bytes(h, s->rows)))) return fail(rc); s->W = w; }
    if ((rc = dalloc(h, &s->prior_E, s->rows))) return fail(rc);
    if ((rc = dalloc(h, &s->prior_used, s->rows))) return fail(rc);
    if ((rc = dalloc(h, &s->prior_rate, s->rows))) return fail(rc);
    if ((rc = dalloc(h, &s->prior_elog, s->rows))) return fail(rc);
    if ((rc = dalloc(h, &s->prior_elog_used, s->rows))) return fail(rc);
    if ((rc = dalloc(h, &s->colsum_used, ld))) return fail(rc);
    if ((rc = dalloc(h, &s->colsum_part, (size_t)s->sweep_blocks * ld))) return fail(rc);
  }
  // exchange buffer: item S rows | sum_u E[theta]   (+ item colsum kept apart)
  h->exch_count = (size_t)m * ld + ld;
  if ((rc = dalloc(h, &h->exch, h->exch_count))) return fail(rc);
  h->it.S = h->exch; h->u.colsum = h->exch + (size_t)m * ld;
  if ((rc = dalloc(h, &h->it.colsum, ld))) return fail(rc);
  h->jacobi = jacobi;
  {
    hpf_lazy::Config lc;
    lc.hier = cfg->hier != 0; lc.bias = cfg->bias != 0; lc.jacobi = jacobi; lc.several = cfg->n_ranks > 1;
    lc.rows[hpf_lazy::USERS] = n != 0; lc.rows[hpf_lazy::ITEMS] = m != 0;
    h->lz = hpf_lazy::State(lc);
  }
  if ((rc = dalloc(h, &h->u_colsum_prev, ld))) return fail(rc);
  // log y! as HGAPRec::log_factorial does it (hgaprec.cc:1563-1570)
  {
    double lf[256];
    logfact_table(lf);
    if ((rc = dalloc(h, &h->logfact, 256))) return fail(rc);
    if ((rc = dalloc(h, &h->flags, 4))) return fail(rc);
    if (hipMemcpyAsync(h->logfact, lf, sizeof lf, hipMemcpyHostToDevice, h->stream) != hipSuccess) return fail(HPF_ERR_HIP);
  }
  if (hipStreamSynchronize(h->stream) != hipSuccess) return fail(HPF_ERR_HIP);
  *out = h;
  return HPF_OK;
}

void hpf_destroy(hpf_handle *h)
{
  if (!h) return;
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  if (h->comm && g_rccl.CommDestroy) { (void)g_rccl.CommDestroy(h->comm); h->comm = nullptr; }
  drop_graph(h);
  if (h->comm_stream) {
    (void)hipStreamSynchronize(h->comm_stream);
    (void)hipEventDestroy(h->ev_ready); (void)hipEventDestroy(h->ev_reduced);
    (void)hipStreamDestroy(h->comm_stream);
  }
  double *ucol = h->u.colsum;  (void)ucol;      // lives inside exch
  h->u.colsum = nullptr;
  double *icol = h->it.colsum; h->it.colsum = nullptr;
  free_side(h->u, false);
  free_side(h->it, true);
  dfree(icol);
  if (!h->exch_external) dfree(h->exch);
  dfree(h->logfact); dfree(h->rowptr_dev); dfree(h->colptr_dev); dfree(h->flags); dfree(h->u_colsum_prev);
  for (int k = 0; k < HPF_HELDOUT_SLOTS; ++k) free_held(h->held[k]);
  for (int k = 0; k < 8; ++k) if (h->held_ev[k]) (void)hipEventDestroy(h->held_ev[k]);
  for (int k = 0; k < 2; ++k) {
    if (h->stage[k]) (void)hipHostFree(h->stage[k]);
    if (h->stage_ev[k]) (void)hipEventDestroy(h->stage_ev[k]);
  }
  for (uint32_t r = 0; r < hpf_handle::RING; ++r)
    for (int e = 0; e < 8; ++e) if (h->evr[r][e]) (void)hipEventDestroy(h->evr[r][e]);
  if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

int hpf_bind_exchange_buffer(hpf_handle *h, void *dev, size_t count)
{
  if (!h || !dev) return HPF_ERR_INVALID;
  if (count < h->exch_count || ((uintptr_t)dev & 15u)) { h->err = "exchange buffer too small or misaligned"; return HPF_ERR_INVALID; }
  if (h->have_csr || h->iterations) { h->err = "bind the exchange buffer before hpf_upload_csr"; return HPF_ERR_INVALID; }
  HIPCHK(h, hipMemsetAsync(dev, 0, h->exch_count * 8, h->stream));
  // keep any item shapes already handed in
  HIPCHK(h, hipMemcpyAsync(dev, h->exch, h->exch_count * 8, hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (!h->exch_external) dfree(h->exch);
  h->exch = (double *)dev; h->exch_external = true;
  h->it.S = h->exch; h->u.colsum = h->exch + (size_t)h->it.rows * h->ld;
  return HPF_OK;
}

int hpf_comm_unique_id(void *id_out)
{
  if (!id_out) return HPF_ERR_INVALID;
  if (load_rccl()) return HPF_ERR_UNSUPPORTED;
  return g_rccl.GetUniqueId(id_out) == 0 ? HPF_OK : HPF_ERR_HIP;
}

int hpf_comm_init(hpf_handle *h, const void *id)
{
  if (!h || !id) return HPF_ERR_INVALID;
  if (h->comm) { h->err = "communicator already initialised"; return HPF_ERR_INVALID; }
  if (const char *e = load_rccl()) { h->err = e; return HPF_ERR_UNSUPPORTED; }
  IdByValue v; memcpy(v.internal, id, HPF_COMM_ID_BYTES);
  HIPCHK(h, hipSetDevice(h->cfg.device));
  const int rc = g_rccl.CommInitRank(&h->comm, (int)h->cfg.n_ranks, v, (int)h->cfg.rank);
  if (rc != 0) { h->comm = nullptr; h->err = std::string("ncclCommInitRank: ") + g_rccl.GetErrorString(rc); return HPF_ERR_HIP; }
  return HPF_OK;
}

int hpf_allreduce_items_begin(hpf_handle *h)
{
  if (!h) return HPF_ERR_INVALID;
  if (!h->comm) { h->err = "hpf_comm_init has not been called"; return HPF_ERR_STATE; }
  if (h->phase != 1) { h->err = "hpf_allreduce_items_begin follows hpf_iterate_local_items"; return HPF_ERR_STATE; }
  if (!h->comm_stream) {
    HIPCHK(h, hipStreamCreateWithFlags(&h->comm_stream, hipStreamNonBlocking));
    HIPCHK(h, hipEventCreateWithFlags(&h->ev_ready, hipEventDisableTiming));
    HIPCHK(h, hipEventCreateWithFlags(&h->ev_reduced, hipEventDisableTiming));
  }
  HIPCHK(h, hipEventRecord(h->ev_ready, h->stream));                 // item sums are final here
  HIPCHK(h, hipStreamWaitEvent(h->comm_stream, h->ev_ready, 0));
  const size_t items = (size_t)h->it.rows * h->ld;
  const int rc = g_rccl.AllReduce(h->exch, h->exch, items, 8, 0, h->comm, (void *)h->comm_stream);
  if (rc != 0) { h->err = std::string("ncclAllReduce: ") + g_rccl.GetErrorString(rc); return HPF_ERR_HIP; }
  h->items_reduce_pending = true;
  return HPF_OK;
}

int hpf_allreduce_exchange(hpf_handle *h)
{
  if (!h) return HPF_ERR_INVALID;
  if (!h->comm) { h->err = "hpf_comm_init has not been called"; return HPF_ERR_STATE; }
  // ncclDouble = 8, ncclSum = 0 (rccl.h:448,467); in place
  if (!h->items_reduce_pending) {               // everything at once, on the stream the kernels use
    const int rc = g_rccl.AllReduce(h->exch, h->exch, h->exch_count, 8, 0, h->comm, (void *)h->stream);
    if (rc != 0) { h->err = std::string("ncclAllReduce: ") + g_rccl.GetErrorString(rc); return HPF_ERR_HIP; }
    return check_comm_async(h);
  }
  // the item part is already on its way: add the [ld] tail (sum_u E[theta]), then
  // let the kernels' stream wait for both
  const size_t items = (size_t)h->it.rows * h->ld;
  HIPCHK(h, hipEventRecord(h->ev_ready, h->stream));
  HIPCHK(h, hipStreamWaitEvent(h->comm_stream, h->ev_ready, 0));
  const int rc = g_rccl.AllReduce(h->exch + items, h->exch + items, h->exch_count - items, 8, 0, h->comm,
                                  (void *)h->comm_stream);
  if (rc != 0) { h->err = std::string("ncclAllReduce: ") + g_rccl.GetErrorString(rc); return HPF_ERR_HIP; }
  HIPCHK(h, hipEventRecord(h->ev_reduced, h->comm_stream));
  HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_reduced, 0));
  h->items_reduce_pending = false;
  return check_comm_async(h);
}

int hpf_start_sums(hpf_handle *h)
{
  if (!h) return HPF_ERR_INVALID;
  if (!h->have_csr) { h->err = "hpf_upload_csr has not been called"; return HPF_ERR_STATE; }
  return ready(h, hpf_lazy::START_SUMS);
}

int hpf_exchange_read(hpf_handle *h, double *host, size_t count)
{
  if (!h || !host || count != h->exch_count) return HPF_ERR_INVALID;
  { int rc = ready(h, hpf_lazy::SWEEP_VECTORS); if (rc) return rc; }
  HIPCHK(h, hipMemcpyAsync(host, h->exch, count * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return HPF_OK;
}

int hpf_exchange_write(hpf_handle *h, const double *host, size_t count)
{
  if (!h || !host || count != h->exch_count) return HPF_ERR_INVALID;
  HIPCHK(h, hipMemcpyAsync(h->exch, host, count * 8, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return HPF_OK;
}

int hpf_exchange_buffer(hpf_handle *h, void **dev, size_t *count)
{
  if (!h || !dev || !count) return HPF_ERR_INVALID;
  *dev = h->exch; *count = h->exch_count;
  return HPF_OK;
}

// common tail of both uploads: h->u.idx / h->u.val / h->rowptr_dev are in place
static int finish_upload(hpf_handle *h, uint64_t nnz)
{
  const uint32_t n = h->u.rows, m = h->it.rows;
  int rc;
  if ((rc = build_csc_device(h, n, m, nnz))) return rc;
  int64_t last = 0;
  HIPCHK(h, hipMemcpyAsync(&last, h->colptr_dev + m, 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if ((uint64_t)last != nnz) { h->err = "internal: item-major view lost nonzeros"; return HPF_ERR_HIP; }
  if ((rc = device_side_work(h, h->u, h->rowptr_dev, n))) return rc;
  if ((rc = device_side_work(h, h->it, h->colptr_dev, m))) return rc;
  if ((rc = build_work_lists_tiled(h, nnz))) return rc;
  HIPCHK(h, hipMemsetAsync(h->flags, 0, 8, h->stream));
  h->iters_counted = 0;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->nnz = nnz; h->have_csr = true;
  return HPF_OK;
}

static int check_rowptr(hpf_handle *h, const int64_t *rowptr, uint32_t n)
{
  if (rowptr[0] != 0) { h->err = "rowptr[0] must be 0"; return HPF_ERR_INVALID; }
  for (uint32_t r = 0; r < n; ++r)
    if (rowptr[r + 1] < rowptr[r]) { h->err = "rowptr not monotone"; return HPF_ERR_INVALID; }
  return HPF_OK;
}

static int alloc_user_nonzeros(hpf_handle *h, uint64_t nnz, bool with_val)
{
  int rc;
  drop_graph(h);
  h->have_csr = false;
  dfree(h->u.idx); dfree(h->u.val); h->u.idx = nullptr; h->u.val = nullptr;
  dfree(h->rowptr_dev); h->rowptr_dev = nullptr;
  if ((rc = dalloc(h, &h->u.idx, (size_t)nnz))) return rc;
  if (with_val && (rc = dalloc(h, &h->u.val, (size_t)nnz))) return rc;
  return dalloc(h, &h->rowptr_dev, (size_t)h->u.rows + 1);
}

int hpf_upload_csr(hpf_handle *h, const int64_t *rowptr, const uint32_t *col, const uint8_t *val)
{
  if (!h || !rowptr) return HPF_ERR_INVALID;
  const uint32_t n = h->u.rows;
  int rc;
  if ((rc = check_rowptr(h, rowptr, n))) return rc;
  const uint64_t nnz = (uint64_t)rowptr[n];
  if (nnz && !col) return HPF_ERR_INVALID;
  if ((rc = alloc_user_nonzeros(h, nnz, val != nullptr))) return rc;
  if ((rc = h2d(h, h->u.idx, col, nnz * 4))) return rc;
  if (val && (rc = h2d(h, h->u.val, val, nnz))) return rc;
  if ((rc = h2d(h, h->rowptr_dev, rowptr, ((size_t)n + 1) * 8))) return rc;
  return finish_upload(h, nnz);
}

int hpf_upload_csr_device(hpf_handle *h, const int64_t *d_rowptr, const uint32_t *d_col, const uint8_t *d_val)
{
  if (!h || !d_rowptr) return HPF_ERR_INVALID;
  const uint32_t n = h->u.rows;
  int rc;
  // only the two ends of the row pointers come to the host; monotonicity is checked on the
  // device while the work lists are cut (seg_plan_kernel)
  int64_t ends[2] = {0, 0};
  HIPCHK(h, hipMemcpyAsync(&ends[0], d_rowptr, 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(&ends[1], d_rowptr + n, 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (ends[0] != 0) { h->err = "rowptr[0] must be 0"; return HPF_ERR_INVALID; }
  if (ends[1] < 0) { h->err = "rowptr not monotone"; return HPF_ERR_INVALID; }
  const uint64_t nnz = (uint64_t)ends[1];
  if (nnz && !d_col) return HPF_ERR_INVALID;
  if ((rc = alloc_user_nonzeros(h, nnz, d_val != nullptr))) return rc;
  if (nnz) HIPCHK(h, hipMemcpyAsync(h->u.idx, d_col, nnz * 4, hipMemcpyDeviceToDevice, h->stream));
  if (nnz && d_val) HIPCHK(h, hipMemcpyAsync(h->u.val, d_val, nnz, hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(h->rowptr_dev, d_rowptr, ((size_t)n + 1) * 8, hipMemcpyDeviceToDevice, h->stream));
  // the sort's first pass bisects the row pointers: they must be monotone BEFORE it runs
  {
    Scratch sc(h);
    uint32_t *bad = nullptr; uint32_t hb = 0;
    if ((rc = sc.alloc(&bad, 1))) return rc;
    hipLaunchKernelGGL(rowptr_check_kernel, dim3(grid_for(n)), dim3(256), 0, h->stream, h->rowptr_dev, n, bad);
    hipError_t e = hipMemcpyAsync(&hb, bad, 4, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) { h->err = std::string("rowptr check: ") + hipGetErrorString(e); return HPF_ERR_HIP; }
    if (hb) { h->err = "rowptr not monotone"; return HPF_ERR_INVALID; }
  }
  return finish_upload(h, nnz);
}

int hpf_get_csc(hpf_handle *h, int64_t *colptr, uint32_t *users, uint8_t *vals)
{
  if (!h) return HPF_ERR_INVALID;
  if (!h->have_csr) { h->err = "hpf_upload_csr has not been called"; return HPF_ERR_STATE; }
  int rc;
  if (colptr && (rc = d2h(h, colptr, h->colptr_dev, ((size_t)h->it.rows + 1) * 8))) return rc;
  if (users && (rc = d2h(h, users, h->it.idx, (size_t)h->nnz * 4))) return rc;
  if (vals) {
    if (!h->it.val) { h->err = "no ratings were uploaded (-binary-data)"; return HPF_ERR_INVALID; }
    if ((rc = d2h(h, vals, h->it.val, (size_t)h->nnz))) return rc;
  }
  return HPF_OK;
}

static int state_dims(const hpf_handle *h, int which, Side **side, uint32_t *rows, uint32_t *cols,
                      int *col0, int *kind)
{
  const int obj = which / 4; *kind = which % 4;
  hpf_handle *hh = const_cast<hpf_handle *>(h);
  switch (obj) {
    case 0: *side = &hh->u;  *rows = h->u.rows;  *cols = h->K; *col0 = 0; return 0;
    case 1: *side = &hh->it; *rows = h->it.rows; *cols = h->K; *col0 = 0; return 0;
    case 2: if (!h->cfg.hier) return -1; *side = &hh->u;  *rows = h->u.rows;  *cols = 1; *col0 = -1; return 0;
    case 3: if (!h->cfg.hier) return -1; *side = &hh->it; *rows = h->it.rows; *cols = 1; *col0 = -1; return 0;
    case 4: if (!h->cfg.bias) return -1; *side = &hh->u;  *rows = h->u.rows;  *cols = 1; *col0 = h->u.bias_col; return 0;
    case 5: if (!h->cfg.bias) return -1; *side = &hh->it; *rows = h->it.rows; *cols = 1; *col0 = h->it.bias_col; return 0;
  }
  return -1;
}

// on_device: `host` is a device pointer (hpf_set_state_device)
static int set_state_impl(hpf_handle *h, hpf_state which, const double *host, size_t count, bool on_device)
{
  if (!h || !host || which < 0 || which >= HPF_NUM_STATE) return HPF_ERR_INVALID;
  Side *s; uint32_t rows, cols; int col0, kind;
  if (state_dims(h, which, &s, &rows, &cols, &col0, &kind)) { h->err = "state not part of this model"; return HPF_ERR_INVALID; }
  const int obj = which / 4;
  int rc;
  auto put = [&](void *dst, const void *src, size_t bytes) -> int {
    if (!on_device) return h2d(h, dst, src, bytes);
    HIPCHK(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return HPF_OK;
  };
  auto put2d = [&](double *dev, uint32_t c0) -> int {
    return on_device ? copy_in_dev(h, dev, h->ld, c0, host, rows, cols) : copy_in(h, dev, h->ld, c0, host, rows, cols);
  };
  // a call that is refused -- or, the bias rate, accepted and ignored -- leaves the handle as it was, the flag word included
  const bool gr_rate = (obj <= 1 && kind == 1 && !h->cfg.hier);
  const size_t want = (obj == 2 || obj == 3) ? (size_t)rows : gr_rate ? (size_t)h->K : (size_t)rows * cols;
  if (count != want) return HPF_ERR_INVALID;
  if (kind == 1 && obj >= 4) return HPF_OK;   // bias rate is the constant 0.3 + m / 0.3 + n
  const bool vector = obj == 2 || obj == 3 || kind == 1;      // xi / eta, or a rate
  if ((rc = ready(h, vector ? hpf_lazy::PATCH_VECTOR : hpf_lazy::PATCH, h->side_of(*s), kind))) return rc;
  // a new state supersedes whatever the kernels flagged about the old one
  HIPCHK(h, hipMemsetAsync(h->flags, 0, 4, h->stream));
  if (obj == 2 || obj == 3) {                 // xi / eta vectors
    double **dst = kind == 0 ? &s->prior_shape_set : kind == 1 ? &s->prior_rate : kind == 2 ? &s->prior_E : &s->prior_elog;
    if (!*dst && (rc = dalloc(h, dst, rows))) return rc;
    rc = put(*dst, host, (size_t)rows * 8);
  } else if (kind == 1) {                     // rate: kept only for export before iteration 0
    dfree(s->rate_set); s->rate_set = nullptr;
    if ((rc = dalloc(h, &s->rate_set, want))) return rc;
    s->rate_set_count = want;
    rc = put(s->rate_set, host, want * 8);
  } else rc = put2d(kind == 0 ? s->S : kind == 2 ? s->E : s->L, (uint32_t)col0);
  if (!rc) h->lz.state_set(obj, kind);
  return rc;
}

int hpf_set_state(hpf_handle *h, hpf_state which, const double *host, size_t count)
{
  return set_state_impl(h, which, host, count, false);
}
int hpf_set_state_device(hpf_handle *h, hpf_state which, const double *dev, size_t count)
{
  return set_state_impl(h, which, dev, count, true);
}

static int get_state_impl(hpf_handle *h, hpf_state which, double *host, size_t count, bool on_device)
{
  if (!h || !host || which < 0 || which >= HPF_NUM_STATE) return HPF_ERR_INVALID;
  Side *s; uint32_t rows, cols; int col0, kind;
  if (state_dims(h, which, &s, &rows, &cols, &col0, &kind)) { h->err = "state not part of this model"; return HPF_ERR_INVALID; }
  const int obj = which / 4;
  const double s0 = h->cfg.s_prior, r0 = h->cfg.r_prior;
  auto get = [&](void *dst, const void *src, size_t bytes) -> int {
    if (!on_device) return d2h(h, dst, src, bytes);
    HIPCHK(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return HPF_OK;
  };
  auto fill = [&](double v, size_t cnt) -> int {         // a constant vector
    std::vector<double> tmp(cnt, v);
    if (!on_device) { memcpy(host, tmp.data(), cnt * 8); return HPF_OK; }
    HIPCHK(h, hipMemcpyAsync(host, tmp.data(), cnt * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return HPF_OK;
  };
  // the exports below read neither S, E nor W, but the xi / eta vectors and the column sums a rate is built from are the
  // sweeps' too: iterations a fall-back made the passes skip are run first (hpf_lazy::SWEEP_VECTORS)
  if (obj == 2 || obj == 3) {
    if (count != rows) return HPF_ERR_INVALID;
    { int rc = ready(h, hpf_lazy::SWEEP_VECTORS); if (rc) return rc; }
    if (kind == 2 || kind == 1) return get(host, kind == 2 ? s->prior_E : s->prior_rate, (size_t)rows * 8);
    if (kind == 3) return get(host, s->prior_elog, (size_t)rows * 8);   // set by the host, then maintained by the sweep
    if (h->iterations == 0) {
      const double *src = s->prior_shape_set;
      if (!src) { h->err = "state was never set"; return HPF_ERR_STATE; }
      return get(host, src, (size_t)rows * 8);
    }
    // after a sweep: shape = s0 + K*s0 (gpbase.hh:877-882)
    return fill(s0 + (double)h->K * s0, rows);
  }
  if (kind == 1) {                            // rate
    const bool gr = (obj <= 1 && !h->cfg.hier);
    const size_t want = gr ? h->K : (size_t)rows * cols;
    if (count != want) return HPF_ERR_INVALID;
    { int rc = ready(h, obj >= 4 ? hpf_lazy::BIAS_RATE : hpf_lazy::SWEEP_VECTORS, h->side_of(*s)); if (rc) return rc; }
    if (obj >= 4) return fill(r0 + s->bias_rate_add, rows);      // gpbase.hh:225-231 via hgaprec.cc:1389,1393
    if (h->iterations == 0) {
      if (!s->rate_set || s->rate_set_count != want) { h->err = "state was never set"; return HPF_ERR_STATE; }
      return get(host, s->rate_set, want * 8);
    }
    if (gr) {                                 // r_k = 0.3 + colsum_k  (gpbase.hh:558-562)
      std::vector<double> cs(h->ld);
      HIPCHK(h, hipMemcpyAsync(cs.data(), s->colsum_used, (size_t)h->ld * 8, hipMemcpyDeviceToHost, h->stream));
      HIPCHK(h, hipStreamSynchronize(h->stream));
      for (uint32_t k = 0; k < h->K; ++k) cs[k] += r0;
      if (!on_device) { memcpy(host, cs.data(), (size_t)h->K * 8); return HPF_OK; }
      HIPCHK(h, hipMemcpyAsync(host, cs.data(), (size_t)h->K * 8, hipMemcpyHostToDevice, h->stream));
      HIPCHK(h, hipStreamSynchronize(h->stream));
      return HPF_OK;
    }
    Scratch sc(h);
    double *tmp = on_device ? host : nullptr; int rc;
    if (!on_device && (rc = sc.alloc(&tmp, want))) return rc;
    hipLaunchKernelGGL(build_rate_kernel, dim3(1024), dim3(256), 0, h->stream, s->prior_used,
                       s->colsum_used, rows, h->K, tmp);
    if ((rc = check_launch(h, "build_rate"))) return rc;
    if (!on_device) return d2h(h, host, tmp, want * 8);
    if (hipStreamSynchronize(h->stream) != hipSuccess) { h->err = "build_rate failed"; return HPF_ERR_HIP; }
    return HPF_OK;
  }
  if (count != (size_t)rows * cols) return HPF_ERR_INVALID;
  { int rc = ready(h, kind == 3 ? hpf_lazy::STATE_ELOG : hpf_lazy::STATE_E, h->side_of(*s)); if (rc) return rc; }
  const double *dev = kind == 0 ? s->S : kind == 2 ? s->E : s->L;
  return on_device ? copy_out_dev(h, dev, h->ld, (uint32_t)col0, host, rows, cols)
                   : copy_out(h, dev, h->ld, (uint32_t)col0, host, rows, cols);
}

int hpf_get_state(hpf_handle *h, hpf_state which, double *host, size_t count)
{
  return get_state_impl(h, which, host, count, false);
}
int hpf_get_state_device(hpf_handle *h, hpf_state which, double *dev, size_t count)
{
  return get_state_impl(h, which, dev, count, true);
}

// ---- snapshot: the loop's device state, verbatim -------------------------------
namespace {
constexpr char SNAP_MAGIC[9] = "HPFSNAP4";
struct SnapHeader {
  char magic[8];                        // "HPFSNAP4" (round 6: the order of a p59 lane's dwords changed, and the header carries sums_dirty / start_sums_done)
  uint32_t n_users, n_items, K, ld, hier, bias, w32, iterations;
  // what else the state is only meaningful with: the priors, the job's shape and
  // the ratings it was fitted to -- a snapshot of another data set of the same dimensions,
  // or of another rank's shard, must not load
  uint32_t n_users_total, rank, n_ranks, novb;
  uint64_t nnz;
  double s_prior, r_prior;
  uint32_t side_flags[2];               // hpf_lazy::State::snap_side_word: what is pending on a side; SNAP_RATE_SET / SNAP_PRIOR_SHAPE_SET: the array follows
  uint32_t derived_word;                // hpf_lazy::State::snap_derived_dirty
  uint32_t more_flags;                  // hpf_lazy::State::snap_more_flags
  uint64_t rate_set_count[2];
  uint64_t total_bytes;
};
struct SnapSection { void *ptr; size_t bytes; };

// every array the iteration reads or the exports are rebuilt from, in a fixed order
void snapshot_sections(hpf_handle *h, const uint64_t rate_cnt[2], const uint32_t flags[2], std::vector<SnapSection> *out)
{
  Side *sides[2] = {&h->u, &h->it};
  for (int k = 0; k < 2; ++k) {
    Side &s = *sides[k];
    const size_t mat = (size_t)s.rows * h->ld * 8, vec = (size_t)s.rows * 8, row = (size_t)h->ld * 8;
    for (void *p : {(void *)s.S, (void *)s.E, (void *)s.L}) out->push_back({p, mat});
    out->push_back({s.W, w_bytes(h, s.rows)});
    for (double *p : {s.prior_E, s.prior_used, s.prior_rate, s.prior_elog, s.prior_elog_used}) out->push_back({p, vec});
    out->push_back({s.colsum, row}); out->push_back({s.colsum_used, row});
    if (flags[k] & hpf_lazy::SNAP_RATE_SET) out->push_back({s.rate_set, (size_t)rate_cnt[k] * 8});
    if (flags[k] & hpf_lazy::SNAP_PRIOR_SHAPE_SET) out->push_back({s.prior_shape_set, vec});
  }
}
void fill_snap_header(hpf_handle *h, SnapHeader *hd)
{
  memset(hd, 0, sizeof *hd);
  memcpy(hd->magic, SNAP_MAGIC, 8);
  hd->n_users = h->u.rows; hd->n_items = h->it.rows; hd->K = h->K; hd->ld = h->ld;
  hd->hier = h->cfg.hier; hd->bias = h->cfg.bias; hd->w32 = h->cfg.w_storage | ((uint32_t)h->wl << 8); hd->iterations = h->iterations;   // storage mode and the row layout in use
  hd->n_users_total = h->cfg.n_users_total; hd->rank = h->cfg.rank; hd->n_ranks = h->cfg.n_ranks;
  hd->novb = h->jacobi ? 1u : 0u; hd->nnz = h->have_csr ? h->nnz : 0;
  hd->s_prior = h->cfg.s_prior; hd->r_prior = h->cfg.r_prior;
  hd->side_flags[0] = h->lz.snap_side_word(hpf_lazy::USERS, h->u.rate_set, h->u.prior_shape_set);
  hd->side_flags[1] = h->lz.snap_side_word(hpf_lazy::ITEMS, h->it.rate_set, h->it.prior_shape_set);
  hd->derived_word = h->lz.snap_derived_dirty();
  hd->more_flags = h->lz.snap_more_flags();
  hd->rate_set_count[0] = h->u.rate_set ? h->u.rate_set_count : 0;
  hd->rate_set_count[1] = h->it.rate_set ? h->it.rate_set_count : 0;
  std::vector<SnapSection> sec;
  snapshot_sections(h, hd->rate_set_count, hd->side_flags, &sec);
  size_t tot = sizeof *hd;
  for (const SnapSection &x : sec) tot += x.bytes;
  hd->total_bytes = tot;
}
}  // namespace

int hpf_snapshot_size(hpf_handle *h, size_t *bytes)
{
  if (!h || !bytes) return HPF_ERR_INVALID;
  // a fall-back that is due changes the size of W: it happens here, so that hpf_snapshot_save finds the size it is handed
  { int rc = ready(h, hpf_lazy::SWEEP_VECTORS); if (rc) return rc; }
  SnapHeader hd; fill_snap_header(h, &hd);
  *bytes = (size_t)hd.total_bytes;
  return HPF_OK;
}

int hpf_snapshot_save(hpf_handle *h, void *host, size_t bytes)
{
  if (!h || !host) return HPF_ERR_INVALID;
  if (h->phase != 0) { h->err = "snapshot inside an iteration"; return HPF_ERR_STATE; }
  { int rc = ready(h, hpf_lazy::FLAGS); if (rc) return rc; }
  SnapHeader hd; fill_snap_header(h, &hd);
  if (bytes != hd.total_bytes) { h->err = "snapshot buffer size differs from hpf_snapshot_size"; return HPF_ERR_INVALID; }
  memcpy(host, &hd, sizeof hd);
  std::vector<SnapSection> sec;
  snapshot_sections(h, hd.rate_set_count, hd.side_flags, &sec);
  char *p = (char *)host + sizeof hd;
  for (const SnapSection &x : sec) {
    int rc = d2h(h, p, x.ptr, x.bytes);
    if (rc) return rc;
    p += x.bytes;
  }
  return HPF_OK;
}

int hpf_snapshot_load(hpf_handle *h, const void *host, size_t bytes)
{
  if (!h || !host || bytes < sizeof(SnapHeader)) return HPF_ERR_INVALID;
  if (h->phase != 0 || h->items_reduce_pending) { h->err = "snapshot load inside an iteration"; return HPF_ERR_STATE; }
  // ---- everything is validated before the handle is touched: a rejected blob leaves it as it was
  SnapHeader hd; memcpy(&hd, host, sizeof hd);
  // a snapshot taken after the rows fell back to plain doubles loads into a handle that still packs them: same job, the
  // handle follows (validated below like everything else, but the layout has to be known to size the sections)
  const bool follow = !memcmp(hd.magic, SNAP_MAGIC, 8) && h->wl == WL_P59 && hd.w32 == (h->cfg.w_storage | ((uint32_t)WL_F64 << 8)) &&
                      hd.n_users == h->u.rows && hd.n_items == h->it.rows && hd.K == h->K && hd.ld == h->ld && hd.total_bytes == bytes;
  if (follow) { int rc0 = ready(h, hpf_lazy::OVERWRITE_ALL); if (!rc0 && h->wl == WL_P59) rc0 = set_rows_f64(h); if (rc0) return rc0; h->fallbacks++; }
  if (memcmp(hd.magic, SNAP_MAGIC, 8) || hd.total_bytes != bytes || hd.n_users != h->u.rows || hd.n_items != h->it.rows ||
      hd.K != h->K || hd.ld != h->ld || hd.hier != h->cfg.hier || hd.bias != h->cfg.bias || hd.w32 != (h->cfg.w_storage | ((uint32_t)h->wl << 8))) {
    h->err = "not a snapshot of this model (shape, flags or storage differ)"; return HPF_ERR_INVALID;
  }
  if (hd.s_prior != h->cfg.s_prior || hd.r_prior != h->cfg.r_prior || hd.n_users_total != h->cfg.n_users_total ||
      hd.rank != h->cfg.rank || hd.n_ranks != h->cfg.n_ranks || hd.novb != (h->jacobi ? 1u : 0u)) {
    h->err = "not a snapshot of this job (priors, rank layout or update order differ)"; return HPF_ERR_INVALID;
  }
  if (hd.nnz != (h->have_csr ? h->nnz : 0)) {
    h->err = "the snapshot was taken on other ratings (nonzero count differs): upload the same CSR first"; return HPF_ERR_INVALID;
  }
  Side *sides[2] = {&h->u, &h->it};
  for (int k = 0; k < 2; ++k) {
    const size_t lim = (size_t)sides[k]->rows * h->K;
    const bool has = hd.side_flags[k] & hpf_lazy::SNAP_RATE_SET;
    if (has != (hd.rate_set_count[k] != 0) || hd.rate_set_count[k] > lim) { h->err = "damaged snapshot header"; return HPF_ERR_INVALID; }
  }
  {
    size_t tot = sizeof hd;
    for (int k = 0; k < 2; ++k) {
      const size_t mat = (size_t)sides[k]->rows * h->ld * 8, vec = (size_t)sides[k]->rows * 8, row = (size_t)h->ld * 8;
      tot += 3 * mat + w_bytes(h, sides[k]->rows) + 5 * vec + 2 * row;
      if (hd.side_flags[k] & hpf_lazy::SNAP_RATE_SET) tot += (size_t)hd.rate_set_count[k] * 8;
      if (hd.side_flags[k] & hpf_lazy::SNAP_PRIOR_SHAPE_SET) tot += vec;
    }
    if (tot != bytes) { h->err = "damaged snapshot header"; return HPF_ERR_INVALID; }
  }
  int rc;
  Scratch sc(h);
  double *new_rate[2] = {nullptr, nullptr}, *new_pss[2] = {nullptr, nullptr};
  for (int k = 0; k < 2; ++k) {                           // optional arrays the snapshot carries
    Side &s = *sides[k];
    if ((hd.side_flags[k] & hpf_lazy::SNAP_RATE_SET) && (rc = sc.alloc(&new_rate[k], (size_t)hd.rate_set_count[k]))) return rc;
    if ((hd.side_flags[k] & hpf_lazy::SNAP_PRIOR_SHAPE_SET) && !s.prior_shape_set && (rc = sc.alloc(&new_pss[k], s.rows))) return rc;
  }
  for (int k = 0; k < 2; ++k) {
    Side &s = *sides[k];
    dfree(s.rate_set); s.rate_set = sc.keep(new_rate[k]); s.rate_set_count = (size_t)hd.rate_set_count[k];
    if (new_pss[k]) s.prior_shape_set = sc.keep(new_pss[k]);
  }
  std::vector<SnapSection> sec;
  snapshot_sections(h, hd.rate_set_count, hd.side_flags, &sec);
  drop_graph(h);
  const char *p = (const char *)host + sizeof hd;
  for (const SnapSection &x : sec) {
    if ((rc = h2d(h, x.ptr, p, x.bytes))) return rc;
    p += x.bytes;
  }
  h->lz.snapshot_loaded(hd.side_flags, hd.derived_word, hd.more_flags);
  h->iterations = hd.iterations;
  h->phase = 0;
  HIPCHK(h, hipMemsetAsync(h->flags, 0, 8, h->stream));
  h->iters_counted = 0;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return HPF_OK;
}

int hpf_iterate(hpf_handle *h, int n_iters)
{
  if (!h || n_iters < 0) return HPF_ERR_INVALID;
  // several ranks -- or one with a communicator of its own (a one-rank RCCL communicator: tests, bench.py --comm library on one
  // GPU) --: whole iterations only when the library owns the exchange
  const bool exchange = h->cfg.n_ranks != 1 || h->comm;
  if (exchange && !h->comm) { h->err = "hpf_iterate with n_ranks > 1 needs hpf_comm_init (or use iterate_local / your all-reduce / iterate_global)"; return HPF_ERR_INVALID; }
  for (int t = 0; t < n_iters; ++t) {
    int rc;
    if (exchange) {
      if ((rc = items_pass(h, PIECES)) || (rc = hpf_allreduce_items_begin(h)) || (rc = iterate_local_users(h)) ||
          (rc = hpf_allreduce_exchange(h)) || (rc = iterate_global(h))) return rc;
    } else if (want_graph(h)) {
      if ((rc = replay_iteration(h))) return rc;
    } else if ((rc = iterate_local(h)) || (rc = iterate_global(h))) return rc;
  }
  return HPF_OK;
}

// the pieces of an iteration, for a caller that owns the exchange: compositions of the four steps (hpf_plan::next_phase)
int hpf_iterate_local_items(hpf_handle *h) { return h ? items_pass(h, PIECES) : HPF_ERR_INVALID; }
int hpf_iterate_local_phi(hpf_handle *h)
{
  if (!h) return HPF_ERR_INVALID;
  const int rc = items_pass(h, EAGER);
  return rc ? rc : run_steps(h, Step::USERS_PASS, Step::USERS_PASS, nullptr);
}
int hpf_iterate_local_sweep(hpf_handle *h) { return h ? run_steps(h, Step::USERS_SWEEP, Step::USERS_SWEEP, nullptr) : HPF_ERR_INVALID; }
int hpf_iterate_local_users(hpf_handle *h) { return h ? iterate_local_users(h) : HPF_ERR_INVALID; }
int hpf_iterate_local(hpf_handle *h) { return h ? iterate_local(h) : HPF_ERR_INVALID; }
int hpf_iterate_global(hpf_handle *h) { return h ? iterate_global(h) : HPF_ERR_INVALID; }

namespace {

// The two fold-in calls are one routine over (own, oth): the side that is folded in, with the pointers of its rows into
// own.idx / own.val, against the frozen one.  hpf_fold_in: (u, it, the CSR's row pointers); hpf_fold_in_items: (it, u, the
// item-major view's column pointers), and the rows with at least long_min nonzeros go to fold_in_long_kernel (0: none do).
struct FoldCall { Side &own, &oth; const int64_t *ptr; uint32_t long_min; const char *who; };

// room for what the rates are exported from before the first sweep (hpf_set_state(THETA_RATE), (XI_SHAPE))
int fold_export_room(hpf_handle *h, Side &u)
{
  int rc;
  const size_t want = h->cfg.hier ? (size_t)u.rows * h->K : (size_t)h->K;
  dfree(u.rate_set); u.rate_set = nullptr;
  if ((rc = dalloc(h, &u.rate_set, want))) return rc;
  u.rate_set_count = want;
  if (h->cfg.hier && !u.prior_shape_set && (rc = dalloc(h, &u.prior_shape_set, u.rows))) return rc;
  return HPF_OK;
}

// all iterations of all rows of the folded-in side: fold_in_kernel, one launch; with long rows (fc.long_min) followed by
// fold_in_long_kernel over the list of them
int fold_fused(hpf_handle *h, const FoldCall &fc, uint32_t n_iters, double tol, uint32_t *iters_out)
{
  const hpf_plan::FoldItemsPlan fp = hpf_plan::fold_items_plan(h->K, h->cfg.bias != 0, fc.long_min);
  if (!fp.wave.ok || (fc.long_min && !fp.ok)) { h->err = "fold_in_kernel: no instance for this column count"; return HPF_ERR_UNSUPPORTED; }
  Side &u = fc.own, &it = fc.oth;
  const uint32_t n = u.rows, m = it.rows, ld = h->ld, ldf = fp.wave.ld;
  const double s0 = h->cfg.s_prior, r0 = h->cfg.r_prior;
  int rc;
  if ((rc = fold_export_room(h, u))) return rc;
  Scratch sc(h);
  double *Wb = nullptr, *part = nullptr, *csum = nullptr; uint32_t *d_iters = nullptr, *d_long = nullptr, *d_nlong = nullptr;
  if ((rc = sc.alloc(&Wb, (size_t)m * ldf)) || (rc = sc.alloc(&part, (size_t)it.sweep_blocks * ld)) || (rc = sc.alloc(&csum, ld))) return rc;
  if (iters_out && (rc = sc.alloc(&d_iters, n))) return rc;
  hipLaunchKernelGGL(fold_derive_w_kernel, dim3(std::max<uint32_t>(1, std::min<uint32_t>((m + 3) / 4, 4096))), dim3(256), 0, h->stream, it.L, Wb, m, ld, ldf,
                     h->K, it.bias_col, it.junk_col);
  // c[k] = sum over the frozen side's rows of E, into a temporary: that side's own column sums stay as they are
  hipLaunchKernelGGL(colsum_partial_kernel, dim3(it.sweep_blocks), dim3(256), 0, h->stream, it.E, m, ld, h->K, part);
  hipLaunchKernelGGL(colsum_finalize_kernel, dim3(ld), dim3(256), 0, h->stream, part, it.sweep_blocks, ld, csum, h->flags);
  if ((rc = check_launch(h, "fold-in set-up"))) return rc;
  uint32_t n_long = 0;
  if (fc.long_min) {
    if ((rc = sc.alloc(&d_long, n)) || (rc = sc.alloc(&d_nlong, 1))) return rc;
    hipLaunchKernelGGL(fold_long_list_kernel, dim3(grid_for(n)), dim3(256), 0, h->stream, fc.ptr, n, fc.long_min, d_long, d_nlong);
    if ((rc = check_launch(h, "fold_long_list_kernel"))) return rc;
    HIPCHK(h, hipMemcpyAsync(&n_long, d_nlong, 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  FoldArgs a;
  a.rowptr = fc.ptr; a.idx = u.idx; a.val = u.val; a.Wb = Wb; a.csum = csum;
  a.S = u.S; a.E = u.E; a.L = u.L; a.rate = u.rate_set;
  a.xi_shape = u.prior_shape_set; a.xi_rate = u.prior_rate; a.xi_E = u.prior_E; a.xi_elog = u.prior_elog;
  a.xi_used = u.prior_used; a.xi_elog_used = u.prior_elog_used;
  a.iters_out = d_iters; a.flags = h->flags;
  a.n = n; a.ld = ld; a.ldf = ldf; a.K = h->K; a.rows_held = fp.wave.rows_held; a.slice = fp.wave.lds_wave_bytes / 8;
  a.n_iters = n_iters; a.hier = h->cfg.hier;
  a.len_max = fc.long_min ? fc.long_min - 1 : 0xffffffffu; a.long_rows = d_long; a.n_long = n_long;
  a.bias_col = u.bias_col; a.junk_col = u.junk_col;
  a.rate_bias = r0 + u.bias_rate_add;
  a.s_prior = s0; a.r_prior = r0; a.tol = tol;
  a.xi_shape_v = s0 + (double)h->K * s0; a.psi_xi_shape = host_digamma(a.xi_shape_v);
  a.elog_prior = host_digamma(s0) - std::log(r0);
  if (!launch_fold((int)fp.wave.R, a, fp.wave.grid(n), fp.wave.lds_block_bytes(), h->stream)) { h->err = "fold_in_kernel: no instance for this column count"; return HPF_ERR_UNSUPPORTED; }
  if ((rc = check_launch(h, "fold_in_kernel"))) return rc;
  if (n_long) {
    if (!launch_fold_long((int)fp.wave.R, a, fp.grid_long(n_long), fp.lds_long_bytes(), h->stream)) { h->err = "fold_in_long_kernel: no instance for this column count"; return HPF_ERR_UNSUPPORTED; }
    if ((rc = check_launch(h, "fold_in_long_kernel"))) return rc;
  }
  // what the rate was built from, where the exports after a sweep look for it
  HIPCHK(h, hipMemcpyAsync(u.colsum_used, csum, (size_t)ld * 8, hipMemcpyDeviceToDevice, h->stream));
  h->lz.folded(h->side_of(u));
  return copy_back(h, {{iters_out, d_iters, (size_t)n * 4}});
}

// A/B route (HPF_FOLD_ROUTE=sweeps under HPF_EXPERIMENTAL=1; never chosen by the library): the same call as n_iters x (the
// phi pass over the folded-in side's rows + its sweep) of the training path, from the prior.  Every row runs n_iters iterations.
int fold_sweeps(hpf_handle *h, const FoldCall &fc, uint32_t n_iters, double tol, uint32_t *iters_out)
{
  if (tol > 0.0) { h->err = "HPF_FOLD_ROUTE=sweeps runs every row for n_iters iterations: tol must be 0"; return HPF_ERR_UNSUPPORTED; }
  Side &u = fc.own, &it = fc.oth;
  const bool items = &u == &h->it;
  const uint32_t n = u.rows, ld = h->ld;
  const double s0 = h->cfg.s_prior, r0 = h->cfg.r_prior;
  int rc;
  if ((rc = fold_export_room(h, u))) return rc;
  hipLaunchKernelGGL(fold_prior_kernel, dim3(grid_for((uint64_t)n * ld)), dim3(256), 0, h->stream, u.S, u.E, u.L,
                     h->cfg.hier ? u.prior_E : nullptr, u.prior_elog, n, ld, h->K, u.bias_col, s0, s0 / r0, host_digamma(s0) - std::log(r0));
  if ((rc = check_launch(h, "fold_prior_kernel"))) return rc;
  h->lz.folded(h->side_of(u));
  if ((rc = ready(h, hpf_lazy::FOLD_SWEEPS_RUN, h->side_of(u)))) return rc;      // the frozen side's xi / eta is not read by the other half
  // the sums of the frozen side the sweep's rate reads: the item side's are the start sums; the user side's own are the
  // product of a user sweep, so an item call takes them into a temporary
  Scratch sc(h);
  double *csum = it.colsum;
  if (items) {
    double *part = nullptr;
    if ((rc = sc.alloc(&part, (size_t)it.sweep_blocks * ld)) || (rc = sc.alloc(&csum, ld))) return rc;
    hipLaunchKernelGGL(colsum_partial_kernel, dim3(it.sweep_blocks), dim3(256), 0, h->stream, it.E, it.rows, ld, h->K, part);
    hipLaunchKernelGGL(colsum_finalize_kernel, dim3(ld), dim3(256), 0, h->stream, part, it.sweep_blocks, ld, csum, h->flags);
    if ((rc = check_launch(h, "fold-in set-up"))) return rc;
  }
  for (uint32_t t = 0; t < n_iters; ++t)
    if ((rc = run_phi(h, u, it, nullptr)) || (rc = run_sweep(h, u, csum, u.colsum))) return rc;
  h->lz.swept(h->side_of(u));                                // FOLD_SWEEPS_END below rebuilds E and Elog from the sums
  uint32_t fl = 0;
  HIPCHK(h, hipMemcpyAsync(&fl, h->flags, 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (fl & 6u) { h->err = "HPF_FOLD_ROUTE=sweeps: the packed rows cannot hold this state (use w_storage = 3)"; return HPF_ERR_UNSUPPORTED; }
  if ((rc = ready(h, hpf_lazy::FOLD_SWEEPS_END, h->side_of(u)))) return rc;      // shape, E and Elog from the raw sums
  if (h->cfg.hier) {
    hipLaunchKernelGGL(build_rate_kernel, dim3(1024), dim3(256), 0, h->stream, u.prior_used, u.colsum_used, n, h->K, u.rate_set);
    if ((rc = check_launch(h, "build_rate"))) return rc;
    std::vector<double> shp(std::max<uint32_t>(n, 1), s0 + (double)h->K * s0);
    if ((rc = h2d(h, u.prior_shape_set, shp.data(), (size_t)n * 8))) return rc;
  } else {
    std::vector<double> cs(ld);
    HIPCHK(h, hipMemcpyAsync(cs.data(), u.colsum_used, (size_t)ld * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (uint32_t k = 0; k < h->K; ++k) cs[k] += r0;
    if ((rc = h2d(h, u.rate_set, cs.data(), (size_t)h->K * 8))) return rc;
  }
  h->lz.folded(h->side_of(u));
  if (iters_out) std::fill(iters_out, iters_out + n, n_iters);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return HPF_OK;
}

// what the two calls check, each before anything is launched, and the route
int fold_call(hpf_handle *h, const FoldCall &fc, uint32_t n_iters, double tol, uint32_t *iters_out)
{
  const std::string who = fc.who;
  if (n_iters == 0) { h->err = who + ": n_iters must be at least 1"; return HPF_ERR_INVALID; }
  if (!(tol >= 0.0)) { h->err = who + ": tol must be a number >= 0"; return HPF_ERR_INVALID; }
  if (!h->have_csr) { h->err = "hpf_upload_csr has not been called"; return HPF_ERR_STATE; }
  if (h->phase != 0) { h->err = who + ": call between iterations"; return HPF_ERR_STATE; }
  int rc;
  if ((rc = ready(h, h->fold_route == 1 ? hpf_lazy::FOLD_SWEEPS : hpf_lazy::FOLD_FUSED, h->side_of(fc.own)))) return rc;
  if (fc.own.rows == 0) return HPF_OK;
  // the folded-in state supersedes whatever the kernels flagged about the old one, like a state handed in
  HIPCHK(h, hipMemsetAsync(h->flags, 0, 4, h->stream));
  if ((rc = h->fold_route == 1 ? fold_sweeps(h, fc, n_iters, tol, iters_out) : fold_fused(h, fc, n_iters, tol, iters_out))) return rc;
  return ready(h, hpf_lazy::FLAGS);
}

}  // namespace

int hpf_fold_in(hpf_handle *h, uint32_t n_iters, double tol, uint32_t *iters_out)
{
  if (!h) return HPF_ERR_INVALID;
  return fold_call(h, {h->u, h->it, h->rowptr_dev, 0u, "hpf_fold_in"}, n_iters, tol, iters_out);
}

int hpf_fold_in_items(hpf_handle *h, uint32_t n_iters, double tol, uint32_t *iters_out)
{
  if (!h) return HPF_ERR_INVALID;
  // users are sharded across ranks: an item's sums would need an exchange per iteration
  if (h->cfg.n_ranks > 1) { h->err = "hpf_fold_in_items: one rank only"; return HPF_ERR_UNSUPPORTED; }
  const uint32_t long_min = h->fold_long_min ? h->fold_long_min : hpf_plan::FOLD_LONG_MIN;
  return fold_call(h, {h->it, h->u, h->colptr_dev, long_min, "hpf_fold_in_items"}, n_iters, tol, iters_out);
}

namespace {
// per-pair log-likelihoods of cnt pairs whose indices lie on the device, into hout (host; page-locked for a bound set),
// summed serially in the order handed in: the map order of hgaprec.cc:1455-1465.  The caller has asked for hpf_lazy::SCORING.
int heldout_run(hpf_handle *h, const uint32_t *du, const uint32_t *di, const int32_t *dy, double *dout, double *hout, size_t cnt,
                double *sum_out, bool pinned)
{
  int rc;
  LLArgs a;
  factor_args(h, a);
  a.u = du; a.i = di; a.y = dy; a.cnt = cnt; a.logfact = h->logfact; a.out = dout; a.binary = h->cfg.binary;
  const uint32_t blocks = (uint32_t)std::min<size_t>((cnt + 15) / 16, 4096);
  hipLaunchKernelGGL(heldout_ll_kernel, dim3(blocks), dim3(256), 0, h->stream, a);
  if ((rc = check_launch(h, "heldout_ll"))) return rc;
  // The sum is a chain of dependent adds in the order handed in -- that order is the contract -- and at 10^6 pairs it is what the
  // call costs (~0.8 ns per pair).  Into page-locked memory the values therefore arrive in pieces, and the host adds piece c
  // while piece c + 1 is on the wire: the DMA disappears behind the chain.  (Pageable memory: one copy, as before.)
  constexpr int PIECES = 8;
  const bool piped = pinned && cnt >= ((size_t)1 << 16);
  hipError_t e = hipSuccess;
  if (piped) {
    for (int c = 0; c < PIECES && e == hipSuccess; ++c)
      if (!h->held_ev[c]) e = hipEventCreateWithFlags(&h->held_ev[c], hipEventDisableTiming);
    const size_t per = (cnt + PIECES - 1) / PIECES;
    for (int c = 0; c < PIECES && e == hipSuccess; ++c) {
      const size_t p0 = std::min(cnt, (size_t)c * per), p1 = std::min(cnt, p0 + per);
      if (p1 > p0) e = hipMemcpyAsync(hout + p0, dout + p0, (p1 - p0) * 8, hipMemcpyDeviceToHost, h->stream);
      if (e == hipSuccess) e = hipEventRecord(h->held_ev[c], h->stream);
    }
    double s = .0;
    for (int c = 0; c < PIECES && e == hipSuccess; ++c) {
      e = hipEventSynchronize(h->held_ev[c]);
      const size_t p0 = std::min(cnt, (size_t)c * per), p1 = std::min(cnt, p0 + per);
      for (size_t p = p0; p < p1; ++p) s += hout[p];
    }
    if (e != hipSuccess) { (void)hipStreamSynchronize(h->stream); h->err = hipGetErrorString(e); return HPF_ERR_HIP; }
    *sum_out = s;
    return HPF_OK;
  }
  if ((rc = copy_back(h, {{hout, dout, cnt * 8}}))) return rc;
  double s = .0;
  for (size_t p = 0; p < cnt; ++p) s += hout[p];
  *sum_out = s;
  return HPF_OK;
}
}  // namespace

int hpf_heldout_ll(hpf_handle *h, const uint32_t *u, const uint32_t *i, const int32_t *y,
                   size_t cnt, double *sum_out, uint64_t *cnt_out)
{
  if (!h || !sum_out) return HPF_ERR_INVALID;
  *sum_out = 0.0; if (cnt_out) *cnt_out = cnt;
  if (cnt == 0) return HPF_OK;
  if (!u || !i || !y) return HPF_ERR_INVALID;
  int rc;
  if ((rc = ready(h, hpf_lazy::SCORING, -1, -1, [&] {
        for (size_t p = 0; p < cnt; ++p)
          if (u[p] >= h->u.rows || i[p] >= h->it.rows) { h->err = "held-out index out of range"; return (int)HPF_ERR_INVALID; }
        return (int)HPF_OK;
      }))) return rc;
  Scratch sc(h);
  uint32_t *du = nullptr, *di = nullptr; int32_t *dy = nullptr; double *dout = nullptr;
  std::vector<double> out(cnt);
  if ((rc = sc.alloc(&du, cnt)) || (rc = sc.alloc(&di, cnt)) || (rc = sc.alloc(&dy, cnt)) || (rc = sc.alloc(&dout, cnt))) return rc;
  HIPCHK(h, hipMemcpyAsync(du, u, cnt * 4, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(di, i, cnt * 4, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(dy, y, cnt * 4, hipMemcpyHostToDevice, h->stream));
  return heldout_run(h, du, di, dy, dout, out.data(), cnt, sum_out, false);
}

// A report step evaluates the SAME validation and test pairs every time (hgaprec.cc:1439-1470 walks the same two maps):
// bound once, a set is validated and uploaded once, and hpf_heldout_ll_bound is the kernel, one DMA of the per-pair
// values into a kept page-locked buffer and the ordered host sum -- the same sum, bit for bit, as hpf_heldout_ll's.
int hpf_heldout_bind(hpf_handle *h, int slot, const uint32_t *u, const uint32_t *i, const int32_t *y, size_t cnt)
{
  if (!h || slot < 0 || slot >= HPF_HELDOUT_SLOTS) return HPF_ERR_INVALID;
  if (cnt && (!u || !i || !y)) return HPF_ERR_INVALID;
  for (size_t p = 0; p < cnt; ++p)
    if (u[p] >= h->u.rows || i[p] >= h->it.rows) { h->err = "held-out index out of range"; return HPF_ERR_INVALID; }
  hpf_handle::HeldSet &hs = h->held[slot];
  HIPCHK(h, hipStreamSynchronize(h->stream));
  free_held(hs);
  hs.cnt = cnt; hs.bound = true;
  if (cnt == 0) return HPF_OK;
  int rc;
  if ((rc = dalloc(h, &hs.du, cnt)) || (rc = dalloc(h, &hs.di, cnt)) || (rc = dalloc(h, &hs.dy, cnt)) || (rc = dalloc(h, &hs.dout, cnt))) { free_held(hs); return rc; }
  if (hipHostMalloc((void **)&hs.hout, cnt * 8, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); free_held(hs); h->err = "hpf_heldout_bind: no page-locked memory"; return HPF_ERR_OOM; }
  if ((rc = h2d(h, hs.du, u, cnt * 4)) || (rc = h2d(h, hs.di, i, cnt * 4)) || (rc = h2d(h, hs.dy, y, cnt * 4))) { free_held(hs); return rc; }
  return HPF_OK;
}

int hpf_heldout_ll_bound(hpf_handle *h, int slot, double *sum_out, uint64_t *cnt_out)
{
  if (!h || !sum_out || slot < 0 || slot >= HPF_HELDOUT_SLOTS) return HPF_ERR_INVALID;
  const hpf_handle::HeldSet &hs = h->held[slot];
  if (!hs.bound) { h->err = "hpf_heldout_ll_bound: nothing bound to this slot"; return HPF_ERR_STATE; }
  *sum_out = 0.0; if (cnt_out) *cnt_out = hs.cnt;
  if (hs.cnt == 0) return HPF_OK;
  if (int rc = ready(h, hpf_lazy::SCORING)) return rc;
  return heldout_run(h, hs.du, hs.di, hs.dy, hs.dout, hs.hout, hs.cnt, sum_out, true);
}

int hpf_elbo(hpf_handle *h, double *out)
{
  if (!h || !out) return HPF_ERR_INVALID;
  *out = 0.0;
  if (!h->have_csr || h->iterations == 0) { h->err = "the ELBO is defined after the first iteration"; return HPF_ERR_STATE; }
  // fp64 W: logsumexp from the hot loop's W and the row maxima of Elog (no exp per
  // element); the f32-stored W is not precise enough for that, it takes the Elog form
  const bool from_w = !h->w32 && h->wl == WL_PLAIN && h->nnz;
  int rc;
  if ((rc = ready(h, from_w ? hpf_lazy::ELBO_FROM_W : hpf_lazy::ELBO))) return rc;
  // per-nonzero term: the user-major work list(s) of the phi pass, one wave per segment
  const uint32_t nb_nnz = (uint32_t)std::min<uint64_t>(((uint64_t)h->u.nseg + 3) / 4 + 1, 16384);
  const uint32_t nb_g = 1024;
  Scratch sc(h);
  double *part = nullptr, *Mt = nullptr, *Mb = nullptr;
  const size_t npart = (size_t)2 * nb_nnz + 2 * nb_g;
  if ((rc = sc.alloc(&part, npart))) return rc;
  std::vector<double> hp(npart, 0.0);
  if (from_w) {
    if ((rc = sc.alloc(&Mt, h->u.rows)) || (rc = sc.alloc(&Mb, h->it.rows))) return rc;
    hipLaunchKernelGGL(rowmax_elog_kernel, dim3((h->u.rows + 255) / 256), dim3(256), 0, h->stream,
                       h->u.L, Mt, h->u.rows, h->ld, h->K, h->u.bias_col, h->u.junk_col);
    hipLaunchKernelGGL(rowmax_elog_kernel, dim3((h->it.rows + 255) / 256), dim3(256), 0, h->stream,
                       h->it.L, Mb, h->it.rows, h->ld, h->K, h->it.bias_col, h->it.junk_col);
  }
  if (from_w && h->u.nseg) {
    ElboNnzWArgs a;
    factor_args(h, a);
    a.segs = h->u.segs; a.nseg = h->u.nseg; a.col = h->u.pass_idx(); a.val = h->u.pass_val();
    a.Wt = (const double *)h->u.W; a.Wb = (const double *)h->it.W; a.Mt = Mt; a.Mb = Mb; a.partial = part;
    a.Lt = h->u.L; a.Lb = h->it.L; a.C = h->C;
    hipLaunchKernelGGL(elbo_nnz_w_kernel, dim3(nb_nnz), dim3(256), 0, h->stream, a);
  }
  if (h->nnz && !from_w && h->u.nseg) {
    ElboNnzArgs a;
    factor_args(h, a);
    a.segs = h->u.segs; a.nseg = h->u.nseg; a.col = h->u.pass_idx(); a.val = h->u.pass_val();
    a.Lt = h->u.L; a.Lb = h->it.L; a.partial = part; a.C = h->C;
    hipLaunchKernelGGL(elbo_nnz_kernel, dim3(nb_nnz), dim3(256), 0, h->stream, a);
  }
  const double s0 = h->cfg.s_prior, ps = s0 + (double)h->K * s0;
  Side *sides[2] = {&h->u, &h->it};
  for (int k = 0; k < 2; ++k) {
    Side &s = *sides[k];
    if (k == 1 && h->cfg.rank != 0) continue;      // replicated item side: counted once
    if (!s.rows) continue;
    ElboGammaArgs g;
    g.S = s.S; g.E = s.E; g.L = s.L; g.prior_used = s.prior_used; g.prior_elog_used = s.prior_elog_used;
    g.colsum_used = s.colsum_used; g.prior_E = s.prior_E; g.prior_elog = s.prior_elog; g.prior_rate = s.prior_rate;
    g.partial = part + (size_t)2 * nb_nnz + (size_t)k * nb_g; g.rows = s.rows; g.ld = h->ld; g.K = h->K;
    g.bias_col = s.bias_col; g.bias_rate_add = s.bias_rate_add; g.s_prior = s0; g.r_prior = h->cfg.r_prior;
    g.lg_s_prior = std::lgamma(s0); g.prior_shape = ps; g.lg_prior_shape = std::lgamma(ps); g.hier = h->cfg.hier;
    hipLaunchKernelGGL(elbo_gamma_kernel, dim3(nb_g), dim3(256), 0, h->stream, g);
  }
  if ((rc = check_launch(h, "elbo"))) return rc;
  if ((rc = copy_back(h, {{hp.data(), part, npart * 8}}))) return rc;
  double s = 0.0;
  for (size_t k = 0; k < npart; ++k) s += hp[k];
  *out = s;
  return HPF_OK;
}

// ---- ranking evaluation ----------------------------------------------------
namespace {
// what every ranking call asks of the handle, of the selected users and of the mask list, once E is known to exist
int rank_check(hpf_handle *h, const uint32_t *users, uint32_t n_sel, const uint64_t *mask_ptr, const uint32_t *mask_items)
{
  if (!h->have_csr) { h->err = "hpf_upload_csr has not been called"; return HPF_ERR_STATE; }
  for (uint32_t b = 0; b < n_sel; ++b)
    if (users[b] >= h->u.rows) { h->err = "user index out of range"; return HPF_ERR_INVALID; }
  if (mask_ptr) {
    const uint64_t nmask = mask_ptr[n_sel];
    if (mask_ptr[0] != 0) { h->err = "mask_ptr[0] must be 0"; return HPF_ERR_INVALID; }
    for (uint32_t b = 0; b < n_sel; ++b) if (mask_ptr[b + 1] < mask_ptr[b]) { h->err = "mask_ptr not monotone"; return HPF_ERR_INVALID; }
    if (nmask && !mask_items) return HPF_ERR_INVALID;
    for (uint64_t j = 0; j < nmask; ++j) if (mask_items[j] >= h->it.rows) { h->err = "mask item out of range"; return HPF_ERR_INVALID; }
  }
  return HPF_OK;
}

// What a fused call (hpf_loo_ranks, hpf_rank_queries, hpf_recommend) settles before it allocates, in the order that decides
// which error a bad call gets: E exists, rank_check, the items q[0 .. nq) it asks about (none for hpf_recommend), the jobs
int fused_ready(hpf_handle *h, const uint32_t *users, uint32_t n_sel, const uint64_t *mask_ptr, const uint32_t *mask_items,
                const uint32_t *q = nullptr, uint64_t nq = 0)
{
  return ready(h, hpf_lazy::SCORING, -1, -1, [&] {
    if (int rc = rank_check(h, users, n_sel, mask_ptr, mask_items)) return rc;
    for (uint64_t k = 0; k < nq; ++k) if (q[k] >= h->it.rows) { h->err = "query item out of range"; return (int)HPF_ERR_INVALID; }
    return (int)HPF_OK;
  });
}

// The unfused ranking calls (hpf_scores, hpf_rank_topn, hpf_item_ranks) keep the scores of a batch of users
// (hpf_plan::score_batch_rows) and run their own kernel over them
struct ScoreCtx : FusedCtx {
  double *d_scores = nullptr;
  using FusedCtx::FusedCtx;

  int prepare(const uint32_t *users, uint32_t n_sel, const uint64_t *mask_ptr, const uint32_t *mask_items)
  {
    int rc;
    if ((rc = ready(h, hpf_lazy::SCORES, -1, -1, [&] { return rank_check(h, users, n_sel, mask_ptr, mask_items); }))) return rc;
    batch = hpf_plan::score_batch_rows(h->it.rows, n_sel);
    if ((rc = upload(users, n_sel, mask_ptr, mask_items))) return rc;
    return alloc(&d_scores, (size_t)batch * h->it.rows);
  }
  // scores (+ mask) of selected rows [b0, b1) into d_scores
  int scores(uint32_t b0, uint32_t b1, bool mask)
  {
    const uint32_t m = h->it.rows, rows = b1 - b0;
    ScoreArgs a;
    factor_args(h, a);
    a.users = d_users + b0; a.scores = d_scores; a.n_sel = rows; a.m = m;
    hipLaunchKernelGGL(score_tile_kernel, dim3((m + 255) / 256, (rows + 15) / 16), dim3(256), 0, h->stream, a);
    if (mask)
      hipLaunchKernelGGL(mask_scores_kernel, dim3(std::min<uint32_t>((rows + 3) / 4, 4096)), dim3(256), 0,
                         h->stream, d_users + b0, rows, h->rowptr_dev, h->u.idx, h->u.val,
                         d_mptr ? d_mptr + b0 : nullptr, d_mitems, d_scores, m);
    return check_launch(h, "score/mask");
  }
};
}  // namespace

int hpf_scores(hpf_handle *h, const uint32_t *users, uint32_t n_sel, double *out)
{
  if (!h || (n_sel && (!users || !out))) return HPF_ERR_INVALID;
  if (!n_sel) return HPF_OK;
  ScoreCtx c(h); int rc;
  if ((rc = c.prepare(users, n_sel, nullptr, nullptr))) return rc;
  const uint32_t m = h->it.rows;
  for (uint32_t b0 = 0; b0 < n_sel; b0 += c.batch) {
    const uint32_t b1 = std::min(n_sel, b0 + c.batch);
    if ((rc = c.scores(b0, b1, false))) return rc;
    HIPCHK(h, hipMemcpyAsync(out + (size_t)b0 * m, c.d_scores, (size_t)(b1 - b0) * m * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  return HPF_OK;
}

int hpf_rank_topn(hpf_handle *h, const uint32_t *users, uint32_t n_sel, const uint64_t *mask_ptr,
                  const uint32_t *mask_items, uint32_t topn, uint32_t *out_items, double *out_scores)
{
  if (!h || topn == 0 || topn > 1024 || (n_sel && (!users || !out_items || !out_scores))) return HPF_ERR_INVALID;
  if (!n_sel) return HPF_OK;
  ScoreCtx c(h); int rc;
  if ((rc = c.prepare(users, n_sel, mask_ptr, mask_items))) return rc;
  const uint32_t NP = hpf_plan::pow2_ceil(topn);
  uint32_t *d_items = nullptr; double *d_sc = nullptr;
  if ((rc = c.alloc(&d_items, (size_t)n_sel * topn)) || (rc = c.alloc(&d_sc, (size_t)n_sel * topn))) return rc;
  for (uint32_t b0 = 0; b0 < n_sel; b0 += c.batch) {
    const uint32_t b1 = std::min(n_sel, b0 + c.batch);
    if ((rc = c.scores(b0, b1, true))) return rc;
    hipLaunchKernelGGL(topn_kernel, dim3(b1 - b0), dim3(256), (size_t)NP * 12, h->stream, c.d_scores, b1 - b0,
                       h->it.rows, topn, NP, d_items + (size_t)b0 * topn, d_sc + (size_t)b0 * topn);
    if ((rc = check_launch(h, "topn_kernel"))) return rc;
  }
  return copy_back(h, {{out_items, d_items, (size_t)n_sel * topn * 4}, {out_scores, d_sc, (size_t)n_sel * topn * 8}});
}

int hpf_item_ranks(hpf_handle *h, const uint32_t *users, uint32_t n_sel, const uint64_t *mask_ptr,
                   const uint32_t *mask_items, const uint32_t *q_sel, const uint32_t *q_item, uint32_t nq,
                   uint32_t *out_rank, double *out_score)
{
  if (!h || (n_sel && !users) || (nq && (!q_sel || !q_item || !out_rank || !out_score))) return HPF_ERR_INVALID;
  if (!nq) return HPF_OK;
  for (uint32_t q = 0; q < nq; ++q)
    if (q_sel[q] >= n_sel || q_item[q] >= h->it.rows) { h->err = "query out of range"; return HPF_ERR_INVALID; }
  ScoreCtx c(h); int rc;
  if ((rc = c.prepare(users, n_sel, mask_ptr, mask_items))) return rc;
  uint32_t *d_qs = nullptr, *d_qi = nullptr, *d_rank = nullptr; double *d_sc = nullptr;
  if ((rc = c.alloc(&d_qs, nq, q_sel)) || (rc = c.alloc(&d_qi, nq, q_item)) || (rc = c.alloc(&d_rank, nq)) || (rc = c.alloc(&d_sc, nq))) return rc;
  for (uint32_t b0 = 0; b0 < n_sel; b0 += c.batch) {
    const uint32_t b1 = std::min(n_sel, b0 + c.batch);
    if ((rc = c.scores(b0, b1, true))) return rc;
    hipLaunchKernelGGL(rank_query_kernel, dim3(std::min<uint32_t>(nq, 16384)), dim3(256), 0, h->stream, c.d_scores,
                       h->it.rows, d_qs, d_qi, nq, b0, b1, d_rank, d_sc);
    if ((rc = check_launch(h, "rank_query_kernel"))) return rc;
  }
  return copy_back(h, {{out_rank, d_rank, (size_t)nq * 4}, {out_score, d_sc, (size_t)nq * 8}});
}

// ---- scoring a saved model: per-pair predictions, fused leave-one-out ranks ----
int hpf_predict(hpf_handle *h, const uint32_t *u, const uint32_t *i, size_t cnt, double *out)
{
  if (!h) return HPF_ERR_INVALID;
  if (cnt == 0) return HPF_OK;
  if (!u || !i || !out) return HPF_ERR_INVALID;
  int rc;
  if ((rc = ready(h, hpf_lazy::SCORING, -1, -1, [&] {
        for (size_t p = 0; p < cnt; ++p)
          if (u[p] >= h->u.rows || i[p] >= h->it.rows) { h->err = "hpf_predict: index out of range"; return (int)HPF_ERR_INVALID; }
        return (int)HPF_OK;
      }))) return rc;
  Scratch sc(h);
  uint32_t *du = nullptr, *di = nullptr; double *dout = nullptr;
  if ((rc = sc.alloc(&du, cnt, u)) || (rc = sc.alloc(&di, cnt, i)) || (rc = sc.alloc(&dout, cnt))) return rc;
  PredictArgs a;
  factor_args(h, a);
  a.u = du; a.i = di; a.cnt = cnt; a.out = dout;
  const uint32_t blocks = (uint32_t)std::min<size_t>((cnt + 15) / 16, 4096);
  hipLaunchKernelGGL(predict_kernel, dim3(blocks), dim3(256), 0, h->stream, a);
  if ((rc = check_launch(h, "predict_kernel"))) return rc;
  return copy_back(h, {{out, dout, cnt * 8}});
}

int hpf_loo_ranks(hpf_handle *h, const uint32_t *users, uint32_t n_sel, const uint64_t *mask_ptr,
                  const uint32_t *mask_items, const uint32_t *q_item, uint32_t item_limit,
                  uint32_t *out_rank, double *out_score, uint32_t *out_masked)
{
  if (!h || (n_sel && (!users || !q_item || !out_rank || !out_score))) return HPF_ERR_INVALID;
  if (!n_sel) return HPF_OK;
  const uint32_t m = h->it.rows;
  if (item_limit > m) { h->err = "item_limit beyond n_items"; return HPF_ERR_INVALID; }
  const uint32_t limit = item_limit ? item_limit : m;
  if (h->ld & 1u) { h->err = "hpf_loo_ranks: odd row stride"; return HPF_ERR_UNSUPPORTED; }
  if (int rc = fused_ready(h, users, n_sel, mask_ptr, mask_items, q_item, n_sel)) return rc;
  FusedCtx c(h); int rc;
  uint32_t *d_q = nullptr, *d_rank = nullptr, *d_masked = nullptr; double *d_sc = nullptr;
  if ((rc = c.upload(users, n_sel, mask_ptr, mask_items)) || (rc = c.bit_rows(n_sel, h->it.rows)) || (rc = c.alloc(&d_q, n_sel, q_item)) || (rc = c.alloc(&d_rank, n_sel)) ||
      (rc = c.alloc(&d_masked, n_sel)) || (rc = c.alloc(&d_sc, n_sel))) return rc;
  for (uint32_t b0 = 0; b0 < n_sel; b0 += c.batch) {
    const uint32_t rows = std::min(n_sel - b0, c.batch);
    if ((rc = c.mask_batch(b0, rows, h->rowptr_dev, h->u.idx, h->u.val))) return rc;
    LooArgs a;
    factor_args(h, a);
    a.users = c.d_users + b0; a.q_item = d_q + b0; a.bits = c.d_bits;
    a.rank = d_rank + b0; a.masked = d_masked + b0; a.score = d_sc + b0;
    a.n_sel = rows; a.limit = limit; a.words = c.words;
    const hpf_plan::RankGrid g = hpf_plan::rank_grid(rows, (limit + 63) / 64);
    a.tiles_per_split = g.tiles_per_split;
    if ((rc = launch_rank(h, "loo_rank_kernel", [&](auto nch) {
          hipLaunchKernelGGL(loo_rank_kernel<decltype(nch)::value>, dim3(g.blocks, g.splits), dim3(256), 0, h->stream, a);
        }))) return rc;
  }
  return copy_back(h, {{out_rank, d_rank, (size_t)n_sel * 4}, {out_score, d_sc, (size_t)n_sel * 8}, {out_masked, d_masked, (size_t)n_sel * 4}});
}

int hpf_rank_queries(hpf_handle *h, const uint32_t *users, uint32_t n_sel, const uint64_t *mask_ptr,
                     const uint32_t *mask_items, const uint64_t *q_ptr, const uint32_t *q_items,
                     uint32_t *out_rank, double *out_score)
{
  if (!h || (n_sel && (!users || !q_ptr))) return HPF_ERR_INVALID;
  if (!n_sel) return HPF_OK;
  const uint32_t m = h->it.rows;
  if (h->ld & 1u) { h->err = "hpf_rank_queries: odd row stride"; return HPF_ERR_UNSUPPORTED; }
  if (q_ptr[0] != 0) { h->err = "q_ptr[0] must be 0"; return HPF_ERR_INVALID; }
  for (uint32_t b = 0; b < n_sel; ++b)
    if (q_ptr[b + 1] < q_ptr[b]) { h->err = "q_ptr not monotone"; return HPF_ERR_INVALID; }
  const uint64_t nq = q_ptr[n_sel];
  if (nq > 0xffffffffull) { h->err = "hpf_rank_queries: more than 2^32 - 1 queries in one call"; return HPF_ERR_INVALID; }
  if (nq && (!q_items || !out_rank || !out_score)) return HPF_ERR_INVALID;
  if (!nq) return ready(h, hpf_lazy::E_IS_SET, -1, -1, [&] { return rank_check(h, users, n_sel, mask_ptr, mask_items); });      // nothing asked: only the checks
  if (int rc = fused_ready(h, users, n_sel, mask_ptr, mask_items, q_items, nq)) return rc;
  FusedCtx c(h); int rc;
  if ((rc = c.upload(users, n_sel, mask_ptr, mask_items)) || (rc = c.bit_rows(n_sel, h->it.rows))) return rc;
  // rows: a selected user with at most RQ_QCAP of its queries (a query's rank does not depend on the user's other
  // queries, so cutting a user is exact); in the order of the selected users, so a batch owns a run of them
  std::vector<uint32_t> row_sel, row_q0, row_nq, first_row;   // first_row[batch index] -> its first row
  for (uint32_t b = 0; b < n_sel; ++b) {
    if (b % c.batch == 0) first_row.push_back((uint32_t)row_sel.size());
    for (uint64_t q = q_ptr[b]; q < q_ptr[b + 1]; q += RQ_QCAP) {
      row_sel.push_back(b % c.batch); row_q0.push_back((uint32_t)q);
      row_nq.push_back((uint32_t)std::min<uint64_t>(RQ_QCAP, q_ptr[b + 1] - q));
    }
  }
  first_row.push_back((uint32_t)row_sel.size());
  const size_t nrows = row_sel.size();
  uint32_t *d_q = nullptr, *d_rank = nullptr, *d_rsel = nullptr, *d_rq0 = nullptr, *d_rnq = nullptr, *d_sitem = nullptr, *d_sperm = nullptr;
  unsigned long long *d_skey = nullptr; double *d_sc = nullptr;
  if ((rc = c.alloc(&d_q, (size_t)nq, q_items)) || (rc = c.alloc(&d_rank, (size_t)nq)) || (rc = c.alloc(&d_sc, (size_t)nq)) ||
      (rc = c.alloc(&d_skey, (size_t)nq)) || (rc = c.alloc(&d_sitem, (size_t)nq)) || (rc = c.alloc(&d_sperm, (size_t)nq)) ||
      (rc = c.alloc(&d_rsel, nrows, row_sel.data())) || (rc = c.alloc(&d_rq0, nrows, row_q0.data())) ||
      (rc = c.alloc(&d_rnq, nrows, row_nq.data()))) return rc;
  size_t bi = 0;
  for (uint32_t b0 = 0; b0 < n_sel; b0 += c.batch, ++bi) {
    const uint32_t r0 = first_row[bi], rows = first_row[bi + 1] - r0;
    if (!rows) continue;
    if ((rc = c.mask_batch(b0, std::min(n_sel - b0, c.batch), h->rowptr_dev, h->u.idx, h->u.val))) return rc;
    RqArgs a;
    factor_args(h, a);
    a.users = c.d_users + b0; a.row_sel = d_rsel + r0; a.row_q0 = d_rq0 + r0; a.row_nq = d_rnq + r0; a.q_item = d_q;
    a.bits = c.d_bits; a.skey = d_skey; a.sitem = d_sitem;
    a.sperm = d_sperm; a.rank = d_rank; a.score = d_sc;
    a.nrows = rows; a.m = m; a.words = c.words;
    const hpf_plan::RankGrid g = hpf_plan::rank_grid(rows, (m + 63) / 64);
    a.tiles_per_split = g.tiles_per_split;
    hipLaunchKernelGGL(rq_threshold_kernel, dim3((rows + 3) / 4), dim3(256), 0, h->stream, a);
    if ((rc = launch_rank(h, "rank_queries_kernel", [&](auto nch) {
          hipLaunchKernelGGL(rank_queries_kernel<decltype(nch)::value>, dim3(g.blocks, g.splits), dim3(256), 0, h->stream, a);
        }))) return rc;
  }
  return copy_back(h, {{out_rank, d_rank, (size_t)nq * 4}, {out_score, d_sc, (size_t)nq * 8}});
}

// Top-N for every selected user.  Up to hpf_plan::TOPN_FUSED_MAX: the sweep of the other two fused calls behind the bit
// rows of a batch of users (topn_sweep_kernel, topn_run).  Above it: hpf_rank_topn's route.
int hpf_recommend(hpf_handle *h, const uint32_t *users, uint32_t n_sel, const uint64_t *mask_ptr,
                  const uint32_t *mask_items, uint32_t topn, uint32_t *out_items, double *out_scores)
{
  if (!h || topn == 0 || topn > hpf_plan::TOPN_MAX || (n_sel && (!users || !out_items || !out_scores))) return HPF_ERR_INVALID;
  if (!n_sel) return HPF_OK;
  if (!hpf_plan::topn_fused(topn)) return hpf_rank_topn(h, users, n_sel, mask_ptr, mask_items, topn, out_items, out_scores);
  const uint32_t m = h->it.rows;
  if (h->ld & 1u) { h->err = "hpf_recommend: odd row stride"; return HPF_ERR_UNSUPPORTED; }
  if (int rc = fused_ready(h, users, n_sel, mask_ptr, mask_items)) return rc;
  FusedCtx c(h); int rc;
  if ((rc = c.upload(users, n_sel, mask_ptr, mask_items)) || (rc = c.bit_rows(n_sel, h->it.rows))) return rc;
  TopnArgs a;
  factor_args(h, a);
  a.bits = c.d_bits; a.words = c.words;
  return topn_run(c, a, m, n_sel, topn, std::min(topn, m), "topn_sweep_kernel",
                  [&](uint32_t b0, uint32_t rows) { return c.mask_batch(b0, rows, h->rowptr_dev, h->u.idx, h->u.val); },
                  [&](auto nch, dim3 grid, const TopnArgs &ta) {
                    hipLaunchKernelGGL(topn_sweep_kernel<decltype(nch)::value>, grid, dim3(256), 0, h->stream, ta);
                  }, out_items, out_scores);
}

// The topn nearest OTHER rows of one side for every selected row: hpf_recommend's sweep, selection and merge with query
// rows and swept rows from one matrix -- the side's E for the dot product, its rows at unit length (unit_rows_kernel; a
// temporary of this call) for the cosine.  No bit rows, no bias, the row itself left out: min(topn, rows - 1) entries a list.
int hpf_similar(hpf_handle *h, int side, const uint32_t *ids, uint32_t n_sel, uint32_t topn, int metric,
                uint32_t *out_ids, double *out_scores)
{
  if (!h) return HPF_ERR_INVALID;
  if (side != 0 && side != 1) { h->err = "hpf_similar: side is 0 (users) or 1 (items)"; return HPF_ERR_INVALID; }
  if (metric != HPF_SIM_COSINE && metric != HPF_SIM_DOT) { h->err = "hpf_similar: unknown metric"; return HPF_ERR_INVALID; }
  if (!hpf_plan::topn_fused(topn)) { h->err = "hpf_similar: topn is 1 .. 256"; return HPF_ERR_INVALID; }
  if (n_sel && (!ids || !out_ids || !out_scores)) { h->err = "hpf_similar: null pointer"; return HPF_ERR_INVALID; }
  if (!n_sel) return HPF_OK;
  Side &s = side ? h->it : h->u;
  const uint32_t m = s.rows;
  if (h->ld & 1u) { h->err = "hpf_similar: odd row stride"; return HPF_ERR_UNSUPPORTED; }
  int rc;
  if ((rc = ready(h, hpf_lazy::FACTORS, side, -1, [&] {
        for (uint32_t b = 0; b < n_sel; ++b)
          if (ids[b] >= m) { h->err = side ? "item index out of range" : "user index out of range"; return (int)HPF_ERR_INVALID; }
        return (int)HPF_OK;
      }))) return rc;
  FusedCtx c(h);
  double *d_unit = nullptr;
  if ((rc = c.upload(ids, n_sel, nullptr, nullptr))) return rc;
  if (metric == HPF_SIM_COSINE) {
    if ((rc = c.alloc(&d_unit, (size_t)m * h->ld))) return rc;
    hipLaunchKernelGGL(unit_rows_kernel, dim3(std::min<uint32_t>((m + 15) / 16, 16384)), dim3(256), 0, h->stream, s.E, d_unit, m, h->ld, h->K);
    if ((rc = check_launch(h, "unit_rows_kernel"))) return rc;
  }
  TopnArgs a;
  a.Et = a.Eb = d_unit ? d_unit : s.E; a.ld = h->ld; a.K = h->K; a.ubias_col = a.ibias_col = -1;
  a.bits = nullptr; a.words = 0;
  return topn_run(c, a, m, n_sel, topn, std::min(topn, m - 1), "similar_sweep_kernel",
                  [](uint32_t, uint32_t) { return (int)HPF_OK; },
                  [&](auto nch, dim3 grid, const TopnArgs &ta) {
                    hipLaunchKernelGGL(similar_sweep_kernel<decltype(nch)::value>, grid, dim3(256), 0, h->stream, ta);
                  }, out_ids, out_scores);
}

// The topn users of every selected item: hpf_recommend transposed.  TopnArgs with the sides exchanged -- the selected items'
// rows of E[beta] are the query rows, the m = n_users rows of E[theta] are swept, the bias columns change places -- behind the
// bit rows of a batch of ITEMS, one bit per user, set from the item-major view (audience_mask_kernel).  Only the fused route.
int hpf_audience(hpf_handle *h, const uint32_t *items, uint32_t n_sel, const uint64_t *mask_ptr,
                 const uint32_t *mask_users, uint32_t topn, uint32_t *out_users, double *out_scores)
{
  if (!h) return HPF_ERR_INVALID;
  if (!hpf_plan::topn_fused(topn)) { h->err = "hpf_audience: topn is 1 .. 256"; return HPF_ERR_INVALID; }
  if (n_sel && (!items || !out_users || !out_scores)) { h->err = "hpf_audience: null pointer"; return HPF_ERR_INVALID; }
  if (!n_sel) return HPF_OK;
  const uint32_t n = h->u.rows;
  if (h->ld & 1u) { h->err = "hpf_audience: odd row stride"; return HPF_ERR_UNSUPPORTED; }
  int rc;
  if ((rc = ready(h, hpf_lazy::SCORING, -1, -1, [&] {
        if (!h->have_csr) { h->err = "hpf_upload_csr has not been called"; return (int)HPF_ERR_STATE; }
        for (uint32_t b = 0; b < n_sel; ++b)
          if (items[b] >= h->it.rows) { h->err = "item index out of range"; return (int)HPF_ERR_INVALID; }
        if (mask_ptr) {
          const uint64_t nmask = mask_ptr[n_sel];
          if (mask_ptr[0] != 0) { h->err = "mask_ptr[0] must be 0"; return (int)HPF_ERR_INVALID; }
          for (uint32_t b = 0; b < n_sel; ++b) if (mask_ptr[b + 1] < mask_ptr[b]) { h->err = "mask_ptr not monotone"; return (int)HPF_ERR_INVALID; }
          if (nmask && !mask_users) { h->err = "hpf_audience: null pointer"; return (int)HPF_ERR_INVALID; }
          for (uint64_t j = 0; j < nmask; ++j) if (mask_users[j] >= n) { h->err = "mask user out of range"; return (int)HPF_ERR_INVALID; }
        }
        return (int)HPF_OK;
      }))) return rc;
  FusedCtx c(h);
  if ((rc = c.upload(items, n_sel, mask_ptr, mask_users)) || (rc = c.bit_rows(n_sel, n))) return rc;
  TopnArgs a;
  a.Et = h->it.E; a.Eb = h->u.E; a.ld = h->ld; a.K = h->K;
  a.ubias_col = h->cfg.bias ? h->it.bias_col : -1;       // of the query rows: E_ibias
  a.ibias_col = h->cfg.bias ? h->u.bias_col : -1;        // of the swept rows: E_ubias
  a.bits = c.d_bits; a.words = c.words;
  return topn_run(c, a, n, n_sel, topn, std::min(topn, n), "audience_sweep_kernel",
                  [&](uint32_t b0, uint32_t rows) { return c.mask_batch(b0, rows, h->colptr_dev, h->it.idx, h->it.val, audience_mask_kernel); },
                  [&](auto nch, dim3 grid, const TopnArgs &ta) {
                    hipLaunchKernelGGL(audience_sweep_kernel<decltype(nch)::value>, grid, dim3(256), 0, h->stream, ta);
                  }, out_users, out_scores);
}

// ---- posterior moments of a score, the optimistic top-N ----
namespace {
// what both calls settle before they allocate: the derived columns fit, the row stride is even
int moments_shape(hpf_handle *h, const char *call, hpf_plan::MomentsPlan *mp)
{
  *mp = hpf_plan::moments_plan(h->K, h->cfg.bias != 0);
  if (!mp->ok) { h->err = std::string(call) + ": 2 K + 2 * bias derived columns exceed HPF_MAX_COLUMNS"; return HPF_ERR_UNSUPPORTED; }
  if (h->ld & 1u) { h->err = std::string(call) + ": odd row stride"; return HPF_ERR_UNSUPPORTED; }
  return HPF_OK;
}
void pair_moment_args(const hpf_handle *h, const hpf_plan::MomentsPlan &mp, PairMomentArgs &a)
{
  factor_args(h, a);
  a.St = h->u.S; a.Sb = h->it.S; a.C = mp.C; a.mean_steps = mp.mean_steps; a.var_steps = mp.var_steps;
}
}  // namespace

// Mean and variance of every pair (pair_moments_kernel): hpf_predict's argument checks behind E and the shapes of both
// sides (hpf_lazy::MOMENTS); no CSR, no temporaries beyond the pairs, the state only read.
int hpf_score_moments(hpf_handle *h, const uint32_t *u, const uint32_t *i, size_t cnt, double *out_mean, double *out_var)
{
  if (!h) return HPF_ERR_INVALID;
  if (cnt == 0) return HPF_OK;
  if (!u || !i) { h->err = "hpf_score_moments: null pointer"; return HPF_ERR_INVALID; }
  hpf_plan::MomentsPlan mp; int rc;
  if ((rc = moments_shape(h, "hpf_score_moments", &mp))) return rc;
  if ((rc = ready(h, hpf_lazy::MOMENTS, -1, -1, [&] {
        for (size_t p = 0; p < cnt; ++p)
          if (u[p] >= h->u.rows || i[p] >= h->it.rows) { h->err = "hpf_score_moments: index out of range"; return (int)HPF_ERR_INVALID; }
        return (int)HPF_OK;
      }))) return rc;
  Scratch sc(h);
  uint32_t *du = nullptr, *di = nullptr;
  PairMomentArgs a;
  pair_moment_args(h, mp, a);
  a.out_ucb = nullptr; a.z = 0.0; a.per = 0; a.cnt = cnt;
  if ((rc = sc.alloc(&du, cnt, u)) || (rc = sc.alloc(&di, cnt, i)) || (rc = sc.alloc(&a.out_mean, cnt)) || (rc = sc.alloc(&a.out_var, cnt))) return rc;
  a.u = du; a.i = di;
  hipLaunchKernelGGL(pair_moments_kernel, dim3(mp.grid_pairs(cnt)), dim3(256), 0, h->stream, a);
  if ((rc = check_launch(h, "pair_moments_kernel"))) return rc;
  return copy_back(h, {{out_mean, a.out_mean, cnt * 8}, {out_var, a.out_var, cnt * 8}});
}

// hpf_recommend ordered by mean + z sd: its checks, bit rows, batches, candidate buffers and merge (topn_run) around
// ucb_sweep_kernel.  Y (every item's derived row) is built once, X for the users of each batch (moment_rows_kernel); both
// are temporaries of the call.  The lists' means, variances and values then come from pair_moments_kernel over the listed
// pairs: the merge's decoded keys are not handed out, a masked item that was listed at +0.0 reports its own value.
int hpf_recommend_ucb(hpf_handle *h, const uint32_t *users, uint32_t n_sel, const uint64_t *mask_ptr, const uint32_t *mask_items,
                      uint32_t topn, double z, uint32_t *out_items, double *out_ucb, double *out_mean, double *out_var)
{
  if (!h) return HPF_ERR_INVALID;
  if (!hpf_plan::topn_fused(topn)) { h->err = "hpf_recommend_ucb: topn is 1 .. 256"; return HPF_ERR_INVALID; }
  if (!(z >= 0.0) || !std::isfinite(z)) { h->err = "hpf_recommend_ucb: z is finite and >= 0 (the key order covers no negative score)"; return HPF_ERR_INVALID; }
  if (n_sel && (!users || !out_items || !out_ucb)) { h->err = "hpf_recommend_ucb: null pointer"; return HPF_ERR_INVALID; }
  if (!n_sel) return HPF_OK;
  const uint32_t m = h->it.rows;
  hpf_plan::MomentsPlan mp; int rc;
  if ((rc = moments_shape(h, "hpf_recommend_ucb", &mp))) return rc;
  if ((rc = ready(h, hpf_lazy::MOMENTS, -1, -1, [&] { return rank_check(h, users, n_sel, mask_ptr, mask_items); }))) return rc;
  FusedCtx c(h);
  if ((rc = c.upload(users, n_sel, mask_ptr, mask_items)) || (rc = c.bit_rows(n_sel, m))) return rc;
  const uint32_t x_rows = mp.x_rows(m, n_sel, topn, h->loo_batch);          // topn_run's batch
  double *X = nullptr, *Y = nullptr;
  if ((rc = c.alloc(&Y, (size_t)m * mp.ldx)) || (rc = c.alloc(&X, (size_t)x_rows * mp.ldx))) return rc;
  MomentRowsArgs ra;
  ra.ld = h->ld; ra.ldx = mp.ldx; ra.K = h->K;
  ra.E = h->it.E; ra.S = h->it.S; ra.sel = nullptr; ra.out = Y; ra.rows = m; ra.item_side = 1;
  ra.bias_col = h->cfg.bias ? h->it.bias_col : -1;
  hipLaunchKernelGGL(moment_rows_kernel, dim3(mp.grid_rows(m)), dim3(256), 0, h->stream, ra);
  if ((rc = check_launch(h, "moment_rows_kernel"))) return rc;
  ra.E = h->u.E; ra.S = h->u.S; ra.out = X; ra.item_side = 0;
  ra.bias_col = h->cfg.bias ? h->u.bias_col : -1;
  TopnArgs a;
  factor_args(h, a);
  a.bits = c.d_bits; a.words = c.words;
  uint32_t *d_items = nullptr;
  if ((rc = topn_run(c, a, m, n_sel, topn, std::min(topn, m), "ucb_sweep_kernel",
                     [&](uint32_t b0, uint32_t rows) {
                       if (rows > x_rows) { h->err = "hpf_recommend_ucb: a batch beyond the derived rows"; return (int)HPF_ERR_HIP; }
                       ra.sel = c.d_users + b0; ra.rows = rows;
                       hipLaunchKernelGGL(moment_rows_kernel, dim3(mp.grid_rows(rows)), dim3(256), 0, h->stream, ra);
                       return c.mask_batch(b0, rows, h->rowptr_dev, h->u.idx, h->u.val);
                     },
                     [&](auto, dim3 grid, const TopnArgs &ta) {
                       UcbArgs ua;
                       static_cast<TopnArgs &>(ua) = ta;
                       ua.X = X; ua.Y = Y; ua.ldx = mp.ldx; ua.C = mp.C; ua.mean_steps = mp.mean_steps; ua.z = z;
                       hipLaunchKernelGGL(ucb_sweep_kernel, grid, dim3(256), 0, h->stream, ua);
                     }, out_items, nullptr, &d_items))) return rc;
  const size_t cnt = (size_t)n_sel * topn;
  PairMomentArgs pa;
  pair_moment_args(h, mp, pa);
  pa.u = c.d_users; pa.i = d_items; pa.per = topn; pa.cnt = cnt; pa.z = z;
  if ((rc = c.alloc(&pa.out_ucb, cnt)) || (rc = c.alloc(&pa.out_mean, cnt)) || (rc = c.alloc(&pa.out_var, cnt))) return rc;
  hipLaunchKernelGGL(pair_moments_kernel, dim3(mp.grid_pairs(cnt)), dim3(256), 0, h->stream, pa);
  if ((rc = check_launch(h, "pair_moments_kernel"))) return rc;
  return copy_back(h, {{out_ucb, pa.out_ucb, cnt * 8}, {out_mean, pa.out_mean, cnt * 8}, {out_var, pa.out_var, cnt * 8}});
}

// ---- one posterior draw: its rows, and the top-N of it ----
namespace {
// gamma_rows_kernel over `rows` rows of one side into out [rows x ld]: sel names the rows (and the counter's row ids), or
// null for rows 0 .. rows - 1
void launch_gamma_rows(hpf_handle *h, int side, const uint32_t *sel, uint32_t rows, uint64_t seed, uint32_t draw, double *out)
{
  const Side &s = side ? h->it : h->u;
  GammaRowsArgs ga;
  ga.E = s.E; ga.S = s.S; ga.sel = sel; ga.out = out; ga.seed = seed; ga.rows = rows; ga.ld = h->ld; ga.K = h->K;
  ga.bias_col = h->cfg.bias ? s.bias_col : -1; ga.object = side ? 1u : 0u; ga.draw = draw;
  hipLaunchKernelGGL(gamma_rows_kernel, dim3(hpf_plan::sample_plan(rows, h->ld).grid), dim3(256), 0, h->stream, ga);
}
}  // namespace

// One draw of a side's rows, dense: gamma_rows_kernel into rows of the handle's stride, sample_pack_kernel into the host
// layout, piece by piece (hpf_plan::sample_piece_rows).  E and the shapes of both sides as for the other posterior calls
// (hpf_lazy::MOMENTS); no CSR, the state only read.
int hpf_sample_state(hpf_handle *h, int side, const uint32_t *ids, uint32_t n_sel, uint64_t seed, uint32_t draw, double *out)
{
  if (!h) return HPF_ERR_INVALID;
  if (side != 0 && side != 1) { h->err = "hpf_sample_state: side is 0 (users) or 1 (items)"; return HPF_ERR_INVALID; }
  if (!n_sel) return HPF_OK;
  if (!out) { h->err = "hpf_sample_state: null pointer"; return HPF_ERR_INVALID; }
  const Side &s = side ? h->it : h->u;
  int rc;
  if ((rc = ready(h, hpf_lazy::MOMENTS, -1, -1, [&] {
        bool ok = ids || n_sel <= s.rows;
        for (uint32_t b = 0; ids && ok && b < n_sel; ++b) ok = ids[b] < s.rows;
        if (!ok) { h->err = side ? "item index out of range" : "user index out of range"; return (int)HPF_ERR_INVALID; }
        return (int)HPF_OK;
      }))) return rc;
  const uint32_t C = h->K + (h->cfg.bias ? 1u : 0u), piece = hpf_plan::sample_piece_rows(n_sel, h->ld);
  std::vector<uint32_t> own;                                     // rows 0 .. n_sel - 1 in several pieces: their ids spelled out
  if (!ids && n_sel > piece) { own.resize(n_sel); for (uint32_t b = 0; b < n_sel; ++b) own[b] = b; ids = own.data(); }
  Scratch sc(h);
  uint32_t *d_ids = nullptr; double *rows_ld = nullptr, *dense = nullptr;
  if ((ids && (rc = sc.alloc(&d_ids, n_sel, ids))) || (rc = sc.alloc(&rows_ld, (size_t)piece * h->ld)) || (rc = sc.alloc(&dense, (size_t)piece * C))) return rc;
  for (uint32_t b0 = 0; b0 < n_sel; b0 += piece) {
    const uint32_t rows = std::min(piece, n_sel - b0);
    launch_gamma_rows(h, side, d_ids ? d_ids + b0 : nullptr, rows, seed, draw, rows_ld);
    hipLaunchKernelGGL(sample_pack_kernel, dim3(grid_for((uint64_t)rows * C)), dim3(256), 0, h->stream, rows_ld, dense, (uint64_t)rows, h->ld, h->K,
                       h->cfg.bias ? s.bias_col : -1);
    if ((rc = check_launch(h, "gamma_rows_kernel/sample_pack_kernel"))) return rc;
    if ((rc = copy_back(h, {{out + (size_t)b0 * C, dense, (size_t)rows * C * 8}}))) return rc;
  }
  return HPF_OK;
}

// hpf_recommend on one posterior draw: its checks, bit rows, batches, candidate buffers and merge (topn_run) and its sweep
// kernel, topn_sweep_kernel, over two temporaries of the call in the place of E -- the item side's draw, built once, and the
// draw of the users of each batch, whose rows the sweep addresses as 0 .. rows - 1 while the counters carry the users' ids.
int hpf_recommend_thompson(hpf_handle *h, const uint32_t *users, uint32_t n_sel, const uint64_t *mask_ptr, const uint32_t *mask_items,
                           uint32_t topn, uint64_t seed, uint32_t draw, uint32_t *out_items, double *out_scores)
{
  if (!h) return HPF_ERR_INVALID;
  if (!hpf_plan::topn_fused(topn)) { h->err = "hpf_recommend_thompson: topn is 1 .. 256"; return HPF_ERR_INVALID; }
  if (n_sel && (!users || !out_items || !out_scores)) { h->err = "hpf_recommend_thompson: null pointer"; return HPF_ERR_INVALID; }
  if (!n_sel) return HPF_OK;
  const uint32_t m = h->it.rows;
  if (h->ld & 1u) { h->err = "hpf_recommend_thompson: odd row stride"; return HPF_ERR_UNSUPPORTED; }
  int rc;
  if ((rc = ready(h, hpf_lazy::MOMENTS, -1, -1, [&] { return rank_check(h, users, n_sel, mask_ptr, mask_items); }))) return rc;
  FusedCtx c(h);
  if ((rc = c.upload(users, n_sel, mask_ptr, mask_items)) || (rc = c.bit_rows(n_sel, m))) return rc;
  const uint32_t t_rows = hpf_plan::topn_batch_users(m, n_sel, hpf_plan::topn_cap(topn), h->loo_batch);     // topn_run's batch
  std::vector<uint32_t> own(t_rows);
  for (uint32_t b = 0; b < t_rows; ++b) own[b] = b;
  double *Tt = nullptr, *Bt = nullptr; uint32_t *d_own = nullptr;
  if ((rc = c.alloc(&Bt, (size_t)m * h->ld)) || (rc = c.alloc(&Tt, (size_t)t_rows * h->ld)) || (rc = c.alloc(&d_own, t_rows, own.data()))) return rc;
  launch_gamma_rows(h, 1, nullptr, m, seed, draw, Bt);
  if ((rc = check_launch(h, "gamma_rows_kernel"))) return rc;
  TopnArgs a;
  factor_args(h, a);
  a.Et = Tt; a.Eb = Bt;
  a.bits = c.d_bits; a.words = c.words;
  return topn_run(c, a, m, n_sel, topn, std::min(topn, m), "topn_sweep_kernel",
                  [&](uint32_t b0, uint32_t rows) {
                    if (rows > t_rows) { h->err = "hpf_recommend_thompson: a batch beyond the sampled rows"; return (int)HPF_ERR_HIP; }
                    launch_gamma_rows(h, 0, c.d_users + b0, rows, seed, draw, Tt);
                    return c.mask_batch(b0, rows, h->rowptr_dev, h->u.idx, h->u.val);
                  },
                  [&](auto nch, dim3 grid, const TopnArgs &ta) {
                    TopnArgs sa = ta;
                    sa.users = d_own;                            // row b of the batch's draw belongs to selected user b0 + b
                    hipLaunchKernelGGL(topn_sweep_kernel<decltype(nch)::value>, grid, dim3(256), 0, h->stream, sa);
                  }, out_items, out_scores);
}

// ---- diversified top-N: greedy MMR over the pool hpf_recommend finds ----
static_assert(HPF_DIVERSE_POOL_MAX == hpf_plan::DIVERSE_POOL_MAX && HPF_DIVERSE_POOL_MAX <= hpf_plan::TOPN_FUSED_MAX,
              "the pool is a list of the fused top-N route, a thread of the workgroup per entry");
namespace {
// compute units of the handle's device: what diverse_plan sizes the persistent grid by (speed only, never results)
uint32_t device_cus(const hpf_handle *h)
{
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->cfg.device) != hipSuccess || cus < 1) return 256;
  return (uint32_t)cus;
}
}  // namespace

// hpf_recommend at topn = pool with the lists left on the device (topn_run), the unit rows of E[beta] as hpf_similar makes
// them, then mmr_kernel per batch of users: the pool's Gram matrix into the workgroups' slabs and the greedy selection.
int hpf_recommend_diverse(hpf_handle *h, const uint32_t *users, uint32_t n_sel, const uint64_t *mask_ptr, const uint32_t *mask_items,
                          uint32_t topn, uint32_t pool, double lambda, uint32_t *out_items, double *out_scores, double *out_maxsim,
                          double *out_mmr)
{
  if (!h) return HPF_ERR_INVALID;
  if (topn < 1 || topn > HPF_DIVERSE_POOL_MAX) { h->err = "hpf_recommend_diverse: topn is 1 .. 256"; return HPF_ERR_INVALID; }
  if (pool < topn || pool > HPF_DIVERSE_POOL_MAX) { h->err = "hpf_recommend_diverse: pool is topn .. 256"; return HPF_ERR_INVALID; }
  if (!(lambda >= 0.0 && lambda <= 1.0)) { h->err = "hpf_recommend_diverse: lambda is in [0, 1]"; return HPF_ERR_INVALID; }
  if (n_sel && (!users || !out_items || !out_scores)) { h->err = "hpf_recommend_diverse: null pointer"; return HPF_ERR_INVALID; }
  if (!n_sel) return HPF_OK;
  const uint32_t m = h->it.rows;
  if (h->ld & 1u) { h->err = "hpf_recommend_diverse: odd row stride"; return HPF_ERR_UNSUPPORTED; }
  int rc;
  if ((rc = fused_ready(h, users, n_sel, mask_ptr, mask_items))) return rc;
  FusedCtx c(h);
  if ((rc = c.upload(users, n_sel, mask_ptr, mask_items)) || (rc = c.bit_rows(n_sel, m))) return rc;
  double *d_unit = nullptr;
  if ((rc = c.alloc(&d_unit, (size_t)m * h->ld))) return rc;
  hipLaunchKernelGGL(unit_rows_kernel, dim3(std::min<uint32_t>((m + 15) / 16, 16384)), dim3(256), 0, h->stream, h->it.E, d_unit, m, h->ld, h->K);
  if ((rc = check_launch(h, "unit_rows_kernel"))) return rc;
  TopnArgs a;
  factor_args(h, a);
  a.bits = c.d_bits; a.words = c.words;
  uint32_t *d_pool = nullptr; double *d_pool_sc = nullptr;
  if ((rc = topn_run(c, a, m, n_sel, pool, std::min(pool, m), "topn_sweep_kernel",
                     [&](uint32_t b0, uint32_t rows) { return c.mask_batch(b0, rows, h->rowptr_dev, h->u.idx, h->u.val); },
                     [&](auto nch, dim3 grid, const TopnArgs &ta) {
                       hipLaunchKernelGGL(topn_sweep_kernel<decltype(nch)::value>, grid, dim3(256), 0, h->stream, ta);
                     }, nullptr, nullptr, &d_pool, &d_pool_sc))) return rc;
  const uint32_t per = std::min(std::max(c.batch, 1u), n_sel);
  const hpf_plan::DiversePlan dp = hpf_plan::diverse_plan(pool, per, h->K, device_cus(h));
  if (!dp.ok) { h->err = "hpf_recommend_diverse: no plan"; return HPF_ERR_INVALID; }
  const size_t cnt = (size_t)n_sel * topn;
  MmrArgs ma;
  ma.U = d_unit; ma.rows = m; ma.ld = h->ld; ma.K = h->K; ma.pool = pool; ma.topn = topn; ma.Pp = dp.Pp; ma.lambda = lambda;
  if ((rc = c.alloc(&ma.slab, (size_t)dp.workgroups * dp.Pp * dp.Pp)) || (rc = c.alloc(&ma.out_items, cnt)) || (rc = c.alloc(&ma.out_scores, cnt)) ||
      (rc = c.alloc(&ma.out_maxsim, cnt)) || (rc = c.alloc(&ma.out_mmr, cnt))) return rc;
  uint32_t *d_items = ma.out_items; double *d_sc = ma.out_scores, *d_ms = ma.out_maxsim, *d_mmr = ma.out_mmr;
  for (uint32_t b0 = 0; b0 < n_sel; b0 += per) {
    const uint32_t rows = std::min(n_sel - b0, per);
    ma.pool_items = d_pool + (size_t)b0 * pool; ma.pool_scores = d_pool_sc + (size_t)b0 * pool; ma.n_sel = rows;
    ma.out_items = d_items + (size_t)b0 * topn; ma.out_scores = d_sc + (size_t)b0 * topn;
    ma.out_maxsim = d_ms + (size_t)b0 * topn; ma.out_mmr = d_mmr + (size_t)b0 * topn;
    hipLaunchKernelGGL(mmr_kernel, dim3(std::min(dp.workgroups, rows)), dim3(256), 0, h->stream, ma);
    if ((rc = check_launch(h, "mmr_kernel"))) return rc;
  }
  return copy_back(h, {{out_items, d_items, cnt * 4}, {out_scores, d_sc, cnt * 8}, {out_maxsim, d_ms, cnt * 8}, {out_mmr, d_mmr, cnt * 8}});
}

// The T largest terms of every pair's score (explain_kernel): hpf_predict's readiness path and argument checks, no CSR,
// the state only read.
static_assert(HPF_EXPLAIN_MAX == hpf_plan::EXPLAIN_MAX && HPF_EXPLAIN_MAX <= 64, "a lane of the wave per returned term");
int hpf_explain(hpf_handle *h, const uint32_t *u, const uint32_t *i, size_t cnt, uint32_t T, uint32_t *out_factor, double *out_contrib)
{
  if (!h) return HPF_ERR_INVALID;
  if (T < 1 || T > HPF_EXPLAIN_MAX) { h->err = "hpf_explain: T is 1 .. 32"; return HPF_ERR_INVALID; }
  if (cnt == 0) return HPF_OK;
  if (!u || !i || !out_factor || !out_contrib) { h->err = "hpf_explain: null pointer"; return HPF_ERR_INVALID; }
  int rc;
  const hpf_plan::ExplainPlan ep = hpf_plan::explain_plan(h->K, h->cfg.bias != 0);
  if ((rc = ready(h, hpf_lazy::SCORING, -1, -1, [&] {
        for (size_t p = 0; p < cnt; ++p)
          if (u[p] >= h->u.rows || i[p] >= h->it.rows) { h->err = "hpf_explain: index out of range"; return (int)HPF_ERR_INVALID; }
        // the bias terms are numbered by their columns: K the user's, K + 1 the item's (hpf_create)
        if (!ep.ok || ep.terms > h->ld || (h->cfg.bias && (h->u.bias_col != (int32_t)h->K || h->it.bias_col != (int32_t)h->K + 1))) {
          h->err = "explain_kernel: no instance for this column count"; return (int)HPF_ERR_UNSUPPORTED;
        }
        return (int)HPF_OK;
      }))) return rc;
  Scratch sc(h);
  ExplainArgs a;
  factor_args(h, a);
  uint32_t *du = nullptr, *di = nullptr;
  if ((rc = sc.alloc(&du, cnt, u)) || (rc = sc.alloc(&di, cnt, i)) || (rc = sc.alloc(&a.out_factor, cnt * T)) || (rc = sc.alloc(&a.out_contrib, cnt * T))) return rc;
  a.u = du; a.i = di; a.cnt = cnt; a.T = T; a.run = hpf_plan::EXPLAIN_RUN;
  if (!launch_explain((int)ep.R, a, ep.grid(cnt), h->stream)) { h->err = "explain_kernel: no instance for this column count"; return HPF_ERR_UNSUPPORTED; }
  if ((rc = check_launch(h, "explain_kernel"))) return rc;
  return copy_back(h, {{out_factor, a.out_factor, cnt * T * 4}, {out_contrib, a.out_contrib, cnt * T * 8}});
}

// Which of the user's own ratings carry a score (because_shape_kernel, because_kernel): the argument checks first -- they
// depend on nothing but the handle's sizes --, then E and Elog of both sides through the one prologue.  The gathered copy
// of the item side, D and the underflow word are temporaries of the call: the handle's state and flags are only read.
static_assert(HPF_BECAUSE_MAX == hpf_plan::BECAUSE_MAX && HPF_BECAUSE_MAX <= 64, "a lane of the wave per returned entry");
int hpf_because(hpf_handle *h, const uint32_t *users, uint32_t n_sel, const uint64_t *t_ptr, const uint32_t *t_items, uint32_t T,
                uint32_t *out_item, double *out_contrib, double *out_sum, double *out_prior)
{
  if (!h) return HPF_ERR_INVALID;
  if (T < 1 || T > HPF_BECAUSE_MAX) { h->err = "hpf_because: T is 1 .. 32"; return HPF_ERR_INVALID; }
  if (!n_sel) return HPF_OK;
  if (!users || !t_ptr) { h->err = "hpf_because: null pointer"; return HPF_ERR_INVALID; }
  if (t_ptr[0] != 0) { h->err = "hpf_because: t_ptr[0] must be 0"; return HPF_ERR_INVALID; }
  for (uint32_t b = 0; b < n_sel; ++b) {
    if (t_ptr[b + 1] < t_ptr[b]) { h->err = "hpf_because: t_ptr decreases"; return HPF_ERR_INVALID; }
    if (users[b] >= h->u.rows) { h->err = "hpf_because: user index out of range"; return HPF_ERR_INVALID; }
  }
  const uint64_t nt = t_ptr[n_sel];
  if (nt && (!t_items || !out_item || !out_contrib)) { h->err = "hpf_because: null pointer"; return HPF_ERR_INVALID; }
  for (uint64_t q = 0; q < nt; ++q)
    if (t_items[q] >= h->it.rows) { h->err = "hpf_because: item index out of range"; return HPF_ERR_INVALID; }
  if (!nt) return HPF_OK;
  if (!h->have_csr) { h->err = "hpf_upload_csr has not been called"; return HPF_ERR_STATE; }
  if (h->phase != 0) { h->err = "hpf_because: call between iterations"; return HPF_ERR_STATE; }
  int rc;
  if ((rc = ready(h, hpf_lazy::BECAUSE))) return rc;
  const hpf_plan::BecausePlan bp = hpf_plan::because_plan(h->K, h->cfg.bias != 0);
  if (!bp.ok || bp.ld < h->K + (h->cfg.bias ? 2u : 0u)) { h->err = "because_kernel: no instance for this column count"; return HPF_ERR_UNSUPPORTED; }
  const uint32_t m = h->it.rows, ld = h->ld, ldf = bp.ld;
  std::vector<uint32_t> t_sel(nt);
  for (uint32_t b = 0; b < n_sel; ++b) std::fill(t_sel.begin() + t_ptr[b], t_sel.begin() + t_ptr[b + 1], b);
  Scratch sc(h);
  double *Wb = nullptr; uint32_t *d_users = nullptr, *d_sel = nullptr, *d_items = nullptr, *d_flag = nullptr;
  BecauseArgs a;
  if ((rc = sc.alloc(&Wb, (size_t)m * ldf)) || (rc = sc.alloc(&a.D, (size_t)n_sel * ldf)) || (rc = sc.alloc(&d_users, n_sel, users)) ||
      (rc = sc.alloc(&d_sel, nt, t_sel.data())) || (rc = sc.alloc(&d_items, nt, t_items)) || (rc = sc.alloc(&d_flag, 1)) ||
      (rc = sc.alloc(&a.out_item, nt * T)) || (rc = sc.alloc(&a.out_contrib, nt * T)) || (rc = sc.alloc(&a.out_sum, nt)) || (rc = sc.alloc(&a.out_prior, nt))) return rc;
  hipLaunchKernelGGL(fold_derive_w_kernel, dim3(std::max<uint32_t>(1, std::min<uint32_t>((m + 3) / 4, 4096))), dim3(256), 0, h->stream, h->it.L, Wb, m, ld, ldf,
                     h->K, h->it.bias_col, h->it.junk_col);
  if ((rc = check_launch(h, "hpf_because set-up"))) return rc;
  a.rowptr = h->rowptr_dev; a.idx = h->u.idx; a.val = h->u.val;
  a.users = d_users; a.t_sel = d_sel; a.t_item = d_items; a.Wb = Wb;
  a.Lt = h->u.L; a.Et = h->u.E; a.Eb = h->it.E;
  a.flags = d_flag; a.nt = nt; a.n_sel = n_sel; a.ld = ld; a.ldf = ldf; a.K = h->K; a.T = T; a.run = hpf_plan::BECAUSE_RUN;
  a.ubias_col = h->cfg.bias ? h->u.bias_col : -1; a.ujunk_col = h->cfg.bias ? h->u.junk_col : -1;
  a.s_prior = h->cfg.s_prior;
  if (!launch_because((int)bp.R, false, a, bp.grid_users(n_sel), h->stream)) { h->err = "because_shape_kernel: no instance for this column count"; return HPF_ERR_UNSUPPORTED; }
  if ((rc = check_launch(h, "because_shape_kernel"))) return rc;
  if (!launch_because((int)bp.R, true, a, bp.grid_pairs(nt), h->stream)) { h->err = "because_kernel: no instance for this column count"; return HPF_ERR_UNSUPPORTED; }
  if ((rc = check_launch(h, "because_kernel"))) return rc;
  uint32_t fl = 0;
  if ((rc = copy_back(h, {{&fl, d_flag, 4}}))) return rc;
  if (fl & 1u) {                                     // before any output reaches the caller
    h->err = "hpf_because: a softmax denominator underflowed to zero (Elog spread > ~700): the state is not a valid HPF state";
    return HPF_ERR_STATE;
  }
  return copy_back(h, {{out_item, a.out_item, nt * T * 4}, {out_contrib, a.out_contrib, nt * T * 8}, {out_sum, a.out_sum, nt * 8}, {out_prior, a.out_prior, nt * 8}});
}

// The topn heaviest rows of every factor column of one side: a batch of columns transposed into a temporary of this call
// (transpose_cols_kernel; hpf_plan::factor_top_batch), then hpf_rank_topn's selection, a workgroup per column over its
// contiguous row (topn_kernel: block_topn as it stands).  Bias columns are never transposed.
int hpf_factor_top(hpf_handle *h, int side, uint32_t topn, uint32_t *out_ids, double *out_vals)
{
  if (!h) return HPF_ERR_INVALID;
  if (side != 0 && side != 1) { h->err = "hpf_factor_top: side is 0 (users) or 1 (items)"; return HPF_ERR_INVALID; }
  if (topn < 1 || topn > hpf_plan::FACTOR_TOP_MAX) { h->err = "hpf_factor_top: topn is 1 .. 1024"; return HPF_ERR_INVALID; }
  if (!out_ids || !out_vals) { h->err = "hpf_factor_top: null pointer"; return HPF_ERR_INVALID; }
  Side &s = side ? h->it : h->u;
  int rc;
  if ((rc = ready(h, hpf_lazy::FACTORS, side))) return rc;
  const uint32_t rows = s.rows, K = h->K, NP = hpf_plan::pow2_ceil(topn);
  const uint32_t batch = hpf_plan::factor_top_batch(rows, K, h->ftop_batch);
  static_assert(hpf_plan::FACTOR_TOP_TILE == 32, "transpose_cols_kernel's tile");
  // a launch holds fewer than 2^32 work-items: a batch is <= 2^26 doubles unless one column alone is longer
  if ((((uint64_t)rows + 31) / 32) * (((uint64_t)batch + 31) / 32) * 256 >= (1ull << 32)) { h->err = "hpf_factor_top: too many rows for one launch"; return HPF_ERR_UNSUPPORTED; }
  Scratch sc(h);
  double *d_cols = nullptr, *d_vals = nullptr; uint32_t *d_ids = nullptr;
  if ((rc = sc.alloc(&d_cols, (size_t)batch * std::max<uint32_t>(rows, 1))) || (rc = sc.alloc(&d_ids, (size_t)K * topn)) || (rc = sc.alloc(&d_vals, (size_t)K * topn))) return rc;
  for (uint32_t k0 = 0; k0 < K; k0 += batch) {
    const uint32_t nc = std::min(batch, K - k0);
    if (rows) {
      hipLaunchKernelGGL(transpose_cols_kernel, dim3((rows + hpf_plan::FACTOR_TOP_TILE - 1) / hpf_plan::FACTOR_TOP_TILE, (nc + hpf_plan::FACTOR_TOP_TILE - 1) / hpf_plan::FACTOR_TOP_TILE),
                         dim3(256), 0, h->stream, s.E, d_cols, rows, h->ld, k0, nc);
      if ((rc = check_launch(h, "transpose_cols_kernel"))) return rc;
    }
    hipLaunchKernelGGL(topn_kernel, dim3(nc), dim3(256), (size_t)NP * 12, h->stream, d_cols, nc, rows, topn, NP,
                       d_ids + (size_t)k0 * topn, d_vals + (size_t)k0 * topn);
    if ((rc = check_launch(h, "topn_kernel"))) return rc;
  }
  return copy_back(h, {{out_ids, d_ids, (size_t)K * topn * 4}, {out_vals, d_vals, (size_t)K * topn * 8}});
}

int hpf_get_work_info(hpf_handle *h, hpf_work_info *out)
{
  if (!h || !out) return HPF_ERR_INVALID;
  memset(out, 0, sizeof *out);
  out->nnz = h->nnz;
  out->user_segments = h->u.nseg;
  out->user_long_rows = h->u.nlong + h->u.nhuge;
  out->user_huge_rows = h->u.nhuge;
  out->item_segments = h->it.nseg;
  out->item_long_rows = h->it.nlong + h->it.nhuge;
  out->item_huge_rows = h->it.nhuge;
  out->phi_G = (uint32_t)h->phiG; out->phi_R = (uint32_t)h->phiR; out->phi_V = (uint32_t)h->phiV;
  out->sweep_G = (uint32_t)h->swG; out->sweep_R = (uint32_t)h->swR;
  out->ld = h->ld;
  out->w_layout = (uint32_t)h->wl;
  out->tiles_user = h->u.tiles; out->tiles_item = h->it.tiles;
  out->tile_rows_user = h->u.tile_rows; out->tile_rows_item = h->it.tile_rows;
  out->heavy_min_nnz_user = h->u.tiles ? h->u.light_below : 0; out->heavy_min_nnz_item = h->it.tiles ? h->it.light_below : 0;
  out->w_fallbacks = h->fallbacks;
  out->notes = h->notes;
  out->start_sums_pending = h->lz.start_sums_pending() ? 1u : 0u;
  out->graph_replay = (h->cfg.n_ranks == 1 && !h->comm) ? ((h->have_csr && want_graph(h)) ? 1u : 0u) : (h->have_csr && split_graph_on(h) ? 2u : 0u);
  out->tile_chunk_user = h->u.chunks ? h->u.chunk_segs : 0; out->tile_chunk_item = h->it.chunks ? h->it.chunk_segs : 0;
  return HPF_OK;
}

int hpf_gather_only(hpf_handle *h, int side, int reps, float *ms_out)
{
  if (!h || !ms_out || reps < 1 || (side != 0 && side != 1)) return HPF_ERR_INVALID;
  if (!h->have_csr) { h->err = "hpf_upload_csr has not been called"; return HPF_ERR_STATE; }
  if (h->w32 || (h->wl == WL_PLAIN && h->phiV != 2)) { h->err = "gather-only probe: rows of 16-byte pieces only"; return HPF_ERR_UNSUPPORTED; }
  int rc;
  if ((rc = ready(h, hpf_lazy::GATHER_PROBE))) return rc;
  Side &own = side ? h->it : h->u, &oth = side ? h->u : h->it;
  PhiArgs a;
  const PhiLaunch pl = phi_setup(h, own, oth, false, a);         // the pass's own workgroups
  *ms_out = 0.0f;
  if (!a.nseg) return HPF_OK;
  Scratch sc(h);
  uint32_t *sink = nullptr;
  if ((rc = sc.alloc(&sink, 1))) return rc;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  hipError_t e = hipEventCreate(&e0);
  if (e == hipSuccess) e = hipEventCreate(&e1);
  bool ok = e == hipSuccess && launch_gather_only(h->phiG, h->phiR, a, sink, pl);      // warm-up
  if (ok) {
    e = hipEventRecord(e0, h->stream);
    for (int r = 0; r < reps && ok; ++r) ok = launch_gather_only(h->phiG, h->phiR, a, sink, pl);
    if (e == hipSuccess) e = hipEventRecord(e1, h->stream);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    float ms = 0.0f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    *ms_out = ms / (float)reps;
  }
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  if (!ok) { h->err = "no gather-only kernel for this shape"; return HPF_ERR_UNSUPPORTED; }
  if (e != hipSuccess) { h->err = std::string("gather-only probe: ") + hipGetErrorString(e); return HPF_ERR_HIP; }
  return check_launch(h, "gather-only probe");
}

int hpf_host_alloc(void **ptr, size_t bytes)
{
  if (!ptr) return HPF_ERR_INVALID;
  *ptr = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { (void)hipGetLastError(); return HPF_ERR_NO_DEVICE; }
  if (hipHostMalloc(ptr, std::max<size_t>(bytes, 1), hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); *ptr = nullptr; return HPF_ERR_OOM; }
  return HPF_OK;
}

int hpf_host_free(void *ptr)
{
  if (!ptr) return HPF_OK;
  if (hipHostFree(ptr) != hipSuccess) { (void)hipGetLastError(); return HPF_ERR_INVALID; }
  return HPF_OK;
}

int hpf_synchronize(hpf_handle *h)
{
  if (!h) return HPF_ERR_INVALID;
  return ready(h, hpf_lazy::FLAGS);
}

int hpf_mean_timing(hpf_handle *h, uint32_t n_last, hpf_timing *out)
{
  if (!h || !out) return HPF_ERR_INVALID;
  memset(out, 0, sizeof *out);
  out->iterations = h->iterations;
  uint32_t n = std::min<uint32_t>(std::min<uint32_t>(n_last, h->ev_count), hpf_handle::RING);
  if (n == 0) return HPF_OK;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (uint32_t k = 0; k < n; ++k) {
    const uint32_t slot = (h->ev_count - 1 - k) % hpf_handle::RING;
    hipEvent_t *ev = h->evr[slot];
    float ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // a graph-replayed iteration is one launch: only its total is known
    if (!h->ring_graphed[slot]) {
      for (int j = 0; j < 5; ++j) HIPCHK(h, hipEventElapsedTime(&ms[j], ev[j], ev[j + 1]));
      HIPCHK(h, hipEventElapsedTime(&ms[7], ev[5], ev[7]));      // exchange the stream waited for
      HIPCHK(h, hipEventElapsedTime(&ms[5], ev[7], ev[6]));      // the item sweep itself
    }
    HIPCHK(h, hipEventElapsedTime(&ms[6], ev[0], ev[6]));
    for (int j = 0; j < 8; ++j) acc[j] += ms[j];
  }
  out->phi_item_ms = (float)(acc[0] / n);
  out->combine_item_ms = (float)(acc[1] / n);
  out->phi_user_ms = (float)(acc[2] / n);
  out->combine_user_ms = (float)(acc[3] / n);
  out->sweep_user_ms = (float)(acc[4] / n);
  out->sweep_item_ms = (float)(acc[5] / n);
  out->iteration_ms = (float)(acc[6] / n);
  out->exchange_wait_ms = (float)(acc[7] / n);
  return HPF_OK;
}

int hpf_last_timing(hpf_handle *h, hpf_timing *out) { return hpf_mean_timing(h, 1, out); }

int hpf_iteration_times(hpf_handle *h, uint32_t n_last, float *ms_out, uint32_t *n_out)
{
  if (!h || !ms_out || !n_out) return HPF_ERR_INVALID;
  *n_out = 0;
  const uint32_t n = std::min<uint32_t>(std::min<uint32_t>(n_last, h->ev_count), hpf_handle::RING);
  if (n == 0) return HPF_OK;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (uint32_t k = 0; k < n; ++k) {                       // oldest first
    const uint32_t slot = (h->ev_count - n + k) % hpf_handle::RING;
    float ms = 0.0f;
    HIPCHK(h, hipEventElapsedTime(&ms, h->evr[slot][0], h->evr[slot][6]));
    ms_out[k] = ms;
  }
  *n_out = n;
  return HPF_OK;
}

int hpf_debug_poke_index(hpf_handle *h, int side, uint64_t pos, uint32_t value, uint32_t *old_value, uint32_t *owner_row)
{
  if (!h || (side != 0 && side != 1)) return HPF_ERR_INVALID;
  if (!h->have_csr) { h->err = "hpf_upload_csr has not been called"; return HPF_ERR_STATE; }
  Side &own = side ? h->it : h->u, &oth = side ? h->u : h->it;
  if (pos >= h->nnz || value >= oth.rows) { h->err = "poke: position or value out of range"; return HPF_ERR_INVALID; }
  uint32_t *arr = own.p_idx ? own.p_idx : own.idx;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  uint32_t old = 0;
  HIPCHK(h, hipMemcpy(&old, arr + pos, 4, hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemcpy(arr + pos, &value, 4, hipMemcpyHostToDevice));
  if (old_value) *old_value = old;
  if (owner_row) {                          // the segment that holds the position names its owner
    std::vector<Seg> segs(own.nseg);
    if (own.nseg) HIPCHK(h, hipMemcpy(segs.data(), own.segs, (size_t)own.nseg * sizeof(Seg), hipMemcpyDeviceToHost));
    *owner_row = 0xffffffffu;
    for (const Seg &sg : segs)
      if ((uint64_t)sg.start <= pos && pos < (uint64_t)sg.start + sg.len) { *owner_row = sg.row; break; }
  }
  drop_graph(h);
  return HPF_OK;
}

int hpf_algorithmic_bytes(hpf_handle *h, uint64_t *phi_user, uint64_t *phi_item, uint64_t *rows)
{
  if (!h) return HPF_ERR_INVALID;
  // SURVEY.md 8(d) with s_a = 8, K' = K + (bias ? 1 : 0) and s_e = the bytes a stored element of W
  // takes: 8 in plain rows, 59/8 in the lossless packed rows (the default at K = 100), 6 / 4 in
  // the opt-in lossy modes -- so that "algorithmic bytes" never exceed what has to move.  The
  // item-side accumulate term nnz*K'*s_a of that formula is, in this
  // formulation, the gather of the item pass (same byte count); the item pass
  // is credited with that term only (its own index / row traffic is not
  // counted), so phi_user + phi_item == B_phi of SURVEY.md exactly.
  const uint64_t Kp = h->K + (h->cfg.bias ? 1u : 0u), nnz = h->nnz;
  const uint64_t by = h->u.val ? 1u : 0u, n = h->u.rows, m = h->it.rows;
  const uint64_t seb = h->w32 ? 32 : h->wl == WL_F48 ? 48 : h->wl == WL_P59 ? 59 : 64, sa = 8;   // BITS per stored W element; bytes per accumulator
  if (phi_user) *phi_user = nnz * (4 + by) + 8 * (n + 1) + nnz * Kp * seb / 8 + n * Kp * seb / 8 + n * Kp * sa;
  if (phi_item) *phi_item = nnz * Kp * seb / 8;
  if (rows) *rows = (n + m) * Kp * 2 * sa + (n + m) * Kp * 2 * seb / 8 + 64 * (n + m);
  return HPF_OK;
}

}  // extern "C"
