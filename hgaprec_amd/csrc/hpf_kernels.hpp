// hpf_kernels.hpp -- hand-written gfx950 (CDNA4, wave64) kernels for the
// hgaprec CAVI inner loop.  No MFMA: the path is gather / elementwise /
// small-group reduction work, HBM- and L2-bound.
//
// Formulation.  The reference computes, per nonzero (u,i,y)
//   phi_k = y * exp(x_k - logsumexp(x)),  x_k = Elog_theta[u,k] + Elog_beta[i,k]
// (hgaprec.cc:206-239 get_phi, matrix.hh:367-389 logsum/lognormalize) and adds
// phi to the shape rows of u and of i (gpbase.hh:175-180).  Because
// exp(a+b) = exp(a)exp(b) and the softmax is invariant to a per-row factor,
// the row sweeps store W = exp(Elog - rowmax(Elog)) once per matrix element
// and the per-nonzero work becomes
//   e_k = Wt[u,k] * Wb[i,k];   phi_k = y * e_k / sum_j e_j
// -- no transcendental in the nnz*K loop.  The two shape scatters become two
// gather passes (user-major over CSR, item-major over CSC) so that every
// shape row is produced by exactly one owner in a fixed order: no atomics,
// bit-reproducible results.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cmath>
#include <type_traits>

#include "hpf_plan.hpp"   // plain C++: the constexpr arithmetic a kernel shares with its plan (fold_part)
#include "hpf_rng.hpp"    // host and device: Philox4x32-10 and the Gamma sampler of gamma_rows_kernel

// Build-time switches (A/B builds of tools/ and profiles/ only; the library ships the defaults)
#ifndef HPF_REDUCE_SCATTER
#define HPF_REDUCE_SCATTER 1   // end of a segment in the packed passes: 1 = the groups' accumulators reduced halving the element list
#endif                         // per level (round 6), 0 = every element on every lane at every level (rounds 1-5); the same bits
#ifndef HPF_P59_PAIRED
#define HPF_P59_PAIRED 1       // order of a p59 lane's dwords: 1 = (low word, stream dword) pairs (round 6), 0 = round 5's
#endif

namespace hpf {

// ---------------------------------------------------------------------
// work item of a phi pass: up to seg_max consecutive nonzeros of ONE owner row
// ---------------------------------------------------------------------
struct Seg {
  int64_t  start;   // first nonzero (index into idx/val)
  uint32_t row;     // owner row
  uint32_t len;     // nonzeros in this segment (may be 0 for an empty row)
  int32_t  pslot;   // >= 0: write the partial sum to partial[pslot] (long row)
                    //  < 0: the row is a single segment, write S[row] directly
  uint32_t pad;
};

struct LongRow { uint32_t row; uint32_t first_slot; uint32_t nslots; uint32_t pad; };

// ---------------------------------------------------------------------
// cross-lane helpers (wave64).  DPP moves for spans inside a 16-lane row,
// ds_bpermute (via __shfl_xor) across rows.
// ---------------------------------------------------------------------
template <int CTRL>
__device__ __forceinline__ double dpp_mov(double v)
{
  int lo = __double2loint(v), hi = __double2hiint(v);
  // every lane reads a live lane under these controls: bound_ctrl frees the destination
  // from being tied to an "old" value (no v_mov copy in front of each v_mov_dpp)
  lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xf, 0xf, true);
  hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}

// sum over aligned groups of G lanes; every lane of the group gets the total
template <int G>
__device__ __forceinline__ double group_sum(double v)
{
  if (G >= 2)  v += dpp_mov<0xB1>(v);    // quad_perm [1,0,3,2]  : lane ^ 1
  if (G >= 4)  v += dpp_mov<0x4E>(v);    // quad_perm [2,3,0,1]  : lane ^ 2
  if (G >= 8)  v += dpp_mov<0x141>(v);   // row_half_mirror      : quad ^ 1
  if (G >= 16) v += dpp_mov<0x140>(v);   // row_mirror           : half ^ 1
  if (G >= 32) v += __shfl_xor(v, 16, 64);
  if (G >= 64) v += __shfl_xor(v, 32, 64);
  return v;
}

template <int G>
__device__ __forceinline__ double group_max(double v)
{
  if (G >= 2)  v = fmax(v, dpp_mov<0xB1>(v));
  if (G >= 4)  v = fmax(v, dpp_mov<0x4E>(v));
  if (G >= 8)  v = fmax(v, dpp_mov<0x141>(v));
  if (G >= 16) v = fmax(v, dpp_mov<0x140>(v));
  if (G >= 32) v = fmax(v, __shfl_xor(v, 16, 64));
  if (G >= 64) v = fmax(v, __shfl_xor(v, 32, 64));
  return v;
}

// 1/x to ~1 ulp: v_rcp_f64 seed + two Newton steps (5 instructions instead
// of the ~15 of an IEEE-exact fp64 division); x is a positive normal number.
// Measured against mpmath on [1e-300, 1e300] (tests/test_gpu_special.py): relative error <= 1.0 u, u = 2^-53 (asserted: 2 u)
__device__ __forceinline__ double fast_rcp(double x)
{
  double r = __builtin_amdgcn_rcp(x);
  double e = fma(-x, r, 1.0);
  r = fma(r, e, r);
  e = fma(-x, r, 1.0);
  return fma(r, e, r);
}

// ---------------------------------------------------------------------
// K1: phi pass.  Template: G lanes per nonzero, R loads per lane, V elements
// per load (8- or 16-byte loads).  The row stride of every device matrix is
// EXACTLY G*R*V elements (hpf_create pads K + 2*bias up to it; the pad columns
// of W hold zeros), so lane g of a group owns columns
//   (g + G*t)*V + v ,  t < R, v < V
// with no column test anywhere, and the stride is a compile-time constant.
// A wave walks one segment; its 64/G groups take consecutive nonzeros, so a
// "batch" is 64/G nonzeros.
//
// Per batch (round 3, VERDICT r2 #1: 188 -> ~60 VALU instructions at K=100):
//   ssum  = sum_k own_k * x_k          two FMA chains + DPP group sum
//   scale = yy / ssum                  v_rcp_f64 + 2 Newton steps (~1 ulp)
//   acc_k += x_k * scale               ONE fma per element: the owner's factor
//                                      own_k is the same for every nonzero of the
//                                      segment, so it multiplies the finished sum
//                                      once (S_k = own_k * acc_k) instead of every term
// The gathers of batch b+1 are in flight while batch b is worked on, in two
// register sets used alternately (no copies).  Inactive slots of the last
// batch gather row 0 and carry yy = 0.
// ---------------------------------------------------------------------
// V elements of type T moved by one 8- or 16-byte access
template <typename T, int V>
struct __attribute__((aligned((sizeof(T) * V > 16) ? 16 : sizeof(T) * V))) vecw { T x[V]; };

struct PhiArgs {
  const Seg      *segs;
  uint32_t        nseg;
  const uint32_t *idx;      // other-side row of each nonzero
  const uint8_t  *val;      // rating (NULL: all ones)
  const void     *W_own;    // [rows_own x G*R*V] of WT (double, or float in the f32-storage mode)
  const void     *W_oth;    // [rows_oth x G*R*V] of WT
  double         *S_own;    // [rows_own x G*R*V]  raw sums (prior added by sweep)
  double         *partial;  // [npartial x G*R*V]
  uint32_t       *flags;    // [0] bit 0: a live nonzero saw sum_k e_k == 0 (underflow of W); bit 1: a sweep had to flush an
                            // entry the p59 rows cannot hold; bit 2: a pass has seen bit 1 -- everything launched since is a
                            // no-op until the host has switched the row layout (hpf_capi.hip, recover_flush)
                            // [1] iterations begun with bits 1 and 2 clear (counted by the item-major pass, which opens an iteration)
  // tiled pass (hpf_build.hpp): workgroup b works on the segments [chunks[b].x, chunks[b].y), one wave
  // per segment in turn; the host lays the chunks out so that b % 8 -- the XCD a workgroup lands on --
  // walks one tile after another.  NULL: the waves stride over the whole list.
  const uint2    *chunks;
  uint32_t        ld;       // row stride of S_own / partial, columns (layouts whose rows do not fix it: codec_f64)
  // Fused sweep epilogue (phi_pass_fused_kernel only): what the row sweep of the owner side reads to write W.
  // A row that is ONE segment has its finished sums in registers at the segment's end; the pass then writes W_own[row] itself
  // and the sweep that follows only takes that row's sums (row_sums_kernel).  flags[0] bit 3: the epilogue met an element the
  // p59 rows cannot hold -- PENDING, so that workgroups of the same launch that start later do not skip; the sums kernel
  // turns it into bit 1 at its entry.
  struct Epi {
    void         *W_out;       // = W_own, writable: the only reader of W_own[row] in this launch is the segment's own load
    const double *prior_E;     // [rows_own] (hier)
    const double *colsum_oth;  // [ld]
    double        s_prior, r_prior, rate_bias;
    uint32_t      K, hier;
    int32_t       bias_col, junk_col;
  } epi;
};

// Entry of every phi-pass kernel.  A sweep that could not store an element in the packed rows raises bit 1;
// the passes that follow must not run on that W: they return at once (and the item-major pass, which opens
// an iteration, turns bit 1 into bit 2, which stops the sweeps as well) until the host -- at its next
// synchronisation point -- has moved the handle to plain fp64 rows and repeats what was skipped.
__device__ __forceinline__ bool phi_pass_skips(const PhiArgs &a, int side)
{
  const uint32_t fl = a.flags[0];
  if (side == 1 && blockIdx.x == 0 && threadIdx.x == 0) {
    if (fl & 2u) atomicOr(a.flags, 4u);
    else if (!(fl & 4u)) atomicAdd(a.flags + 1, 1u);
  }
  return (fl & 6u) != 0u;
}

// the segments of this wave: first, end, stride
struct SegRange { uint32_t s, end, step; };
__device__ __forceinline__ SegRange seg_range(const PhiArgs &a)
{
  SegRange r;
  if (a.chunks) {
    const uint2 c = a.chunks[blockIdx.x];
    r.s = __builtin_amdgcn_readfirstlane(c.x + (threadIdx.x >> 6));
    r.end = __builtin_amdgcn_readfirstlane(c.y);
    r.step = blockDim.x >> 6;
  } else {
    r.s = __builtin_amdgcn_readfirstlane((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    r.end = a.nseg;
    r.step = (gridDim.x * blockDim.x) >> 6;
  }
  return r;
}

// an item-major pass over no nonzeros at all still opens the iteration (phi_pass_skips)
__global__ void phi_open_kernel(PhiArgs a) { (void)phi_pass_skips(a, 1); }

// one batch: x = the gathered rows (one nonzero per group), yf = its rating
// factor as a float (0 for an empty slot)
template <typename WT, int G, int R, int V>
__device__ __forceinline__ void phi_batch(const vecw<WT, V> (&x)[R], const vecw<double, V> (&own)[R],
                                          vecw<double, V> (&acc)[R], float yf, bool &underflow)
{
  double s[2] = {0.0, 0.0};              // two FMA chains: the dependent latency is halved
#pragma unroll
  for (int e = 0; e < R * V; ++e) {
    const double o = own[e / V].x[e % V], xv = (double)x[e / V].x[e % V];
    s[e & 1] = (e < 2) ? o * xv : fma(o, xv, s[e & 1]);
  }
  const double ssum = group_sum<G>((R * V > 1) ? s[0] + s[1] : s[0]);
  const double yy = (double)yf;
  const bool ok = ssum > 0.0;
  underflow |= (yf > 0.0f) && !ok;
  const double scale = ok ? yy * fast_rcp(ssum) : 0.0;
#pragma unroll
  for (int t = 0; t < R; ++t)
#pragma unroll
    for (int v = 0; v < V; ++v) acc[t].x[v] = fma((double)x[t].x[v], scale, acc[t].x[v]);
}

// WT: storage type of W.  Arithmetic and accumulators are fp64 either way.
// SIDE only names the instantiation (0 = user-major pass over CSR, 1 =
// item-major pass over CSC) so that profilers report the passes apart.
template <typename WT, int G, int R, int V, int SIDE>
__global__ __launch_bounds__(256) void phi_pass_kernel(PhiArgs a)
{
  constexpr int NG = 64 / G;             // nonzeros per batch
  constexpr uint32_t LD = G * R * V;     // row stride, elements
  const int lane = threadIdx.x & 63;
  const int g = lane % G;                // column lane
  const int q = lane / G;                // group = nonzero slot in a batch
  if (phi_pass_skips(a, SIDE)) return;
  const SegRange sr = seg_range(a);
  const WT *W_own = (const WT *)a.W_own + (size_t)g * V;
  const WT *W_oth = (const WT *)a.W_oth + (size_t)g * V;
  bool underflow = false;

  for (uint32_t s = sr.s; s < sr.end; s += sr.step) {
    const Seg sg = a.segs[s];            // wave-uniform: scalar loads
    const uint32_t len = sg.len;
    const int64_t start = sg.start;

    vecw<double, V> own[R], acc[R];
    {
      const WT *wo = W_own + (size_t)sg.row * LD;
#pragma unroll
      for (int t = 0; t < R; ++t) {
        const vecw<WT, V> raw = *reinterpret_cast<const vecw<WT, V> *>(wo + (size_t)G * t * V);
#pragma unroll
        for (int v = 0; v < V; ++v) { own[t].x[v] = (double)raw.x[v]; acc[t].x[v] = 0.0; }
      }
    }

    if (len > 0) {
      // indices / rating factors of the current and the next chunk of 64 nonzeros, one
      // per lane.  The factor is yy = (y > 1 ? y : 1) -- "if (y > 1) phi.scale(y)",
      // hgaprec.cc:1355-1356: a rating that wrapped to 0 in the reference's uint8 store is
      // not scaled -- as a float (exact), 0 beyond the end of the segment.
      auto load_i = [&](uint32_t o) -> uint32_t { return (o < len) ? a.idx[start + o] : 0u; };
      auto load_y = [&](uint32_t o) -> float {
        if (o >= len) return 0.0f;
        if (!a.val) return 1.0f;
        const uint32_t y = a.val[start + o];
        return (y > 1u) ? (float)y : 1.0f;
      };
      uint32_t cur_i = load_i((uint32_t)lane), nxt_i = load_i(64u + lane);
      float cur_y = load_y((uint32_t)lane), nxt_y = load_y(64u + lane);

      const uint32_t nb = (len + NG - 1) / NG;      // batches
      vecw<WT, V> xa[R], xb[R];
      float ya, yb = 0.0f;
      auto gather = [&](vecw<WT, V> (&x)[R], float &y, uint32_t b) {
        const int src = (int)((b % G) * NG) + q;
        const uint32_t in = (uint32_t)__shfl((int)cur_i, src, 64);
        y = __shfl(cur_y, src, 64);
        const WT *p = W_oth + (size_t)in * LD;
#pragma unroll
        for (int t = 0; t < R; ++t) x[t] = *reinterpret_cast<const vecw<WT, V> *>(p + (size_t)G * t * V);
      };
      auto next_chunk = [&](uint32_t b) {           // batch b opens a new chunk of 64
        cur_i = nxt_i; cur_y = nxt_y;
        const uint32_t o = (b / G + 1) * 64u + lane;
        nxt_i = load_i(o); nxt_y = load_y(o);
      };
      // Two register sets, refilled right after their batch is consumed: 1-2 batches of
      // gathers are in flight behind the one being worked on.  The steady loop has no
      // conditional gather (a conditional one costs a third register set and a copy per
      // round); the last one to three batches are peeled.  G is even, so only even batch
      // numbers open a chunk.
      gather(xa, ya, 0);
      if (nb > 1) gather(xb, yb, 1);
      uint32_t bb = 0;
      for (; bb + 3 < nb; bb += 2) {
        phi_batch<WT, G, R, V>(xa, own, acc, ya, underflow);
        __builtin_amdgcn_sched_barrier(0);   // the refill stays behind the last use of xa
        if (((bb + 2) % G) == 0) next_chunk(bb + 2);
        gather(xa, ya, bb + 2);
        phi_batch<WT, G, R, V>(xb, own, acc, yb, underflow);
        __builtin_amdgcn_sched_barrier(0);
        gather(xb, yb, bb + 3);
      }
      phi_batch<WT, G, R, V>(xa, own, acc, ya, underflow);
      if (bb + 1 < nb) {
        const bool third = bb + 2 < nb;
        __builtin_amdgcn_sched_barrier(0);
        if (third) {
          if (((bb + 2) % G) == 0) next_chunk(bb + 2);
          gather(xa, ya, bb + 2);
        }
        phi_batch<WT, G, R, V>(xb, own, acc, yb, underflow);
        if (third) phi_batch<WT, G, R, V>(xa, own, acc, ya, underflow);
      }
    }

    // ---- reduce the 64/G group accumulators, apply the owner's factor, write the row (or partial)
    double *dst = ((sg.pslot >= 0) ? a.partial + (size_t)sg.pslot * LD : a.S_own + (size_t)sg.row * LD) + (size_t)g * V;
#pragma unroll
    for (int t = 0; t < R; ++t) {
#pragma unroll
      for (int v = 0; v < V; ++v) {
        double r = acc[t].x[v];
        if (G <= 32) r += __shfl_xor(r, 32, 64);
        if (G <= 16) r += __shfl_xor(r, 16, 64);
        if (G <= 8)  r += __shfl_xor(r, 8, 64);
        if (G <= 4)  r += __shfl_xor(r, 4, 64);
        acc[t].x[v] = own[t].x[v] * r;
      }
      if (q == 0) *reinterpret_cast<vecw<double, V> *>(dst + (size_t)G * t * V) = acc[t];
    }
  }
  if (__any(underflow) && lane == 0) atomicOr(a.flags, 1u);
}

// ---------------------------------------------------------------------
// K1 over PACKED rows of W.  Both phi passes sit at the rate at which L2 misses are filled
// (DESIGN.md section 6): the only lever left is 128-byte lines per gathered row.
//
//   p59  (the default whenever it shortens the row; LOSSLESS): every W is a positive fp64 in
//        [2^-126, 2) or zero, so its sign bit and the four high exponent bits carry nothing:
//        52 mantissa + 7 exponent bits = 59 bits per element.  K = 100: 104 columns in 768 bytes
//        = six lines instead of seven.  A W below 2^-126 of its row maximum (an Elog spread
//        above 88 inside a row) cannot be stored: the sweep flushes it to zero and raises flag
//        bit 1 (hpf_config.w_storage = 3 keeps plain fp64 rows for such states).
//   f48  (hpf_config.w_storage = 2, opt-in, LOSSY): the top 48 bits of the fp64 value
//        (36 mantissa bits, rounded to nearest even: 2^-37 relative).  K = 100: five lines.
//
// A row is L 16-byte pieces per lane for G lanes, INTERLEAVED: piece t of lane g sits at byte
// (t*G + g)*16, so that one load instruction of a lane group reads G*16 contiguous bytes.  The
// 4L dwords of a lane hold E elements; lane g owns columns e*G + g.  Layout of a lane's dwords
//   p59: LOGICAL dwords k = 0 .. E + S - 1: k < E is the low 32 mantissa bits of element k; the S dwords from E on are
//        a stream of 27-bit fields (7 exponent bits above 20 mantissa bits; the all-zero element stands for 0 and
//        reads back as 2^-127), element e at bit 27 e of the stream.  PHYSICALLY, logical dword k sits at place
//        codec_p59<L>::pos(k) of the lane's 4L (p59_pos at run time): since round 6 the low word of element e at the
//        even place 2e beside stream dword e at the odd place 2e + 1 (HPF_P59_PAIRED; 0 = the logical order itself).
//        pos is one-to-one into [0, 4L) for every L in both orders (static_assert in hpf_probe.hip)
//   f48: d[0..E)  high dwords; then the 16-bit low parts, two per dword
// Row stride of the fp64 matrices (S, E, Elog) and of the exchange buffer: ld = G*E columns.
// Arithmetic and accumulators are fp64 in every mode.
// ---------------------------------------------------------------------
//   f64  plain fp64 elements in the same interleaved pieces, two per piece (E = 2L).  What a handle falls back to
//        when a state turns up that p59 cannot hold (hpf_capi.hip, recover_flush) and what hpf_config.w_storage = 3
//        asks for from the start.
//        The row stride of S / partial stays that of the packed shape it stands in for (PhiArgs::ld <= G * E).
enum { WL_PLAIN = 0, WL_F48 = 2, WL_P59 = 3, WL_F64 = 4 };      // layout codes (hpf_work_info.w_layout)

template <int L> struct codec_f64 {
  static constexpr int E = 2 * L;
  static constexpr bool fixed_ld = false;
  static __device__ __forceinline__ double get(const uint32_t (&d)[4 * L], int e)
  {
    return __hiloint2double((int)d[2 * e + 1], (int)d[2 * e]);
  }
};

template <int L> struct codec_f48 {
  static constexpr bool fixed_ld = true;
  static constexpr int E = (8 * L) / 3;                   // 2 5 8 10 13 16 18 21
  static_assert(E + (E + 1) / 2 <= 4 * L, "lane dwords overflow");
  static __device__ __forceinline__ double get(const uint32_t (&d)[4 * L], int e)
  {
    const uint32_t lw = d[E + e / 2];
    return __hiloint2double((int)d[e], (int)((e & 1) ? (lw & 0xffff0000u) : (lw << 16)));
  }
};

template <int L> struct codec_p59 {
  static constexpr bool fixed_ld = true;
  static constexpr int E = (128 * L) / 59;                // 2 4 6 8 10 13 15 17
  static constexpr int S = (27 * E + 31) / 32;            // dwords of the field stream
  static_assert(E + S <= 4 * L, "lane dwords overflow");
  // Place of logical dword k among the lane's 4L (k < E: low word of element k; k >= E: dword k - E of the field stream).
  // Round 6: PAIRED -- the low word of element e sits at the even place 2e and stream dword j at the odd place 2j + 1 (the
  // E - 2L low words that find no even place take the odd places the stream leaves free).  A decoded element is the register
  // PAIR (low word, high word) and the high word is computed from the stream: with the low word in an even register and a
  // stream dword that is dead by then beside it, the pair is formed in place -- the elements are decoded from the last to the
  // first, so that stream dword e has been consumed by the elements above e when element e overwrites it.  In the round-5
  // order (all low words, then the stream) every other low word had to be copied into a fresh pair first: 11 v_mov per batch
  // of 93 VALU instructions and 12 more registers (tools/count_isa.py; profiles/r06/experiments.md 1).
  // pos_as names the order explicitly (hpf_probe.hip asserts at compile time that BOTH orders place the E + S logical dwords
  // one-to-one into [0, 4L)); pos is the order this build uses.
  static constexpr __host__ __device__ int pos_as(bool paired, int k)
  {
    if (!paired) return k;
    return k < E ? (k < 2 * L ? 2 * k : 2 * (S + k - 2 * L) + 1) : 2 * (k - E) + 1;
  }
  static constexpr __host__ __device__ int pos(int k) { return pos_as(HPF_P59_PAIRED != 0, k); }
  static __device__ __forceinline__ double get(const uint32_t (&d)[4 * L], int e)
  {
    const int o = 27 * e, i = E + o / 32, sh = o % 32;    // compile-time after unrolling
    uint32_t f;
    if (sh == 0) f = d[pos(i)];
    else if (sh + 27 <= 32) f = d[pos(i)] >> sh;
    else f = __builtin_amdgcn_alignbit(d[pos(i + 1)], d[pos(i)], sh);
    // exponent field + 896.  The all-zero element (padding columns, a flushed entry) decodes to
    // 2^-127 = 5.9e-39 instead of 0 -- no compare and two selects per element: products of two such
    // entries are 3e-77, below any sum they could join by sixty orders.  Mask and bias in ONE
    // instruction: v_and_or_b32 takes no literal on gfx9, so the mask sits in an SGPR and the bias in
    // a VGPR (the compiler left to itself emits v_and + v_or with literals)
    uint32_t hi;
    asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(hi) : "v"(f), "s"(0x7ffffffu), "v"(0x38000000u));
    return __hiloint2double((int)hi, (int)d[pos(e)]);
  }
};

// ---- writing packed rows (row sweep, derive_w): a group of lanes builds the row in LDS -- the
// 27-bit fields of p59 straddle dwords, so they are OR-ed in (ds_or_b32: order-free, hence
// deterministic) -- and copies it out with 16-byte stores.  `buf` has the layout of the row.
struct PackedRow { uint32_t G, E, L, row_bytes, lgG; };  // of the phi kernel shape (G = 1 << lgG: no integer division)

__device__ __forceinline__ uint32_t packed_dword_index(const PackedRow &pk, uint32_t g, uint32_t d)
{
  return ((((d >> 2) << pk.lgG) + g) << 2) + (d & 3u);   // piece (d/4) of lane g, word d%4
}

__device__ __forceinline__ void packed_clear(uint32_t *buf, const PackedRow &pk, uint32_t li, uint32_t nl)
{
  for (uint32_t d = li; d < pk.row_bytes / 4; d += nl) buf[d] = 0u;
}

// codec_p59<L>::pos at run time (the LDS writers take the shape from PackedRow)
__device__ __forceinline__ uint32_t p59_pos(const PackedRow &pk, uint32_t k)
{
  if (!HPF_P59_PAIRED) return k;
  const uint32_t S = (27u * pk.E + 31u) / 32u;
  return k < pk.E ? (k < 2u * pk.L ? 2u * k : 2u * (S + k - 2u * pk.L) + 1u) : 2u * (k - pk.E) + 1u;
}

// What an element w puts into a p59 lane: its low word and its 27-bit field (both writers, p59_put and the register form of
// the row sweep).  Representable: exponent field 897..1023, i.e. 2^-126 <= w < 2.  Anything else -- zero, a smaller
// value, and what a valid state never holds: w >= 2, infinities, NaN, negative numbers -- is stored as
// the all-zero element; only an exact +0 does so without being reported (flushed).  live = false: a slot past the end of
// the row, which holds the all-zero element whatever w is
struct P59Words { uint32_t lo, f; bool flushed; };
__device__ __forceinline__ P59Words p59_words(double w, bool live = true)
{
  const uint32_t hi = (uint32_t)__double2hiint(w), lo = (uint32_t)__double2loint(w);
  const bool tiny = hi < 0x38100000u || hi >= 0x40000000u;
  P59Words r;
  r.flushed = live && tiny && !(hi == 0u && lo == 0u);
  r.f = (tiny || !live) ? 0u : hi - 0x38000000u;
  r.lo = (tiny || !live) ? 0u : lo;
  return r;
}

// returns true when a nonzero w had to be flushed (below 2^-126)
__device__ __forceinline__ bool p59_put(uint32_t *buf, const PackedRow &pk, uint32_t c, double w)
{
  const uint32_t g = c & (pk.G - 1u), e = c >> pk.lgG;
  const P59Words pw = p59_words(w);
  const uint32_t f = pw.f;
  buf[packed_dword_index(pk, g, p59_pos(pk, e))] = pw.lo;
  const uint32_t o = 27u * e, i = pk.E + o / 32u, sh = o % 32u;
  if (f) {
    atomicOr(&buf[packed_dword_index(pk, g, p59_pos(pk, i))], f << sh);
    if (sh > 5u) atomicOr(&buf[packed_dword_index(pk, g, p59_pos(pk, i + 1))], f >> (32u - sh));
  }
  return pw.flushed;
}

__device__ __forceinline__ void f48_put(uint32_t *buf, const PackedRow &pk, uint32_t c, double w)
{
  const uint32_t g = c & (pk.G - 1u), e = c >> pk.lgG;
  unsigned long long b = (unsigned long long)__double_as_longlong(w);
  b += 0x7fffull + ((b >> 16) & 1ull);                    // round to nearest even at bit 16
  buf[packed_dword_index(pk, g, e)] = (uint32_t)(b >> 32);
  atomicOr(&buf[packed_dword_index(pk, g, pk.E + e / 2)], (uint32_t)((b >> 16) & 0xffffull) << (16u * (e & 1u)));
}

__device__ __forceinline__ void packed_copy_out(const uint32_t *buf, void *W, size_t row, const PackedRow &pk,
                                                uint32_t li, uint32_t nl)
{
  uint4 *dst = reinterpret_cast<uint4 *>((unsigned char *)W + row * (size_t)pk.row_bytes);
  const uint4 *src = reinterpret_cast<const uint4 *>(buf);
  for (uint32_t p = li; p < pk.row_bytes / 16; p += nl) dst[p] = src[p];
}

// one batch over E element slots: x = the gathered rows in OthC's layout (LT pieces per lane)
// element c of a row of plain doubles in interleaved pieces (codec_f64): piece e/2 of lane g, half e%2
__device__ __forceinline__ void f64_put(void *W, size_t row, const PackedRow &pk, uint32_t c, double w)
{
  const uint32_t g = c & (pk.G - 1u), e = c >> pk.lgG;
  double *d = reinterpret_cast<double *>((unsigned char *)W + row * (size_t)pk.row_bytes);
  d[((((e >> 1) << pk.lgG) + g) << 1) + (e & 1u)] = w;
}

// ---- reduce-scatter of a wave's 64 / G group accumulators (phi_segments) --------------------------------------------
// element slots a lane holds after the levels at lane distances D, D/2, ..., G
template <int G, int N, int D = 32> struct scatter_len_at { static constexpr int value = D >= G ? scatter_len_at<G, (N + 1) / 2, D / 2>::value : N; };
template <int G, int N> struct scatter_len_at<G, N, 0> { static constexpr int value = N; };
template <int G, int E> struct scatter_len { static constexpr int value = scatter_len_at<G, E, 32>::value; };

// one level at lane distance D over the first N slots of v / w (w: the owner's factors, selected alongside); o, n: the run
// of element slots this lane holds -- [o, o + n) -- before and after
template <int G, int E, int D, int N = E>
__device__ __forceinline__ void reduce_scatter(double (&v)[E], double (&w)[E], int lane, uint32_t &o, uint32_t &n)
{
  if constexpr (D >= G && D >= 1) {
    constexpr int NA = (N + 1) / 2;                       // the half a lane with bit D clear keeps
    const bool up = (lane & D) != 0;
#pragma unroll
    for (int j = 0; j < NA; ++j) {
      const bool hasB = NA + j < N;
      const double A = v[j], B = hasB ? v[NA + j] : 0.0;
      if constexpr (D == 32 || D == 16) {
        // gfx950's v_permlane32_swap / v_permlane16_swap exchange the upper half (the odd 16-lane rows) of one register with
        // the lower half (the even rows) of another: with A and B as the two registers, afterwards the FIRST holds, on the
        // lanes that keep A, their own A and, on the lanes that keep B, the partner's B -- and the second the other two.
        // Their sum is mine + the partner's on every lane: no select, no LDS crossbar.
        const uint32_t alo = (uint32_t)__double2loint(A), ahi = (uint32_t)__double2hiint(A);
        const uint32_t blo = (uint32_t)__double2loint(B), bhi = (uint32_t)__double2hiint(B);
        double x, y;
        if constexpr (D == 32) {
          const auto lo = __builtin_amdgcn_permlane32_swap(alo, blo, false, false), hi = __builtin_amdgcn_permlane32_swap(ahi, bhi, false, false);
          x = __hiloint2double((int)hi[0], (int)lo[0]); y = __hiloint2double((int)hi[1], (int)lo[1]);
        } else {
          const auto lo = __builtin_amdgcn_permlane16_swap(alo, blo, false, false), hi = __builtin_amdgcn_permlane16_swap(ahi, bhi, false, false);
          x = __hiloint2double((int)hi[0], (int)lo[0]); y = __hiloint2double((int)hi[1], (int)lo[1]);
        }
        v[j] = x + y;
      } else {
        const double mine = up ? B : A, send = up ? A : B;
        v[j] = mine + (D == 8 ? dpp_mov<0x128>(send) /* row_ror:8 = lane ^ 8 inside a 16-lane row */ : __shfl_xor(send, D, 64));
      }
      if (hasB) w[j] = up ? w[NA + j] : w[j];
    }
    o += up ? (uint32_t)NA : 0u;
    n = up ? (n > (uint32_t)NA ? n - (uint32_t)NA : 0u) : (n < (uint32_t)NA ? n : (uint32_t)NA);
    reduce_scatter<G, E, D / 2, NA>(v, w, lane, o, n);
  }
}

template <class OthC, int E, int G, int LT>
__device__ __forceinline__ void phi_batch_packed(const uint32_t (&x)[4 * LT], const double (&own)[E],
                                                 double (&acc)[E], float yf, bool &underflow)
{
  double xv[E];
#pragma unroll
  for (int e = E - 1; e >= 0; --e) xv[e] = OthC::get(x, e);     // last to first: codec_p59::pos
  double s[2] = {0.0, 0.0};
#pragma unroll
  for (int e = 0; e < E; ++e) s[e & 1] = (e < 2) ? own[e] * xv[e] : fma(own[e], xv[e], s[e & 1]);
  const double ssum = group_sum<G>((E > 1) ? s[0] + s[1] : s[0]);
  const double yy = (double)yf;
  const bool ok = ssum > 0.0;
  underflow |= (yf > 0.0f) && !ok;
  const double scale = ok ? yy * fast_rcp(ssum) : 0.0;
#pragma unroll
  for (int e = 0; e < E; ++e) acc[e] = fma(xv[e], scale, acc[e]);
}

// The segments of one wave, over rows of 16-byte pieces: the owner's row in OwnC's layout (LO pieces per
// lane), the gathered rows in OthC's (LT pieces).  E = OwnC::E element slots are worked on (OthC::E >= E; the
// library only instantiates OwnC = OthC -- the two-layout form is what the fp64-shadow experiment of round 4
// ran on, profiles/r04/experiments.md 1).  W_own / W_oth already point at this lane's first piece.
// FUSE (the owner's rows are p59): a segment that is its whole row also writes W_own[row] -- the row sweep's psi / exp / row
// maximum / packing, by the sweep's own device functions on the totals the lanes hold after the reduce-scatter (the same
// bits).  pkbuf: this wave's row of LDS (G * LO * 4 dwords), cso: the other side's column sums in LDS (zeros from K on).
struct PsiRate { double xs, corr, ri; };
__device__ __forceinline__ PsiRate psi_parts_rate(double x, double rt);
__device__ __forceinline__ double exp_neg(double c);

template <class OwnC, class OthC, int G, int LO, int LT, bool FUSE = false>
__device__ __forceinline__ void phi_segments(const PhiArgs &a, const SegRange &sr, const unsigned char *W_own,
                                             const unsigned char *W_oth, int lane, bool &underflow,
                                             uint32_t *pkbuf = nullptr, const double *cso = nullptr)
{
  constexpr int NG = 64 / G;
  constexpr int E = OwnC::E;
  static_assert(OthC::E >= E, "the gathered layout must cover the owner's element slots");
  const uint32_t LD = OwnC::fixed_ld ? (uint32_t)(G * E) : a.ld;       // columns: stride of S / partial
  constexpr uint32_t ROWO = G * LO * 16, ROWT = G * LT * 16;           // bytes of a row of W, either layout
  const int g = lane % G, q = lane / G;

  auto load_own = [&](uint32_t (&d)[4 * LO], const unsigned char *base) {
#pragma unroll
    for (int t = 0; t < LO; ++t) {
      const uint4 v = *reinterpret_cast<const uint4 *>(base + (size_t)t * G * 16);
      d[4 * t] = v.x; d[4 * t + 1] = v.y; d[4 * t + 2] = v.z; d[4 * t + 3] = v.w;
    }
  };
  auto load_row = [&](uint32_t (&d)[4 * LT], const unsigned char *base) {
#pragma unroll
    for (int t = 0; t < LT; ++t) {
      const uint4 v = *reinterpret_cast<const uint4 *>(base + (size_t)t * G * 16);
      d[4 * t] = v.x; d[4 * t + 1] = v.y; d[4 * t + 2] = v.z; d[4 * t + 3] = v.w;
    }
  };
  // 64 indices / ratings of a segment from offset o on (zeros past its end)
  auto load_i = [&](int64_t start, uint32_t len, uint32_t o) -> uint32_t { return (o < len) ? a.idx[start + o] : 0u; };
  auto load_y = [&](int64_t start, uint32_t len, uint32_t o) -> float {
    if (o >= len) return 0.0f;
    if (!a.val) return 1.0f;
    const uint32_t y = a.val[start + o];
    return (y > 1u) ? (float)y : 1.0f;
  };

  // The wave's segments are one stream: the descriptor of the next segment and its first 64
  // indices are fetched while the current one is worked on, so that a segment starts with its
  // owner row and its first two batches of gathers in flight together -- one memory round trip
  // instead of three in a row (descriptor, indices, rows).  Rows of fifty nonzeros (C2's users)
  // and the runs of a tiled pass are a handful of batches long: the round trips were most of them.
  if (sr.s >= sr.end) return;
  Seg sgn = a.segs[sr.s];
  uint32_t nxt_i = load_i(sgn.start, sgn.len, (uint32_t)lane);
  float nxt_y = load_y(sgn.start, sgn.len, (uint32_t)lane);
  for (uint32_t s = sr.s; s < sr.end; s += sr.step) {
    const Seg sg = sgn;
    const bool more = s + sr.step < sr.end;
    if (more) sgn = a.segs[s + sr.step];
    const uint32_t len = sg.len;
    const int64_t start = sg.start;
    uint32_t cur_i = nxt_i;
    float cur_y = nxt_y;
    const uint32_t nb = (len + NG - 1) / NG;
    uint32_t xa[4 * LT], xb[4 * LT];
    float ya = 0.0f, yb = 0.0f;
    auto gather = [&](uint32_t (&x)[4 * LT], float &y, uint32_t b) {
      const int src = (int)((b % G) * NG) + q;
      const uint32_t in = (uint32_t)__shfl((int)cur_i, src, 64);
      y = __shfl(cur_y, src, 64);
      load_row(x, W_oth + (size_t)in * ROWT);
    };
    // chunk c has become the current one: fetch the one after it -- of this segment, or the
    // first one of the next segment
    auto fetch_after = [&](uint32_t c) {
      const uint32_t o = (c + 1) * 64u;
      const bool same = o < len;                        // scalar selects, no branch: one masked load each
      const int64_t st = same ? start : sgn.start;
      const uint32_t ln = same ? len : (more ? sgn.len : 0u), of = same ? o : 0u;
      nxt_i = load_i(st, ln, of + lane); nxt_y = load_y(st, ln, of + lane);
    };
    auto next_chunk = [&](uint32_t b) {
      cur_i = nxt_i; cur_y = nxt_y;
      fetch_after(b / G);
    };
    double own[E], acc[E];
    {
      uint32_t r[4 * LO];
      load_own(r, W_own + (size_t)sg.row * ROWO);
      gather(xa, ya, 0);          // unconditional (a conditional gather costs copies and waits): past the
      gather(xb, yb, 1);          // segment's end the index reads 0 -- row 0, loaded and never used
      fetch_after(0);
#pragma unroll
      for (int e = E - 1; e >= 0; --e) { own[e] = OwnC::get(r, e); acc[e] = 0.0; }
    }
    if (len > 0) {
      // same schedule as phi_pass_kernel: two register sets, peeled tail
      uint32_t bb = 0;
      for (; bb + 3 < nb; bb += 2) {
        phi_batch_packed<OthC, E, G, LT>(xa, own, acc, ya, underflow);
        __builtin_amdgcn_sched_barrier(0);
        if (((bb + 2) % G) == 0) next_chunk(bb + 2);
        gather(xa, ya, bb + 2);
        phi_batch_packed<OthC, E, G, LT>(xb, own, acc, yb, underflow);
        __builtin_amdgcn_sched_barrier(0);
        gather(xb, yb, bb + 3);
      }
      phi_batch_packed<OthC, E, G, LT>(xa, own, acc, ya, underflow);
      if (bb + 1 < nb) {
        const bool third = bb + 2 < nb;
        __builtin_amdgcn_sched_barrier(0);
        if (third) {
          if (((bb + 2) % G) == 0) next_chunk(bb + 2);
          gather(xa, ya, bb + 2);
        }
        phi_batch_packed<OthC, E, G, LT>(xb, own, acc, yb, underflow);
        if (third) phi_batch_packed<OthC, E, G, LT>(xa, own, acc, ya, underflow);
      }
    }
    double *dst = ((sg.pslot >= 0) ? a.partial + (size_t)sg.pslot * LD : a.S_own + (size_t)sg.row * LD) + g;
#if HPF_REDUCE_SCATTER
    // The 64 / G groups' accumulators, reduced HALVING the element list at every level instead of keeping every element on
    // every lane: at lane distance d a lane whose bit d is clear keeps the first half of its list and hands the second half to
    // its partner, and the other way round -- the same pairs are added as in the butterfly below (a + b on one lane is b + a
    // on the other: the same bits), but a level moves half the elements of the one before: 13 -> 7 -> 4 -> 2 (-> 1) shuffles
    // instead of 13 per level, and in the end lane (q, g) holds the totals of a contiguous run of element slots [o, o + n)
    // of column lane g, which ALL lanes then store at once.  The owner's factors follow by selects (no shuffle).
    {
      uint32_t o = 0, n = E;
      reduce_scatter<G, E, 32>(acc, own, lane, o, n);
      constexpr int NF = scatter_len<G, E>::value;          // element slots a lane ends with, at most
#pragma unroll
      for (int j = 0; j < NF; ++j) {
        const uint32_t e = o + (uint32_t)j;
        if ((uint32_t)j < n && (OwnC::fixed_ld || e * G + (uint32_t)g < LD)) dst[(size_t)e * G] = own[j] * acc[j];
      }
      if constexpr (FUSE) {
        static_assert(OwnC::fixed_ld && LO == LT, "the epilogue writes p59 rows");
        if (sg.pslot < 0) {                                   // wave-uniform: the row is this one segment
          const PhiArgs::Epi &ep = a.epi;
          const PackedRow pk = {(uint32_t)G, (uint32_t)E, (uint32_t)LO, (uint32_t)(G * LO * 16), (uint32_t)__builtin_ctz(G)};
          const double pr = ep.hier ? ep.prior_E[sg.row] : ep.r_prior;
          // Columns, LDS addresses and masks below depend on the lane alone: left to itself the compiler computes them once
          // in front of the segment loop and carries them through the batch loop -- in scratch, the registers being taken.
          // Behind these two empty statements they are a dozen integer instructions per row instead.
          uint32_t eo = o, en = n, el = (uint32_t)lane;
          asm volatile("" : "+v"(eo), "+v"(en), "+v"(el));
          const uint32_t eg = el % (uint32_t)G;
          double wl[NF], wmax = 0.0;
#pragma unroll
          for (int j = 0; j < NF; ++j) {
            const uint32_t c = (eo + (uint32_t)j) * G + eg;
            const bool live = (uint32_t)j < en, fac = c < ep.K;
            double sv = own[j] * acc[j];                      // what went to S: a value of its own, never one factor of an fma
            asm volatile("" : "+v"(sv));
            const double sh = fmax(ep.s_prior + sv, 1e-30);
            double rt = pr + cso[live ? c : 0u];
            rt = fmax(fac ? rt : ep.rate_bias, 1e-30);
            const PsiRate ps = psi_parts_rate(sh, rt);
            double w = ps.xs * exp_neg(ps.corr) * ps.ri;
            w = (fac || (int32_t)c == ep.bias_col) ? w : ((int32_t)c == ep.junk_col ? 1.0 : 0.0);
            wl[j] = live ? w : 0.0;
            wmax = fmax(wmax, wl[j]);
          }
          wmax = group_max<64>(wmax);
          const double inv = (wmax > 0.0) ? fast_rcp(wmax) : 0.0;
          bool fl = false;
          packed_clear(pkbuf, pk, el, 64u);
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
#pragma unroll
          for (int j = 0; j < NF; ++j)
            if ((uint32_t)j < en) fl |= p59_put(pkbuf, pk, (eo + (uint32_t)j) * G + eg, wl[j] * inv);
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
          packed_copy_out(pkbuf, ep.W_out, sg.row, pk, el, 64u);
          __builtin_amdgcn_wave_barrier();                    // the next row's clear stays behind this copy
          if (__any(fl) && el == 0u) atomicOr(a.flags, 8u);
        }
      }
    }
#else
#pragma unroll
    for (int e = 0; e < E; ++e) {
      double r = acc[e];
      if (G <= 32) r += __shfl_xor(r, 32, 64);
      if (G <= 16) r += __shfl_xor(r, 16, 64);
      if (G <= 8)  r += __shfl_xor(r, 8, 64);
      if (G <= 4)  r += __shfl_xor(r, 4, 64);
      if (q == 0 && (OwnC::fixed_ld || (uint32_t)(e * G + g) < LD)) dst[(size_t)e * G] = own[e] * r;
    }
#endif
  }
}

// Three waves per SIMD (168 VGPRs).  Round 6 built and measured the other ways of spending the registers -- a fourth wave
// with the owner's factors in LDS, rows read by half their lanes (twice the nonzeros per batch, two waves) -- and an LDS pad
// that takes waves away: 3 -> 2 waves cost 7-18 %, every build that spills inside the batch loop loses far more (a scratch
// reload waits behind every gather in flight), and none reaches the one below (profiles/r06/experiments.md 2, 3;
// pass_builds_prototype.diff keeps the code).
template <template <int> class CodecT, int G, int L, int SIDE, bool FUSE>
__device__ __forceinline__ void phi_pass_packed_body(const PhiArgs &a)
{
  constexpr int LDC = G * CodecT<L>::E;
  __shared__ uint32_t pkbuf[FUSE ? 4 * G * L * 4 : 1];     // a packed row per wave (the epilogue builds W_own[row] in it)
  __shared__ double cso[FUSE ? LDC : 1];                   // the other side's column sums
  if (phi_pass_skips(a, SIDE)) return;
  const int lane = threadIdx.x & 63;
  if constexpr (FUSE) {
    for (uint32_t c = threadIdx.x; c < (uint32_t)LDC; c += blockDim.x) cso[c] = c < a.epi.K ? a.epi.colsum_oth[c] : 0.0;
    __syncthreads();
  }
  const SegRange sr = seg_range(a);
  bool underflow = false;
  phi_segments<CodecT<L>, CodecT<L>, G, L, L, FUSE>(a, sr, (const unsigned char *)a.W_own + (size_t)(lane % G) * 16,
                                                    (const unsigned char *)a.W_oth + (size_t)(lane % G) * 16, lane, underflow,
                                                    FUSE ? pkbuf + (threadIdx.x >> 6) * (G * L * 4) : nullptr, FUSE ? cso : nullptr);
  if (__any(underflow) && lane == 0) atomicOr(a.flags, 1u);
}

template <template <int> class CodecT, int G, int L, int SIDE>
__global__ __launch_bounds__(256, 3) void phi_pass_packed_kernel(PhiArgs a) { phi_pass_packed_body<CodecT, G, L, SIDE, false>(a); }

// the pass over p59 rows with the fused sweep epilogue (phi_segments, FUSE).  SIDE stays the LAST template argument: the
// benchmark's counter passes tell the two passes apart by it
template <int G, int L, int SIDE>
__global__ __launch_bounds__(256, 3) void phi_pass_fused_kernel(PhiArgs a) { phi_pass_packed_body<codec_p59, G, L, SIDE, true>(a); }

// ---------------------------------------------------------------------
// Measurement only (hpf_gather_only): a phi pass with the arithmetic taken out.  Same work
// list, same index stream, same rows, same two register sets -- the gathered pieces are folded
// with XORs into one register and nothing is written.  Its time is what the memory system
// needs for the pass's access pattern; bench.py prints it beside the pass (roofline block).
// Rows of L 16-byte pieces per lane at stride G*16: the packed layouts and plain fp64 rows with
// 16-byte loads (V = 2) alike.
// ---------------------------------------------------------------------
template <int G, int LO, int LT>
__device__ __forceinline__ void gather_only_segments(const PhiArgs &a, const SegRange &sr, const unsigned char *W_own,
                                                     const unsigned char *W_oth, int lane, uint4 &acc)
{
  constexpr int NG = 64 / G;
  constexpr uint32_t ROWO = G * LO * 16, ROWT = G * LT * 16;
  const int q = lane / G;
  auto load_own = [&](uint4 (&d)[LO], const unsigned char *base) {
#pragma unroll
    for (int t = 0; t < LO; ++t) d[t] = *reinterpret_cast<const uint4 *>(base + (size_t)t * G * 16);
  };
  auto load_row = [&](uint4 (&d)[LT], const unsigned char *base) {
#pragma unroll
    for (int t = 0; t < LT; ++t) d[t] = *reinterpret_cast<const uint4 *>(base + (size_t)t * G * 16);
  };
  auto fold = [&](const uint4 (&d)[LT]) {
#pragma unroll
    for (int t = 0; t < LT; ++t) { acc.x ^= d[t].x; acc.y ^= d[t].y; acc.z ^= d[t].z; acc.w ^= d[t].w; }
  };
  auto load_i = [&](int64_t start, uint32_t len, uint32_t o) -> uint32_t { return (o < len) ? a.idx[start + o] : 0u; };
  if (sr.s >= sr.end) return;
  Seg sgn = a.segs[sr.s];                           // the pass's stream of segments (phi_segments)
  uint32_t nxt_i = load_i(sgn.start, sgn.len, (uint32_t)lane);
  for (uint32_t s = sr.s; s < sr.end; s += sr.step) {
    const Seg sg = sgn;
    const bool more = s + sr.step < sr.end;
    if (more) sgn = a.segs[s + sr.step];
    const uint32_t len = sg.len;
    const int64_t start = sg.start;
    uint32_t cur_i = nxt_i;
    const uint32_t nb = (len + NG - 1) / NG;
    uint4 xa[LT], xb[LT];
    auto gather = [&](uint4 (&x)[LT], uint32_t b) {
      const int src = (int)((b % G) * NG) + q;
      const uint32_t in = (uint32_t)__shfl((int)cur_i, src, 64);
      load_row(x, W_oth + (size_t)in * ROWT);
    };
    auto fetch_after = [&](uint32_t c) {
      const uint32_t o = (c + 1) * 64u;
      const bool same = o < len;
      const int64_t st = same ? start : sgn.start;
      const uint32_t ln = same ? len : (more ? sgn.len : 0u), of = same ? o : 0u;
      nxt_i = load_i(st, ln, of + lane);
    };
    auto next_chunk = [&](uint32_t b) { cur_i = nxt_i; fetch_after(b / G); };
    {
      uint4 r[LO];
      load_own(r, W_own + (size_t)sg.row * ROWO); gather(xa, 0); gather(xb, 1); fetch_after(0);
#pragma unroll
      for (int t = 0; t < LO; ++t) { acc.x ^= r[t].x; acc.y ^= r[t].y; acc.z ^= r[t].z; acc.w ^= r[t].w; }
    }
    if (len == 0) continue;
    uint32_t bb = 0;
    for (; bb + 3 < nb; bb += 2) {
      fold(xa);
      __builtin_amdgcn_sched_barrier(0);
      if (((bb + 2) % G) == 0) next_chunk(bb + 2);
      gather(xa, bb + 2);
      fold(xb);
      __builtin_amdgcn_sched_barrier(0);
      gather(xb, bb + 3);
    }
    fold(xa);
    if (bb + 1 < nb) {
      const bool third = bb + 2 < nb;
      __builtin_amdgcn_sched_barrier(0);
      if (third) {
        if (((bb + 2) % G) == 0) next_chunk(bb + 2);
        gather(xa, bb + 2);
      }
      fold(xb);
      if (third) fold(xa);
    }
  }
}

template <int G, int L>
__global__ __launch_bounds__(256) void gather_only_kernel(PhiArgs a, uint32_t *sink)
{
  const int lane = threadIdx.x & 63;
  const SegRange sr = seg_range(a);
  uint4 acc = {0u, 0u, 0u, 0u};
  gather_only_segments<G, L, L>(a, sr, (const unsigned char *)a.W_own + (size_t)(lane % G) * 16,
                                (const unsigned char *)a.W_oth + (size_t)(lane % G) * 16, lane, acc);
  if ((acc.x ^ acc.y ^ acc.z ^ acc.w) == 0x9e3779b9u) sink[0] = 1u;      // keeps the loads alive
}

// long rows: S[row] = sum over its segments' partials, in segment order.
// One wave per long row; a lane owns the column pairs (2 lane, 2 lane + 1) and (128 + 2 lane, ...) -- 16-byte loads
// (round 4; ld is even and rows are 16-byte aligned) -- and the slot loop is unrolled 16-fold, so 32 independent loads
// are in flight per lane (the longest row -- thousands of slots for a blockbuster item -- sets the kernel's duration:
// it is a latency chain).  The adds of a column stay in slot order.
struct ColQuad { double a0, a1, b0, b1; };
__device__ __forceinline__ ColQuad combine_columns(const double *partial, uint32_t first_slot, uint32_t nslots, uint32_t ld, uint32_t c)
{
  const bool two = c + 128 < ld;
  const double2 *p0 = reinterpret_cast<const double2 *>(partial + (size_t)first_slot * ld + c);
  const double2 *p1 = two ? p0 + 64 : p0;
  const size_t st = ld / 2;                        // row stride in double2
  ColQuad s = {0.0, 0.0, 0.0, 0.0};
  uint32_t q = 0;
  // N slots' loads in flight, then their adds in slot order
  auto round = [&](auto n_tag) {
    constexpr int N = decltype(n_tag)::value;
    double2 v0[N], v1[N];
#pragma unroll
    for (int j = 0; j < N; ++j) { v0[j] = p0[(size_t)(q + j) * st]; v1[j] = p1[(size_t)(q + j) * st]; }
#pragma unroll
    for (int j = 0; j < N; ++j) { s.a0 += v0[j].x; s.a1 += v0[j].y; s.b0 += v1[j].x; s.b1 += v1[j].y; }
    q += N;
  };
  while (q + 16 <= nslots) round(std::integral_constant<int, 16>());
  // the last < 16 slots: a round of eight and one of four where they fit, only the last < 4 one by one (round 6: walked one
  // by one -- load, wait, add -- the last twelve of a 44-slot quarter were a chain of twelve round trips.  The same loads, the
  // same adds in the same order: the same bits.  A first attempt padded the tail to sixteen CLAMPED loads instead: the light
  // rows of two or three slots then paid for sixteen, and everything got slower -- profiles/r06/experiments.md 9)
  if (q + 8 <= nslots) round(std::integral_constant<int, 8>());
  if (q + 4 <= nslots) round(std::integral_constant<int, 4>());
  for (; q < nslots; ++q) { const double2 u = p0[(size_t)q * st], w = p1[(size_t)q * st]; s.a0 += u.x; s.a1 += u.y; s.b0 += w.x; s.b1 += w.y; }
  return s;
}

__global__ __launch_bounds__(256) void combine_partials_kernel(const LongRow *rows, uint32_t nrows,
                                                               const double *partial, double *S, uint32_t ld,
                                                               const uint32_t *flags)
{
  if (flags[0] & 6u) return;                       // the pass before it did not run (phi_pass_skips)
  const int lane = threadIdx.x & 63;
  const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
  for (uint32_t r = wave; r < nrows; r += nwaves) {
    const LongRow lr = rows[r];
    for (uint32_t c = 2 * lane; c < ld; c += 256) {
      const ColQuad s = combine_columns(partial, lr.first_slot, lr.nslots, ld, c);
      double2 *d = reinterpret_cast<double2 *>(S + (size_t)lr.row * ld + c);
      d[0] = make_double2(s.a0, s.a1);
      if (c + 128 < ld) d[64] = make_double2(s.b0, s.b1);
    }
  }
}

// The heavy rows of a TILED side carry one partial per tile they meet (C2's items 184, C4's 176): a single wave walking
// that chain is a dozen round trips in a row.  Those rows -- more than COMBINE_SPLIT partials; build_tiled_side puts them
// behind the others in the list -- get a WORKGROUP each (round 4): the four waves take a quarter of the slots each
// (contiguous quarters, cut by the slot count alone) and the four sums are added in wave order.  Which kernel a row gets,
// and hence the order of its sum, is a function of its slot count: the same bits on every run.
constexpr uint32_t COMBINE_SPLIT = 64;
__global__ __launch_bounds__(256) void combine_partials_wg_kernel(const LongRow *rows, uint32_t nrows,
                                                                  const double *partial, double *S, uint32_t ld,
                                                                  const uint32_t *flags)
{
  extern __shared__ double combine_part[];         // [4][ld]: the launch sizes it
  if (flags[0] & 6u) return;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  double *mine = combine_part + (size_t)wv * ld;
  for (uint32_t r = blockIdx.x; r < nrows; r += gridDim.x) {
    const LongRow lr = rows[r];
    const uint32_t per = (lr.nslots + 3) / 4;
    const uint32_t q0 = min(per * wv, lr.nslots), q1 = min(q0 + per, lr.nslots);
    for (uint32_t c = 2 * lane; c < ld; c += 256) {
      const ColQuad s = combine_columns(partial, lr.first_slot + q0, q1 - q0, ld, c);
      mine[c] = s.a0; mine[c + 1] = s.a1;
      if (c + 128 < ld) { mine[c + 128] = s.b0; mine[c + 129] = s.b1; }
    }
    __syncthreads();
    for (uint32_t c = threadIdx.x; c < ld; c += 256)
      S[(size_t)lr.row * ld + c] = ((combine_part[c] + combine_part[ld + c]) + combine_part[2 * ld + c]) + combine_part[3 * ld + c];
    __syncthreads();
  }
}

// ---------------------------------------------------------------------
// digamma for x > 0, in the split form the sweep needs:
//     psi(x) = log(xs) - corr ,   exp(psi(x)) = xs * exp(-corr)
// x < 10 is shifted by exactly 10 with psi(x) = psi(x+10) - P'(x)/P(x),
// P(x) = prod_{j<10}(x+j) (one reciprocal instead of ten), then the asymptotic
// series (A&S 6.3.18) through x^-14 at xs >= 10.  Stands where the reference
// calls gsl_sf_psi (gpbase.hh:260).
// Accuracy.  No absolute figure holds on the whole range (psi(1e-30) = -1e30; one ulp of psi(1e18) is 7e-15).  The
// rounding model tests/test_gpu_special.py asserts against mpmath is, with u = 2^-53,
//     |psi_dev - psi| <= u (3 log xs + 16 corr + |psi|)        (1.1e-15 at x = 10, 1.2e-14 at x = 0.3)
// and the largest error / bound measured on an MI355X (digamma_pos; 4000 log-uniform x in [1e-30, 1e18], 6000 uniform
// in [0.3, 12], both neighbours of 10, the root 1.4616..., 1e30, 1e100, 1e300) is, per band of x,
//     [1e-30, 0.3) 0.35    [0.3, 10) 0.34    [10, 1e3) 0.49    [1e3, 1e300] 0.50
// Every output is finite up to x = 1e300, where t, p and dp below are inf: the selects drop them.
// ---------------------------------------------------------------------
struct PsiParts { double xs, corr; };

__device__ __forceinline__ PsiParts psi_parts(double x)
{
  // sum_{j<10} 1/(x+j): the terms pair up, 1/(x+j) + 1/(x+9-j) = (2x+9)/(t + j(9-j))
  // with t = x(x+9), so P(x) = Q(t) = prod_{j<5}(t + c_j), c = 0, 8, 14, 18, 20, and
  // the sum is (2x+9) Q'(t)/Q(t): half the multiplies of the direct product.
  // Branch-free (round 3): 94-99 % of the shapes are below 10 (tools/shape_distribution.py),
  // so the shift is always computed and dropped by two selects when x >= 10 -- the callers'
  // column loops then stay one straight block the scheduler can interleave.
  const bool small = x < 10.0;
  const double t = x * (x + 9.0);
  double p = t, dp = 1.0;                       // j = 0: f = t
  const double cj[4] = {8.0, 14.0, 18.0, 20.0};
#pragma unroll
  for (int j = 0; j < 4; ++j) { const double f = t + cj[j]; dp = fma(dp, f, p); p *= f; }
  dp *= fma(2.0, x, 9.0);
  // x >= 10: p may overflow to inf for x > ~1e30 (dp too): the select below drops both
  const double shift = small ? dp * fast_rcp(p) : 0.0;
  x = small ? x + 10.0 : x;
  const double xi = fast_rcp(x), x2 = xi * xi;
  double s = 1.0 / 12.0;
  s = fma(-x2, s, 691.0 / 32760.0);
  s = fma(-x2, s, 1.0 / 132.0);
  s = fma(-x2, s, 1.0 / 240.0);
  s = fma(-x2, s, 1.0 / 252.0);
  s = fma(-x2, s, 1.0 / 120.0);
  s = fma(-x2, s, 1.0 / 12.0);
  PsiParts r;
  r.xs = x;
  r.corr = fma(x2, s, fma(0.5, xi, shift));
  return r;
}

// psi_parts for the row sweep, which also needs 1 / rate of the same element: the three reciprocals -- 1/P(x),
// 1/(x + 10), 1/rate -- are ONE v_rcp_f64 (+ two Newton steps) of their product and six multiplies instead of three
// reciprocals of five instructions each (C2 user sweep 0.445 -> 0.425 ms, profiles/r04/experiments.md 8).  P(x) <= 19^10,
// the shifted x <= 20 and any rate a model can take keep the product far inside the range; where x >= 10 (no shift) P is
// replaced by 1, so that an overflowed product never enters.  ri = 1 / rt to ~2 ulp (the exported E is an IEEE
// division, materialize_es_kernel; this one feeds the column sums and W).  What does enter is xs * rt, which has to stay
// finite and normal: a shape of 1e300 takes rates up to 1e8 only.
// Measured against mpmath on an MI355X (tests/test_gpu_special.py; x as for psi_parts, rt log-uniform in [1e-6, 1e12],
// the make_nonzero floor 1e-30 against x in [0.3, 100], rt <= 1 for x >= 1e100), u = 2^-53:
//     ri                          relative error <= 2.2 u                                      (asserted: 4 u)
//     W = xs exp_neg(corr) ri     against exp(psi(x)) / rt, relative error / (u (16 corr + 10)), per band of x:
//                                 [1e-30, 0.3) 0.31    [0.3, 10) 0.31    [10, 1e3) 0.39    [1e3, 1e300] 0.31   (asserted: 1)
// The shared reciprocal: r = 1 / (pp * xs * rt) with pp = P(x) (1 where x >= 10) and xs the shifted x.  Both the full sweep
// (psi_parts_rate) and the sums-only one (rate_rcp) take 1 / rt = r * pq from it: one instruction sequence, the same bits.
struct RateRcpParts { bool small; double pp, xs, pq, r, dp; };
__device__ __forceinline__ RateRcpParts rate_rcp_parts(double x, double rt)
{
  RateRcpParts q;
  q.small = x < 10.0;
  const double t = x * (x + 9.0);
  double p = t, dp = 1.0;
  const double cj[4] = {8.0, 14.0, 18.0, 20.0};
#pragma unroll
  for (int j = 0; j < 4; ++j) { const double f = t + cj[j]; dp = fma(dp, f, p); p *= f; }
  q.dp = dp * fma(2.0, x, 9.0);
  q.pp = q.small ? p : 1.0;
  q.xs = q.small ? x + 10.0 : x;
  q.pq = q.pp * q.xs;
  q.r = fast_rcp(q.pq * rt);
  return q;
}
// 1 / rt alone: what psi_parts_rate returns as ri (the dp chain is dead code here)
__device__ __forceinline__ double rate_rcp(double x, double rt)
{
  const RateRcpParts q = rate_rcp_parts(x, rt);
  return q.r * q.pq;
}

__device__ __forceinline__ PsiRate psi_parts_rate(double x, double rt)
{
  const RateRcpParts q = rate_rcp_parts(x, rt);
  const bool small = q.small;
  const double dp = q.dp, pp = q.pp, xs = q.xs, pq = q.pq, r = q.r;
  PsiRate o;
  o.ri = r * pq;
  const double ipq = r * rt;                    // 1 / (pp * xs)
  const double xi = ipq * pp, x2 = xi * xi;
  const double shift = small ? dp * (ipq * xs) : 0.0;
  double sr = 1.0 / 12.0;
  sr = fma(-x2, sr, 691.0 / 32760.0);
  sr = fma(-x2, sr, 1.0 / 132.0);
  sr = fma(-x2, sr, 1.0 / 240.0);
  sr = fma(-x2, sr, 1.0 / 252.0);
  sr = fma(-x2, sr, 1.0 / 120.0);
  sr = fma(-x2, sr, 1.0 / 12.0);
  o.xs = xs;
  o.corr = fma(x2, sr, fma(0.5, xi, shift));
  return o;
}

// a * b + c with c a wave-uniform constant held in an SGPR pair
__device__ __forceinline__ double fma_uc(double a, double b, double c)
{
  double d;
  asm("v_fma_f64 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "s"(c));
  return d;
}

// exp(-c) for c >= 0 (the sweep's exp(psi(shape)) = xs * exp(-corr)): n = rint(-c log2 e),
// r = -c - n ln2 in two pieces, a degree-13 Taylor polynomial on |r| <= ln2/2 (remainder
// 4e-18), scaled by 2^n with v_ldexp_f64 (which also delivers the gradual underflow);
// c >= 746 gives exactly 0 (c = 745 the smallest denormal).  Without the library exp's
// special-case selects for positive arguments, infinities and NaN.
// Measured against mpmath on an MI355X (tests/test_gpu_special.py; 20 000 c uniform in [0, 708], 2000 log-uniform
// down to 1e-20, 500 in [708, 746], ln2/2 and its neighbours, ln2): relative error <= 1.22 u, u = 2^-53, wherever
// the result is normal (asserted: 4 u); every denormal result equal to the correctly rounded one (asserted: within
// one denormal spacing).
__device__ __forceinline__ double exp_neg(double c)
{
  const double z = -fmin(c, 750.0);
  const double n = rint(z * 1.4426950408889634);
  double r = fma(n, -6.93147180369123816490e-01, z);      // ln2 high part (fdlibm split)
  r = fma(n, -1.90821492927058770002e-10, r);
  // Horner with the coefficient as the (wave-uniform) addend of a three-address v_fma_f64:
  // left to itself the compiler keeps the coefficients in VGPRs and spends a v_mov per step
  // on copying each into the accumulator of a two-address v_fmac
  double p = 1.0 / 6227020800.0;
  p = fma_uc(p, r, 1.0 / 479001600.0);
  p = fma_uc(p, r, 1.0 / 39916800.0);
  p = fma_uc(p, r, 1.0 / 3628800.0);
  p = fma_uc(p, r, 1.0 / 362880.0);
  p = fma_uc(p, r, 1.0 / 40320.0);
  p = fma_uc(p, r, 1.0 / 5040.0);
  p = fma_uc(p, r, 1.0 / 720.0);
  p = fma_uc(p, r, 1.0 / 120.0);
  p = fma_uc(p, r, 1.0 / 24.0);
  p = fma_uc(p, r, 1.0 / 6.0);
  p = fma(p, r, 0.5);
  p = fma(p, r, 1.0);
  p = fma(p, r, 1.0);
  return ldexp(p, (int)n);
}

__device__ __forceinline__ double digamma_pos(double x)
{
  const PsiParts r = psi_parts(x);
  return log(r.xs) - r.corr;
}

// ---------------------------------------------------------------------
// K2/K3 (+K4, K5, K7): row sweep.  One G-lane group per row, column
// g + G*t in register slot t.  For every row (reference steps B/C, D, E/F of
// hgaprec.cc:1370-1414; non-hier: 944-956, 1252-1268):
//   shape = s_prior + S            (S = raw phi sums; left raw: shape and E are
//                                   materialised on demand, materialize_es_kernel)
//   rate  = prior_rate(row) + colsum_other[k]        k < K
//           r_prior + n_other_total                   bias column
//   E = shape/rate
//   W = exp(Elog)/rowmax = [xs*exp(-corr)/rate] / rowmax   (no log in the loop;
//       Elog = psi(shape) - log(rate) itself is only exported: elog_kernel)
//   hier: xi/eta update  E_prior(row) = (s0 + K*s0) / (r0 + sum_k E[row,k])
//   block partial column sums of E  (-> colsum kernel, fixed order)
// ---------------------------------------------------------------------
struct SweepArgs {
  const double *S;          // [rows x ld] raw phi sums (read only)
  void         *W;          // [rows x ld] double, or float when w32; packed / f64 rows: [rows x pk.row_bytes]
  uint32_t      w32;
  const double *prior_E;    // [rows] E[xi] / E[eta] the rate uses (hier); updated by prior_update_kernel
  double       *prior_rate; // [rows] out: rate of the xi/eta Gamma, r0 + sum_k E[row,k]
  double        psi_prior_shape; // psi(s0 + K*s0), constant, from the host (prior_update_kernel)
  const double *colsum_oth; // [ld]   sum over the other side's rows of E
  double       *colsum_used;// [ld]   out: copy of colsum_oth -- what this rate was built from (export of *_rate.tsv,
                            //        and what a W-only repeat of this sweep reads); NULL: no copy (the repeat itself)
  double       *colsum_part;// [nblocks x ld]
  uint32_t      rows, ld, K;
  PackedRow     pk;         // rows of W in 16-byte pieces (every mode but SW_PLAIN): the phi kernel's G, E, L and the row bytes
  uint32_t     *flags;      // bit 1: a nonzero W below 2^-126 was flushed by the p59 layout; bit 2: do not run
  int32_t       bias_col;   // column holding this side's bias (-1: none)
  int32_t       junk_col;   // column holding the other side's bias (-1: none)
  double        bias_rate_add;  // n_other_total for the bias column
  double        s_prior, r_prior;
  uint32_t      hier;
  const uint32_t *row_done; // row_sums_kernel: bit r % 32 of word r / 32 = the pass before it wrote W[r] (its fused epilogue)
};

// how a sweep writes the rows of W
enum { SW_PLAIN = 0,      // double (or float, a.w32) at stride G*R: no column test
       SW_LDS_F48 = 2,    // the group builds the packed row in LDS (any G): the 48-bit layout ...
       SW_LDS_P59 = 3,    // ... and p59 where the register form below has no shape (64-lane groups of the pass)
       SW_F64 = 4,        // plain doubles into interleaved pieces (codec_f64): 8-byte stores, no staging
       SW_REG_P59 = 5 };  // p59 built in REGISTERS (round 4): the sweep's group is twice the pass's

// lane ^ GP for the power-of-two distances a sweep group spans
template <int GP>
__device__ __forceinline__ uint32_t lane_xor(uint32_t v)
{
  if (GP == 8)  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xf, 0xf, true);      // row_ror:8
  if (GP == 4)  return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x101F);                        // xor 4 (bit mode)
  if (GP == 16) return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x401F);                        // xor 16
  return (uint32_t)__shfl_xor((int)v, GP, 64);
}

// the p59 shape a register-building sweep of R slots serves: the pass gives a nonzero GP = G/2 lanes with E elements
// each, the sweep's lane (gp, h) owns the elements e = h + 2t.  E <= 10 is even (L <= 5), above that odd: R names it.
template <int R> struct p59_of_slots {
  static constexpr int E = R <= 5 ? 2 * R : 2 * R - 1;
  static constexpr int L = (59 * E + 127) / 128;
  static constexpr bool valid = R != 6 && R <= 9 && codec_p59<L>::E == E;
};

// element e of a lane's dwords D (p59): its low word, and its 27-bit field OR-ed into the stream.  Compile-time places.
template <int E, int L>
__device__ __forceinline__ void p59_place(uint32_t (&D)[4 * L], int e, uint32_t lo, uint32_t f)
{
  using C = codec_p59<L>;
  const int o = 27 * e, i = E + o / 32, sh = o % 32;
  D[C::pos(e)] = lo;
  D[C::pos(i)] |= f << sh;
  if (sh > 5) D[C::pos(i + 1)] |= f >> (32 - sh);
}

// MODE = SW_PLAIN: W is stored as double (or float, a.w32) and the row stride IS G*R (hpf_create): no column test.
// Rows in pieces (every other mode): the stride a.ld = G_phi * E may be smaller than G*R; the slots from tb on then
// also hold columns past the end of the row, whose loads and stores are masked.
// SUMS (row_sums_kernel): the sweep after a pass with the fused epilogue.  Same grid, same group -> rows mapping, same csum /
// rsum / red[] / colsum_part order; a wave whose rows ALL had their W written by the pass (a.row_done) computes only
// ri and e = sh * ri for them -- no series, no exp, no packing, no store to W -- and every other wave runs the full body.
template <int G, int R, int MODE, bool SUMS>
__device__ __forceinline__ void row_sweep_rows(const SweepArgs &a)
{
  constexpr bool PIECES = MODE != SW_PLAIN;
  constexpr bool LDSPK = MODE == SW_LDS_F48 || MODE == SW_LDS_P59;
  const uint32_t LD = PIECES ? a.ld : (uint32_t)(G * R);
  __shared__ uint32_t pkbuf[LDSPK ? 512 * R : 1];  // 256/G groups x (<= 2*G*R dwords of packed row)
  __shared__ double red[4][G * R];       // per-wave column partials
  const uint32_t fl0 = a.flags[0];
  if (fl0 & 4u) return;                  // a pass has found W unusable (phi_pass_skips): nothing runs until the host has dealt with it
  if constexpr (SUMS) {                  // the epilogue's pending bit becomes bit 1 here: no workgroup of that pass is left to skip
    if ((fl0 & 8u) && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(a.flags, 2u);
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int g = lane % G, q = lane / G;
  const uint32_t K = a.K;
  const uint32_t grp = (blockIdx.x * blockDim.x + threadIdx.x) / G;
  const uint32_t ngrp = (gridDim.x * blockDim.x) / G;
  if (a.colsum_used && blockIdx.x == 0)            // what this rate is built from, kept for the export and for a repeat
    for (uint32_t c = threadIdx.x; c < LD; c += blockDim.x) a.colsum_used[c] = a.colsum_oth[c];

  // Slot t of a lane is column g + G*t.  Slots below tb = K / G hold factor columns in
  // every lane: rate = prior(row) + column sum of the other side, E enters the sums -- no
  // column test at all (round 3).  The one or two slots from tb on mix factor columns with
  // this side's bias column (constant rate, E in no sum), the other side's bias slot
  // (W = 1 before the row-max scaling: Elog 0) and padding (W = 0); the branch between
  // the two bodies is wave-uniform.
  const uint32_t tb = K / G;
  double csum[R], cso[R];
#pragma unroll
  for (int t = 0; t < R; ++t) {
    const uint32_t c = g + G * t;
    csum[t] = 0.0;
    cso[t] = (c < K) ? a.colsum_oth[c] : 0.0;
  }
  const double rate_bias = a.r_prior + a.bias_rate_add;
  const double s_prior = a.s_prior;
  const bool hier = a.hier != 0;
  bool flushed = false;

  // software pipeline: the next row's raw sums and prior are loaded before this row is
  // worked on (the ~90 fp64 instructions per element then cover the load latency).
  // HPF_SWEEP_PIPE = 2 (tools/sweep_probe only) holds TWO rows ahead: measured in round 5, no gain (experiments.md)
#ifndef HPF_SWEEP_PIPE
#define HPF_SWEEP_PIPE 1
#endif
  double snx[R]; double prn = a.r_prior;
#if HPF_SWEEP_PIPE == 2
  double sn2[R]; double pr2 = a.r_prior;
#endif
  // SUMS: the done bits of the wave's 64 / G consecutive rows (one word: the run is aligned to its own length), fetched with the row
  uint32_t dnn = 0u;
  auto fetch_row = [&](uint32_t r_, double (&dst)[R], double &pdst) {
    if (r_ < a.rows) {
#pragma unroll
      for (int t = 0; t < R; ++t) dst[t] = (!PIECES || (uint32_t)(g + G * t) < LD) ? a.S[(size_t)r_ * LD + g + G * t] : 0.0;
      if (hier) pdst = a.prior_E[r_];
      if constexpr (SUMS) dnn = a.row_done[(r_ - (uint32_t)q) >> 5];
    }
  };
  fetch_row(grp, snx, prn);
#if HPF_SWEEP_PIPE == 2
  fetch_row(grp + ngrp, sn2, pr2);
#endif
  for (uint32_t row = grp; row < a.rows; row += ngrp) {
    const size_t base = (size_t)row * LD;
    double w[R];
#pragma unroll
    for (int t = 0; t < R; ++t) w[t] = snx[t];
    const double pr = prn;
    const uint32_t dn = dnn;
#if HPF_SWEEP_PIPE == 2
#pragma unroll
    for (int t = 0; t < R; ++t) snx[t] = sn2[t];
    prn = pr2;
    fetch_row(row + 2 * ngrp, sn2, pr2);
#else
    fetch_row(row + ngrp, snx, prn);
#endif
    if constexpr (SUMS) {
      constexpr uint32_t NR = 64 / G;                          // rows of a wave
      const uint32_t r0 = row - (uint32_t)q, left = a.rows - r0;
      const uint32_t need = (1u << (left < NR ? left : NR)) - 1u;
      if (__builtin_amdgcn_readfirstlane((int)(((dn >> (r0 & 31u)) & need) == need))) {
        double rs = 0.0;
#pragma unroll
        for (int t = 0; t < R; ++t) {
          const bool mixed = (uint32_t)t >= tb;
          const uint32_t c = g + G * t;
          const double sh = fmax(s_prior + w[t], 1e-30);
          double rt = pr + cso[t];
          if (mixed) { asm volatile(""); rt = (c < K) ? rt : rate_bias; }
          rt = fmax(rt, 1e-30);
          const double ri = rate_rcp(sh, rt);
          double e = sh * ri;
          if (mixed) { asm volatile(""); e = (c < K) ? e : 0.0; }
          rs += e; csum[t] += e;
        }
        rs = group_sum<G>(rs);
        if (hier && g == 0) a.prior_rate[row] = a.r_prior + rs;
        continue;
      }
    }
    double wmax = 0.0, rsum = 0.0;
#pragma unroll
    for (int t = 0; t < R; ++t) {
      const bool mixed = (uint32_t)t >= tb;         // wave-uniform
      const uint32_t c = g + G * t;
      // GPBase::make_nonzero (gpbase.hh:27-44: "if (!(av > .0)) a = 1e-30") as one v_max_f64:
      // the same for zero, negative and NaN; a value in (0, 1e-30) -- which a shape
      // s_prior + sum >= 0.3 or a rate prior + column sum cannot take -- would become 1e-30
      const double sh = fmax(s_prior + w[t], 1e-30);
      double rt = pr + cso[t];
      // (the empty asm keeps these wave-uniform fix-ups real branches: if-converted, their
      // selects would run in every slot)
      if (mixed) { asm volatile(""); rt = (c < K) ? rt : rate_bias; }
      rt = fmax(rt, 1e-30);
      const PsiRate ps = psi_parts_rate(sh, rt);    // psi(shape) in its split form and 1 / rate, one reciprocal for both
      const double ri = ps.ri;                      // ~2 ulp; the exported E is an IEEE sh / rt
      double e = sh * ri;                           //   (materialize_es_kernel); this one feeds sums
      if (mixed) { asm volatile(""); e = (c < K) ? e : 0.0; }
      rsum += e; csum[t] += e;
      double wl = ps.xs * exp_neg(ps.corr) * ri;    // exp(psi(shape) - log(rate))
      if (mixed) { asm volatile(""); wl = (c < K || (int32_t)c == a.bias_col) ? wl : ((int32_t)c == a.junk_col ? 1.0 : 0.0); }
      w[t] = wl;
      wmax = fmax(wmax, wl);
    }
    wmax = group_max<G>(wmax);
    rsum = group_sum<G>(rsum);
    const double inv = (wmax > 0.0) ? fast_rcp(wmax) : 0.0;
    if constexpr (MODE == SW_REG_P59) {
      // The pass gives a nonzero GP = G/2 lanes; packed lane gp holds the elements e = 0..E-1 of the columns
      // e*GP + gp.  This sweep's lane g = gp + GP*h owns the slots t, i.e. the columns g + G*t = (h + 2t)*GP + gp:
      // the elements e = h + 2t of packed lane gp -- the even ones (h = 0) or the odd ones (h = 1).  The two lanes
      // swap their (low word, 27-bit field) pairs, each then holds all E elements and builds the lane's 4L dwords
      // with compile-time shifts; h = 0 stores the even 16-byte pieces, h = 1 the odd ones.  No LDS, no atomics.
      using P = p59_of_slots<R>;
      if constexpr (P::valid) {
        constexpr int E = P::E, L = P::L, GP = G / 2;
        const int gp = g % GP;
        const bool h = g >= GP;
        uint32_t D[4 * L];
#pragma unroll
        for (int i = 0; i < 4 * L; ++i) D[i] = 0u;
#pragma unroll
        for (int t = 0; t < R; ++t) {
          const bool pair = 2 * t + 1 < E;                // element 2t + 1 exists (E odd: the last slot of h = 1 is past the row)
          const double v = w[t] * inv;
          const bool live = pair || !h;
          const P59Words pw = p59_words(v, live);         // representable: 2^-126 <= w < 2
          flushed |= pw.flushed;
          const uint32_t of = pw.f, ol = pw.lo;
          const uint32_t pf = lane_xor<GP>(of), pl = lane_xor<GP>(ol);
          p59_place<E, L>(D, 2 * t, h ? pl : ol, h ? pf : of);
          if (pair) p59_place<E, L>(D, 2 * t + 1, h ? ol : pl, h ? of : pf);
        }
        // h = 0 stores the even pieces, h = 1 the odd ones.  The choice is ARITHMETIC (v_bfi_b32 under a lane mask): written
        // as a select between two elements of D the compiler turns it into a run-time index into the register array --
        // a chain of 24 compares per word
        const uint32_t hm = h ? 0xffffffffu : 0u;
        auto pick = [&](uint32_t odd, uint32_t even) -> uint32_t { return (odd & hm) | (even & ~hm); };
        uint4 *dst = reinterpret_cast<uint4 *>((unsigned char *)a.W + (size_t)row * (size_t)(GP * L * 16)) + gp + (h ? GP : 0);
#pragma unroll
        for (int j = 0; 2 * j < L; ++j) {
          const int p0 = 2 * j, p1 = 2 * j + 1;
          if (p1 < L) {
            dst[(size_t)p0 * GP] = make_uint4(pick(D[4 * p1], D[4 * p0]), pick(D[4 * p1 + 1], D[4 * p0 + 1]),
                                              pick(D[4 * p1 + 2], D[4 * p0 + 2]), pick(D[4 * p1 + 3], D[4 * p0 + 3]));
          } else if (!h) {
            dst[(size_t)p0 * GP] = make_uint4(D[4 * p0], D[4 * p0 + 1], D[4 * p0 + 2], D[4 * p0 + 3]);
          }
        }
      }
    } else if constexpr (LDSPK) {
      uint32_t *buf = pkbuf + (threadIdx.x / G) * (2 * G * R);
      packed_clear(buf, a.pk, (uint32_t)g, (uint32_t)G);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // the group's lanes exchange through LDS: clear, put, copy out
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int t = 0; t < R; ++t)
        if ((uint32_t)(g + G * t) < LD) {
          if (MODE == SW_LDS_P59) flushed |= p59_put(buf, a.pk, g + G * t, w[t] * inv);
          else f48_put(buf, a.pk, g + G * t, w[t] * inv);
        }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      packed_copy_out(buf, a.W, row, a.pk, (uint32_t)g, (uint32_t)G);
      __builtin_amdgcn_wave_barrier();                             // the next row's clear stays behind this copy
    } else if constexpr (MODE == SW_F64) {
#pragma unroll
      for (int t = 0; t < R; ++t)
        if ((uint32_t)(g + G * t) < a.pk.G * a.pk.E) f64_put(a.W, row, a.pk, g + G * t, (uint32_t)(g + G * t) < LD ? w[t] * inv : 0.0);
    } else if (a.w32) {
#pragma unroll
      for (int t = 0; t < R; ++t) ((float *)a.W)[base + g + G * t] = (float)(w[t] * inv);
    } else {
#pragma unroll
      for (int t = 0; t < R; ++t) ((double *)a.W)[base + g + G * t] = w[t] * inv;
    }
    // thetarate/betarate (gpbase.hh:877-889,912-925 via hgaprec.cc:1398-1414): the rate goes
    // out here; shape / rate and psi(shape) - log(rate) -- an IEEE division and a log that
    // only one lane in G would work on -- are prior_update_kernel's, over all rows at once
    if (hier && g == 0) a.prior_rate[row] = a.r_prior + rsum;
  }
  if (flushed) atomicOr(a.flags, 2u);

  // block partial column sums, fixed order: groups of a wave, then waves
#pragma unroll
  for (int t = 0; t < R; ++t) {
    double v = csum[t];
    if (G <= 32) v += __shfl_xor(v, 32, 64);
    if (G <= 16) v += __shfl_xor(v, 16, 64);
    if (G <= 8)  v += __shfl_xor(v, 8, 64);
    if (G <= 4)  v += __shfl_xor(v, 4, 64);
    if (q == 0) red[wv][g + G * t] = v;
  }
  __syncthreads();
  for (uint32_t c = threadIdx.x; c < LD; c += blockDim.x)
    a.colsum_part[(size_t)blockIdx.x * LD + c] = (c < K) ? red[0][c] + red[1][c] + red[2][c] + red[3][c] : 0.0;
}

template <int G, int R, int MODE>
__global__ __launch_bounds__(256) void row_sweep_kernel(SweepArgs a) { row_sweep_rows<G, R, MODE, false>(a); }

template <int G, int R, int MODE>
__global__ __launch_bounds__(256) void row_sums_kernel(SweepArgs a) { row_sweep_rows<G, R, MODE, true>(a); }

// xi / eta after a sweep (hier): remember what the rate just used (export, ELBO), then
//   E = (s0 + K s0) / rate ,  Elog = psi(s0 + K s0) - log(rate)        gpbase.hh:877-925
// with the rate the sweep left in prior_rate.  One thread per row.
__global__ __launch_bounds__(256) void prior_update_kernel(double *prior_E, double *prior_used,
                                                           const double *prior_rate, double *prior_elog,
                                                           double *prior_elog_used, uint32_t rows,
                                                           double prior_shape, double psi_prior_shape, const uint32_t *flags)
{
  if (flags[0] & 4u) return;
  for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += gridDim.x * blockDim.x) {
    const double rt = prior_rate[r];
    prior_used[r] = prior_E[r];
    prior_elog_used[r] = prior_elog[r];
    prior_E[r] = prior_shape / rt;
    prior_elog[r] = psi_prior_shape - log(rt);
  }
}

// shape = s_prior + S_raw (in place) and E = shape / rate for export, held-out
// likelihood, ranking and ELBO: the hot loop itself only needs W and the
// column sums, so the sweep does not spend 16 B/element of writes on them.
// (The sweep's own E, which only feeds the column / row sums, is sh * rcp(rate): <= 1 ulp apart.)
__global__ void materialize_es_kernel(double *S, double *E, const double *prior_used,
                                      const double *colsum_used, uint32_t rows, uint32_t ld, uint32_t K,
                                      int32_t bias_col, double bias_rate_add, double s_prior,
                                      double r_prior, uint32_t hier)
{
  const size_t n = (size_t)rows * ld;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n;
       e += (size_t)gridDim.x * blockDim.x) {
    const uint32_t row = (uint32_t)(e / ld), c = (uint32_t)(e % ld);
    double sh = 0.0, ev = 0.0;
    if (c < K || (int32_t)c == bias_col) {
      sh = s_prior + S[e];
      double rt = (c < K) ? (hier ? prior_used[row] : r_prior) + colsum_used[c] : r_prior + bias_rate_add;
      sh = (sh > 0.0) ? sh : 1e-30;
      rt = (rt > 0.0) ? rt : 1e-30;
      ev = sh / rt;
    }
    S[e] = sh;
    E[e] = ev;
  }
}

// Elog = psi(shape) - log(rate), materialised on demand for export
// (gpbase.hh:248-262): rate rebuilt from what the last sweep used
__global__ void elog_kernel(const double *S, const double *prior_used, const double *colsum_used,
                            double *L, uint32_t rows, uint32_t ld, uint32_t K, int32_t bias_col,
                            double bias_rate_add, double r_prior, uint32_t hier)
{
  const size_t n = (size_t)rows * ld;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n;
       e += (size_t)gridDim.x * blockDim.x) {
    const uint32_t row = (uint32_t)(e / ld), c = (uint32_t)(e % ld);
    double l = 0.0;
    if (c < K || (int32_t)c == bias_col) {
      const double sh = S[e];
      double rt = (c < K) ? (hier ? prior_used[row] : r_prior) + colsum_used[c] : r_prior + bias_rate_add;
      rt = (rt > 0.0) ? rt : 1e-30;
      l = digamma_pos(sh > 0.0 ? sh : 1e-30) - log(rt);
    }
    L[e] = l;
  }
}

// out[c] = sum over block partials: one 256-thread block per column, each
// thread sums a fixed strided subset in order, then a fixed-shape LDS tree --
// the order depends only on nblocks, so the result is bit-reproducible
__global__ __launch_bounds__(256) void colsum_finalize_kernel(const double *part, uint32_t nblocks,
                                                              uint32_t ld, double *out, const uint32_t *flags)
{
  __shared__ double red[256];
  if (flags[0] & 4u) return;
  const uint32_t c = blockIdx.x;
  double s = 0.0;
  for (uint32_t b = threadIdx.x; b < nblocks; b += 256) s += part[(size_t)b * ld + c];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[c] = red[0];
}

// plain column sums of E over rows (used once after hpf_set_state):
// block partials in the same layout as the sweep's
__global__ __launch_bounds__(256) void colsum_partial_kernel(const double *E,
    uint32_t rows, uint32_t ld, uint32_t K, double *part)
{
  // thread c accumulates column c over this block's slice of rows
  const uint32_t per = (rows + gridDim.x - 1) / gridDim.x;
  const uint32_t r0 = blockIdx.x * per;
  const uint32_t r1 = (r0 + per < rows) ? r0 + per : rows;
  for (uint32_t c = threadIdx.x; c < ld; c += blockDim.x) {
    double s = 0.0;
    if (c < K)
      for (uint32_t r = r0; r < r1; ++r) s += E[(size_t)r * ld + c];
    part[(size_t)blockIdx.x * ld + c] = s;
  }
}

// W = exp(L - rowmax(L)) over the live columns (after hpf_set_state(ELOG))
// wmode: 0 double, 1 float, WL_F48 / WL_P59 the packed layouts (built per row in LDS), WL_F64 plain doubles in
// interleaved pieces
__global__ __launch_bounds__(256) void derive_w_kernel(const double *L, void *W, uint32_t wmode, uint32_t rows,
                                uint32_t ld, uint32_t K, int32_t bias_col,
                                int32_t junk_col, PackedRow pk, uint32_t *flags)
{
  __shared__ uint32_t pkbuf[4][2304];            // a packed row per wave (<= 64 lanes x 8 pieces x 16 B + slack)
  const int lane = threadIdx.x & 63;
  const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
  uint32_t *buf = pkbuf[threadIdx.x >> 6];
  const bool packed = wmode == WL_P59 || wmode == WL_F48;
  const uint32_t cols = (wmode == WL_F64) ? pk.G * pk.E : ld;          // f64 rows: the padding slots past ld hold zeros
  bool flushed = false;
  for (uint32_t row = wave; row < rows; row += nwaves) {
    double m = -1.0e308;
    for (uint32_t c = lane; c < ld; c += 64) {
      const bool live = c < K || (int32_t)c == bias_col || (int32_t)c == junk_col;
      if (live) m = fmax(m, L[(size_t)row * ld + c]);
    }
    m = group_max<64>(m);
    if (packed) {
      packed_clear(buf, pk, (uint32_t)lane, 64u);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
    for (uint32_t c = lane; c < cols; c += 64) {
      const bool live = c < K || (int32_t)c == bias_col || (int32_t)c == junk_col;
      const double wv = (live && c < ld) ? exp(L[(size_t)row * ld + c] - m) : 0.0;
      if (wmode == WL_P59) flushed |= p59_put(buf, pk, c, wv);
      else if (wmode == WL_F48) f48_put(buf, pk, c, wv);
      else if (wmode == WL_F64) f64_put(W, row, pk, c, wv);
      else if (wmode == 1) ((float *)W)[(size_t)row * ld + c] = (float)wv;
      else ((double *)W)[(size_t)row * ld + c] = wv;
    }
    if (packed) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      packed_copy_out(buf, W, row, pk, (uint32_t)lane, 64u);
      __builtin_amdgcn_wave_barrier();
    }
  }
  if (flushed) atomicOr(flags, 2u);
}

// ---------------------------------------------------------------------
// Fold-in (hpf_fold_in; HGAPRec::test(), hgaprec.cc:2257-2346): every user-side CAVI iteration of a NEW user against a
// frozen item side, in one launch.  One wave owns one user from the prior to its stop; lane l holds the columns
// l + 64 t, t < R, of the user's row.  Between iterations the user lives in registers -- own (the W form of theta and of
// the bias: exp(Elog) over the row maximum), ev (E), sh (shape) and the scalars of xi -- and goes to memory once, when it
// stops.  The item rows are gathered from a plain fp64 copy Wb = exp(Elog beta - row max) of stride ldf (fold_derive_w_kernel:
// not the handle's packed W); a user whose rows fit the wave's slice of LDS (len <= rows_held <= 64) gathers them in the
// first iteration only and reads them back from LDS afterwards -- the same doubles, so both paths give the same bits.  A
// lane reads from LDS only what it stored itself: no barrier.
// Per nonzero, in CSR order (two at a time for the latency of the 64-lane sum; the accumulation stays in CSR order):
//   ssum = sum_c own_c x_c ,  acc_c += x_c * yy / ssum ;  at the end of the row S_c = own_c * acc_c      (phi_batch's form)
// then steps B, D-user and E of the iteration on the row in registers (row_sweep_kernel's arithmetic, E by an IEEE division).
// hpf_fold_in_items is the same with the sides exchanged: the rows are the new ITEMS in item-major order, the gathered copy
// is built from the user side, and an item with many ratings goes to fold_in_long_kernel below.
// ---------------------------------------------------------------------
struct FoldArgs {
  const int64_t  *rowptr;   // [n + 1] CSR of the users (hpf_fold_in_items: the column pointers of the item-major view)
  const uint32_t *idx;      // item (user) of each nonzero
  const uint8_t  *val;      // rating (NULL: all ones)
  const double   *Wb;       // [n_items x ldf] exp(Elog - row max) of the item side, bias and junk columns included
  const double   *csum;     // [>= K] c_k = sum_i E[beta_ik]
  double *S, *E, *L;        // [n x ld] out: shape, E, Elog of the user side
  double *rate;             // out: hier [n x K], else the K-vector (written by user 0's wave)
  double *xi_shape, *xi_rate, *xi_E, *xi_elog, *xi_used, *xi_elog_used;   // [n] out (hier)
  uint32_t *iters_out;      // [n] out, may be NULL
  uint32_t *flags;          // bit 0: a softmax denominator underflowed
  uint32_t n, ld, ldf, K, rows_held, slice, n_iters, hier;
  uint32_t len_max;         // fold_in_kernel skips the rows with more nonzeros: fold_in_long_kernel's (0xffffffff: none)
  const uint32_t *long_rows; uint32_t n_long;   // fold_in_long_kernel: its rows
  int32_t  bias_col, junk_col;
  double   rate_bias;       // r_prior + n_items (the owner is a user) / + n_users_total (an item)
  double   s_prior, r_prior, tol;
  double   xi_shape_v, psi_xi_shape;    // s0 + K s0 and its digamma
  double   elog_prior;      // psi(s0) - log(r0): Elog of every object at the prior
};

template <int R>
__device__ __forceinline__ double fold_dot(const double (&x)[R], const double (&own)[R])
{
  double s[2] = {0.0, 0.0};
#pragma unroll
  for (int e = 0; e < R; ++e) s[e & 1] = (e < 2) ? own[e] * x[e] : fma(own[e], x[e], s[e & 1]);
  return group_sum<64>((R > 1) ? s[0] + s[1] : s[0]);
}
template <int R>
__device__ __forceinline__ void fold_add(const double (&x)[R], double (&acc)[R], double ssum, double yy, bool &underflow)
{
  const bool ok = ssum > 0.0;
  underflow |= !ok;
  const double scale = ok ? yy * fast_rcp(ssum) : 0.0;
#pragma unroll
  for (int t = 0; t < R; ++t) acc[t] = fma(x[t], scale, acc[t]);
}

// The state of one row between iterations, a copy per lane: its columns l + 64 t (own: the W form, ev: E, sh: shape) and
// the scalars of xi / eta.  fold_in_kernel keeps one per wave, fold_in_long_kernel the same one in every wave of a workgroup.
template <int R>
struct FoldRow {
  double own[R], ev[R], sh[R], acc[R];
  double pr, pr_used, pel, pel_used, xrate;              // E[xi] of the previous step (the constant r_prior without hier) ...
  double dmax, emax;                                     // max_k |E - E_before| and max_k E of the last update
};

// shape sums acc -> shape, E and the W form of the row; rate = prk + use * c_k (the bias column: rb).  Returns
// sum_k E (k < K) and leaves max_k |E - E_before| and max_k E in dmax / emax
template <int R>
__device__ __forceinline__ double fold_update(const FoldArgs &a, int lane, FoldRow<R> &r, double prk, double use, double rb)
{
  const uint32_t K = a.K;
  const double s0 = a.s_prior;
  double wl[R], wmax = 0.0, rsum = 0.0;
  double dmax = 0.0, emax = 0.0;
#pragma unroll
  for (int t = 0; t < R; ++t) {
    const uint32_t c = (uint32_t)lane + 64u * t;
    const bool fk = c < K, fb = (int32_t)c == a.bias_col;
    const double cs = fk ? a.csum[c] : 0.0;
    const double shp = fmax(s0 + r.own[t] * r.acc[t], 1e-30);        // GPBase::make_nonzero, as the sweep has it
    const double rt = fmax(fk ? fma(cs, use, prk) : rb, 1e-30);
    const PsiRate ps = psi_parts_rate(shp, rt);
    const double e = (fk || fb) ? shp / rt : 0.0;
    const double ek = fk ? e : 0.0;
    dmax = fmax(dmax, fk ? fabs(e - r.ev[t]) : 0.0);
    emax = fmax(emax, ek);
    rsum += ek;
    const double w = ps.xs * exp_neg(ps.corr) * ps.ri;               // exp(psi(shape) - log(rate))
    wl[t] = (fk || fb) ? w : ((int32_t)c == a.junk_col ? 1.0 : 0.0);
    wmax = fmax(wmax, wl[t]);
    r.sh[t] = shp; r.ev[t] = e;
  }
  wmax = group_max<64>(wmax);
  r.dmax = group_max<64>(dmax);
  r.emax = group_max<64>(emax);
  const double inv = (wmax > 0.0) ? fast_rcp(wmax) : 0.0;
#pragma unroll
  for (int t = 0; t < R; ++t) r.own[t] = wl[t] * inv;
  return group_sum<64>(rsum);
}

// the prior: every Gamma object at shape s_prior, rate r_prior
template <int R>
__device__ __forceinline__ void fold_start(const FoldArgs &a, int lane, FoldRow<R> &r)
{
  const double r0 = a.r_prior;
  r.pr = a.hier ? a.s_prior / r0 : r0;
  r.pr_used = r0; r.pel = a.elog_prior; r.pel_used = a.elog_prior; r.xrate = r0;
#pragma unroll
  for (int t = 0; t < R; ++t) { r.own[t] = 0.0; r.acc[t] = 0.0; r.ev[t] = 0.0; }
  (void)fold_update<R>(a, lane, r, r0, 0.0, r0);
}

// the nonzeros [begin, end) of the row that starts at `start` (begin a multiple of 64), in order, two in flight, into r.acc.
// held: the row fits the wave's slice `rows` of LDS -- gathered and stored there when !from_lds, read back from there
// otherwise (cur_i / cur_y then still hold the row's indices and ratings)
template <int R>
__device__ __forceinline__ void fold_walk(const FoldArgs &a, int lane, FoldRow<R> &r, int64_t start, uint32_t begin, uint32_t end,
                                          bool held, bool from_lds, double *rows, uint32_t &cur_i, float &cur_y, bool &underflow)
{
  const uint32_t LDF = a.ldf;
  auto get = [&](double (&x)[R], uint32_t j, uint32_t jrow) {
    if (from_lds) {
#pragma unroll
      for (int t = 0; t < R; ++t) { const uint32_t c = (uint32_t)lane + 64u * t; x[t] = (c < LDF) ? rows[(size_t)jrow * LDF + c] : 0.0; }
    } else {
      const uint32_t in = (uint32_t)__builtin_amdgcn_readlane((int)cur_i, (int)j);
      const double *p = a.Wb + (size_t)in * LDF;
#pragma unroll
      for (int t = 0; t < R; ++t) { const uint32_t c = (uint32_t)lane + 64u * t; x[t] = (c < LDF) ? p[c] : 0.0; }
      if (held) {
#pragma unroll
        for (int t = 0; t < R; ++t) { const uint32_t c = (uint32_t)lane + 64u * t; if (c < LDF) rows[(size_t)jrow * LDF + c] = x[t]; }
      }
    }
  };
  auto rating = [&](uint32_t j) -> double { return (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(cur_y), (int)j)); };
  for (uint32_t base = begin; base < end; base += 64u) {
    const uint32_t cnt = (end - base < 64u) ? end - base : 64u;
    if (!from_lds) {
      // the factor is yy = (y > 1 ? y : 1), hgaprec.cc:1355-1356, as in the phi pass
      cur_i = ((uint32_t)lane < cnt) ? a.idx[start + base + lane] : 0u;
      cur_y = 1.0f;
      if (a.val && (uint32_t)lane < cnt) { const uint32_t y = a.val[start + base + lane]; cur_y = (y > 1u) ? (float)y : 1.0f; }
    }
    uint32_t j = 0;
    double xa[R], xb[R];
    for (; j + 1 < cnt; j += 2) {
      get(xa, j, base + j);
      get(xb, j + 1, base + j + 1);
      const double sa = fold_dot<R>(xa, r.own), sb = fold_dot<R>(xb, r.own);
      fold_add<R>(xa, r.acc, sa, rating(j), underflow);
      fold_add<R>(xb, r.acc, sb, rating(j + 1), underflow);
    }
    if (j < cnt) {
      get(xa, j, base + j);
      fold_add<R>(xa, r.acc, fold_dot<R>(xa, r.own), rating(j), underflow);
    }
  }
}

// B, D-owner: shape and rate of the row and of its bias from the sums in r.acc; E: xi / eta from the new row
template <int R>
__device__ __forceinline__ void fold_step(const FoldArgs &a, int lane, FoldRow<R> &r)
{
  r.pr_used = r.pr; r.pel_used = r.pel;
  const double rsum = fold_update<R>(a, lane, r, r.pr, 1.0, a.rate_bias);
  if (a.hier) {
    r.xrate = a.r_prior + rsum;
    r.pr = a.xi_shape_v / r.xrate;
    r.pel = a.psi_xi_shape - log(r.xrate);
  }
}

// row u has stopped after `it` iterations: its state goes out, once (one wave)
template <int R>
__device__ __forceinline__ void fold_store(const FoldArgs &a, int lane, const FoldRow<R> &r, uint32_t u, uint32_t it)
{
  const uint32_t K = a.K;
  const bool hier = a.hier != 0;
  const size_t ro = (size_t)u * a.ld;
#pragma unroll
  for (int t = 0; t < R; ++t) {
    const uint32_t c = (uint32_t)lane + 64u * t;
    if (c >= a.ld) continue;
    const bool fk = c < K, fb = (int32_t)c == a.bias_col;
    const double rt = fmax(fk ? r.pr_used + a.csum[c] : a.rate_bias, 1e-30);
    a.S[ro + c] = (fk || fb) ? r.sh[t] : 0.0;
    a.E[ro + c] = r.ev[t];
    a.L[ro + c] = (fk || fb) ? digamma_pos(r.sh[t]) - log(rt) : 0.0;
    if (fk && hier) a.rate[(size_t)u * K + c] = rt;
    if (fk && !hier && u == 0) a.rate[c] = rt;
  }
  if (lane == 0) {
    if (hier) {
      a.xi_shape[u] = a.xi_shape_v; a.xi_rate[u] = r.xrate; a.xi_E[u] = r.pr; a.xi_elog[u] = r.pel;
      a.xi_used[u] = r.pr_used; a.xi_elog_used[u] = r.pel_used;
    }
    if (a.iters_out) a.iters_out[u] = it;
  }
}

template <int R>
__global__ __launch_bounds__(256) void fold_in_kernel(FoldArgs a)
{
  extern __shared__ double fold_rows[];                  // four slices of a.slice doubles, one per wave
  const int lane = threadIdx.x & 63;
  double *rows = fold_rows + (size_t)(threadIdx.x >> 6) * a.slice;
  bool underflow = false;
  const uint32_t w0 = __builtin_amdgcn_readfirstlane((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  const uint32_t nw = (gridDim.x * blockDim.x) >> 6;

  for (uint32_t u = w0; u < a.n; u += nw) {
    const int64_t start = a.rowptr[u];
    const uint32_t len = (uint32_t)(a.rowptr[u + 1] - start);
    if (len > a.len_max) continue;                       // fold_in_long_kernel's (hpf_fold_in_items)
    const bool held = len <= a.rows_held;
    FoldRow<R> r;
    uint32_t cur_i = 0; float cur_y = 0.0f;
    fold_start<R>(a, lane, r);

    uint32_t it = 0;
    for (;;) {
#pragma unroll
      for (int t = 0; t < R; ++t) r.acc[t] = 0.0;
      fold_walk<R>(a, lane, r, start, 0u, len, held, held && it > 0 /* wave-uniform */, rows, cur_i, cur_y, underflow);
      fold_step<R>(a, lane, r);
      ++it;
      if (it >= a.n_iters) break;
      if (a.tol > 0.0 && it >= 2 && r.dmax <= a.tol * r.emax) break;
    }
    fold_store<R>(a, lane, r, u, it);
  }
  if (__any(underflow) && lane == 0) atomicOr(a.flags, 1u);
}

// Long rows (hpf_fold_in_items): one WORKGROUP of WAVES waves owns row long_rows[i] from the prior to
// its stop.  Every wave keeps the same copy of the row's state (FoldRow).  Per iteration wave w walks its part of the
// row's nonzeros (hpf_plan::fold_part: contiguous, whole 64-blocks, a function of len and WAVES only) with fold_in_kernel's
// loop, leaves its sums in its LDS slice, and after a barrier every wave adds the WAVES slices in wave order -- a fixed
// order, no atomics -- and runs the same update on the same sums.  Whether the row stops is decided ONCE, by wave 0, and
// read by all from LDS: two barriers per iteration, each reached by every wave (a wave with an empty part adds +0.0), so
// no wave can leave the loop alone.  Long rows never fit LDS: every iteration gathers from Wb.
template <int R, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void fold_in_long_kernel(FoldArgs a)
{
  extern __shared__ double fold_part[];                  // [WAVES][R][64] partial sums, then the stop word
  const int lane = threadIdx.x & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  volatile uint32_t *stop = (volatile uint32_t *)(fold_part + (size_t)WAVES * R * 64);
  bool underflow = false;

  for (uint32_t li = blockIdx.x; li < a.n_long; li += gridDim.x) {       // workgroup-uniform
    const uint32_t u = a.long_rows[li];
    const int64_t start = a.rowptr[u];
    const uint32_t len = (uint32_t)(a.rowptr[u + 1] - start);
    const hpf_plan::FoldPart part = hpf_plan::fold_part(len, (uint32_t)WAVES, wave);
    FoldRow<R> r;
    uint32_t cur_i = 0; float cur_y = 0.0f;
    fold_start<R>(a, lane, r);

    uint32_t it = 0;
    for (;;) {
#pragma unroll
      for (int t = 0; t < R; ++t) r.acc[t] = 0.0;
      fold_walk<R>(a, lane, r, start, part.begin, part.end, false, false, nullptr, cur_i, cur_y, underflow);
#pragma unroll
      for (int t = 0; t < R; ++t) fold_part[((size_t)wave * R + t) * 64 + lane] = r.acc[t];
      __syncthreads();
#pragma unroll
      for (int t = 0; t < R; ++t) {
        double s = fold_part[(size_t)t * 64 + lane];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) s += fold_part[((size_t)w * R + t) * 64 + lane];
        r.acc[t] = s;
      }
      fold_step<R>(a, lane, r);
      ++it;
      if (wave == 0 && lane == 0) *stop = (it >= a.n_iters || (a.tol > 0.0 && it >= 2 && r.dmax <= a.tol * r.emax)) ? 1u : 0u;
      __syncthreads();                                   // ... which also ends the reads of this iteration's partial sums
      if (__builtin_amdgcn_readfirstlane(*stop)) break;  // the next write of the word lies behind the next barrier
    }
    if (wave == 0) fold_store<R>(a, lane, r, u, it);
  }
  if (__any(underflow) && lane == 0) atomicOr(a.flags, 1u);
}

// the rows fold_in_long_kernel owns: those with at least long_min nonzeros, in any order (a row's result does not depend
// on its place in the list)
__global__ void fold_long_list_kernel(const int64_t *rowptr, uint32_t n, uint32_t long_min, uint32_t *list, uint32_t *count)
{
  for (uint32_t u = blockIdx.x * blockDim.x + threadIdx.x; u < n; u += gridDim.x * blockDim.x)
    if ((uint64_t)(rowptr[u + 1] - rowptr[u]) >= long_min) list[atomicAdd(count, 1u)] = u;
}

// the item rows the fold-in kernel gathers: Wb = exp(L - rowmax(L)) over the live columns as plain doubles at stride
// ldf (zeros beyond), from the handle's Elog at stride ld.  A wave per row, like derive_w_kernel.
__global__ __launch_bounds__(256) void fold_derive_w_kernel(const double *L, double *Wb, uint32_t rows, uint32_t ld, uint32_t ldf,
                                                            uint32_t K, int32_t bias_col, int32_t junk_col)
{
  const int lane = threadIdx.x & 63;
  const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
  for (uint32_t row = wave; row < rows; row += nwaves) {
    double m = -1.0e308;
    for (uint32_t c = lane; c < ld; c += 64) {
      const bool live = c < K || (int32_t)c == bias_col || (int32_t)c == junk_col;
      if (live) m = fmax(m, L[(size_t)row * ld + c]);
    }
    m = group_max<64>(m);
    for (uint32_t c = lane; c < ldf; c += 64) {
      const bool live = c < K || (int32_t)c == bias_col || (int32_t)c == junk_col;
      Wb[(size_t)row * ldf + c] = (live && c < ld) ? exp(L[(size_t)row * ld + c] - m) : 0.0;
    }
  }
}

// the prior on the user side (fold-in through the training kernels, HPF_FOLD_ROUTE=sweeps): shape s0, E = s0 / r0,
// Elog = psi(s0) - log(r0) in the live columns of S, E and L; xi likewise
__global__ void fold_prior_kernel(double *S, double *E, double *L, double *xi_E, double *xi_elog, uint32_t rows, uint32_t ld,
                                  uint32_t K, int32_t bias_col, double s0, double e0, double l0)
{
  const size_t n = (size_t)rows * ld;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
    const uint32_t c = (uint32_t)(e % ld);
    const bool live = c < K || (int32_t)c == bias_col;
    S[e] = live ? s0 : 0.0; E[e] = live ? e0 : 0.0; L[e] = live ? l0 : 0.0;
    if (c == 0 && xi_E) { xi_E[e / ld] = e0; xi_elog[e / ld] = l0; }
  }
}

// ---------------------------------------------------------------------
// K6: held-out log-likelihood per pair (rating_likelihood_hier,
// hgaprec.cc:1538-1560; rating_likelihood 1503-1536).  One 16-lane group
// per pair; the per-pair values are summed on the host in the given order.
// ---------------------------------------------------------------------
// log y! for y = 0 .. 255 as HGAPRec::log_factorial does it (hgaprec.cc:1563-1570): the serial sum of log i
inline void logfact_table(double lf[256])
{
  lf[0] = std::log(1.0); lf[1] = lf[0];
  for (uint32_t y = 2; y < 256; ++y) lf[y] = lf[y - 1] + std::log((double)y);
}

struct LLArgs {
  const uint32_t *u, *i;
  const int32_t  *y;
  uint64_t        cnt;
  const double   *Et, *Eb;     // [n x ld], [m x ld]
  const double   *logfact;     // [256]
  double         *out;         // [cnt]
  uint32_t        ld, K;
  int32_t         ubias_col, ibias_col;   // -1 without -bias
  uint32_t        binary;
};

__global__ __launch_bounds__(256) void heldout_ll_kernel(LLArgs a)
{
  constexpr int G = 16;
  const int lane = threadIdx.x & 63, g = lane % G;
  const uint64_t grp = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
  const uint64_t ngrp = ((uint64_t)gridDim.x * blockDim.x) / G;
  for (uint64_t p0 = 0; p0 < a.cnt; p0 += ngrp) {
    const uint64_t p = p0 + grp;
    const bool ok = p < a.cnt;
    const uint32_t u = ok ? a.u[p] : 0u, it = ok ? a.i[p] : 0u;
    const double *et = a.Et + (size_t)u * a.ld, *eb = a.Eb + (size_t)it * a.ld;
    double s = 0.0;
    if (ok)
      for (uint32_t c = g; c < a.K; c += G) s = fma(et[c], eb[c], s);
    s = group_sum<G>(s);
    if (ok && g == 0) {
      if (a.ubias_col >= 0) s += et[a.ubias_col] + eb[a.ibias_col];
      if (s < 1e-30) s = 1e-30;
      const uint32_t y = (uint32_t)a.y[p] & 0xffu;       // yval_t wrap
      double ll;
      if (a.binary) ll = (y == 0) ? -s : log(1.0 - exp(-s));
      else ll = (double)y * log(s) - s - a.logfact[y];
      a.out[p] = ll;
    }
  }
}

// ---------------------------------------------------------------------
// ELBO (HGAPRec::logl, hgaprec.cc:2160-2255), report-time only.
// Per nonzero the reference adds  sum_k y*sphi_k*(x_k - log sphi_k) - sum_k E_t E_b
// with sphi = yy*softmax(x), yy = (y > 1 ? y : 1); since
// x_k - log sphi_k = logsumexp(x) - log yy for every k, the first sum is
// y*yy*(logsumexp(x) - log yy).  One 16-lane group per nonzero; block partials.
// ---------------------------------------------------------------------
struct ElboNnzArgs {
  const Seg      *segs;     // the user-major work list of the phi pass: (row, start, len)
  uint32_t        nseg;
  const uint32_t *col;
  const uint8_t  *val;
  const double   *Lt, *Lb, *Et, *Eb;
  double         *partial;  // [gridDim.x]
  uint32_t        ld, K, C; // C = live columns (K or K+2)
  int32_t         ubias_col, ibias_col;
};

// logsumexp over the C live columns of lt + lb, by the G lanes of a group (every lane gets it): the maximum first, so
// that no spread of Elog overflows or underflows the sum
template <int G>
__device__ __forceinline__ double elog_logsumexp(const double *lt, const double *lb, uint32_t C, int g)
{
  double mx = -1.0e308;
  for (uint32_t c = g; c < C; c += G) mx = fmax(mx, lt[c] + lb[c]);
  mx = group_max<G>(mx);
  double se = 0.0;
  for (uint32_t c = g; c < C; c += G) se += exp(lt[c] + lb[c] - mx);
  se = group_sum<G>(se);
  return mx + log(se);
}

// one wave per segment (its user is known: no search for the owner of a
// nonzero), the wave's four 16-lane groups take the segment's nonzeros in turn
__global__ __launch_bounds__(256) void elbo_nnz_kernel(ElboNnzArgs a)
{
  constexpr int G = 16;
  __shared__ double red[256 / G];
  const int lane = threadIdx.x & 63, g = lane % G, q = lane / G;
  const uint32_t grp_in_block = threadIdx.x / G;
  const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
  double acc = 0.0;
  for (uint32_t s = wave; s < a.nseg; s += nwaves) {
    const Seg sg = a.segs[s];
    const double *lt = a.Lt + (size_t)sg.row * a.ld, *et = a.Et + (size_t)sg.row * a.ld;
    for (uint32_t o = 0; o < sg.len; o += 64 / G) {
      const bool ok = o + q < sg.len;
      const int64_t j = sg.start + o + q;
      const uint32_t it = ok ? a.col[j] : 0u;
      const double y = (ok && a.val) ? (double)a.val[j] : 1.0;
      const double *lb = a.Lb + (size_t)it * a.ld, *eb = a.Eb + (size_t)it * a.ld;
      double dot = 0.0;
      const double lse = elog_logsumexp<G>(lt, lb, a.C, g);
      for (uint32_t c = g; c < a.K; c += G) dot = fma(et[c], eb[c], dot);
      dot = group_sum<G>(dot);
      if (ok && g == 0) {
        const double yy = (y > 1.0) ? y : 1.0;
        double v = y * yy * (lse - log(yy)) - dot;
        if (a.ubias_col >= 0) v -= et[a.ubias_col] + eb[a.ibias_col];
        acc += v;
      }
    }
  }
  if (g == 0) red[grp_in_block] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (uint32_t k = 0; k < blockDim.x / G; ++k) s += red[k];
    a.partial[blockIdx.x] = s;
  }
}

// The same term from the hot loop's own arrays: W = exp(L - M) with M = the row
// maximum of L over the live columns (0 in the other side's bias slot), so
//   logsumexp(x) = log(sum_k Wt[u,k] * Wb[i,k]) + Mt[u] + Mb[i]
// -- no exp per element, one pass over the row pair instead of two.  fp64 W only.
// Where the two rows peak at different columns every product Wt * Wb is small: once their combined spread passes ~745
// the sum is 0 and its log -inf, and below 2^-1022 it is subnormal and has lost digits.  A nonzero whose sum is not at
// least ELBO_W_ZMIN -- 2^-960: what subnormal or flushed W cost a sum that large is below 2^-100 of it -- is therefore
// evaluated in the Elog form of elbo_nnz_kernel instead (a group-uniform branch: the sum is on every lane).
constexpr double ELBO_W_ZMIN = 0x1p-960;

struct ElboNnzWArgs {
  const Seg      *segs;
  uint32_t        nseg;
  const uint32_t *col;
  const uint8_t  *val;
  const double   *Wt, *Wb, *Et, *Eb;   // [rows x ld]
  const double   *Mt, *Mb;             // [rows] row maxima of Elog
  const double   *Lt, *Lb;             // [rows x ld] Elog, read only below ELBO_W_ZMIN
  double         *partial;             // [gridDim.x]
  uint32_t        ld, K, C;            // C = live columns (K or K+2)
  int32_t         ubias_col, ibias_col;
};

__global__ __launch_bounds__(256) void elbo_nnz_w_kernel(ElboNnzWArgs a)
{
  constexpr int G = 16;
  __shared__ double red[256 / G];
  const int lane = threadIdx.x & 63, g = lane % G, q = lane / G;
  const uint32_t grp_in_block = threadIdx.x / G;
  const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
  double acc = 0.0;
  for (uint32_t s = wave; s < a.nseg; s += nwaves) {
    const Seg sg = a.segs[s];
    const double *wt = a.Wt + (size_t)sg.row * a.ld, *et = a.Et + (size_t)sg.row * a.ld;
    const double mt = a.Mt[sg.row];
    for (uint32_t o = 0; o < sg.len; o += 64 / G) {
      const bool ok = o + q < sg.len;
      const int64_t j = sg.start + o + q;
      const uint32_t it = ok ? a.col[j] : 0u;
      const double y = (ok && a.val) ? (double)a.val[j] : 1.0;
      const double *wb = a.Wb + (size_t)it * a.ld, *eb = a.Eb + (size_t)it * a.ld;
      double z = 0.0, dot = 0.0;
      for (uint32_t c = g; c < a.ld; c += G) z = fma(wt[c], wb[c], z);       // padding columns hold 0
      for (uint32_t c = g; c < a.K; c += G) dot = fma(et[c], eb[c], dot);
      z = group_sum<G>(z);
      dot = group_sum<G>(dot);
      double lse;
      if (z >= ELBO_W_ZMIN) lse = log(z) + mt + a.Mb[it];
      else lse = elog_logsumexp<G>(a.Lt + (size_t)sg.row * a.ld, a.Lb + (size_t)it * a.ld, a.C, g);
      if (ok && g == 0) {
        const double yy = (y > 1.0) ? y : 1.0;
        double v = y * yy * (lse - log(yy)) - dot;
        if (a.ubias_col >= 0) v -= et[a.ubias_col] + eb[a.ibias_col];
        acc += v;
      }
    }
  }
  if (g == 0) red[grp_in_block] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (uint32_t k = 0; k < blockDim.x / G; ++k) s += red[k];
    a.partial[blockIdx.x] = s;
  }
}

// M[row] = max over the live columns of Elog (the other side's bias slot counts as 0)
__global__ void rowmax_elog_kernel(const double *L, double *M, uint32_t rows, uint32_t ld, uint32_t K,
                                   int32_t bias_col, int32_t junk_col)
{
  const uint32_t row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= rows) return;
  const double *l = L + (size_t)row * ld;
  double m = -1.0e308;
  for (uint32_t c = 0; c < K; ++c) m = fmax(m, l[c]);
  if (bias_col >= 0) m = fmax(m, l[bias_col]);
  if (junk_col >= 0) m = fmax(m, 0.0);
  M[row] = m;
}

// Gamma terms of one side (compute_elbo_term_helper, gpbase.hh:360-387,717-741)
// plus, with hier, of its xi/eta array (gpbase.hh:951-969); block partials.
struct ElboGammaArgs {
  const double *S, *E, *L;               // [rows x ld] shape, E, Elog
  const double *prior_used, *prior_elog_used;   // hier: E / Elog of xi (eta) the rate used
  const double *colsum_used;             // [ld]
  const double *prior_E, *prior_elog, *prior_rate;   // the xi / eta array itself
  double       *partial;                 // [gridDim.x]
  uint32_t      rows, ld, K;
  int32_t       bias_col;
  double        bias_rate_add, s_prior, r_prior, lg_s_prior, prior_shape, lg_prior_shape;
  uint32_t      hier;
};

__global__ __launch_bounds__(256) void elbo_gamma_kernel(ElboGammaArgs a)
{
  __shared__ double red[256];
  const double s0 = a.s_prior, r0 = a.r_prior, lr0 = log(r0);
  double acc = 0.0;
  const size_t n = (size_t)a.rows * a.ld;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n;
       e += (size_t)gridDim.x * blockDim.x) {
    const uint32_t row = (uint32_t)(e / a.ld), c = (uint32_t)(e % a.ld);
    const bool real = c < a.K, isb = (int32_t)c == a.bias_col;
    if (real || isb) {
      const double sh = a.S[e], ev = a.E[e], el = a.L[e];
      const bool h = real && a.hier;
      double b = real ? (a.hier ? a.prior_used[row] : r0) + a.colsum_used[c] : r0 + a.bias_rate_add;
      const double av = (sh > 0.0) ? sh : 1e-30;
      b = (b > 0.0) ? b : 1e-30;
      double t = s0 * (h ? a.prior_elog_used[row] : lr0) + (s0 - 1.0) * el;
      t -= (h ? a.prior_used[row] : r0) * ev + a.lg_s_prior;
      t -= av * log(b) + (av - 1.0) * el;
      t += b * ev + lgamma(av);
      acc += t;
    }
    if (a.hier && c == 0) {            // the GPArray element of this row
      const double av = a.prior_shape, b = a.prior_rate[row], ev = a.prior_E[row], el = a.prior_elog[row];
      double t = s0 * lr0 + (s0 - 1.0) * el;
      t -= r0 * ev + a.lg_s_prior;
      t -= av * log(b) + (av - 1.0) * el;
      t += b * ev + a.lg_prior_shape;
      acc += t;
    }
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) a.partial[blockIdx.x] = red[0];
}

// ---------------------------------------------------------------------
// Ranking evaluation (report steps): compute_precision / compute_itemrank
// (hgaprec.cc:1703-1848, 1606-1701).  The reference scores EVERY item for each
// sampled user (prediction_score_hier, hgaprec.cc:1966-1991), zeroes training
// and validation items, qsorts all m scores and walks the top 100.  Here:
//   score_tile_kernel   dense E_theta[sel] x E_beta^T on the fp64 matrix cores
//                       (v_mfma_f64_16x16x4_f64) -- the one GEMM-shaped piece
//   mask_scores_kernel  training (rating > 0) and validation items -> 0.0
//   topn_kernel         exact top-N per user (block_topn): 8-pass radix select
//                       on the 64-bit score pattern, ties by ascending item index
//                       (= glibc's stable merge-sort qsort), bitonic sort of N
//   rank_query_kernel   position of one item in the full order (itemrank)
// One order (ranks_before), one sort (bitonic_sort) and one selection (block_topn)
// serve every ranking kernel of this file.
// ---------------------------------------------------------------------
typedef double double4_t __attribute__((ext_vector_type(4)));

struct ScoreArgs {
  const uint32_t *users;    // [n_sel] selected user rows
  const double   *Et, *Eb;  // [n x ld], [m x ld]
  double         *scores;   // [n_sel x m]
  uint32_t        n_sel, m, ld, K;
  int32_t         ubias_col, ibias_col;
};

// block = 4 waves; wave w: 16 users x 64 items (4 MFMA tiles of 16x16)
__global__ __launch_bounds__(256) void score_tile_kernel(ScoreArgs a)
{
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r16 = lane & 15, kq = lane >> 4;
  const uint32_t u0 = blockIdx.y * 16, i0 = (blockIdx.x * 4 + wv) * 64;
  if (i0 >= a.m) return;
  const uint32_t usel = u0 + r16;
  const uint32_t urow = usel < a.n_sel ? a.users[usel] : 0u;
  const double *pa = a.Et + (size_t)urow * a.ld;
  const double *pb[4]; bool okb[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const uint32_t it = i0 + 16 * t + r16;
    okb[t] = it < a.m;
    pb[t] = a.Eb + (size_t)(okb[t] ? it : 0u) * a.ld;
  }
  double4_t acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = (double4_t){0.0, 0.0, 0.0, 0.0};
  for (uint32_t k0 = 0; k0 < a.K; k0 += 4) {
    const uint32_t k = k0 + kq;
    const bool okk = k < a.K;
    const double av = (okk && usel < a.n_sel) ? pa[k] : 0.0;       // A[i = lane%16][k = lane/16]
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const double bv = (okk && okb[t]) ? pb[t][k] : 0.0;         // B[k = lane/16][j = lane%16]
      acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[t], 0, 0, 0);
    }
  }
  // D (4 doubles per lane): register r holds D[i = lane/16 + 4*r][j = lane%16]
  // (verified against a dense product in tests/test_gpu_ranking.py)
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const uint32_t it = i0 + 16 * t + r16;
    if (it >= a.m) continue;
    const double bi = a.ibias_col >= 0 ? a.Eb[(size_t)it * a.ld + a.ibias_col] : 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const uint32_t us = u0 + kq + 4 * r;
      if (us >= a.n_sel) continue;
      double v = acc[t][r];
      if (a.ubias_col >= 0) v += a.Et[(size_t)a.users[us] * a.ld + a.ubias_col] + bi;   // s += Eb_u + Eb_i
      a.scores[(size_t)us * a.m + it] = v;
    }
  }
}

// What is masked for selected user b (row u of the training matrix): its training items with a stored rating > 0 (a
// uint8-wrapped 0 is NOT skipped: "_ratings.r(n,m) > 0") and the caller's mask list (validation items).  The 64 lanes of
// one wave share the walk; f(item) may meet an item twice.
template <typename F>
__device__ __forceinline__ void masked_items(uint32_t u, uint32_t b, int lane, const int64_t *rowptr, const uint32_t *col,
                                             const uint8_t *val, const uint64_t *mask_ptr, const uint32_t *mask_items, F &&f)
{
  if (rowptr)
    for (int64_t j = rowptr[u] + lane; j < rowptr[u + 1]; j += 64)
      if (!val || val[j] > 0) f(col[j]);
  if (mask_ptr)
    for (uint64_t j = mask_ptr[b] + lane; j < mask_ptr[b + 1]; j += 64) f(mask_items[j]);
}

// one wave per selected user: zero the scores of its masked items
__global__ void mask_scores_kernel(const uint32_t *users, uint32_t n_sel, const int64_t *rowptr,
                                   const uint32_t *col, const uint8_t *val, const uint64_t *mask_ptr,
                                   const uint32_t *mask_items, double *scores, uint32_t m)
{
  const int lane = threadIdx.x & 63;
  const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
  for (uint32_t b = wave; b < n_sel; b += nwaves) {
    double *row = scores + (size_t)b * m;
    masked_items(users[b], b, lane, rowptr, col, val, mask_ptr, mask_items, [&](uint32_t it) { row[it] = 0.0; });
  }
}

__device__ __forceinline__ unsigned long long score_key(double v)
{
  return (unsigned long long)__double_as_longlong(v);     // scores are >= +0.0: bit order = value order
}

// THE order of every ranking result: the larger key first, of equal keys the smaller item
__device__ __forceinline__ bool ranks_before(unsigned long long ka, uint32_t ia, unsigned long long kb, uint32_t ib)
{
  return ka > kb || (ka == kb && ia < ib);
}

// Bitonic sort of the P (a power of two) entries (sk[e], si[e]) in LDS into that order, by NT threads of which this is
// thread `tid`; barrier() stands between one step's exchanges and the next step's reads (and behind the last)
template <uint32_t NT, typename Barrier>
__device__ __forceinline__ void bitonic_sort(unsigned long long *sk, uint32_t *si, uint32_t P, uint32_t tid, Barrier &&barrier)
{
  for (uint32_t k = 2; k <= P; k <<= 1)
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t t = tid; t < P; t += NT) {
        const uint32_t x = t ^ j;
        if (x > t) {
          const bool up = (t & k) == 0;           // "up" block: best entries first
          const unsigned long long ka = sk[t], kb = sk[x]; const uint32_t ia = si[t], ib = si[x];
          if (ranks_before(ka, ia, kb, ib) != up) { sk[t] = kb; sk[x] = ka; si[t] = ib; si[x] = ia; }
        }
      }
      barrier();
    }
}

// Exact top-N of a list of entries by one workgroup of 256 threads: 8-pass radix select on the 64-bit key, the entries
// above the N-th key gathered, its ties taken in ascending i, bitonic sort; NP = pow2 >= N in dynamic LDS (NP * 12 bytes).
// The list is src: entries i < n(), of which those with present(i) count, each a key(i) and an item(i).  All it asks of
// the list is that equal keys come in ascending item order as i ascends.  Ne = the entries wanted (<= N, <= the present
// ones); the N - Ne places behind them are padded (item 0xffffffff, score 0.0).
template <typename Src>
__device__ __forceinline__ void block_topn(const Src &src, uint32_t N, uint32_t Ne, uint32_t NP, uint32_t *out_items, double *out_scores)
{
  extern __shared__ unsigned char smem[];
  unsigned long long *ck = (unsigned long long *)smem;            // [NP] candidate keys
  uint32_t *ci = (uint32_t *)(ck + NP);                          // [NP] candidate items
  __shared__ uint32_t hist[256];
  __shared__ unsigned long long s_prefix;
  __shared__ uint32_t s_remaining, s_cnt, s_wtot[4], s_eq_taken;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint32_t L = src.n();

  for (uint32_t k = tid; k < NP; k += 256) { ck[k] = 0ull; ci[k] = 0xffffffffu; }
  if (tid == 0) { s_prefix = 0ull; s_remaining = Ne; s_cnt = 0; s_eq_taken = 0; }
  __syncthreads();
  if (Ne > 0) {
    for (int pass = 0; pass < 8; ++pass) {
      const int shift = 56 - 8 * pass;
      hist[tid] = 0;
      __syncthreads();
      const unsigned long long prefix = s_prefix;
      for (uint32_t i = tid; i < L; i += 256) {
        if (!src.present(i)) continue;
        const unsigned long long key = src.key(i);
        if (pass == 0 || (key >> (shift + 8)) == prefix) atomicAdd(&hist[(key >> shift) & 255ull], 1u);
      }
      __syncthreads();
      if (tid == 0) {
        uint32_t cum = 0, rem = s_remaining; int d = 255;
        for (; d > 0; --d) { if (cum + hist[d] >= rem) break; cum += hist[d]; }
        s_remaining = rem - cum;
        s_prefix = (prefix << 8) | (unsigned long long)d;
      }
      __syncthreads();
    }
    const unsigned long long T = s_prefix;       // key of the Ne-th best entry
    const uint32_t need_eq = s_remaining;         // how many of the == T to take (lowest items)
    for (uint32_t i = tid; i < L; i += 256) {
      if (!src.present(i)) continue;
      const unsigned long long key = src.key(i);
      if (key > T) { const uint32_t p = atomicAdd(&s_cnt, 1u); if (p < NP) { ck[p] = key; ci[p] = src.item(i); } }
    }
    __syncthreads();
    const uint32_t base = s_cnt;                  // = Ne - need_eq
    for (uint32_t c0 = 0; c0 < L; c0 += 256) {    // ties in ascending item order
      const uint32_t i = c0 + tid;
      const bool eq = src.present(i) && src.key(i) == T;
      const unsigned long long bal = __ballot(eq);
      const uint32_t before = __popcll(bal & ((1ull << lane) - 1ull));
      if (lane == 0) s_wtot[wv] = (uint32_t)__popcll(bal);
      __syncthreads();
      uint32_t woff = 0, tot = 0;
      for (uint32_t w = 0; w < 4; ++w) { if (w < wv) woff += s_wtot[w]; tot += s_wtot[w]; }
      const uint32_t taken = s_eq_taken;
      const uint32_t pos = taken + woff + before;
      if (eq && pos < need_eq && base + pos < NP) { ck[base + pos] = T; ci[base + pos] = src.item(i); }
      __syncthreads();
      if (tid == 0) s_eq_taken = taken + tot;
      __syncthreads();
      if (s_eq_taken >= need_eq) break;
    }
    __syncthreads();
    bitonic_sort<256>(ck, ci, NP, tid, [] { __syncthreads(); });
  }
  for (uint32_t k = tid; k < N; k += 256) {
    out_items[k] = k < Ne ? ci[k] : 0xffffffffu;
    out_scores[k] = k < Ne ? __longlong_as_double((long long)ck[k]) : 0.0;
  }
}

// a row of m scores as such a list: entry i is item i
struct RowEntries {
  const double *row; uint32_t m;
  __device__ __forceinline__ uint32_t n() const { return m; }
  __device__ __forceinline__ bool present(uint32_t i) const { return i < m; }
  __device__ __forceinline__ unsigned long long key(uint32_t i) const { return score_key(row[i]); }
  __device__ __forceinline__ uint32_t item(uint32_t i) const { return i; }
};

// exact top-N of one row of scores per block (256 threads); NP = pow2 >= N
__global__ __launch_bounds__(256) void topn_kernel(const double *scores, uint32_t n_sel, uint32_t m,
                                                   uint32_t N, uint32_t NP, uint32_t *out_items,
                                                   double *out_scores)
{
  const uint32_t b = blockIdx.x;
  if (b >= n_sel) return;
  block_topn(RowEntries{scores + (size_t)b * m, m}, N, N < m ? N : m, NP, out_items + (size_t)b * N, out_scores + (size_t)b * N);
}

// rank position (0-based) of item q_item[q] in the full descending order of
// row q_sel[q] (ties by ascending item index); one block per query
__global__ __launch_bounds__(256) void rank_query_kernel(const double *scores, uint32_t m,
                                                         const uint32_t *q_sel, const uint32_t *q_item,
                                                         uint32_t nq, uint32_t sel0, uint32_t sel1,
                                                         uint32_t *out_rank, double *out_score)
{
  __shared__ uint32_t red[256];
  for (uint32_t q = blockIdx.x; q < nq; q += gridDim.x) {
    const uint32_t b = q_sel[q];
    if (b < sel0 || b >= sel1) continue;           // not in this batch of rows (uniform per block)
    const double *row = scores + (size_t)(b - sel0) * m;
    const uint32_t it = q_item[q];
    const unsigned long long kq = score_key(row[it]);
    uint32_t c = 0;
    for (uint32_t i = threadIdx.x; i < m; i += 256) {
      const unsigned long long k = score_key(row[i]);
      c += ranks_before(k, i, kq, it) ? 1u : 0u;
    }
    red[threadIdx.x] = c;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
      __syncthreads();
    }
    if (threadIdx.x == 0) { out_rank[q] = red[0]; out_score[q] = row[it]; }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------
// Scoring a saved model (-rmse, -msr).
//   predict_kernel      the rate of one (user, item) pair per 16-lane group: the dot product of
//                       heldout_ll_kernel, handed out instead of its likelihood
//   loo_mask_kernel     training (rating > 0) and mask-list items of a batch of users as BITS
//   loo_rank_kernel     fused score-and-count: where ONE item per user stands among all items.
//                       Scores a 16 x 64 tile per wave on the fp64 matrix cores with the MFMA sequence
//                       of score_tile_kernel (so every score carries the same bits), compares it in
//                       registers with the user's threshold and counts; no score reaches memory.
// ---------------------------------------------------------------------
struct PredictArgs {
  const uint32_t *u, *i;
  uint64_t        cnt;
  const double   *Et, *Eb;     // [n x ld], [m x ld]
  double         *out;         // [cnt]
  uint32_t        ld, K;
  int32_t         ubias_col, ibias_col;   // -1 without -bias
};

__global__ __launch_bounds__(256) void predict_kernel(PredictArgs a)
{
  constexpr int G = 16;
  const int lane = threadIdx.x & 63, g = lane % G;
  const uint64_t grp = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
  const uint64_t ngrp = ((uint64_t)gridDim.x * blockDim.x) / G;
  for (uint64_t p0 = 0; p0 < a.cnt; p0 += ngrp) {
    const uint64_t p = p0 + grp;
    const bool ok = p < a.cnt;
    const uint32_t u = ok ? a.u[p] : 0u, it = ok ? a.i[p] : 0u;
    const double *et = a.Et + (size_t)u * a.ld, *eb = a.Eb + (size_t)it * a.ld;
    double s = 0.0;
    if (ok)
      for (uint32_t c = g; c < a.K; c += G) s = fma(et[c], eb[c], s);
    s = group_sum<G>(s);
    if (ok && g == 0) {
      if (a.ubias_col >= 0) s += et[a.ubias_col] + eb[a.ibias_col];
      a.out[p] = s;
    }
  }
}

// one wave per user of the batch: bit i of row b is set when item i is masked for that user (masked_items).  Rows are
// `words` 64-bit words, written as dwords.
__global__ void loo_mask_kernel(const uint32_t *users, uint32_t n_sel, const int64_t *rowptr,
                                const uint32_t *col, const uint8_t *val, const uint64_t *mask_ptr,
                                const uint32_t *mask_items, uint32_t *bits, uint32_t words)
{
  const int lane = threadIdx.x & 63;
  const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
  for (uint32_t b = wave; b < n_sel; b += nwaves) {
    uint32_t *row = bits + (size_t)b * words * 2;
    masked_items(users[b], b, lane, rowptr, col, val, mask_ptr, mask_items,
                 [&](uint32_t it) { atomicOr(&row[it >> 5], 1u << (it & 31u)); });
  }
}

struct LooArgs {
  const uint32_t *users;    // [n_sel] user rows of this batch
  const uint32_t *q_item;   // [n_sel] the item whose position is asked for
  const double   *Et, *Eb;  // [n x ld], [m x ld]
  const uint64_t *bits;     // [n_sel x words] masked items
  uint32_t       *rank;     // [n_sel] zeroed; counts are added
  uint32_t       *masked;   // [n_sel] zeroed; distinct masked items below limit
  double         *score;    // [n_sel]
  uint32_t        n_sel, limit, ld, K, words;
  uint32_t        tiles_per_split;   // 64-item tiles per blockIdx.y
  int32_t         ubias_col, ibias_col;
};

constexpr int LOO_KC = 32;            // columns of an item tile staged at once
constexpr int LOO_LDS_STRIDE = 34;    // doubles per staged row: the 16 rows x 2 k of a half wave fall into 32 different bank pairs

// ---- the item sweep of the two fused rank kernels ---------------------------------------------------------------------
// A wave's A fragments: the rows of E_theta of its 16 users, A[i = lane%16][k = 4 s + lane/16] for MFMA step s.  NCH > 0:
// K <= 32 * NCH <= 128 and they stay in registers; NCH == 0: read per step like score_tile_kernel does (K up to
// HPF_MAX_COLUMNS).
template <int NCH>
struct AFrag {
  double reg[NCH > 0 ? NCH * 8 : 1];
  const double *pa; uint32_t K, kq; bool ok;
  __device__ __forceinline__ AFrag(const double *row, bool row_ok, uint32_t K_, uint32_t kq_) : pa(row), K(K_), kq(kq_), ok(row_ok)
  {
    if (NCH > 0) {
#pragma unroll
      for (int s = 0; s < NCH * 8; ++s) reg[s] = load((uint32_t)s);
    }
  }
  __device__ __forceinline__ double load(uint32_t s) const { const uint32_t k = 4u * s + kq; return (ok && k < K) ? pa[k] : 0.0; }
};

// Workgroup = 4 waves = 64 users or rows (16 per wave) x one split of the item range: the 64-item tiles [t0, t1) of
// blockIdx.y.  The 64 x 32 pieces of the item rows go through LDS (`tile`; 16-byte loads, the next piece on its way
// while this one is multiplied) and are shared by the four waves.  Per output ONE accumulator chain over k0 = 0, 4, 8,
// ... with the tail padded by zeros -- exactly the MFMAs score_tile_kernel issues.  epi(tl, acc) gets each tile's
// scores before the biases: register r of acc[t] holds the wave's user kq + 4 r, item 64 tl + 16 t + r16.
template <int NCH, typename Epi>
__device__ __forceinline__ void rank_sweep(const AFrag<NCH> &A, const double *Eb, uint32_t limit, uint32_t ld, uint32_t K,
                                           uint32_t tiles_per_split, double *tile, Epi &&epi)
{
  const int tid = threadIdx.x, lane = tid & 63;
  const int r16 = lane & 15, kq = lane >> 4;
  const uint32_t nsteps = (K + 3) / 4;                           // MFMAs per output, as in score_tile_kernel
  const uint32_t ntiles = (limit + 63) / 64;
  const uint32_t t0 = blockIdx.y * tiles_per_split, t1 = min(ntiles, t0 + tiles_per_split);
  const uint32_t nchunks = (K + LOO_KC - 1) / LOO_KC;

  // this thread's four 16-byte pieces of a 64 x 32 chunk: piece p = tid + 256 j -> row p / 16, columns 2 (p % 16), +1
  double2 pre[4];
  auto fetch = [&](uint32_t tile_i, uint32_t chunk) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t p = (uint32_t)tid + 256u * j, row = p >> 4, c = chunk * LOO_KC + 2u * (p & 15u);
      const uint32_t it = tile_i * 64 + row;
      double2 v = make_double2(0.0, 0.0);
      if (it < limit && c < K) {                                 // c is even and ld is even: c + 1 < ld
        v = *(const double2 *)(Eb + (size_t)it * ld + c);
        if (c + 1 >= K) v.y = 0.0;
      }
      pre[j] = v;
    }
  };
  if (t0 < t1) fetch(t0, 0);
  for (uint32_t tl = t0; tl < t1; ++tl) {
    double4_t acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = (double4_t){0.0, 0.0, 0.0, 0.0};
    auto stage = [&](uint32_t ch) {
      __syncthreads();                                         // the previous chunk has been read
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t p = (uint32_t)tid + 256u * j;
        *(double2 *)&tile[(p >> 4) * LOO_LDS_STRIDE + 2u * (p & 15u)] = pre[j];
      }
      __syncthreads();
      if (ch + 1 < nchunks) fetch(tl, ch + 1);
      else if (tl + 1 < t1) fetch(tl + 1, 0);
    };
    if (NCH > 0) {
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch)
        if ((uint32_t)ch < nchunks) {
          stage((uint32_t)ch);
#pragma unroll
          for (int s = 0; s < 8; ++s)
            if ((uint32_t)(ch * 8 + s) < nsteps) {
#pragma unroll
              for (int t = 0; t < 4; ++t) {
                const double bv = tile[(16 * t + r16) * LOO_LDS_STRIDE + 4 * s + kq];   // B[k = lane/16][j = lane%16]
                acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(A.reg[ch * 8 + s], bv, acc[t], 0, 0, 0);
              }
            }
        }
    } else {
      for (uint32_t ch = 0; ch < nchunks; ++ch) {
        stage(ch);
        for (uint32_t s = 0; s < 8 && ch * 8 + s < nsteps; ++s) {
          const double av = A.load(ch * 8 + s);
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            const double bv = tile[(16 * t + r16) * LOO_LDS_STRIDE + 4 * s + kq];
            acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[t], 0, 0, 0);
          }
        }
      }
    }
    epi(tl, acc);
  }
}

// ---- what the epilogues of the fused kernels share (a: LooArgs, RqArgs or TopnArgs) --------------------------------------
// E_ubias of selected user `sel` and E_ibias of item `it`; 0.0 without -bias or where there is no such user or item
template <typename Args>
__device__ __forceinline__ double user_bias(const Args &a, uint32_t sel, bool ok)
{
  return (ok && a.ubias_col >= 0) ? a.Et[(size_t)a.users[sel] * a.ld + a.ubias_col] : 0.0;
}
template <typename Args>
__device__ __forceinline__ double item_bias(const Args &a, uint32_t it, bool ok)
{
  return (ok && a.ibias_col >= 0) ? a.Eb[(size_t)it * a.ld + a.ibias_col] : 0.0;
}
// is item `it` masked for selected user `sel`?
template <typename Args>
__device__ __forceinline__ bool item_masked(const Args &a, uint32_t sel, uint32_t it)
{
  return (a.bits[(size_t)sel * a.words + (it >> 6)] >> (it & 63u)) & 1ull;
}
// Key of an epilogue register: the sweep's dot product v, + (E_ubias + E_ibias) with -bias, +0.0 where bit `bit` of the
// user's mask word w of this tile is set
__device__ __forceinline__ unsigned long long epilogue_key(double v, bool bias, double ub, double bi, unsigned long long w, int bit)
{
  if (bias) v += ub + bi;                                        // s += Eb_u + Eb_i
  if ((w >> bit) & 1ull) v = 0.0;
  return score_key(v);
}

// The threshold s(b, t) comes from the sweep's arithmetic: a 16 x 16 tile whose column j is the row of user j's query
// item, of which the diagonal is kept.  Every score and the threshold then get + (E_ubias + E_ibias).
template <int NCH>
__global__ __launch_bounds__(256) void loo_rank_kernel(LooArgs a)
{
  __shared__ double tile[64 * LOO_LDS_STRIDE];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int r16 = lane & 15, kq = lane >> 4;
  const uint32_t ub0 = blockIdx.x * 64 + wv * 16;              // first user of this wave
  const uint32_t usel = ub0 + r16;
  const bool uok = usel < a.n_sel;
  const uint32_t urow = uok ? a.users[usel] : 0u;
  const double *pa = a.Et + (size_t)urow * a.ld;
  const uint32_t nsteps = (a.K + 3) / 4;
  const AFrag<NCH> A(pa, uok, a.K, (uint32_t)kq);

  // ---- thresholds: D[i][j] = E_theta[user i] . E_beta[query item of user j], diagonal kept
  const uint32_t myq = uok ? a.q_item[usel] : 0u;
  double thr[4]; uint32_t tq[4]; bool live[4];
  {
    const double *pq = a.Eb + (size_t)myq * a.ld;
    double4_t acc = (double4_t){0.0, 0.0, 0.0, 0.0};
    if (NCH > 0) {
#pragma unroll
      for (int s = 0; s < NCH * 8; ++s)
        if ((uint32_t)s < nsteps) {
          const uint32_t k = 4u * s + kq;
          const double bv = (uok && k < a.K) ? pq[k] : 0.0;
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(A.reg[s], bv, acc, 0, 0, 0);
        }
    } else {
      for (uint32_t s = 0; s < nsteps; ++s) {
        const uint32_t k = 4u * s + kq;
        const double bv = (uok && k < a.K) ? pq[k] : 0.0;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(A.load(s), bv, acc, 0, 0, 0);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int src = (kq + 4 * r) + 16 * kq;                  // the lane that holds D[i][i] for i = kq + 4 r, in register r
      double v = __shfl(acc[r], src);
      const uint32_t us = ub0 + kq + 4 * r;
      live[r] = us < a.n_sel;
      tq[r] = live[r] ? a.q_item[us] : 0u;
      if (live[r] && a.ubias_col >= 0)
        v += a.Et[(size_t)a.users[us] * a.ld + a.ubias_col] + a.Eb[(size_t)tq[r] * a.ld + a.ibias_col];
      if (live[r] && item_masked(a, us, tq[r])) v = 0.0;
      if (tq[r] >= a.limit) live[r] = false;                   // outside the ranked range: rank 0, score 0.0
      thr[r] = v;
    }
  }

  // ---- item sweep
  uint32_t cnt[4] = {0, 0, 0, 0}, msk[4] = {0, 0, 0, 0};
  double ubv[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const uint32_t us = ub0 + kq + 4 * r;
    ubv[r] = user_bias(a, us, us < a.n_sel);
  }
  rank_sweep<NCH>(A, a.Eb, a.limit, a.ld, a.K, a.tiles_per_split, tile, [&](uint32_t tl, const double4_t (&acc)[4]) {
    // epilogue: register r of tile t holds user kq + 4 r, item 64 tl + 16 t + r16
    const uint32_t i0 = tl * 64;
    unsigned long long w[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const uint32_t us = ub0 + kq + 4 * r;
      w[r] = us < a.n_sel ? a.bits[(size_t)us * a.words + tl] : 0ull;
      if (r16 == 0) {
        const uint32_t left = a.limit - i0;                    // > 0: the tile starts below the limit
        msk[r] += (uint32_t)__popcll(left >= 64 ? w[r] : (w[r] & ((1ull << left) - 1ull)));
      }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const uint32_t it = i0 + 16 * t + r16;
      const bool iok = it < a.limit;
      const double bi = item_bias(a, it, iok);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        double v = acc[t][r];                                  // epilogue_key spelled out, as the bias loads of the threshold
                                                               // above are: these two sites keep the code this kernel had (profiles/r10)
        if (a.ubias_col >= 0) v += ubv[r] + bi;                // s += Eb_u + Eb_i
        if ((w[r] >> (16 * t + r16)) & 1ull) v = 0.0;
        const unsigned long long k = score_key(v), kt = score_key(thr[r]);
        cnt[r] += (iok && live[r] && it != tq[r] && ranks_before(k, it, kt, tq[r])) ? 1u : 0u;
      }
    }
  });
  // one reduction per user block: over the 16 lanes that share kq
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    uint32_t c = cnt[r];
    for (int o = 8; o > 0; o >>= 1) c += __shfl_xor(c, o);
    const uint32_t us = ub0 + kq + 4 * r;
    if (r16 == 0 && us < a.n_sel) {
      if (c) atomicAdd(&a.rank[us], c);
      if (msk[r]) atomicAdd(&a.masked[us], msk[r]);
      if (blockIdx.y == 0) a.score[us] = live[r] ? thr[r] : 0.0;
    }
  }
}

// ---------------------------------------------------------------------
// Every test item of a user in one pass (hpf_rank_queries, -eval-all).
//   rq_threshold_kernel  s(b, t) of every query of a ROW (one selected user with <= RQ_QCAP of its queries) from the
//                        MFMA chain of score_tile_kernel, masked like loo_rank_kernel's threshold; the row's
//                        thresholds sorted best first, with the permutation back to the caller's order
//   rank_queries_kernel  the same sweep (rank_sweep); each score finds by binary search how many of its row's sorted
//                        thresholds come before or equal it and counts into an LDS histogram; prefix sums are the ranks
// ---------------------------------------------------------------------
constexpr int RQ_QCAP = 32;           // queries of one row (hgaprec_amd/capi.py mirrors it as RANK_QUERIES_QCAP)
static_assert(RQ_QCAP <= 64 && RQ_QCAP % 16 == 0, "a row's thresholds are sorted by one wave, 16 per MFMA chain");

struct RqArgs {
  const uint32_t *users;    // [batch] user rows of this batch of selected users
  const uint32_t *row_sel;  // [nrows] selected user of the row, relative to the batch
  const uint32_t *row_q0;   // [nrows] first query of the row (index into q_item and the arrays below)
  const uint32_t *row_nq;   // [nrows] 1 .. RQ_QCAP
  const uint32_t *q_item;   // [queries]
  const double   *Et, *Eb;  // [n x ld], [m x ld]
  const uint64_t *bits;     // [batch x words] masked items
  unsigned long long *skey; // [queries] a row's thresholds, best first, at row_q0 + s
  uint32_t       *sitem;    // [queries] ... their items
  uint32_t       *sperm;    // [queries] ... and the query each came from
  uint32_t       *rank;     // [queries] zeroed; counts are added
  double         *score;    // [queries]
  uint32_t        nrows, m, ld, K, words;
  uint32_t        tiles_per_split;   // 64-item tiles per blockIdx.y
  int32_t         ubias_col, ibias_col;
};

// One wave per row.  A 16 x 16 tile whose 16 rows are ALL the row's user and whose column j is the item of query
// 16 c + j: every output row holds the 16 thresholds, no shuffle needed (loo_rank_kernel has one query per user and
// keeps a diagonal instead; a row's queries are consecutive, so here one chain serves 16 of them).  Same chain per
// output as score_tile_kernel: k0 = 0, 4, 8, ... with the tail padded by zeros, then + (E_ubias + E_ibias).
__global__ __launch_bounds__(256) void rq_threshold_kernel(RqArgs a)
{
  __shared__ unsigned long long sk[4][RQ_QCAP];
  __shared__ uint32_t si[4][RQ_QCAP];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r16 = lane & 15, kq = lane >> 4;
  const uint32_t row = blockIdx.x * 4 + wv;
  const bool rok = row < a.nrows;
  const uint32_t sel = rok ? a.row_sel[row] : 0u, q0 = rok ? a.row_q0[row] : 0u, Q = rok ? a.row_nq[row] : 0u;
  const uint32_t urow = rok ? a.users[sel] : 0u;
  const double *pa = a.Et + (size_t)urow * a.ld;
  for (uint32_t c = 0; 16 * c < Q; ++c) {
    const uint32_t j = 16 * c + r16;
    const bool ok = j < Q;
    const uint32_t it = ok ? a.q_item[q0 + j] : 0u;
    const double *pq = a.Eb + (size_t)it * a.ld;
    double4_t acc = (double4_t){0.0, 0.0, 0.0, 0.0};
    for (uint32_t k0 = 0; k0 < a.K; k0 += 4) {
      const uint32_t k = k0 + kq;
      const double av = k < a.K ? pa[k] : 0.0;                   // A[i][k]: the same user in every row i
      const double bv = (ok && k < a.K) ? pq[k] : 0.0;           // B[k = lane/16][j = lane%16]
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
    }
    if (kq == 0 && ok) {                                         // register 0 of lane j: D[0][j]
      double v = acc[0];
      if (a.ubias_col >= 0) v += pa[a.ubias_col] + pq[a.ibias_col];
      if (item_masked(a, sel, it)) v = 0.0;
      sk[wv][j] = score_key(v); si[wv][j] = it;
      a.score[q0 + j] = v;
    }
  }
  __syncthreads();
  if ((uint32_t)lane < Q) {                                      // rank sort: key descending, item ascending, then query
    const unsigned long long ke = sk[wv][lane]; const uint32_t ie = si[wv][lane];
    uint32_t pos = 0;
    for (uint32_t f = 0; f < Q; ++f) {
      const unsigned long long kf = sk[wv][f]; const uint32_t jf = si[wv][f];
      pos += (ranks_before(kf, jf, ke, ie) || (kf == ke && jf == ie && f < (uint32_t)lane)) ? 1u : 0u;
    }
    a.skey[q0 + pos] = ke; a.sitem[q0 + pos] = ie; a.sperm[q0 + pos] = q0 + (uint32_t)lane;
  }
}

constexpr int RQ_CNT_STRIDE = RQ_QCAP + 1;

// Workgroup = 4 waves = 64 rows (16 per wave) x one split of the item range; staging, A fragments and MFMA order are
// rank_sweep's.  The 64 rows' sorted thresholds and a histogram [row][p] live in LDS.  A score (key, item) adds 1
// at p = the number of its row's thresholds that come before or equal it; p = Q (it precedes none: one comparison
// with the row's worst threshold, kept in registers) adds nothing.  "Before or equal" puts a queried item behind its
// own threshold and behind every duplicate of it.  The rank of the threshold at sorted position s is the sum of the
// histogram over 0 .. s.
template <int NCH>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void rank_queries_kernel(RqArgs a)
{
  __shared__ double tile[64 * LOO_LDS_STRIDE];
  __shared__ unsigned long long tk[64 * RQ_QCAP];
  __shared__ uint32_t ti[64 * RQ_QCAP];
  __shared__ uint32_t cn[64 * RQ_CNT_STRIDE];
  __shared__ uint32_t s_nq[64], s_sel[64];                         // per row: its queries (0: no such row), its user of the batch
  __shared__ double s_ub[64];                                       // ... and E_ubias of that user
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int r16 = lane & 15, kq = lane >> 4;
  const uint32_t rb0 = blockIdx.x * 64;                          // first row of this workgroup
  const uint32_t rsel = rb0 + wv * 16 + r16;
  const bool uok = rsel < a.nrows;
  const uint32_t urow = uok ? a.users[a.row_sel[rsel]] : 0u;
  const double *pa = a.Et + (size_t)urow * a.ld;
  const AFrag<NCH> A(pa, uok, a.K, (uint32_t)kq);

  // ---- the rows' sorted thresholds into LDS, histogram zeroed
  for (uint32_t e = tid; e < 64u * RQ_QCAP; e += 256) {
    const uint32_t lr = e / RQ_QCAP, s = e % RQ_QCAP, row = rb0 + lr;
    unsigned long long k = 0ull; uint32_t it = 0u;
    if (row < a.nrows && s < a.row_nq[row]) { const uint32_t q = a.row_q0[row] + s; k = a.skey[q]; it = a.sitem[q]; }
    tk[e] = k; ti[e] = it;
  }
  for (uint32_t e = tid; e < 64u * RQ_CNT_STRIDE; e += 256) cn[e] = 0u;
  if (tid < 64) {
    const uint32_t row = rb0 + tid;
    const bool ok = row < a.nrows;
    const uint32_t sel = ok ? a.row_sel[row] : 0u;
    s_nq[tid] = ok ? a.row_nq[row] : 0u; s_sel[tid] = sel;
    s_ub[tid] = user_bias(a, sel, ok);
  }
  __syncthreads();

  // ---- item sweep
  rank_sweep<NCH>(A, a.Eb, a.m, a.ld, a.K, a.tiles_per_split, tile, [&](uint32_t tl, const double4_t (&acc)[4]) {
    // epilogue: register r of tile t holds local row wv 16 + kq + 4 r, item 64 tl + 16 t + r16.  What a row needs is
    // read from LDS per tile (kept in registers it would cost the second wave per SIMD)
    const uint32_t i0 = tl * 64;
    double bi[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const uint32_t it = i0 + 16 * t + r16;
      bi[t] = item_bias(a, it, it < a.m);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const uint32_t lr = wv * 16 + kq + 4 * r, Q = s_nq[lr];
      if (Q) {
        const unsigned long long w = a.bits[(size_t)s_sel[lr] * a.words + tl];
        const unsigned long long wk = tk[lr * RQ_QCAP + Q - 1];  // the row's worst threshold
        const uint32_t wi = ti[lr * RQ_QCAP + Q - 1];
        const double ub = s_ub[lr];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const uint32_t it = i0 + 16 * t + r16;
          const unsigned long long k = epilogue_key(acc[t][r], a.ubias_col >= 0, ub, bi[t], w, 16 * t + r16);
          if (it < a.m && ranks_before(k, it, wk, wi)) {         // strictly before the worst threshold
            uint32_t lo = 0, hi = Q - 1;                         // the first threshold this score is strictly before
            while (lo < hi) {
              const uint32_t mid = (lo + hi) >> 1;
              const unsigned long long kt = tk[lr * RQ_QCAP + mid];
              bool before = k > kt;                              // ranks_before, the threshold's item read only at a tie
              if (k == kt) before = it < ti[lr * RQ_QCAP + mid];
              if (before) hi = mid; else lo = mid + 1;
            }
            atomicAdd(&cn[lr * RQ_CNT_STRIDE + lo], 1u);
          }
        }
      }
    }
  });
  __syncthreads();
  if (tid < 64) {
    const uint32_t row = rb0 + tid;
    if (row < a.nrows) {
      const uint32_t Q = a.row_nq[row], q0 = a.row_q0[row];
      uint32_t run = 0;
      for (uint32_t s = 0; s < Q; ++s) {
        run += cn[tid * RQ_CNT_STRIDE + s];
        if (run) atomicAdd(&a.rank[a.sperm[q0 + s]], run);
      }
    }
  }
}

// ---------------------------------------------------------------------
// Top-N for every user without a score matrix (hpf_recommend, -recommend).
//   topn_sweep_kernel  the same sweep (rank_sweep); a score that can still be among the best `topn` of its (user, split)
//                      is appended to that pair's candidate buffer in global memory, which the owning wave sorts and cuts
//                      back to `topn` (compaction) whenever a further tile might not fit, raising the bar for what follows
//   topn_merge_kernel  the exact top-N of a user's segments: block_topn, the selection topn_kernel runs over a row of
//                      scores, over the (key, item) lists the sweep left
// Masked items score +0.0 and stay candidates; order and padding are topn_kernel's.
// ---------------------------------------------------------------------
constexpr int TOPN_CAP_MAX = 512;     // entries of a candidate buffer at the largest fused topn (hpf_plan::topn_cap(TOPN_FUSED_MAX))

struct TopnArgs {
  const uint32_t *users;    // [n_sel] user rows of this batch
  const double   *Et, *Eb;  // [n x ld], [m x ld]
  const uint64_t *bits;     // [n_sel x words] masked items
  unsigned long long *ckey; // [n_sel x splits x cap] candidate keys of segment (user, split) ...
  uint32_t       *citem;    // ... and items
  uint32_t       *ccount;   // [n_sel x splits] entries a segment holds after the sweep: <= topn, sorted best first
  uint32_t       *out_items;   // [n_sel x topn]
  double         *out_scores;  // [n_sel x topn]
  uint32_t        n_sel, m, ld, K, words;
  uint32_t        tiles_per_split;   // 64-item tiles per blockIdx.y
  uint32_t        splits, topn, cap, lg_cap;   // cap = 1 << lg_cap <= TOPN_CAP_MAX, cap >= topn + 64
  int32_t         ubias_col, ibias_col;
};

// The lanes of ONE wave hand each other data through LDS and through the buffers they own: what was written is complete
// and visible to the wave's other lanes behind this (no other wave is waited for)
__device__ __forceinline__ void wave_sync()
{
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

// One wave sorts the c <= cap entries of a segment by (key descending, item ascending) in its LDS scratch and writes the
// best min(c, topn) back; *worst = the last key kept.  c, topn are the same in every lane.
__device__ __forceinline__ uint32_t topn_compact(unsigned long long *gk, uint32_t *gi, uint32_t c, uint32_t topn,
                                                 unsigned long long *sk, uint32_t *si, uint32_t lane, unsigned long long *worst)
{
  uint32_t P = 64; while (P < c) P <<= 1;                        // c <= cap, a power of two >= 128: P <= cap
  for (uint32_t e = lane; e < P; e += 64) { const bool ok = e < c; sk[e] = ok ? gk[e] : 0ull; si[e] = ok ? gi[e] : 0xffffffffu; }
  wave_sync();
  bitonic_sort<64>(sk, si, P, lane, [] { wave_sync(); });
  const uint32_t keep = c < topn ? c : topn;
  for (uint32_t e = lane; e < keep; e += 64) { gk[e] = sk[e]; gi[e] = si[e]; }
  *worst = keep ? sk[keep - 1] : 0ull;
  wave_sync();                                                   // the scratch is free again, the segment rewritten
  return keep;
}

// What stands between the sweep's dot product and a candidate's key, by caller.  hpf_recommend: + (E_ubias + E_ibias) with
// -bias, +0.0 where the user's mask word of the tile names the item, nothing left out.  hpf_similar (query rows and swept
// rows from ONE matrix, a.Et == a.Eb): no bias, no bit rows (a.bits is not read), and the swept row whose id is the query
// row's own is no candidate.
struct RecommendEpi {
  static constexpr bool SKIP_SELF = false;
  static __device__ __forceinline__ bool bias(const TopnArgs &a) { return a.ubias_col >= 0; }
  static __device__ __forceinline__ double ubias(const TopnArgs &a, uint32_t us, bool ok) { return user_bias(a, us, ok); }
  static __device__ __forceinline__ double ibias(const TopnArgs &a, uint32_t it, bool ok) { return item_bias(a, it, ok); }
  static __device__ __forceinline__ unsigned long long mask_word(const TopnArgs &a, uint32_t us, uint32_t tl, bool live)
  {
    return live ? a.bits[(size_t)us * a.words + tl] : 0ull;
  }
};
struct SimilarEpi {
  static constexpr bool SKIP_SELF = true;
  static __device__ __forceinline__ bool bias(const TopnArgs &) { return false; }
  static __device__ __forceinline__ double ubias(const TopnArgs &, uint32_t, bool) { return 0.0; }
  static __device__ __forceinline__ double ibias(const TopnArgs &, uint32_t, bool) { return 0.0; }
  static __device__ __forceinline__ unsigned long long mask_word(const TopnArgs &, uint32_t, uint32_t, bool) { return 0ull; }
};

// Workgroup = 4 waves = 64 users (16 per wave) x one split of the item range, as loo_rank_kernel.  A wave owns its 16
// users' segments: no other wave reads or writes them.  Per user in LDS: the entries its segment holds and the least key
// still accepted, `lo`.  lo = 0 until the first compaction (every item is a candidate), then the worst kept key + 1: items
// ascend through a split, so a later item that ties the worst kept key comes behind it and cannot be among the best.
// The body of topn_sweep_kernel (Epi = RecommendEpi) and of similar_sweep_kernel (SimilarEpi).
template <int NCH, typename Epi>
__device__ __forceinline__ void topn_sweep_body(const TopnArgs &a)
{
  __shared__ double tile[64 * LOO_LDS_STRIDE];
  __shared__ unsigned long long scr_k[4 * TOPN_CAP_MAX];          // per wave: the entries being sorted
  __shared__ uint32_t scr_i[4 * TOPN_CAP_MAX];
  __shared__ unsigned long long s_lo[64];
  __shared__ uint32_t s_cnt[64];
  __shared__ double s_ub[64];                                       // E_ubias of the user
  __shared__ uint32_t s_self[64];                                   // SKIP_SELF: the user's own row among the swept ones
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int r16 = lane & 15, kq = lane >> 4;
  const uint32_t ub0 = blockIdx.x * 64;                          // first user of this workgroup
  const uint32_t usel = ub0 + wv * 16 + r16;
  const bool uok = usel < a.n_sel;
  const uint32_t urow = uok ? a.users[usel] : 0u;
  const double *pa = a.Et + (size_t)urow * a.ld;
  const AFrag<NCH> A(pa, uok, a.K, (uint32_t)kq);
  unsigned long long *sk = scr_k + wv * TOPN_CAP_MAX;
  uint32_t *si = scr_i + wv * TOPN_CAP_MAX;

  if (tid < 64) {
    const uint32_t us = ub0 + tid;
    s_cnt[tid] = 0u; s_lo[tid] = 0ull;
    s_ub[tid] = Epi::ubias(a, us, us < a.n_sel);
    if (Epi::SKIP_SELF) s_self[tid] = us < a.n_sel ? a.users[us] : 0xffffffffu;
  }
  __syncthreads();

  rank_sweep<NCH>(A, a.Eb, a.m, a.ld, a.K, a.tiles_per_split, tile, [&](uint32_t tl, const double4_t (&acc)[4]) {
    // epilogue: register r of tile t holds local user wv 16 + kq + 4 r, item 64 tl + 16 t + r16
    const uint32_t i0 = tl * 64;
    double bi[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const uint32_t it = i0 + 16 * t + r16;
      bi[t] = Epi::ibias(a, it, it < a.m);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const uint32_t lr = wv * 16 + kq + 4 * r, us = ub0 + lr;
      const bool live = us < a.n_sel;
      const unsigned long long w = Epi::mask_word(a, us, tl, live);
      const unsigned long long lo = s_lo[lr];
      const double ub = s_ub[lr];
      const uint32_t self = Epi::SKIP_SELF ? s_self[lr] : 0u;
      uint32_t cnt = s_cnt[lr];                                  // <= cap - 64: the 64 items of a tile fit
      // first entry of the segment (a batch's buffers hold < 2^26 entries: hpf_plan::topn_batch_users)
      const uint32_t e0 = live ? (us * a.splits + blockIdx.y) << a.lg_cap : 0u;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const uint32_t it = i0 + 16 * t + r16;
        const unsigned long long k = epilogue_key(acc[t][r], Epi::bias(a), ub, bi[t], w, 16 * t + r16);
        const bool take = live && it < a.m && k >= lo && !(Epi::SKIP_SELF && it == self);
        const uint32_t grp = (uint32_t)(__ballot(take) >> (16 * kq)) & 0xffffu;   // the 16 lanes that share this user
        if (take) {
          const uint32_t slot = cnt + (uint32_t)__popc(grp & ((1u << r16) - 1u));
          a.ckey[e0 + slot] = k; a.citem[e0 + slot] = it;
        }
        cnt += (uint32_t)__popc(grp);
      }
      if (r16 == 0) s_cnt[lr] = cnt;
      __builtin_amdgcn_sched_barrier(0);                         // one user's state at a time: the K = 100 instance has no register to spare
    }
    wave_sync();
    // users of this wave whose buffer might not hold another tile: the whole wave compacts them, one after the other
    const uint32_t c16 = lane < 16 ? s_cnt[wv * 16 + lane] : 0u;
    unsigned long long full = __ballot(c16 > a.cap - 64u);
    while (full) {
      const uint32_t lr = wv * 16 + (uint32_t)__ffsll((long long)full) - 1u;
      full &= full - 1ull;
      const size_t seg = (size_t)(ub0 + lr) * a.splits + blockIdx.y;
      const uint32_t c = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_cnt[lr]);
      unsigned long long worst;
      const uint32_t keep = topn_compact(a.ckey + (seg << a.lg_cap), a.citem + (seg << a.lg_cap), c, a.topn, sk, si, (uint32_t)lane, &worst);
      if (lane == 0) { s_cnt[lr] = keep; s_lo[lr] = worst + 1ull; }    // c > cap - 64 >= topn: keep == topn
      wave_sync();
    }
  });

  // the end of the split: every segment sorted and cut to its best topn
  wave_sync();
  for (uint32_t uu = 0; uu < 16; ++uu) {
    const uint32_t lr = wv * 16 + uu, us = ub0 + lr;
    if (us >= a.n_sel) break;
    const size_t seg = (size_t)us * a.splits + blockIdx.y;
    const uint32_t c = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_cnt[lr]);
    unsigned long long worst;
    const uint32_t keep = topn_compact(a.ckey + (seg << a.lg_cap), a.citem + (seg << a.lg_cap), c, a.topn, sk, si, (uint32_t)lane, &worst);
    if (lane == 0) a.ccount[seg] = keep;
  }
}

// hpf_recommend's sweep
template <int NCH>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void topn_sweep_kernel(TopnArgs a)
{
  topn_sweep_body<NCH, RecommendEpi>(a);
}

// ---------------------------------------------------------------------
// Nearest rows in factor space (hpf_similar, -similar-items / -similar-users).
//   unit_rows_kernel     U = the rows of E over the K factor columns at unit length, for the cosine
//   similar_sweep_kernel topn_sweep_kernel's sweep and selection with query rows and swept rows from ONE matrix (U, or E
//                        itself for the dot product), the query row left out of its own list; topn_merge_kernel follows
// ---------------------------------------------------------------------
template <int NCH>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void similar_sweep_kernel(TopnArgs a)
{
  topn_sweep_body<NCH, SimilarEpi>(a);
}

// ---------------------------------------------------------------------
// The top-N users of every item (hpf_audience, -audience).
//   audience_mask_kernel   training (rating > 0) and mask-list USERS of a batch of items as bits: loo_mask_kernel over the
//                          item-major view, a long column walked by a whole workgroup
//   audience_sweep_kernel  topn_sweep_kernel's sweep and selection with the sides exchanged: the caller fills TopnArgs with
//                          Et = E[beta] (query rows: the selected items), Eb = E[theta] (swept rows: the users), m = n_users
//                          and the bias columns exchanged; topn_merge_kernel follows
// ---------------------------------------------------------------------
// The policy needs nothing beyond what RecommendEpi has: with the sides exchanged `ubias` reads E_ibias of the query item,
// `ibias` E_ubias of the swept user, epilogue_key adds their ONE parenthesised sum (commutative, so the bits of hpf_scores)
// and the mask word is the item's word of USER bits.  The type and the kernel carry their own names for launch_rank's
// error text and for profiles.
struct AudienceEpi : RecommendEpi {};

template <int NCH>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void audience_sweep_kernel(TopnArgs a)
{
  topn_sweep_body<NCH, AudienceEpi>(a);
}

constexpr uint32_t AUDIENCE_LONG_MIN = 4096;     // users of a column from which a workgroup walks it, not a wave

// Bit u of row b is set when user u is masked for item items[b]: masked_items over the item-major view (colptr, usr, val)
// and the caller's list.  Workgroups of four waves.  First a wave per item of the batch: its list and, where the column has
// fewer than AUDIENCE_LONG_MIN users, its column.  Then a workgroup per item: the long columns, 256 users a step (item
// columns are heavy-tailed: a wave alone would walk the longest in thousands of dependent steps while the rest of the
// launch has long finished).  Rows are `words` 64-bit words, written as dwords; every usr[j] is below 64 words.
__global__ __launch_bounds__(256) void audience_mask_kernel(const uint32_t *items, uint32_t n_sel, const int64_t *colptr,
                                                            const uint32_t *usr, const uint8_t *val, const uint64_t *mask_ptr,
                                                            const uint32_t *mask_users, uint32_t *bits, uint32_t words)
{
  const int lane = threadIdx.x & 63;
  const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
  for (uint32_t b = wave; b < n_sel; b += nwaves) {
    uint32_t *row = bits + (size_t)b * words * 2;
    const uint32_t i = items[b];
    const bool is_long = colptr[i + 1] - colptr[i] >= (int64_t)AUDIENCE_LONG_MIN;
    masked_items(i, b, lane, is_long ? nullptr : colptr, usr, val, mask_ptr, mask_users,
                 [&](uint32_t u) { atomicOr(&row[u >> 5], 1u << (u & 31u)); });
  }
  for (uint32_t b = blockIdx.x; b < n_sel; b += gridDim.x) {
    const uint32_t i = items[b];
    const int64_t j0 = colptr[i], j1 = colptr[i + 1];
    if (j1 - j0 < (int64_t)AUDIENCE_LONG_MIN) continue;
    uint32_t *row = bits + (size_t)b * words * 2;
    for (int64_t j = j0 + threadIdx.x; j < j1; j += blockDim.x)
      if (!val || val[j] > 0) atomicOr(&row[usr[j] >> 5], 1u << (usr[j] & 31u));
  }
}

constexpr int UNIT_G = 16;            // lanes per row: one DPP row; 16 lanes x 16 bytes = two 128-byte lines per step

// U[r, k] = x_k / sqrt(sum_k x_k^2), x_k = E[r, k] 2^-e with 2^e the power of two of the row's largest entry: x_k is exact
// (unless it falls below the normal range, 2^-1022 of the largest entry, where it no longer matters), the largest is in
// [1, 2), every square is <= 4 and the sum <= 4 K; a square that underflows adds nothing.  So a row scaled by a power of
// two has the same U, bit for bit.  sqrt and / are the correctly rounded ones.  Lane g of a row's 16 adds the squares of
// columns 2 g, 2 g + 1, 2 g + 32, ... in that order, group_sum adds the 16: the order depends on K alone.  An all-zero row
// gives zeros; columns >= K (bias, padding) are written as zeros.  E finite and >= +0.0, ld even.
__global__ __launch_bounds__(256) void unit_rows_kernel(const double *E, double *U, uint32_t rows, uint32_t ld, uint32_t K)
{
  const uint32_t g = threadIdx.x & (UNIT_G - 1);
  const uint32_t per_block = 256 / UNIT_G;
  for (uint32_t r = blockIdx.x * per_block + threadIdx.x / UNIT_G; r < rows; r += gridDim.x * per_block) {   // the same r in a row's 16 lanes
    const double *pe = E + (size_t)r * ld;
    double *pu = U + (size_t)r * ld;
    auto piece = [&](uint32_t c) {                               // columns c, c + 1 of the row; c is even and ld is even
      double2 v = *(const double2 *)(pe + c);
      if (c + 1 >= K) v.y = 0.0;
      return v;
    };
    double mx = 0.0;
    for (uint32_t c = 2 * g; c < K; c += 2 * UNIT_G) { const double2 v = piece(c); mx = fmax(mx, fmax(v.x, v.y)); }
    mx = group_max<UNIT_G>(mx);
    int e = 0;
    (void)frexp(mx, &e);                                         // mx = f 2^e, f in [0.5, 1): the largest x is 2 f
    double s = 0.0;
    for (uint32_t c = 2 * g; c < K; c += 2 * UNIT_G) {
      const double2 v = piece(c);
      const double x = ldexp(v.x, 1 - e), y = ldexp(v.y, 1 - e);
      s += x * x; s += y * y;
    }
    const double nrm = sqrt(group_sum<UNIT_G>(s));
    for (uint32_t c = 2 * g; c < ld; c += 2 * UNIT_G) {
      double2 u = make_double2(0.0, 0.0);
      if (c < K && mx > 0.0) {
        const double2 v = piece(c);
        u.x = ldexp(v.x, 1 - e) / nrm; u.y = ldexp(v.y, 1 - e) / nrm;
      }
      *(double2 *)(pu + c) = u;
    }
  }
}

// The segments of one user as block_topn's list: entry i is slot i % cap of segment i / cap, present when the slot is below
// the segment's count.  Segments are sorted and cover ascending item ranges, so walking i upwards meets equal keys in
// ascending item order -- which is all block_topn asks of a list.
struct SegmentEntries {
  const unsigned long long *gk; const uint32_t *gi, *gc;          // the user's keys, items and counts per segment
  uint32_t L, cap, lg_cap;                                       // L = splits x cap <= 1025 x 512
  __device__ __forceinline__ uint32_t n() const { return L; }
  __device__ __forceinline__ bool present(uint32_t i) const { return i < L && (i & (cap - 1u)) < gc[i >> lg_cap]; }
  __device__ __forceinline__ unsigned long long key(uint32_t i) const { return gk[i]; }
  __device__ __forceinline__ uint32_t item(uint32_t i) const { return gi[i]; }
};

// One workgroup per user: block_topn over what the sweep left of it.  NP = pow2 >= topn; Ne = the entries a list has before
// its padding: min(topn, m) for hpf_recommend, min(topn, m - 1) for hpf_similar (the row itself is no candidate).
__global__ __launch_bounds__(256) void topn_merge_kernel(TopnArgs a, uint32_t NP, uint32_t Ne)
{
  const uint32_t b = blockIdx.x;
  if (b >= a.n_sel) return;
  const size_t e0 = ((size_t)b * a.splits) << a.lg_cap;
  block_topn(SegmentEntries{a.ckey + e0, a.citem + e0, a.ccount + (size_t)b * a.splits, a.splits << a.lg_cap, a.cap, a.lg_cap},
             a.topn, Ne, NP, a.out_items + (size_t)b * a.topn, a.out_scores + (size_t)b * a.topn);
}

// ---------------------------------------------------------------------
// Posterior moments of a score and the optimistic top-N (hpf_score_moments, hpf_recommend_ucb).
// Under the mean-field posterior Var(theta_uk beta_ik) = vt s + q vb with q = E[theta]^2, vt = q / shape(theta),
// p = E[beta]^2, vb = p / shape(beta), s = p + vb: the variance of a score is the dot product of the derived rows
//   X_u = [ vt_0 .. vt_{K-1} | q_0 .. q_{K-1}   | (bias:) Var ubias_u, 1.0 ]
//   Y_i = [ s_0 .. s_{K-1}   | vb_0 .. vb_{K-1} | (bias:) 1.0, Var ibias_i ]
// taken by the chain hpf_scores issues for C = 2 K + 2 * bias columns.  Every operation is one fp64 operation, nothing is
// contracted, / and sqrt are the correctly rounded ones.
//   moment_rows_kernel   X of a batch of selected users, or Y of every item
//   ucb_sweep_kernel     topn_sweep_kernel's sweep and selection with two chains per output, ordered by mean + z sd
//   pair_moments_kernel  mean and variance of single pairs, from the sweep's arithmetic
// ---------------------------------------------------------------------
// e^2 / shape: the variance of a Gamma from its expectation and its shape; *sq = e^2
__device__ __forceinline__ double gamma_var(double e, double shape, double *sq)
{
#pragma clang fp contract(off)
  const double q = e * e;
  *sq = q;
  return q / shape;
}
// Column c of the derived row of a row of E and S (shapes): X where item_side is false, Y where it is true.  bias_col < 0:
// no bias columns.  Columns from C on are the padding: 0.0.
__device__ __forceinline__ double moment_column(const double *e, const double *s, uint32_t c, uint32_t K, int32_t bias_col, bool item_side)
{
#pragma clang fp contract(off)
  double q;
  if (c < 2 * K) {
    const uint32_t k = c < K ? c : c - K;
    const double v = gamma_var(e[k], s[k], &q);
    if (!item_side) return c < K ? v : q;                        // vt | q
    if (c >= K) return v;                                        // vb
    const double sum = q + v;                                    // s = p + vb
    return sum;
  }
  if (bias_col < 0 || c > 2 * K + 1) return 0.0;
  const bool own = (c == 2 * K) != item_side;                    // X: Var ubias, 1.0; Y: 1.0, Var ibias
  return own ? gamma_var(e[bias_col], s[bias_col], &q) : 1.0;
}

struct MomentRowsArgs {
  const double   *E, *S;     // [side rows x ld] expectations and shapes of the side
  const uint32_t *sel;       // [rows] the side's rows to derive from, or null: rows 0 .. rows - 1
  double         *out;       // [rows x ldx]
  uint32_t        rows, ld, ldx, K;
  int32_t         bias_col;  // -1 without -bias
  uint32_t        item_side;
};

// a thread per element of the derived rows, the padding columns included
__global__ __launch_bounds__(256) void moment_rows_kernel(MomentRowsArgs a)
{
  const uint64_t n = (uint64_t)a.rows * a.ldx;
  for (uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (uint64_t)gridDim.x * 256) {
    const uint32_t r = (uint32_t)(e / a.ldx), c = (uint32_t)(e % a.ldx);
    const size_t src = (size_t)(a.sel ? a.sel[r] : r) * a.ld;
    a.out[e] = moment_column(a.E + src, a.S + src, c, a.K, a.bias_col, a.item_side != 0);
  }
}

// mean + z sd of a score, three operations
__device__ __forceinline__ double ucb_value(double mean, double var, double z)
{
#pragma clang fp contract(off)
  const double sd = sqrt(var);
  const double t = z * sd;
  return mean + t;
}

struct UcbArgs : TopnArgs {
  const double *X;          // [n_sel x ldx] derived rows of this batch's users
  const double *Y;          // [m x ldx] derived rows of the items
  uint32_t      ldx, C;     // stride and columns of the derived rows
  uint32_t      mean_steps; // MFMAs of the mean chain: the derived columns begin at column 4 mean_steps of the concatenation
  double        z;
};

// rank_sweep over the concatenation [the K columns of E, zeros up to 4 mean_steps | the C derived columns]: the same LDS
// staging and MFMA order, the A rows read per step (rank_sweep's NCH == 0 route: K + C columns do not fit in registers).
// After mean_steps MFMAs the accumulators are the scores hpf_scores returns; they are set aside and the chain starts again
// from zero over the derived columns.  epi(tl, mean, var) gets both sets in rank_sweep's register layout.  A function of
// its own, not a parameter of rank_sweep: the kernels that call that one keep their code.
template <typename Epi>
__device__ __forceinline__ void moment_sweep(const UcbArgs &a, const double *pa, const double *px, bool row_ok, double *tile, Epi &&epi)
{
  const int tid = threadIdx.x, lane = tid & 63;
  const int r16 = lane & 15, kq = lane >> 4;
  const uint32_t K = a.K, K4 = 4u * a.mean_steps, KT = K4 + a.C;
  const uint32_t nsteps = (KT + 3) / 4;
  const uint32_t ntiles = (a.m + 63) / 64;
  const uint32_t t0 = blockIdx.y * a.tiles_per_split, t1 = min(ntiles, t0 + a.tiles_per_split);
  const uint32_t nchunks = (KT + LOO_KC - 1) / LOO_KC;

  // this thread's four 16-byte pieces of a 64 x 32 chunk, as in rank_sweep; K4, C, ld and ldx are even: a piece lies in one part
  double2 pre[4];
  auto fetch = [&](uint32_t tile_i, uint32_t chunk) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t p = (uint32_t)tid + 256u * j, row = p >> 4, c = chunk * LOO_KC + 2u * (p & 15u);
      const uint32_t it = tile_i * 64 + row;
      double2 v = make_double2(0.0, 0.0);
      if (it < a.m) {
        if (c < K) {
          v = *(const double2 *)(a.Eb + (size_t)it * a.ld + c);
          if (c + 1 >= K) v.y = 0.0;
        } else if (c >= K4 && c < KT) v = *(const double2 *)(a.Y + (size_t)it * a.ldx + (c - K4));
      }
      pre[j] = v;
    }
  };
  auto a_load = [&](uint32_t s) {
    const uint32_t k = 4u * s + kq;
    if (!row_ok) return 0.0;
    if (k < K4) return k < K ? pa[k] : 0.0;
    return k < KT ? px[k - K4] : 0.0;
  };
  if (t0 < t1) fetch(t0, 0);
  for (uint32_t tl = t0; tl < t1; ++tl) {
    double4_t acc[4], mean[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = mean[t] = (double4_t){0.0, 0.0, 0.0, 0.0};
    for (uint32_t ch = 0; ch < nchunks; ++ch) {
      __syncthreads();                                         // the previous chunk has been read
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t p = (uint32_t)tid + 256u * j;
        *(double2 *)&tile[(p >> 4) * LOO_LDS_STRIDE + 2u * (p & 15u)] = pre[j];
      }
      __syncthreads();
      if (ch + 1 < nchunks) fetch(tl, ch + 1);
      else if (tl + 1 < t1) fetch(tl + 1, 0);
      for (uint32_t s = 0; s < 8 && ch * 8 + s < nsteps; ++s) {
        if (ch * 8 + s == a.mean_steps) {                      // the mean chain has ended
#pragma unroll
          for (int t = 0; t < 4; ++t) { mean[t] = acc[t]; acc[t] = (double4_t){0.0, 0.0, 0.0, 0.0}; }
        }
        const double av = a_load(ch * 8 + s);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const double bv = tile[(16 * t + r16) * LOO_LDS_STRIDE + 4 * s + kq];
          acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[t], 0, 0, 0);
        }
      }
    }
    epi(tl, mean, acc);
  }
}

// hpf_recommend_ucb's sweep: topn_sweep_body's selection (candidate buffers, compaction, lo, a wave owning 16 users;
// topn_merge_kernel follows) behind moment_sweep.  A candidate's key is that of mean + z sd, with the mean's
// + (E_ubias + E_ibias) as epilogue_key adds it and +0.0 for a masked item.  z >= 0 and both moments >= +0.0: the key
// order is the order of the values.  The body is topn_sweep_body's with the second accumulator set, spelled out so that
// the three kernels built from that one keep their code.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void ucb_sweep_kernel(UcbArgs a)
{
  __shared__ double tile[64 * LOO_LDS_STRIDE];
  __shared__ unsigned long long scr_k[4 * TOPN_CAP_MAX];          // per wave: the entries being sorted
  __shared__ uint32_t scr_i[4 * TOPN_CAP_MAX];
  __shared__ unsigned long long s_lo[64];
  __shared__ uint32_t s_cnt[64];
  __shared__ double s_ub[64];                                       // E_ubias of the user
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int r16 = lane & 15, kq = lane >> 4;
  const uint32_t ub0 = blockIdx.x * 64;                          // first user of this workgroup
  const uint32_t usel = ub0 + wv * 16 + r16;
  const bool uok = usel < a.n_sel;
  const double *pa = a.Et + (size_t)(uok ? a.users[usel] : 0u) * a.ld;
  const double *px = a.X + (size_t)(uok ? usel : 0u) * a.ldx;
  unsigned long long *sk = scr_k + wv * TOPN_CAP_MAX;
  uint32_t *si = scr_i + wv * TOPN_CAP_MAX;

  if (tid < 64) {
    const uint32_t us = ub0 + tid;
    s_cnt[tid] = 0u; s_lo[tid] = 0ull;
    s_ub[tid] = user_bias(a, us, us < a.n_sel);
  }
  __syncthreads();

  moment_sweep(a, pa, px, uok, tile, [&](uint32_t tl, const double4_t (&mean)[4], const double4_t (&var)[4]) {
    // epilogue: register r of tile t holds local user wv 16 + kq + 4 r, item 64 tl + 16 t + r16
    const uint32_t i0 = tl * 64;
    double bi[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const uint32_t it = i0 + 16 * t + r16;
      bi[t] = item_bias(a, it, it < a.m);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const uint32_t lr = wv * 16 + kq + 4 * r, us = ub0 + lr;
      const bool live = us < a.n_sel;
      const unsigned long long w = live ? a.bits[(size_t)us * a.words + tl] : 0ull;
      const unsigned long long lo = s_lo[lr];
      const double ub = s_ub[lr];
      uint32_t cnt = s_cnt[lr];                                  // <= cap - 64: the 64 items of a tile fit
      const uint32_t e0 = live ? (us * a.splits + blockIdx.y) << a.lg_cap : 0u;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const uint32_t it = i0 + 16 * t + r16;
        double mu = mean[t][r];
        if (a.ubias_col >= 0) mu += ub + bi[t];                  // s += Eb_u + Eb_i
        double v = ucb_value(mu, var[t][r], a.z);
        if ((w >> (16 * t + r16)) & 1ull) v = 0.0;
        const unsigned long long k = score_key(v);
        const bool take = live && it < a.m && k >= lo;
        const uint32_t grp = (uint32_t)(__ballot(take) >> (16 * kq)) & 0xffffu;   // the 16 lanes that share this user
        if (take) {
          const uint32_t slot = cnt + (uint32_t)__popc(grp & ((1u << r16) - 1u));
          a.ckey[e0 + slot] = k; a.citem[e0 + slot] = it;
        }
        cnt += (uint32_t)__popc(grp);
      }
      if (r16 == 0) s_cnt[lr] = cnt;
    }
    wave_sync();
    // users of this wave whose buffer might not hold another tile: the whole wave compacts them, one after the other
    const uint32_t c16 = lane < 16 ? s_cnt[wv * 16 + lane] : 0u;
    unsigned long long full = __ballot(c16 > a.cap - 64u);
    while (full) {
      const uint32_t lr = wv * 16 + (uint32_t)__ffsll((long long)full) - 1u;
      full &= full - 1ull;
      const size_t seg = (size_t)(ub0 + lr) * a.splits + blockIdx.y;
      const uint32_t c = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_cnt[lr]);
      unsigned long long worst;
      const uint32_t keep = topn_compact(a.ckey + (seg << a.lg_cap), a.citem + (seg << a.lg_cap), c, a.topn, sk, si, (uint32_t)lane, &worst);
      if (lane == 0) { s_cnt[lr] = keep; s_lo[lr] = worst + 1ull; }    // c > cap - 64 >= topn: keep == topn
      wave_sync();
    }
  });

  // the end of the split: every segment sorted and cut to its best topn
  wave_sync();
  for (uint32_t uu = 0; uu < 16; ++uu) {
    const uint32_t lr = wv * 16 + uu, us = ub0 + lr;
    if (us >= a.n_sel) break;
    const size_t seg = (size_t)us * a.splits + blockIdx.y;
    const uint32_t c = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_cnt[lr]);
    unsigned long long worst;
    const uint32_t keep = topn_compact(a.ckey + (seg << a.lg_cap), a.citem + (seg << a.lg_cap), c, a.topn, sk, si, (uint32_t)lane, &worst);
    if (lane == 0) a.ccount[seg] = keep;
  }
}

struct PairMomentArgs {
  const uint32_t *u, *i;       // [cnt] the pairs; per > 0: pair p is (u[p / per], i[p]) -- the lists of hpf_recommend_ucb -- and
  uint32_t        per;         //   an item 0xffffffff is a list's padding: 0.0 in every output
  uint64_t        cnt;
  const double   *Et, *Eb, *St, *Sb;   // [n x ld], [m x ld] expectations and shapes
  double         *out_mean, *out_var, *out_ucb;   // [cnt]; each may be null
  double          z;           // out_ucb = mean + z sd
  uint32_t        ld, K, C;
  uint32_t        mean_steps, var_steps;
  int32_t         ubias_col, ibias_col;   // -1 without -bias
};

// A wave takes 16 pairs: the A rows are the pairs' user rows, the B rows their item rows, and of the 16 x 16 tile the
// diagonal is kept (as loo_rank_kernel takes its threshold) -- the MFMAs, operands and order of the sweep, so a pair's
// mean and variance are the sweep's bits and those of hpf_scores.  The derived columns are formed on the way
// (moment_column: the operations of moment_rows_kernel, so the same bits).
__global__ __launch_bounds__(256) void pair_moments_kernel(PairMomentArgs a)
{
  const int lane = threadIdx.x & 63, r16 = lane & 15, kq = lane >> 4;
  const uint64_t wave = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 6, nwaves = ((uint64_t)gridDim.x * 256) >> 6;
  for (uint64_t p0 = wave * 16; p0 < a.cnt; p0 += nwaves * 16) {
    const uint64_t p = p0 + r16;
    uint32_t it = p < a.cnt ? a.i[p] : 0xffffffffu;
    const bool ok = p < a.cnt && !(a.per && it == 0xffffffffu);
    const uint32_t u = ok ? a.u[a.per ? p / a.per : p] : 0u;
    if (!ok) it = 0u;
    const double *et = a.Et + (size_t)u * a.ld, *st = a.St + (size_t)u * a.ld;
    const double *eb = a.Eb + (size_t)it * a.ld, *sb = a.Sb + (size_t)it * a.ld;
    double4_t mean = (double4_t){0.0, 0.0, 0.0, 0.0}, var = mean;
    for (uint32_t s = 0; s < a.mean_steps; ++s) {
      const uint32_t k = 4u * s + kq;
      const bool in = ok && k < a.K;
      mean = __builtin_amdgcn_mfma_f64_16x16x4f64(in ? et[k] : 0.0, in ? eb[k] : 0.0, mean, 0, 0, 0);
    }
    for (uint32_t s = 0; s < a.var_steps; ++s) {
      const uint32_t c = 4u * s + kq;
      const bool in = ok && c < a.C;
      const double xv = in ? moment_column(et, st, c, a.K, a.ubias_col, false) : 0.0;
      const double yv = in ? moment_column(eb, sb, c, a.K, a.ibias_col, true) : 0.0;
      var = __builtin_amdgcn_mfma_f64_16x16x4f64(xv, yv, var, 0, 0, 0);
    }
    // D[i][i] for i = kq + 4 r sits in register r of lane i + 16 kq: the lanes with r16 % 4 == kq hold their own pair's
    if ((r16 & 3) == kq) {
      const int r = r16 >> 2;
      double mu = r == 0 ? mean[0] : r == 1 ? mean[1] : r == 2 ? mean[2] : mean[3];
      double vr = r == 0 ? var[0] : r == 1 ? var[1] : r == 2 ? var[2] : var[3];
      if (ok && a.ubias_col >= 0) mu += et[a.ubias_col] + eb[a.ibias_col];        // s += Eb_u + Eb_i
      if (!ok) mu = vr = 0.0;
      if (p < a.cnt) {
        if (a.out_mean) a.out_mean[p] = mu;
        if (a.out_var) a.out_var[p] = vr;
        if (a.out_ucb) a.out_ucb[p] = ok ? ucb_value(mu, vr, a.z) : 0.0;
      }
    }
  }
}

// ---------------------------------------------------------------------
// One posterior draw of a side's rows (hpf_sample_state, hpf_recommend_thompson).
//   gamma_rows_kernel   out[r][c] = a Gamma(S, S / E) variate (hpf_rng::gamma_sample) for the K factor columns and the
//                       side's own bias column, 0.0 for every other column of the row: the junk column and the padding up
//                       to ld.  The rows stand in for rows of E behind topn_sweep_kernel, whose chain is padded with zeros.
//                       A variate is a function of (seed, draw, object, the row's id on its side, column) alone.
//   sample_pack_kernel  the sampled rows as hpf_sample_state hands them out: K factor columns, then the bias
// The rejection loop of the sampler diverges inside a wave (about one lane in twenty tries again): a plain bounded loop in
// registers, nothing crosses lanes, no LDS.
// ---------------------------------------------------------------------
struct GammaRowsArgs {
  const double   *E, *S;     // [side rows x ld] expectations and shapes of the side
  const uint32_t *sel;       // [rows] the side's rows to draw, also the counter's row ids; or null: rows 0 .. rows - 1
  double         *out;       // [rows x ld]
  uint64_t        seed;
  uint32_t        rows, ld, K;
  int32_t         bias_col;  // the side's own bias column, -1 without -bias
  uint32_t        object;    // 0: user side, 1: item side
  uint32_t        draw;
};

// a thread per element of the output rows, the columns that are not sampled included
__global__ __launch_bounds__(256) void gamma_rows_kernel(GammaRowsArgs a)
{
  const uint64_t n = (uint64_t)a.rows * a.ld;
  for (uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (uint64_t)gridDim.x * 256) {
    const uint32_t r = (uint32_t)(e / a.ld), c = (uint32_t)(e % a.ld);
    double v = 0.0;
    if (c < a.K || (int32_t)c == a.bias_col) {
      const uint32_t id = a.sel ? a.sel[r] : r;
      const size_t src = (size_t)id * a.ld + c;
      v = hpf_rng::gamma_sample(a.seed, a.draw, a.object, id, c, a.E[src], a.S[src], nullptr);
    }
    a.out[e] = v;
  }
}

// dense [rows x C], C = K + (bias_col >= 0): columns 0 .. K - 1 of a sampled row, then its bias column
__global__ __launch_bounds__(256) void sample_pack_kernel(const double *rows_ld, double *out, uint64_t rows, uint32_t ld, uint32_t K, int32_t bias_col)
{
  const uint32_t C = K + (bias_col >= 0 ? 1u : 0u);
  const uint64_t n = rows * C;
  for (uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (uint64_t)gridDim.x * 256) {
    const uint64_t r = e / C; const uint32_t c = (uint32_t)(e % C);
    out[e] = rows_ld[r * ld + (c < K ? c : (uint32_t)bias_col)];
  }
}

// ---------------------------------------------------------------------
// Diversified top-N: greedy maximal marginal relevance over a user's candidate pool (hpf_recommend_diverse; DESIGN.md
// section 4l).
//   mmr_kernel   a workgroup per selected user, a persistent grid.  Gram phase: the cosines of the pool's items -- rows of U
//                (unit_rows_kernel) gathered by id, the MFMA chain of score_tile_kernel per output -- into the workgroup's
//                slab of device memory.  Selection phase: thread j owns pool entry j; per round a key, an arg-max over the
//                workgroup (ties to the smaller j) and one row of the slab.
// Every line of the selection is one fp64 operation, nothing contracted, the division the correctly rounded one.
// ---------------------------------------------------------------------
struct MmrArgs {
  const double   *U;            // [rows x ld] unit rows of E[beta]
  const uint32_t *pool_items;   // [n_sel x pool] hpf_recommend's lists at topn = pool
  const double   *pool_scores;  // [n_sel x pool]
  double         *slab;         // [gridDim.x x Pp x Pp]
  uint32_t       *out_items;    // [n_sel x topn]
  double         *out_scores, *out_maxsim, *out_mmr;
  double          lambda;
  uint32_t        rows, ld, K, n_sel, pool, topn, Pp;
};

__global__ __launch_bounds__(256) void mmr_kernel(MmrArgs a)
{
#pragma clang fp contract(off)
  constexpr uint32_t W = hpf_plan::DIVERSE_WAVES, STRIP = hpf_plan::DIVERSE_STRIP;
  static_assert(W * 64 == hpf_plan::DIVERSE_POOL_MAX, "a thread per pool entry");
  __shared__ uint32_t s_item[hpf_plan::DIVERSE_POOL_MAX];
  __shared__ uint32_t s_P;
  __shared__ double   s_r0;
  __shared__ double   s_key[2][W];
  __shared__ uint32_t s_pos[2][W];
  static_assert(sizeof(s_item) + sizeof(s_P) + 4 /* s_r0 is aligned to 8 */ + sizeof(s_r0) + sizeof(s_key) + sizeof(s_pos) == hpf_plan::DIVERSE_LDS_BYTES, "DiversePlan::lds_bytes");
  const uint32_t j = threadIdx.x, lane = j & 63u, wv = j >> 6, r16 = lane & 15u, kq = lane >> 4;
  double *G = a.slab + (size_t)blockIdx.x * a.Pp * a.Pp;
  const double om = 1.0 - a.lambda;
  for (uint32_t b = blockIdx.x; b < a.n_sel; b += gridDim.x) {
    // ---- the pool: the prefix of the list whose scores are > +0.0 (and whose items exist: nothing is gathered out of U)
    uint32_t c = 0xffffffffu; double r = 0.0;
    if (j < a.pool) { c = a.pool_items[(size_t)b * a.pool + j]; r = a.pool_scores[(size_t)b * a.pool + j]; }
    const bool in = j < a.pool && r > 0.0 && c < a.rows;
    __syncthreads();                                             // the user before is over: its P, its slab, its last round
    if (j == 0) { s_P = a.pool; s_r0 = r; }
    __syncthreads();
    if (!in && j < a.pool) atomicMin(&s_P, j);
    s_item[j] = in ? c : 0u;
    __syncthreads();
    const uint32_t P = s_P, side = (P + 15u) / 16u;

    // ---- Gram phase: tile (ti, tj) = U[pool rows of ti] x U[pool rows of tj]^T, strips of STRIP tiles of one tile row
    for (uint32_t s = wv; s < hpf_plan::diverse_strips(side); s += W) {
      const hpf_plan::DiverseStrip st = hpf_plan::diverse_strip(s, side);
      const uint32_t ti = st.ti, tj0 = st.tj0;
      const uint32_t ja = ti * 16 + r16;
      const bool oka = ja < P;
      const double *pa = a.U + (size_t)s_item[ja & (hpf_plan::DIVERSE_POOL_MAX - 1)] * a.ld;
      const double *pb[STRIP]; bool okb[STRIP];
#pragma unroll
      for (uint32_t t = 0; t < STRIP; ++t) {
        const uint32_t jb = (tj0 + t) * 16 + r16;
        okb[t] = tj0 + t < side && jb < P;
        pb[t] = a.U + (size_t)s_item[jb & (hpf_plan::DIVERSE_POOL_MAX - 1)] * a.ld;
      }
      double4_t acc[STRIP];
#pragma unroll
      for (uint32_t t = 0; t < STRIP; ++t) acc[t] = (double4_t){0.0, 0.0, 0.0, 0.0};
      for (uint32_t k0 = 0; k0 < a.K; k0 += 4) {
        const uint32_t k = k0 + kq;
        const bool okk = k < a.K;
        const double av = (okk && oka) ? pa[k] : 0.0;              // A[i = lane%16][k = lane/16]
#pragma unroll
        for (uint32_t t = 0; t < STRIP; ++t) {
          const double bv = (okk && okb[t]) ? pb[t][k] : 0.0;     // B[k = lane/16][j = lane%16]
          acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[t], 0, 0, 0);
        }
      }
      // register q holds D[i = lane/16 + 4 q][j = lane%16]; rows and columns < side * 16 <= Pp stay inside the slab
#pragma unroll
      for (uint32_t t = 0; t < STRIP; ++t) {
        if (tj0 + t >= side) continue;
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q)
          G[(size_t)(ti * 16 + kq + 4 * q) * a.Pp + (tj0 + t) * 16 + r16] = acc[t][q];
      }
    }
    __syncthreads();

    // ---- selection phase
    bool alive = j < P;
    const double rel = alive ? r / s_r0 : 0.0;
    double pen = 0.0;
    const uint32_t picks = a.topn < P ? a.topn : P;
    const size_t o0 = (size_t)b * a.topn;
    for (uint32_t t = 0; t < picks; ++t) {
      const double lr = a.lambda * rel;
      const double op = om * pen;
      const double key = lr - op;
      double bk = alive ? key : -INFINITY; uint32_t bj = alive ? j : 0xffffffffu;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const double ok = __shfl_xor(bk, d, 64);
        const uint32_t oj = (uint32_t)__shfl_xor((int)bj, d, 64);
        if (oj != 0xffffffffu && (bj == 0xffffffffu || ok > bk || (ok == bk && oj < bj))) { bk = ok; bj = oj; }
      }
      const uint32_t buf = t & 1u;
      if (lane == 0) { s_key[buf][wv] = bk; s_pos[buf][wv] = bj; }
      __syncthreads();                                           // two buffers: round t + 1 writes the other one
      bk = s_key[buf][0]; bj = s_pos[buf][0];
#pragma unroll
      for (uint32_t w = 1; w < W; ++w) {
        const double ok = s_key[buf][w]; const uint32_t oj = s_pos[buf][w];
        if (oj != 0xffffffffu && (bj == 0xffffffffu || ok > bk || (ok == bk && oj < bj))) { bk = ok; bj = oj; }
      }
      if (j == bj) {
        a.out_items[o0 + t] = c; a.out_scores[o0 + t] = r; a.out_maxsim[o0 + t] = pen; a.out_mmr[o0 + t] = key;
        alive = false;
      }
      if (alive && bj < P) pen = fmax(pen, G[(size_t)bj * a.Pp + j]);   // one entry at least is alive in every round: bj < P
    }
    for (uint32_t t = picks + j; t < a.topn; t += 256) {
      a.out_items[o0 + t] = 0xffffffffu; a.out_scores[o0 + t] = 0.0; a.out_maxsim[o0 + t] = 0.0; a.out_mmr[o0 + t] = 0.0;
    }
  }
}

// ---------------------------------------------------------------------
// Why a score is what it is (hpf_explain, hpf_factor_top; -explain, -topic-items / -topic-users).
//   explain_kernel      the T largest of the K (+ 2) non-negative terms of a pair's score, a wave per pair
//   transpose_cols_kernel  a batch of columns of E as rows, through LDS; topn_kernel (block_topn) then takes the heaviest
//                       rows of each column from a contiguous row
// ---------------------------------------------------------------------
struct ExplainArgs {
  const uint32_t *u, *i;       // [cnt] the pairs
  uint64_t        cnt;
  const double   *Et, *Eb;     // [n x ld], [m x ld]
  uint32_t       *out_factor;  // [cnt x T]
  double         *out_contrib; // [cnt x T]
  uint32_t        ld, K, T, run;          // run: consecutive pairs a wave takes per trip (hpf_plan::EXPLAIN_RUN)
  int32_t         ubias_col, ibias_col;   // K and K + 1 with -bias (the terms' numbers), -1 without
};

// the largest key of the wave, in every lane (keys are unsigned 64-bit patterns: score_key)
__device__ __forceinline__ unsigned long long wave_max_key(unsigned long long k)
{
  auto mx = [](unsigned long long a, double b) { const unsigned long long kb = (unsigned long long)__double_as_longlong(b); return a > kb ? a : kb; };
  auto as_d = [](unsigned long long a) { return __longlong_as_double((long long)a); };     // bits only: a move, no arithmetic
  k = mx(k, dpp_mov<0xB1>(as_d(k)));
  k = mx(k, dpp_mov<0x4E>(as_d(k)));
  k = mx(k, dpp_mov<0x141>(as_d(k)));
  k = mx(k, dpp_mov<0x140>(as_d(k)));
  k = mx(k, __shfl_xor(as_d(k), 16, 64));
  k = mx(k, __shfl_xor(as_d(k), 32, 64));
  return k;
}
// the smallest id of the wave, in every lane
__device__ __forceinline__ uint32_t wave_min_id(uint32_t v)
{
  auto mn = [](uint32_t a, int b) { return a < (uint32_t)b ? a : (uint32_t)b; };
  v = mn(v, __builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, true));
  v = mn(v, __builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, true));
  v = mn(v, __builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xf, 0xf, true));
  v = mn(v, __builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xf, 0xf, true));
  v = mn(v, __shfl_xor((int)v, 16, 64));
  v = mn(v, __shfl_xor((int)v, 32, 64));
  return v;
}

// One wave per pair; lane l holds the terms l + 64 t, t < R: c_k = E[theta_u k] * E[beta_i k] for k < K -- ONE IEEE
// multiplication, nothing added to it, so the double handed out is the host's product bit for bit -- and with -bias the
// copies E[ubias_u] (term K) and E[ibias_i] (term K + 1), the reference's K + 2 layout (hgaprec.cc:1347-1353).  Then up to T
// rounds: every lane offers the best of its live terms (the first of equal keys: the smallest id a lane holds), the wave
// takes the largest key (wave_max_key) and among the lanes that offered it the smallest id (wave_min_id) -- ranks_before's
// order -- and the lane that owns the winner retires it: a bit of a per-lane mask, so no register is indexed by a
// run-time value.  Lane r keeps the result of round r and the wave stores its T results at once; rounds beyond the terms
// a score has leave the padding (0xffffffff, 0.0).  A wave walks `run` consecutive pairs and reloads the user's row only
// when the user changes (a recommend list is a run of one user).  Reads E only.
template <int R>
__global__ __launch_bounds__(256) void explain_kernel(ExplainArgs a)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t w0 = (uint64_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
  const uint64_t nw = ((uint64_t)gridDim.x * blockDim.x) >> 6;
  const uint32_t K = a.K, C = K + (a.ubias_col >= 0 ? 2u : 0u);
  const uint32_t rounds = a.T < C ? a.T : C;
  uint32_t live0 = 0;                                      // bit t: term lane + 64 t exists
#pragma unroll
  for (int t = 0; t < R; ++t) live0 |= (lane + 64u * t < C) ? (1u << t) : 0u;

  for (uint64_t base = w0 * a.run; base < a.cnt; base += nw * a.run) {
    double th[R];
    uint32_t cur_u = 0xffffffffu;
    for (uint32_t j = 0; j < a.run && base + j < a.cnt; ++j) {
      const uint64_t p = base + j;
      const uint32_t u = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.u[p]), it = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.i[p]);
      if (u != cur_u) {                                    // wave-uniform
        const double *et = a.Et + (size_t)u * a.ld;
#pragma unroll
        for (int t = 0; t < R; ++t) { const uint32_t c = lane + 64u * t; th[t] = (c < C) ? et[c] : 0.0; }
        cur_u = u;
      }
      const double *eb = a.Eb + (size_t)it * a.ld;
      unsigned long long key[R];
#pragma unroll
      for (int t = 0; t < R; ++t) {
        const uint32_t c = lane + 64u * t;
        const double b = (c < C) ? eb[c] : 0.0;
        const double term = (int32_t)c == a.ubias_col ? th[t] : (int32_t)c == a.ibias_col ? b : th[t] * b;
        key[t] = score_key(term);
      }
      uint32_t live = live0, res_id = 0xffffffffu;
      unsigned long long res_key = 0ull;
      for (uint32_t r = 0; r < rounds; ++r) {
        unsigned long long bk = 0ull; uint32_t bid = 0xffffffffu;
#pragma unroll
        for (int t = 0; t < R; ++t) {
          const bool take = ((live >> t) & 1u) && (bid == 0xffffffffu || key[t] > bk);
          bk = take ? key[t] : bk; bid = take ? lane + 64u * t : bid;
        }
        const unsigned long long wk = wave_max_key(bk);
        const uint32_t wid = wave_min_id((bk == wk) ? bid : 0xffffffffu);     // r < C: a live term exists
        if (lane == (wid & 63u)) live &= ~(1u << (wid >> 6));
        if (lane == r) { res_id = wid; res_key = wk; }
      }
      if (lane < a.T) {
        a.out_factor[p * a.T + lane] = res_id;
        a.out_contrib[p * a.T + lane] = __longlong_as_double((long long)res_key);
      }
    }
  }
}

// out[(c - c0) x rows + r] = E[r x ld + c] for the columns c0 <= c < c0 + nc: a tile of 32 rows x 32 columns per workgroup
// through LDS (33 doubles a row: the transposed read meets 32 different banks), 256-byte runs on both sides
__global__ __launch_bounds__(256) void transpose_cols_kernel(const double *E, double *out, uint32_t rows, uint32_t ld, uint32_t c0, uint32_t nc)
{
  __shared__ double tile[32][33];
  const uint32_t tx = threadIdx.x & 31u, ty = threadIdx.x >> 5;
  const uint32_t r0 = blockIdx.x * 32u, k0 = blockIdx.y * 32u;
#pragma unroll
  for (uint32_t j = 0; j < 32; j += 8) {
    const uint32_t r = r0 + ty + j, c = k0 + tx;
    tile[ty + j][tx] = (r < rows && c < nc) ? E[(size_t)r * ld + c0 + c] : 0.0;
  }
  __syncthreads();
#pragma unroll
  for (uint32_t j = 0; j < 32; j += 8) {
    const uint32_t c = k0 + ty + j, r = r0 + tx;
    if (r < rows && c < nc) out[(size_t)c * rows + r] = tile[tx][ty + j];
  }
}

// ---------------------------------------------------------------------
// Because you rated (hpf_because; -because).  A user's shape is the prior plus a sum over the user's
// ratings of yy * phi, so E[theta_uc] and with it every score splits over the user's history:
//   phi_uic = own_c x_ic / ssum_i ,  ssum_i = sum_c own_c x_ic        own = exp(Elog theta_u - row max), x_i = Wb[i] (the
//                                                                     fold-in's W forms; K + 2 entries with bias)
//   D_uc    = s_prior + sum_i yy_i phi_uic                            because_shape_kernel, the sum in CSR order
//   g_c     = E[theta_uc] E[beta_jc] / D_uc  (c < K),  g_K = E[ubias_u] / D_uK
//   c(i->j) = yy_i sum_c phi_uic g_c = yy_i / ssum_i * sum_c x_ic (own_c g_c)                    because_kernel
//   prior(j) = s_prior sum_c g_c
// Reads E and Elog of both sides and the CSR; writes temporaries and outputs of the call only -- the underflow of a
// softmax denominator goes to the CALL's flag word, not the handle's.
// ---------------------------------------------------------------------
struct BecauseArgs {
  const int64_t  *rowptr;      // [n + 1] CSR of the users
  const uint32_t *idx;         // item of each nonzero
  const uint8_t  *val;         // rating (NULL: all ones)
  const uint32_t *users;       // [n_sel] selected users
  const uint32_t *t_sel;       // [nt] which selected user a target pair belongs to
  const uint32_t *t_item;      // [nt] the target item
  const double   *Wb;          // [n_items x ldf] exp(Elog - row max) of the item side (fold_derive_w_kernel)
  const double   *Lt, *Et, *Eb;// [n x ld], [n x ld], [m x ld]
  double         *D;           // [n_sel x ldf] because_shape_kernel's output
  uint32_t       *out_item;    // [nt x T]
  double         *out_contrib; // [nt x T]
  double         *out_sum, *out_prior;    // [nt]
  uint32_t       *flags;       // bit 0: a softmax denominator underflowed
  uint64_t        nt;
  uint32_t        n_sel, ld, ldf, K, T, run;      // run: consecutive pairs a wave takes per trip (hpf_plan::BECAUSE_RUN)
  int32_t         ubias_col, ujunk_col;           // of the user side's rows: K and K + 1 with -bias, -1 without
  double          s_prior;
};

// the W form of user u's row, lane l its columns l + 64 t: the same bits in both kernels
template <int R>
__device__ __forceinline__ void because_own(const BecauseArgs &a, uint32_t lane, uint32_t u, double (&own)[R])
{
  const double *lt = a.Lt + (size_t)u * a.ld;
  double l[R], m = -1.0e308;
#pragma unroll
  for (int t = 0; t < R; ++t) {
    const uint32_t c = lane + 64u * t;
    const bool live = c < a.K || (int32_t)c == a.ubias_col || (int32_t)c == a.ujunk_col;
    l[t] = live ? lt[c] : -1.0e308;
    m = fmax(m, l[t]);
  }
  m = group_max<64>(m);
#pragma unroll
  for (int t = 0; t < R; ++t) own[t] = (l[t] > -1.0e308) ? exp(l[t] - m) : 0.0;
}

// sum_c x_c w_c in every lane, the SAME bits in every lane: fold_dot's chains, with the lane's own sum rounded before it
// meets the other lanes'.  (With one column per lane the compiler otherwise fuses the lane's product into the first
// cross-lane addition -- fma(own, x, partner's product) on one lane, the mirror image on the partner -- and the two disagree
// in the last bit; a contribution is handed out by one lane and summed by another.)
template <int R>
__device__ __forceinline__ double because_dot(const double (&x)[R], const double (&w)[R])
{
#pragma clang fp contract(off)
  double s[2] = {0.0, 0.0};
#pragma unroll
  for (int e = 0; e < R; ++e) s[e & 1] = (e < 2) ? w[e] * x[e] : fma(w[e], x[e], s[e & 1]);
  const double v = (R > 1) ? s[0] + s[1] : s[0];
  return group_sum<64>(v);
}

// One walk over the `len` nonzeros of the row that starts at `start`, in CSR order: visit(x, yy, item) per nonzero with the
// item's gathered row, the factor yy = (y > 1 ? y : 1) of the phi pass (hgaprec.cc:1355-1356) and the item.  A block of 64
// indices and ratings sits one per lane; two rows are in flight, visited in order.
template <int R, typename Visit>
__device__ __forceinline__ void because_walk(const BecauseArgs &a, uint32_t lane, int64_t start, uint32_t len, Visit &&visit)
{
  const uint32_t LDF = a.ldf;
  for (uint32_t base = 0; base < len; base += 64u) {
    const uint32_t cnt = (len - base < 64u) ? len - base : 64u;
    const uint32_t ci = (lane < cnt) ? a.idx[start + base + lane] : 0u;
    float cy = 1.0f;
    if (a.val && lane < cnt) { const uint32_t y = a.val[start + base + lane]; cy = (y > 1u) ? (float)y : 1.0f; }
    auto item = [&](uint32_t j) { return (uint32_t)__builtin_amdgcn_readlane((int)ci, (int)j); };
    auto rating = [&](uint32_t j) { return (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(cy), (int)j)); };
    auto get = [&](double (&x)[R], uint32_t it) {
      const double *p = a.Wb + (size_t)it * LDF;
#pragma unroll
      for (int t = 0; t < R; ++t) { const uint32_t c = lane + 64u * t; x[t] = (c < LDF) ? p[c] : 0.0; }
    };
    uint32_t j = 0;
    double xa[R], xb[R];
    for (; j + 1 < cnt; j += 2) {
      const uint32_t ia = item(j), ib = item(j + 1);
      get(xa, ia);
      get(xb, ib);
      visit(xa, rating(j), ia);
      visit(xb, rating(j + 1), ib);
    }
    if (j < cnt) { const uint32_t ia = item(j); get(xa, ia); visit(xa, rating(j), ia); }
  }
}

// D of every selected user: a wave per user, one walk
template <int R>
__global__ __launch_bounds__(256) void because_shape_kernel(BecauseArgs a)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t w0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
  const uint32_t nw = (gridDim.x * blockDim.x) >> 6;
  bool underflow = false;
  for (uint32_t b = w0; b < a.n_sel; b += nw) {
    const uint32_t u = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.users[b]);
    const int64_t start = a.rowptr[u];
    const uint32_t len = (uint32_t)(a.rowptr[u + 1] - start);
    double own[R], acc[R];
    because_own<R>(a, lane, u, own);
#pragma unroll
    for (int t = 0; t < R; ++t) acc[t] = 0.0;
    because_walk<R>(a, lane, start, len, [&](const double (&x)[R], double yy, uint32_t) {
      fold_add<R>(x, acc, because_dot<R>(x, own), yy, underflow);
    });
#pragma unroll
    for (int t = 0; t < R; ++t) {
      const uint32_t c = lane + 64u * t;
      if (c < a.ldf) a.D[(size_t)b * a.ldf + c] = (c < a.K || (int32_t)c == a.ubias_col) ? a.s_prior + own[t] * acc[t] : 0.0;
    }
  }
  if (__any(underflow) && lane == 0) atomicOr(a.flags, 1u);
}

// A wave per target pair (a run of consecutive pairs per trip: the user's row is set up again only when the user changes).
// own_c g_c stays in registers; per history item one wave-wide sum for the softmax denominator and one for the
// contribution.  The T best so far live in lanes 0 .. T - 1, sorted in ranks_before's order with the empty places
// (key 0, item 0xffffffff) last: the lanes that rank before a new entry are a prefix, so a ballot counts the insertion
// place and the lanes behind it take their left neighbour's entry.  out_sum adds every contribution in CSR order.
template <int R>
__global__ __launch_bounds__(256) void because_kernel(BecauseArgs a)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t w0 = (uint64_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
  const uint64_t nw = ((uint64_t)gridDim.x * blockDim.x) >> 6;
  const uint32_t K = a.K, T = a.T;
  bool underflow = false;
  for (uint64_t base = w0 * a.run; base < a.nt; base += nw * a.run) {
    double own[R], th[R], dd[R];
    uint32_t cur_sel = 0xffffffffu, len = 0;
    int64_t start = 0;
    for (uint32_t r = 0; r < a.run && base + r < a.nt; ++r) {
      const uint64_t q = base + r;
      const uint32_t sel = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.t_sel[q]), tj = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.t_item[q]);
      if (sel != cur_sel) {                                // wave-uniform
        const uint32_t u = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.users[sel]);
        start = a.rowptr[u];
        len = (uint32_t)(a.rowptr[u + 1] - start);
        because_own<R>(a, lane, u, own);
#pragma unroll
        for (int t = 0; t < R; ++t) {
          const uint32_t c = lane + 64u * t;
          const bool shaped = c < K || (int32_t)c == a.ubias_col;
          th[t] = shaped ? a.Et[(size_t)u * a.ld + c] : 0.0;
          dd[t] = shaped ? a.D[(size_t)sel * a.ldf + c] : 1.0;
        }
        cur_sel = sel;
      }
      double og[R], gs = 0.0;
#pragma unroll
      for (int t = 0; t < R; ++t) {
        const uint32_t c = lane + 64u * t;
        const double g = (c < K) ? th[t] * a.Eb[(size_t)tj * a.ld + c] / dd[t] : (int32_t)c == a.ubias_col ? th[t] / dd[t] : 0.0;
        gs += g;
        og[t] = own[t] * g;
      }
      const double prior = a.s_prior * group_sum<64>(gs);
      unsigned long long tk = 0ull;
      uint32_t ti = 0xffffffffu;
      double sum = 0.0;
      because_walk<R>(a, lane, start, len, [&](const double (&x)[R], double yy, uint32_t it) {
        // the contribution handed out is a rounded double and out_sum the sum of THOSE doubles: no multiply fused into the add
#pragma clang fp contract(off)
        const double ssum = because_dot<R>(x, own), num = because_dot<R>(x, og);
        const bool ok = ssum > 0.0;
        underflow |= !ok;
        const double contrib = ok ? num * (yy * fast_rcp(ssum)) : 0.0;
        sum += contrib;
        const unsigned long long key = score_key(contrib);
        const uint32_t pos = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(lane < T && ranks_before(tk, ti, key, it)));
        if (pos < T) {                                     // wave-uniform
          const unsigned long long pk = __shfl_up(tk, 1, 64);
          const uint32_t pi = __shfl_up(ti, 1, 64);
          if (lane == pos) { tk = key; ti = it; }
          else if (lane > pos) { tk = pk; ti = pi; }
        }
      });
      if (lane < T) {
        a.out_item[q * T + lane] = ti;
        a.out_contrib[q * T + lane] = __longlong_as_double((long long)tk);
      }
      if (lane == 0) { a.out_sum[q] = sum; a.out_prior[q] = prior; }
    }
  }
  if (__any(underflow) && lane == 0) atomicOr(a.flags, 1u);
}

// materialise the per-element rate matrix for export (htheta_rate.tsv):
// rate[row,k] = prior_used[row] + colsum[k]   (gpbase.hh:163-173,218-223)
__global__ void build_rate_kernel(const double *prior_used, const double *colsum,
                                  uint32_t rows, uint32_t K, double *out)
{
  const size_t n = (size_t)rows * K;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n;
       e += (size_t)gridDim.x * blockDim.x)
    out[e] = prior_used[e / K] + colsum[e % K];
}

// single-column staging for the bias objects (host <-> padded layout)
__global__ void column_scatter_kernel(const double *src, double *dst_col, uint32_t rows, uint32_t ld)
{
  for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += gridDim.x * blockDim.x)
    dst_col[(size_t)r * ld] = src[r];
}
__global__ void column_gather_kernel(const double *src_col, double *dst, uint32_t rows, uint32_t ld)
{
  for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += gridDim.x * blockDim.x)
    dst[r] = src_col[(size_t)r * ld];
}

}  // namespace hpf
