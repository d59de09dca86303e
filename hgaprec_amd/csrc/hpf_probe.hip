// hpf_probe.hip -- TEST-ONLY entry points onto the inline device functions of hpf_kernels.hpp
// (libhpf_probe.so; tests/devprobe.py loads it, the library and the CLI do not link it).
//
// Every kernel here calls the very function the hot path calls -- fast_rcp, psi_parts / digamma_pos,
// psi_parts_rate, exp_neg, p59_put / packed_copy_out, p59_place, codec_p59<L>::get -- on one array element
// per thread, so that tests/test_gpu_special.py can hold each of them against mpmath on its own.  Nothing is
// re-implemented: a change of a coefficient in the header changes what these return.
//
// All entry points take HOST pointers, allocate, copy, launch one small kernel, synchronise, copy back and
// return the hipError_t (0 = success).  Arrays hold at most PROBE_MAX_N elements.
//
// The second half launches the report kernels themselves -- heldout_ll_kernel, elbo_nnz_kernel, elbo_nnz_w_kernel,
// rowmax_elog_kernel, elbo_gamma_kernel -- on the caller's arrays and grid (tests/test_gpu_report_terms.py), and
// unit_rows_kernel as hpf_similar launches it (probe_unit_rows; tests/test_gpu_similar.py), and mmr_kernel as
// hpf_recommend_diverse launches it, on a pool and unit rows of the test's (probe_mmr; tests/test_gpu_diverse.py).
#include "hpf_kernels.hpp"

#include <algorithm>
#include <vector>

using namespace hpf;

namespace {

constexpr int PROBE_MAX_N = 100000;

// ---- codec_p59<L>::pos maps the E + S logical dwords one-to-one into the lane's 4L, in BOTH dword orders
template <int L, bool PAIRED>
constexpr bool p59_pos_is_injective()
{
  using C = codec_p59<L>;
  bool seen[4 * L] = {};
  for (int k = 0; k < C::E + C::S; ++k) {
    const int p = C::pos_as(PAIRED, k);
    if (p < 0 || p >= 4 * L || seen[p]) return false;
    seen[p] = true;
  }
  return true;
}
template <int L> constexpr bool p59_pos_ok() { return p59_pos_is_injective<L, true>() && p59_pos_is_injective<L, false>(); }
static_assert(p59_pos_ok<1>() && p59_pos_ok<2>() && p59_pos_ok<3>() && p59_pos_ok<4>() && p59_pos_ok<5>() &&
              p59_pos_ok<6>() && p59_pos_ok<7>() && p59_pos_ok<8>(),
              "codec_p59<L>::pos must place the E + S logical dwords of a lane one-to-one into [0, 4L)");

// ---- device buffers that free themselves, and the copy / launch / copy skeleton
struct DevBuf {
  void *p = nullptr;
  ~DevBuf() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 1); }
  template <typename T> T *as() const { return static_cast<T *>(p); }
};

#define PROBE_TRY(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) return (int)e_; } while (0)

int finish_launch()
{
  PROBE_TRY(hipGetLastError());
  PROBE_TRY(hipDeviceSynchronize());
  return 0;
}

inline dim3 grid_for(int n) { return dim3((unsigned)((n + 255) / 256)); }

// ---- the special functions, one element per thread
__global__ void rcp_kernel(const double *x, double *out, int n)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = fast_rcp(x[i]);
}

__global__ void psi_kernel(const double *x, double *psi, double *xs, double *corr, int n)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const PsiParts r = psi_parts(x[i]);
  xs[i] = r.xs;
  corr[i] = r.corr;
  psi[i] = digamma_pos(x[i]);
}

__global__ void sweep_elem_kernel(const double *x, const double *rt, double *w, double *ri, double *corr, int n)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const PsiRate ps = psi_parts_rate(x[i], rt[i]);
  ri[i] = ps.ri;
  corr[i] = ps.corr;
  w[i] = ps.xs * exp_neg(ps.corr) * ps.ri;      // row_sweep_kernel: exp(psi(shape) - log(rate))
}

__global__ void exp_neg_kernel(const double *c, double *out, int n)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = exp_neg(c[i]);
}

// ---- p59 rows.  One workgroup of G threads per row; thread g is packed lane g and owns the columns e * G + g.
// Columns from ncols on are "past the row's length": the LDS writer never puts them (row_sweep_kernel tests the
// column against the stride), the register writer places the all-zero element (its `live` test).
__global__ void p59_write_lds_kernel(PackedRow pk, uint32_t ncols, const double *w, unsigned char *rows, uint32_t *flushed)
{
  __shared__ uint32_t buf[64 * 8 * 4];             // G <= 64 lanes x L <= 8 pieces x 4 dwords
  const uint32_t g = threadIdx.x, G = pk.G, ld = G * pk.E;
  const size_t row = blockIdx.x;
  packed_clear(buf, pk, g, G);
  __syncthreads();
  for (uint32_t e = 0; e < pk.E; ++e) {
    const uint32_t c = g + G * e;
    uint32_t fl = 0u;
    if (c < ncols) fl = p59_put(buf, pk, c, w[row * ld + c]) ? 1u : 0u;
    flushed[row * ld + c] = fl;
  }
  __syncthreads();
  packed_copy_out(buf, rows, row, pk, g, G);
}

// the slot count R of the register-building sweep that serves p59 rows of L pieces (p59_of_slots)
template <int L> struct slots_of_p59 {
  static constexpr int E = codec_p59<L>::E;
  static constexpr int R = E <= 10 ? E / 2 : (E + 1) / 2;
  static_assert(p59_of_slots<R>::valid && p59_of_slots<R>::E == E && p59_of_slots<R>::L == L,
                "every p59 shape L = 1..8 has a register-building sweep");
};

template <int L>
__global__ void p59_write_reg_kernel(uint32_t G, uint32_t ncols, const double *w, unsigned char *rows, uint32_t *flushed)
{
  using P = p59_of_slots<slots_of_p59<L>::R>;
  constexpr int E = P::E;
  const uint32_t g = threadIdx.x, ld = G * (uint32_t)E;
  const size_t row = blockIdx.x;
  uint32_t D[4 * L];
#pragma unroll
  for (int i = 0; i < 4 * L; ++i) D[i] = 0u;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const uint32_t c = g + G * (uint32_t)e;
    const bool live = c < ncols;
    const P59Words pw = p59_words(live ? w[row * ld + c] : 0.0, live);
    flushed[row * ld + c] = pw.flushed ? 1u : 0u;
    p59_place<E, L>(D, e, pw.lo, pw.f);
  }
  // piece t of lane g at byte (t * G + g) * 16 of the row
  uint4 *dst = reinterpret_cast<uint4 *>(rows + row * (size_t)(G * L * 16)) + g;
#pragma unroll
  for (int t = 0; t < L; ++t) dst[(size_t)t * G] = make_uint4(D[4 * t], D[4 * t + 1], D[4 * t + 2], D[4 * t + 3]);
}

// the reader, as phi_segments loads and decodes a row: L 16-byte pieces per lane, elements from the last to the first
template <int L>
__global__ void p59_read_kernel(uint32_t G, const unsigned char *rows, double *out)
{
  using C = codec_p59<L>;
  const uint32_t g = threadIdx.x, ld = G * (uint32_t)C::E;
  const size_t row = blockIdx.x;
  const unsigned char *base = rows + row * (size_t)(G * L * 16) + (size_t)g * 16;
  uint32_t d[4 * L];
#pragma unroll
  for (int t = 0; t < L; ++t) {
    const uint4 v = *reinterpret_cast<const uint4 *>(base + (size_t)t * G * 16);
    d[4 * t] = v.x; d[4 * t + 1] = v.y; d[4 * t + 2] = v.z; d[4 * t + 3] = v.w;
  }
#pragma unroll
  for (int e = C::E - 1; e >= 0; --e) out[row * ld + (uint32_t)e * G + g] = C::get(d, e);
}

__global__ void p59_pos_kernel(PackedRow pk, uint32_t n, uint32_t *out)
{
  const uint32_t k = threadIdx.x;
  if (k < n) out[k] = p59_pos(pk, k);
}

PackedRow packed_row(int G, int L)
{
  PackedRow pk;
  pk.G = (uint32_t)G; pk.L = (uint32_t)L; pk.E = (uint32_t)((128 * L) / 59); pk.row_bytes = (uint32_t)(G * L) * 16u;
  pk.lgG = 0; while ((1u << pk.lgG) < (uint32_t)G) ++pk.lgG;
  return pk;
}

template <int L>
int p59_round_trip(int G, int writer, uint32_t nrows, uint32_t ncols, const double *w_in, double *w_out,
                   uint32_t *flushed_out, unsigned char *rows_out)
{
  const PackedRow pk = packed_row(G, L);
  const size_t n = (size_t)nrows * pk.G * pk.E, row_bytes = (size_t)nrows * pk.row_bytes;
  DevBuf w, out, fl, rows;
  PROBE_TRY(w.alloc(n * sizeof(double)));
  PROBE_TRY(out.alloc(n * sizeof(double)));
  PROBE_TRY(fl.alloc(n * sizeof(uint32_t)));
  PROBE_TRY(rows.alloc(row_bytes));
  PROBE_TRY(hipMemcpy(w.p, w_in, n * sizeof(double), hipMemcpyHostToDevice));
  PROBE_TRY(hipMemset(rows.p, 0xa5, row_bytes));           // a writer must store every byte of the row
  if (writer == 0)
    hipLaunchKernelGGL(p59_write_lds_kernel, dim3(nrows), dim3((unsigned)G), 0, 0, pk, ncols, w.as<double>(),
                       rows.as<unsigned char>(), fl.as<uint32_t>());
  else
    hipLaunchKernelGGL((p59_write_reg_kernel<L>), dim3(nrows), dim3((unsigned)G), 0, 0, (uint32_t)G, ncols, w.as<double>(),
                       rows.as<unsigned char>(), fl.as<uint32_t>());
  if (const int rc = finish_launch()) return rc;
  hipLaunchKernelGGL((p59_read_kernel<L>), dim3(nrows), dim3((unsigned)G), 0, 0, (uint32_t)G, rows.as<unsigned char>(),
                     out.as<double>());
  if (const int rc = finish_launch()) return rc;
  PROBE_TRY(hipMemcpy(w_out, out.p, n * sizeof(double), hipMemcpyDeviceToHost));
  PROBE_TRY(hipMemcpy(flushed_out, fl.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (rows_out) PROBE_TRY(hipMemcpy(rows_out, rows.p, row_bytes, hipMemcpyDeviceToHost));
  return 0;
}

template <int L>
void p59_static_pos(uint32_t *out, uint32_t *n)
{
  using C = codec_p59<L>;
  *n = (uint32_t)(C::E + C::S);
  for (int k = 0; k < C::E + C::S; ++k) out[k] = (uint32_t)C::pos(k);
}

bool array_ok(int n) { return n >= 0 && n <= PROBE_MAX_N; }

}  // namespace

#define PROBE_API extern "C" __attribute__((visibility("default")))

PROBE_API int probe_max_n(void) { return PROBE_MAX_N; }

// out[i] = fast_rcp(x[i])
PROBE_API int probe_rcp(int n, const double *x, double *out)
{
  if (!array_ok(n)) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  DevBuf dx, dout;
  PROBE_TRY(dx.alloc(n * sizeof(double)));
  PROBE_TRY(dout.alloc(n * sizeof(double)));
  PROBE_TRY(hipMemcpy(dx.p, x, n * sizeof(double), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(rcp_kernel, grid_for(n), dim3(256), 0, 0, dx.as<double>(), dout.as<double>(), n);
  if (const int rc = finish_launch()) return rc;
  PROBE_TRY(hipMemcpy(out, dout.p, n * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

// psi_out[i] = digamma_pos(x[i]);  (xs_out[i], corr_out[i]) = psi_parts(x[i])
PROBE_API int probe_psi(int n, const double *x, double *psi_out, double *xs_out, double *corr_out)
{
  if (!array_ok(n)) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  DevBuf dx, d[3];
  PROBE_TRY(dx.alloc(n * sizeof(double)));
  for (DevBuf &b : d) PROBE_TRY(b.alloc(n * sizeof(double)));
  PROBE_TRY(hipMemcpy(dx.p, x, n * sizeof(double), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(psi_kernel, grid_for(n), dim3(256), 0, 0, dx.as<double>(), d[0].as<double>(), d[1].as<double>(),
                     d[2].as<double>(), n);
  if (const int rc = finish_launch()) return rc;
  PROBE_TRY(hipMemcpy(psi_out, d[0].p, n * sizeof(double), hipMemcpyDeviceToHost));
  PROBE_TRY(hipMemcpy(xs_out, d[1].p, n * sizeof(double), hipMemcpyDeviceToHost));
  PROBE_TRY(hipMemcpy(corr_out, d[2].p, n * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

// (xs, corr, ri) = psi_parts_rate(x[i], rt[i]);  w_out[i] = xs * exp_neg(corr) * ri -- one element of the row sweep
PROBE_API int probe_sweep_elem(int n, const double *x, const double *rt, double *w_out, double *ri_out, double *corr_out)
{
  if (!array_ok(n)) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  DevBuf dx, drt, d[3];
  PROBE_TRY(dx.alloc(n * sizeof(double)));
  PROBE_TRY(drt.alloc(n * sizeof(double)));
  for (DevBuf &b : d) PROBE_TRY(b.alloc(n * sizeof(double)));
  PROBE_TRY(hipMemcpy(dx.p, x, n * sizeof(double), hipMemcpyHostToDevice));
  PROBE_TRY(hipMemcpy(drt.p, rt, n * sizeof(double), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(sweep_elem_kernel, grid_for(n), dim3(256), 0, 0, dx.as<double>(), drt.as<double>(), d[0].as<double>(),
                     d[1].as<double>(), d[2].as<double>(), n);
  if (const int rc = finish_launch()) return rc;
  PROBE_TRY(hipMemcpy(w_out, d[0].p, n * sizeof(double), hipMemcpyDeviceToHost));
  PROBE_TRY(hipMemcpy(ri_out, d[1].p, n * sizeof(double), hipMemcpyDeviceToHost));
  PROBE_TRY(hipMemcpy(corr_out, d[2].p, n * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

// out[i] = exp_neg(c[i])
PROBE_API int probe_exp_neg(int n, const double *c, double *out)
{
  if (!array_ok(n)) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  DevBuf dc, dout;
  PROBE_TRY(dc.alloc(n * sizeof(double)));
  PROBE_TRY(dout.alloc(n * sizeof(double)));
  PROBE_TRY(hipMemcpy(dc.p, c, n * sizeof(double), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(exp_neg_kernel, grid_for(n), dim3(256), 0, 0, dc.as<double>(), dout.as<double>(), n);
  if (const int rc = finish_launch()) return rc;
  PROBE_TRY(hipMemcpy(out, dout.p, n * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

// nrows p59 rows of G lanes x L pieces (E = 128 L / 59 elements per lane, G * E columns): the first ncols columns of
// every row of w_in are encoded by `writer` -- 0: p59_put into LDS + packed_copy_out, 1: p59_place<E, L> in registers --
// and ALL G * E columns are decoded with codec_p59<L>::get into w_out.  flushed_out[row][column]: the writer reported
// the element as flushed.  rows_out (may be NULL): the nrows * G * L * 16 bytes of the rows as written.
PROBE_API int probe_p59(int L, int G, int writer, uint32_t nrows, uint32_t ncols, const double *w_in, double *w_out,
                        uint32_t *flushed_out, unsigned char *rows_out)
{
  if (L < 1 || L > 8 || (G != 4 && G != 8 && G != 16 && G != 32 && G != 64) || (writer != 0 && writer != 1))
    return (int)hipErrorInvalidValue;
  const uint32_t ld = (uint32_t)(G * ((128 * L) / 59));
  if (nrows == 0 || ncols > ld || (size_t)nrows * ld > (size_t)PROBE_MAX_N) return (int)hipErrorInvalidValue;
  switch (L) {
#define P59_L(LL) case LL: return p59_round_trip<LL>(G, writer, nrows, ncols, w_in, w_out, flushed_out, rows_out);
    P59_L(1) P59_L(2) P59_L(3) P59_L(4) P59_L(5) P59_L(6) P59_L(7) P59_L(8)
#undef P59_L
  }
  return (int)hipErrorInvalidValue;
}

// the place of each of the E + S logical dwords of a p59 lane of L pieces: run_time_out from p59_pos on the device (what
// the LDS writer uses, shape from PackedRow), compile_time_out from codec_p59<L>::pos (the reader and the register writer).
// Both arrays hold 4 L entries at most; *n_out = E + S.
PROBE_API int probe_p59_pos(int L, int G, uint32_t *run_time_out, uint32_t *compile_time_out, uint32_t *n_out)
{
  if (L < 1 || L > 8 || (G != 4 && G != 8 && G != 16 && G != 32 && G != 64)) return (int)hipErrorInvalidValue;
  switch (L) {
#define POS_L(LL) case LL: p59_static_pos<LL>(compile_time_out, n_out); break;
    POS_L(1) POS_L(2) POS_L(3) POS_L(4) POS_L(5) POS_L(6) POS_L(7) POS_L(8)
#undef POS_L
  }
  const PackedRow pk = packed_row(G, L);
  DevBuf d;
  PROBE_TRY(d.alloc(32 * sizeof(uint32_t)));
  hipLaunchKernelGGL(p59_pos_kernel, dim3(1), dim3(64), 0, 0, pk, *n_out, d.as<uint32_t>());
  if (const int rc = finish_launch()) return rc;
  PROBE_TRY(hipMemcpy(run_time_out, d.p, *n_out * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return 0;
}

// whether the library was built with the paired dword order (HPF_P59_PAIRED)
PROBE_API int probe_p59_paired(void) { return HPF_P59_PAIRED ? 1 : 0; }

// ---- the report kernels themselves (tests/test_gpu_report_terms.py): heldout_ll_kernel, elbo_nnz_kernel,
// elbo_nnz_w_kernel, rowmax_elog_kernel and elbo_gamma_kernel launched on the caller's arrays with the caller's grid.
// Every index is checked against the arrays here, before anything is launched; matrices hold at most PROBE_MAX_MAT doubles.
namespace {

constexpr size_t PROBE_MAX_MAT = (size_t)1 << 22;
constexpr int PROBE_MAX_GRID = 4096;

bool grid_ok(int g) { return g >= 1 && g <= PROBE_MAX_GRID; }
bool mat_ok(uint32_t rows, uint32_t ld) { return rows >= 1 && ld >= 1 && (size_t)rows * ld <= PROBE_MAX_MAT; }
bool bias_ok(int32_t ucol, int32_t icol, uint32_t ld)
{
  if (ucol < 0 && icol < 0) return true;
  return ucol >= 0 && icol >= 0 && (uint32_t)ucol < ld && (uint32_t)icol < ld;
}

template <typename T>
int to_device(DevBuf &d, const T *src, size_t n)
{
  PROBE_TRY(d.alloc(n * sizeof(T)));
  if (n) PROBE_TRY(hipMemcpy(d.p, src, n * sizeof(T), hipMemcpyHostToDevice));
  return 0;
}

// the segment list, the nonzeros and the four factor matrices of a per-nonzero ELBO kernel
struct NnzInputs {
  DevBuf segs, col, val, a, b, et, eb;
  int upload(uint32_t nseg, const int64_t *seg_start, const uint32_t *seg_row, const uint32_t *seg_len, uint64_t nnz,
             const uint32_t *col_in, const uint8_t *val_in, const double *A, const double *B, const double *Et,
             const double *Eb, uint32_t rows_t, uint32_t rows_b, uint32_t ld)
  {
    std::vector<Seg> sg(nseg);
    for (uint32_t s = 0; s < nseg; ++s) {
      if (seg_row[s] >= rows_t || seg_start[s] < 0 || (uint64_t)seg_start[s] + seg_len[s] > nnz) return (int)hipErrorInvalidValue;
      sg[s].start = seg_start[s]; sg[s].row = seg_row[s]; sg[s].len = seg_len[s]; sg[s].pslot = -1; sg[s].pad = 0;
    }
    for (uint64_t j = 0; j < nnz; ++j) if (col_in[j] >= rows_b) return (int)hipErrorInvalidValue;
    if (int rc = to_device(segs, sg.data(), (size_t)nseg)) return rc;
    if (int rc = to_device(col, col_in, (size_t)nnz)) return rc;
    if (val_in) if (int rc = to_device(val, val_in, (size_t)nnz)) return rc;
    if (int rc = to_device(a, A, (size_t)rows_t * ld)) return rc;
    if (int rc = to_device(b, B, (size_t)rows_b * ld)) return rc;
    if (int rc = to_device(et, Et, (size_t)rows_t * ld)) return rc;
    return to_device(eb, Eb, (size_t)rows_b * ld);
  }
};

}  // namespace

// the table of log y!, y = 0 .. 255, that hpf_create hands to heldout_ll_kernel
PROBE_API void probe_logfact(double *lf256) { logfact_table(lf256); }

// out[p] = heldout_ll_kernel's value of pair p, from a launch of grid_blocks blocks of 256 threads
PROBE_API int probe_heldout_ll(int grid_blocks, const uint32_t *u, const uint32_t *i, const int32_t *y, uint64_t cnt,
                               const double *Et, uint32_t n, const double *Eb, uint32_t m, uint32_t ld, uint32_t K,
                               int32_t ubias_col, int32_t ibias_col, uint32_t binary, const double *logfact, double *out)
{
  if (!grid_ok(grid_blocks) || cnt > (uint64_t)PROBE_MAX_N || !mat_ok(n, ld) || !mat_ok(m, ld) || K > ld ||
      !bias_ok(ubias_col, ibias_col, ld))
    return (int)hipErrorInvalidValue;
  for (uint64_t p = 0; p < cnt; ++p) if (u[p] >= n || i[p] >= m) return (int)hipErrorInvalidValue;
  if (cnt == 0) return 0;
  DevBuf du, di, dy, det, deb, dlf, dout;
  if (int rc = to_device(du, u, (size_t)cnt)) return rc;
  if (int rc = to_device(di, i, (size_t)cnt)) return rc;
  if (int rc = to_device(dy, y, (size_t)cnt)) return rc;
  if (int rc = to_device(det, Et, (size_t)n * ld)) return rc;
  if (int rc = to_device(deb, Eb, (size_t)m * ld)) return rc;
  if (int rc = to_device(dlf, logfact, 256)) return rc;
  PROBE_TRY(dout.alloc(cnt * sizeof(double)));
  PROBE_TRY(hipMemset(dout.p, 0xff, cnt * sizeof(double)));     // a pair the kernel skipped reads back as NaN
  LLArgs a;
  a.u = du.as<uint32_t>(); a.i = di.as<uint32_t>(); a.y = dy.as<int32_t>(); a.cnt = cnt;
  a.Et = det.as<double>(); a.Eb = deb.as<double>(); a.logfact = dlf.as<double>(); a.out = dout.as<double>();
  a.ld = ld; a.K = K; a.ubias_col = ubias_col; a.ibias_col = ibias_col; a.binary = binary;
  hipLaunchKernelGGL(heldout_ll_kernel, dim3((unsigned)grid_blocks), dim3(256), 0, 0, a);
  if (const int rc = finish_launch()) return rc;
  PROBE_TRY(hipMemcpy(out, dout.p, cnt * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

// partial[b] = block b's sum of elbo_nnz_kernel over the segments (seg_row, seg_start, seg_len); val may be NULL (all ones)
PROBE_API int probe_elbo_nnz(int grid_blocks, uint32_t nseg, const int64_t *seg_start, const uint32_t *seg_row,
                             const uint32_t *seg_len, uint64_t nnz, const uint32_t *col, const uint8_t *val,
                             const double *Lt, const double *Lb, const double *Et, const double *Eb, uint32_t rows_t,
                             uint32_t rows_b, uint32_t ld, uint32_t K, uint32_t C, int32_t ubias_col, int32_t ibias_col,
                             double *partial)
{
  if (!grid_ok(grid_blocks) || nseg > (uint32_t)PROBE_MAX_N || nnz > (uint64_t)PROBE_MAX_N || !mat_ok(rows_t, ld) ||
      !mat_ok(rows_b, ld) || K > C || C > ld || !bias_ok(ubias_col, ibias_col, ld))
    return (int)hipErrorInvalidValue;
  NnzInputs in;
  if (int rc = in.upload(nseg, seg_start, seg_row, seg_len, nnz, col, val, Lt, Lb, Et, Eb, rows_t, rows_b, ld)) return rc;
  DevBuf dpart;
  PROBE_TRY(dpart.alloc((size_t)grid_blocks * sizeof(double)));
  PROBE_TRY(hipMemset(dpart.p, 0xff, (size_t)grid_blocks * sizeof(double)));
  ElboNnzArgs a;
  a.segs = in.segs.as<Seg>(); a.nseg = nseg; a.col = in.col.as<uint32_t>(); a.val = val ? in.val.as<uint8_t>() : nullptr;
  a.Lt = in.a.as<double>(); a.Lb = in.b.as<double>(); a.Et = in.et.as<double>(); a.Eb = in.eb.as<double>();
  a.partial = dpart.as<double>(); a.ld = ld; a.K = K; a.C = C; a.ubias_col = ubias_col; a.ibias_col = ibias_col;
  hipLaunchKernelGGL(elbo_nnz_kernel, dim3((unsigned)grid_blocks), dim3(256), 0, 0, a);
  if (const int rc = finish_launch()) return rc;
  PROBE_TRY(hipMemcpy(partial, dpart.p, (size_t)grid_blocks * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

// the same of elbo_nnz_w_kernel: W and the row maxima M as given (hpf_elbo builds them from Elog), Lt / Lb for the
// nonzeros whose sum of W products is too small
PROBE_API int probe_elbo_nnz_w(int grid_blocks, uint32_t nseg, const int64_t *seg_start, const uint32_t *seg_row,
                               const uint32_t *seg_len, uint64_t nnz, const uint32_t *col, const uint8_t *val,
                               const double *Wt, const double *Wb, const double *Mt, const double *Mb, const double *Lt,
                               const double *Lb, const double *Et, const double *Eb, uint32_t rows_t, uint32_t rows_b,
                               uint32_t ld, uint32_t K, uint32_t C, int32_t ubias_col, int32_t ibias_col, double *partial)
{
  if (!grid_ok(grid_blocks) || nseg > (uint32_t)PROBE_MAX_N || nnz > (uint64_t)PROBE_MAX_N || !mat_ok(rows_t, ld) ||
      !mat_ok(rows_b, ld) || K > C || C > ld || !bias_ok(ubias_col, ibias_col, ld))
    return (int)hipErrorInvalidValue;
  NnzInputs in;
  if (int rc = in.upload(nseg, seg_start, seg_row, seg_len, nnz, col, val, Wt, Wb, Et, Eb, rows_t, rows_b, ld)) return rc;
  DevBuf dmt, dmb, dlt, dlb, dpart;
  if (int rc = to_device(dmt, Mt, (size_t)rows_t)) return rc;
  if (int rc = to_device(dmb, Mb, (size_t)rows_b)) return rc;
  if (int rc = to_device(dlt, Lt, (size_t)rows_t * ld)) return rc;
  if (int rc = to_device(dlb, Lb, (size_t)rows_b * ld)) return rc;
  PROBE_TRY(dpart.alloc((size_t)grid_blocks * sizeof(double)));
  PROBE_TRY(hipMemset(dpart.p, 0xff, (size_t)grid_blocks * sizeof(double)));
  ElboNnzWArgs a;
  a.segs = in.segs.as<Seg>(); a.nseg = nseg; a.col = in.col.as<uint32_t>(); a.val = val ? in.val.as<uint8_t>() : nullptr;
  a.Wt = in.a.as<double>(); a.Wb = in.b.as<double>(); a.Et = in.et.as<double>(); a.Eb = in.eb.as<double>();
  a.Mt = dmt.as<double>(); a.Mb = dmb.as<double>(); a.Lt = dlt.as<double>(); a.Lb = dlb.as<double>();
  a.partial = dpart.as<double>(); a.ld = ld; a.K = K; a.C = C; a.ubias_col = ubias_col; a.ibias_col = ibias_col;
  hipLaunchKernelGGL(elbo_nnz_w_kernel, dim3((unsigned)grid_blocks), dim3(256), 0, 0, a);
  if (const int rc = finish_launch()) return rc;
  PROBE_TRY(hipMemcpy(partial, dpart.p, (size_t)grid_blocks * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

// M[row] = rowmax_elog_kernel's maximum of row `row` of L, launched as hpf_elbo launches it
PROBE_API int probe_rowmax_elog(const double *L, uint32_t rows, uint32_t ld, uint32_t K, int32_t bias_col, int32_t junk_col,
                                double *M)
{
  if (!mat_ok(rows, ld) || K > ld || bias_col >= (int32_t)ld || junk_col >= (int32_t)ld) return (int)hipErrorInvalidValue;
  DevBuf dl, dm;
  if (int rc = to_device(dl, L, (size_t)rows * ld)) return rc;
  PROBE_TRY(dm.alloc((size_t)rows * sizeof(double)));
  hipLaunchKernelGGL(rowmax_elog_kernel, dim3((rows + 255) / 256), dim3(256), 0, 0, dl.as<double>(), dm.as<double>(), rows, ld,
                     K, bias_col, junk_col);
  if (const int rc = finish_launch()) return rc;
  PROBE_TRY(hipMemcpy(M, dm.p, (size_t)rows * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

// U = unit_rows_kernel's rows of E ([rows x ld], ld even, K <= ld factor columns), launched as hpf_similar launches it
PROBE_API int probe_unit_rows(const double *E, uint32_t rows, uint32_t ld, uint32_t K, double *U)
{
  if (!mat_ok(rows, ld) || (ld & 1u) || K < 1 || K > ld) return (int)hipErrorInvalidValue;
  DevBuf de, du;
  const size_t n = (size_t)rows * ld;
  if (int rc = to_device(de, E, n)) return rc;
  PROBE_TRY(du.alloc(n * sizeof(double)));
  PROBE_TRY(hipMemset(du.p, 0xff, n * sizeof(double)));           // an element the kernel skipped reads back as NaN
  hipLaunchKernelGGL(unit_rows_kernel, dim3(std::min<uint32_t>((rows + 15) / 16, 16384)), dim3(256), 0, 0, de.as<double>(),
                     du.as<double>(), rows, ld, K);
  if (const int rc = finish_launch()) return rc;
  PROBE_TRY(hipMemcpy(U, du.p, n * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

// partial[b] = block b's sum of elbo_gamma_kernel.  S, E, L: [rows x ld]; colsum_used: [ld]; prior_used, prior_elog_used,
// prior_E, prior_elog, prior_rate: [rows], read with hier only (may be NULL without)
PROBE_API int probe_elbo_gamma(int grid_blocks, const double *S, const double *E, const double *L, const double *prior_used,
                               const double *prior_elog_used, const double *colsum_used, const double *prior_E,
                               const double *prior_elog, const double *prior_rate, uint32_t rows, uint32_t ld, uint32_t K,
                               int32_t bias_col, double bias_rate_add, double s_prior, double r_prior, double lg_s_prior,
                               double prior_shape, double lg_prior_shape, uint32_t hier, double *partial)
{
  if (!grid_ok(grid_blocks) || !mat_ok(rows, ld) || K > ld || bias_col >= (int32_t)ld) return (int)hipErrorInvalidValue;
  if (hier && !(prior_used && prior_elog_used && prior_E && prior_elog && prior_rate)) return (int)hipErrorInvalidValue;
  DevBuf ds, de, dl, dcs, dpr[5], dpart;
  const size_t n = (size_t)rows * ld;
  if (int rc = to_device(ds, S, n)) return rc;
  if (int rc = to_device(de, E, n)) return rc;
  if (int rc = to_device(dl, L, n)) return rc;
  if (int rc = to_device(dcs, colsum_used, (size_t)ld)) return rc;
  const double *pr[5] = {prior_used, prior_elog_used, prior_E, prior_elog, prior_rate};
  if (hier) for (int k = 0; k < 5; ++k) if (int rc = to_device(dpr[k], pr[k], (size_t)rows)) return rc;
  PROBE_TRY(dpart.alloc((size_t)grid_blocks * sizeof(double)));
  PROBE_TRY(hipMemset(dpart.p, 0xff, (size_t)grid_blocks * sizeof(double)));
  ElboGammaArgs g;
  g.S = ds.as<double>(); g.E = de.as<double>(); g.L = dl.as<double>(); g.colsum_used = dcs.as<double>();
  g.prior_used = dpr[0].as<double>(); g.prior_elog_used = dpr[1].as<double>(); g.prior_E = dpr[2].as<double>();
  g.prior_elog = dpr[3].as<double>(); g.prior_rate = dpr[4].as<double>();
  g.partial = dpart.as<double>(); g.rows = rows; g.ld = ld; g.K = K; g.bias_col = bias_col; g.bias_rate_add = bias_rate_add;
  g.s_prior = s_prior; g.r_prior = r_prior; g.lg_s_prior = lg_s_prior; g.prior_shape = prior_shape;
  g.lg_prior_shape = lg_prior_shape; g.hier = hier;
  hipLaunchKernelGGL(elbo_gamma_kernel, dim3((unsigned)grid_blocks), dim3(256), 0, 0, g);
  if (const int rc = finish_launch()) return rc;
  PROBE_TRY(hipMemcpy(partial, dpart.p, (size_t)grid_blocks * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

// mmr_kernel as hpf_recommend_diverse launches it, for ONE user, on the caller's pool and unit rows: U [rows x ld] (K factor
// columns), pool_items / pool_scores [P] in list order (the kernel takes the prefix with a score > +0.0), out_* [topn]
PROBE_API int probe_mmr(const double *U, uint32_t rows, uint32_t ld, uint32_t K, const uint32_t *pool_items, const double *pool_scores,
                        uint32_t P, uint32_t topn, double lambda, uint32_t *out_items, double *out_scores, double *out_maxsim,
                        double *out_mmr)
{
  if (!mat_ok(rows, ld) || K < 1 || K > ld || topn < 1 || topn > hpf_plan::DIVERSE_POOL_MAX || !(lambda >= 0.0 && lambda <= 1.0))
    return (int)hipErrorInvalidValue;
  const hpf_plan::DiversePlan dp = hpf_plan::diverse_plan(P, 1, K, 256);
  if (!dp.ok) return (int)hipErrorInvalidValue;
  DevBuf du, dpi, dps, dslab, doi, dos, dom, dok;
  if (int rc = to_device(du, U, (size_t)rows * ld)) return rc;
  if (int rc = to_device(dpi, pool_items, (size_t)P)) return rc;
  if (int rc = to_device(dps, pool_scores, (size_t)P)) return rc;
  PROBE_TRY(dslab.alloc((size_t)dp.workgroups * dp.slab_bytes));
  PROBE_TRY(doi.alloc((size_t)topn * 4));
  PROBE_TRY(dos.alloc((size_t)topn * 8));
  PROBE_TRY(dom.alloc((size_t)topn * 8));
  PROBE_TRY(dok.alloc((size_t)topn * 8));
  PROBE_TRY(hipMemset(dslab.p, 0xff, (size_t)dp.workgroups * dp.slab_bytes));    // a cosine the Gram phase skipped reads back as NaN
  PROBE_TRY(hipMemset(doi.p, 0xee, (size_t)topn * 4));
  PROBE_TRY(hipMemset(dos.p, 0xff, (size_t)topn * 8));
  PROBE_TRY(hipMemset(dom.p, 0xff, (size_t)topn * 8));
  PROBE_TRY(hipMemset(dok.p, 0xff, (size_t)topn * 8));
  MmrArgs a;
  a.U = du.as<double>(); a.pool_items = dpi.as<uint32_t>(); a.pool_scores = dps.as<double>(); a.slab = dslab.as<double>();
  a.out_items = doi.as<uint32_t>(); a.out_scores = dos.as<double>(); a.out_maxsim = dom.as<double>(); a.out_mmr = dok.as<double>();
  a.lambda = lambda; a.rows = rows; a.ld = ld; a.K = K; a.n_sel = 1; a.pool = P; a.topn = topn; a.Pp = dp.Pp;
  hipLaunchKernelGGL(mmr_kernel, dim3(dp.workgroups), dim3(256), 0, 0, a);
  if (const int rc = finish_launch()) return rc;
  PROBE_TRY(hipMemcpy(out_items, doi.p, (size_t)topn * 4, hipMemcpyDeviceToHost));
  PROBE_TRY(hipMemcpy(out_scores, dos.p, (size_t)topn * 8, hipMemcpyDeviceToHost));
  PROBE_TRY(hipMemcpy(out_maxsim, dom.p, (size_t)topn * 8, hipMemcpyDeviceToHost));
  PROBE_TRY(hipMemcpy(out_mmr, dok.p, (size_t)topn * 8, hipMemcpyDeviceToHost));
  return 0;
}
