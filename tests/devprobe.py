"""ctypes loader of libhpf_probe.so (hgaprec_amd/csrc/hpf_probe.hip): the inline device functions of
hpf_kernels.hpp -- fast_rcp, the two digammas, exp_neg, the p59 writers and reader -- one array element per
thread, for tests/test_gpu_special.py -- and the report kernels themselves (heldout_ll_kernel, elbo_nnz_kernel,
elbo_nnz_w_kernel, rowmax_elog_kernel, elbo_gamma_kernel) on the caller's arrays and grid, for
tests/test_gpu_report_terms.py.  Test infrastructure: the package itself never loads this library."""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

LIB_PATH = Path(__file__).resolve().parent.parent / "hgaprec_amd" / "libhpf_probe.so"

_lib = None


class ProbeError(RuntimeError):
    pass


def load():
    global _lib
    if _lib is not None:
        return _lib
    # one HIP runtime per process: torch first, as hgaprec_amd.capi.load_library does
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not LIB_PATH.exists():
        raise ProbeError(f"{LIB_PATH} not found: build it with `make -C hgaprec_amd/csrc all`")
    lib = C.CDLL(str(LIB_PATH))
    dp, u32p = C.POINTER(C.c_double), C.POINTER(C.c_uint32)
    lib.probe_max_n.restype = C.c_int
    lib.probe_rcp.argtypes = [C.c_int, dp, dp]
    lib.probe_psi.argtypes = [C.c_int, dp, dp, dp, dp]
    lib.probe_sweep_elem.argtypes = [C.c_int, dp, dp, dp, dp, dp]
    lib.probe_exp_neg.argtypes = [C.c_int, dp, dp]
    lib.probe_p59.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint32, dp, dp, u32p, C.POINTER(C.c_uint8)]
    lib.probe_p59_pos.argtypes = [C.c_int, C.c_int, u32p, u32p, u32p]
    lib.probe_p59_paired.restype = C.c_int
    _lib = lib
    return lib


def _check(rc, what):
    if rc != 0:
        raise ProbeError(f"{what}: HIP error {rc}")


def _in(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def rcp(x):
    x = _in(x)
    out = np.empty_like(x)
    _check(load().probe_rcp(x.size, _dp(x), _dp(out)), "probe_rcp")
    return out


def psi(x):
    """-> digamma_pos(x), and (xs, corr) of psi_parts(x)"""
    x = _in(x)
    p, xs, corr = np.empty_like(x), np.empty_like(x), np.empty_like(x)
    _check(load().probe_psi(x.size, _dp(x), _dp(p), _dp(xs), _dp(corr)), "probe_psi")
    return p, xs, corr


def sweep_elem(x, rt):
    """-> W = xs * exp_neg(corr) * ri, ri and corr of psi_parts_rate(x, rt)"""
    x, rt = _in(x), _in(rt)
    assert x.shape == rt.shape
    w, ri, corr = np.empty_like(x), np.empty_like(x), np.empty_like(x)
    _check(load().probe_sweep_elem(x.size, _dp(x), _dp(rt), _dp(w), _dp(ri), _dp(corr)), "probe_sweep_elem")
    return w, ri, corr


def exp_neg(c):
    c = _in(c)
    out = np.empty_like(c)
    _check(load().probe_exp_neg(c.size, _dp(c), _dp(out)), "probe_exp_neg")
    return out


def p59_E(L):
    return (128 * L) // 59


def p59(L, G, writer, w, ncols=None):
    """w: [nrows, G * E] doubles.  The first ncols columns of every row are encoded by writer 0 (p59_put in LDS +
    packed_copy_out) or 1 (p59_place in registers); -> (all G * E columns decoded by codec_p59<L>::get, the flushed
    report per element, the rows' bytes [nrows, G * L * 16])"""
    w = _in(w)
    ld = G * p59_E(L)
    assert w.ndim == 2 and w.shape[1] == ld
    ncols = ld if ncols is None else int(ncols)
    out = np.empty_like(w)
    flushed = np.empty(w.shape, np.uint32)
    rows = np.empty((w.shape[0], G * L * 16), np.uint8)
    _check(load().probe_p59(L, G, writer, w.shape[0], ncols, _dp(w), _dp(out),
                            flushed.ctypes.data_as(C.POINTER(C.c_uint32)), rows.ctypes.data_as(C.POINTER(C.c_uint8))),
           "probe_p59")
    return out, flushed, rows


def p59_pos(L, G):
    """-> (p59_pos on the device, codec_p59<L>::pos at compile time): the places of the E + S logical dwords"""
    rt, ct, n = np.zeros(32, np.uint32), np.zeros(32, np.uint32), C.c_uint32(0)
    u32p = C.POINTER(C.c_uint32)
    _check(load().probe_p59_pos(L, G, rt.ctypes.data_as(u32p), ct.ctypes.data_as(u32p), C.byref(n)), "probe_p59_pos")
    return rt[: n.value].copy(), ct[: n.value].copy()


def p59_paired():
    return bool(load().probe_p59_paired())


# ---- the report kernels themselves (tests/test_gpu_report_terms.py) -------------------------------------------------
# Every wrapper checks every index against the arrays it hands over and raises BEFORE anything is launched.
_report_bound = False


def _report_lib():
    global _report_bound
    lib = load()
    if not _report_bound:
        dp, u32p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
        i64p, u8p = C.POINTER(C.c_int64), C.POINTER(C.c_uint8)
        u32, i32 = C.c_uint32, C.c_int32
        lib.probe_logfact.argtypes = [dp]
        lib.probe_logfact.restype = None
        lib.probe_heldout_ll.argtypes = [C.c_int, u32p, u32p, i32p, C.c_uint64, dp, u32, dp, u32, u32, u32, i32, i32, u32, dp, dp]
        nnz_head = [C.c_int, u32, i64p, u32p, u32p, C.c_uint64, u32p, u8p]
        nnz_tail = [u32, u32, u32, u32, u32, i32, i32, dp]
        lib.probe_elbo_nnz.argtypes = nnz_head + [dp] * 4 + nnz_tail
        lib.probe_elbo_nnz_w.argtypes = nnz_head + [dp] * 8 + nnz_tail
        lib.probe_rowmax_elog.argtypes = [dp, u32, u32, u32, i32, i32, dp]
        lib.probe_elbo_gamma.argtypes = [C.c_int] + [dp] * 9 + [u32, u32, u32, i32] + [C.c_double] * 6 + [u32, dp]
        _report_bound = True
    return lib


def _mat(a, ld=None):
    a = _in(a)
    if a.ndim != 2 or a.shape[0] < 1 or (ld is not None and a.shape[1] != ld):
        raise ValueError(f"expected a [rows x {ld}] matrix, got {a.shape}")
    return a


def _vec(a, dtype, n=None):
    a = np.ascontiguousarray(a, dtype=dtype)
    if a.ndim != 1 or (n is not None and a.size != n):
        raise ValueError(f"expected {n} elements, got {a.shape}")
    return a


def _as(a, ctype):
    return a.ctypes.data_as(C.POINTER(ctype))


def _bias_cols(ubias_col, ibias_col, ld):
    if (ubias_col < 0) != (ibias_col < 0) or ubias_col >= ld or ibias_col >= ld:
        raise ValueError(f"bias columns {ubias_col}, {ibias_col} outside [0, {ld})")


def logfact():
    """the table of log y!, y = 0 .. 255, built by the function hpf_create builds it with"""
    lf = np.empty(256)
    _report_lib().probe_logfact(_dp(lf))
    return lf


def heldout_ll(grid_blocks, u, i, y, Et, Eb, K, ubias_col=-1, ibias_col=-1, binary=False, lf=None):
    """-> heldout_ll_kernel's value of every pair, from grid_blocks blocks.  y: any int32 (the kernel wraps it)"""
    Et = _mat(Et)
    ld = Et.shape[1]
    Eb = _mat(Eb, ld)
    u, i = _vec(u, np.uint32), _vec(i, np.uint32, len(u))
    y = _vec(np.asarray(y, dtype=np.int64).astype(np.int32), np.int32, u.size)
    lf = logfact() if lf is None else _vec(lf, np.float64, 256)
    if grid_blocks < 1 or K > ld:
        raise ValueError("grid_blocks >= 1 and K <= ld")
    _bias_cols(ubias_col, ibias_col, ld)
    if u.size and (u.max() >= Et.shape[0] or i.max() >= Eb.shape[0]):
        raise ValueError("pair index out of range")
    out = np.empty(u.size)
    _check(_report_lib().probe_heldout_ll(grid_blocks, _as(u, C.c_uint32), _as(i, C.c_uint32), _as(y, C.c_int32), u.size,
                                          _dp(Et), Et.shape[0], _dp(Eb), Eb.shape[0], ld, K, ubias_col, ibias_col,
                                          int(bool(binary)), _dp(lf), _dp(out)), "probe_heldout_ll")
    return out


def _segments(seg_row, seg_start, seg_len, col, val, rows_t, rows_b):
    seg_row, seg_len = _vec(seg_row, np.uint32), _vec(seg_len, np.uint32, len(seg_row))
    seg_start = _vec(seg_start, np.int64, seg_row.size)
    col = _vec(col, np.uint32)
    val = None if val is None else _vec(val, np.uint8, col.size)
    if seg_row.size and (seg_row.max() >= rows_t or seg_start.min() < 0
                         or (seg_start + seg_len.astype(np.int64)).max() > col.size):
        raise ValueError("segment outside the rows or the nonzeros")
    if col.size and col.max() >= rows_b:
        raise ValueError("column index out of range")
    return seg_row, seg_start, seg_len, col, val


def _nnz_call(fn, what, grid_blocks, segs, mats, rows_t, rows_b, ld, K, Cc, ubias_col, ibias_col):
    seg_row, seg_start, seg_len, col, val = segs
    if grid_blocks < 1 or not (K <= Cc <= ld):
        raise ValueError("grid_blocks >= 1 and K <= C <= ld")
    _bias_cols(ubias_col, ibias_col, ld)
    partial = np.empty(grid_blocks)
    _check(fn(grid_blocks, seg_row.size, _as(seg_start, C.c_int64), _as(seg_row, C.c_uint32), _as(seg_len, C.c_uint32),
              col.size, _as(col, C.c_uint32), None if val is None else _as(val, C.c_uint8), *[_dp(m) for m in mats],
              rows_t, rows_b, ld, K, Cc, ubias_col, ibias_col, _dp(partial)), what)
    return partial


def elbo_nnz(grid_blocks, seg_row, seg_start, seg_len, col, val, Lt, Lb, Et, Eb, K, Cc, ubias_col=-1, ibias_col=-1):
    """-> the grid_blocks block partials of elbo_nnz_kernel over the given segments (wave w of the grid takes the
    segments w, w + 4 grid_blocks, ...)"""
    Lt = _mat(Lt)
    ld = Lt.shape[1]
    Lb, Et, Eb = _mat(Lb, ld), _mat(Et, ld), _mat(Eb, ld)
    if Et.shape[0] != Lt.shape[0] or Eb.shape[0] != Lb.shape[0]:
        raise ValueError("E and Elog differ in rows")
    segs = _segments(seg_row, seg_start, seg_len, col, val, Lt.shape[0], Lb.shape[0])
    return _nnz_call(_report_lib().probe_elbo_nnz, "probe_elbo_nnz", grid_blocks, segs, (Lt, Lb, Et, Eb), Lt.shape[0],
                     Lb.shape[0], ld, K, Cc, ubias_col, ibias_col)


def elbo_nnz_w(grid_blocks, seg_row, seg_start, seg_len, col, val, Wt, Wb, Mt, Mb, Lt, Lb, Et, Eb, K, Cc,
               ubias_col=-1, ibias_col=-1):
    """the same of elbo_nnz_w_kernel, from W (padding columns 0) and the row maxima as given"""
    Wt = _mat(Wt)
    ld = Wt.shape[1]
    Wb, Lt, Lb, Et, Eb = _mat(Wb, ld), _mat(Lt, ld), _mat(Lb, ld), _mat(Et, ld), _mat(Eb, ld)
    rows_t, rows_b = Wt.shape[0], Wb.shape[0]
    Mt, Mb = _vec(Mt, np.float64, rows_t), _vec(Mb, np.float64, rows_b)
    if not (Lt.shape[0] == Et.shape[0] == rows_t and Lb.shape[0] == Eb.shape[0] == rows_b):
        raise ValueError("W, Elog and E differ in rows")
    segs = _segments(seg_row, seg_start, seg_len, col, val, rows_t, rows_b)
    return _nnz_call(_report_lib().probe_elbo_nnz_w, "probe_elbo_nnz_w", grid_blocks, segs,
                     (Wt, Wb, Mt, Mb, Lt, Lb, Et, Eb), rows_t, rows_b, ld, K, Cc, ubias_col, ibias_col)


def one_nonzero_per_block(rows, cols):
    """-> (seg_row, seg_start, seg_len) that give nonzero b = (rows[b], cols[b]) to block b alone: four segments per block,
    one per wave, the first with the nonzero and three of length 0 -- partial[b] is then the term of nonzero b"""
    rows = np.asarray(rows, np.uint32)
    nb = rows.size
    seg_row = np.repeat(rows, 4)
    seg_start = np.repeat(np.arange(nb, dtype=np.int64), 4)
    seg_len = np.tile(np.array([1, 0, 0, 0], np.uint32), nb)
    return seg_row, seg_start, seg_len


def rowmax_elog(L, K, bias_col=-1, junk_col=-1):
    L = _mat(L)
    ld = L.shape[1]
    if K > ld or bias_col >= ld or junk_col >= ld:
        raise ValueError("column outside the row")
    M = np.empty(L.shape[0])
    _check(_report_lib().probe_rowmax_elog(_dp(L), L.shape[0], ld, K, bias_col, junk_col, _dp(M)), "probe_rowmax_elog")
    return M


def elbo_gamma(grid_blocks, S, E, L, colsum_used, K, s_prior, r_prior, lg_s_prior, bias_col=-1, bias_rate_add=0.0,
               hier=False, prior_used=None, prior_elog_used=None, prior_E=None, prior_elog=None, prior_rate=None,
               prior_shape=0.0, lg_prior_shape=0.0):
    """-> the grid_blocks block partials of elbo_gamma_kernel; every field of ElboGammaArgs in host arrays"""
    S = _mat(S)
    rows, ld = S.shape
    E, L = _mat(E, ld), _mat(L, ld)
    if E.shape[0] != rows or L.shape[0] != rows:
        raise ValueError("S, E and L differ in rows")
    cs = _vec(colsum_used, np.float64, ld)
    if grid_blocks < 1 or K > ld or bias_col >= ld:
        raise ValueError("grid_blocks >= 1, K <= ld, bias_col < ld")
    pr = [None] * 5
    if hier:
        pr = [_vec(a, np.float64, rows) for a in (prior_used, prior_elog_used, prior_E, prior_elog, prior_rate)]
    partial = np.empty(grid_blocks)
    _check(_report_lib().probe_elbo_gamma(grid_blocks, _dp(S), _dp(E), _dp(L), *[None if a is None else _dp(a) for a in pr[:2]],
                                          _dp(cs), *[None if a is None else _dp(a) for a in pr[2:]], rows, ld, K, bias_col,
                                          bias_rate_add, s_prior, r_prior, lg_s_prior, prior_shape, lg_prior_shape,
                                          int(bool(hier)), _dp(partial)), "probe_elbo_gamma")
    return partial
