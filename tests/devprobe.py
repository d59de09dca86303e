"""ctypes loader of libhpf_probe.so (hgaprec_amd/csrc/hpf_probe.hip): the inline device functions of
hpf_kernels.hpp -- fast_rcp, the two digammas, exp_neg, the p59 writers and reader -- one array element per
thread, for tests/test_gpu_special.py.  Test infrastructure: the package itself never loads this library."""
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
