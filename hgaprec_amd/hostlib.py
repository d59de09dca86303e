"""ctypes binding of libhgaprec_host.so -- the C++ host side of the reference
interface (CLI/Env naming, TSV reader -> CSR, MT19937 start state, TSV
writers, stop rule).  No HIP involved; used by the CPU tests and by Python
callers that want the reference's file semantics without the CLI."""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np

_PKG = Path(__file__).resolve().parent
# HGAPREC_HOST_LIB: load another build of the same library (the ASan/UBSan one,
# tests/test_host_sanitizers.py)
LIB_PATH = Path(os.environ.get("HGAPREC_HOST_LIB") or _PKG / "libhgaprec_host.so")
_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise RuntimeError(f"{LIB_PATH} not found: run __graft_entry__.build()")
    L = C.CDLL(str(LIB_PATH))
    vp, dp, u32p = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint32)
    L.hg_prefix.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
    L.hg_open_output.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.c_char_p, C.c_size_t]
    L.hg_ratings_new.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.c_uint32]
    L.hg_ratings_new.restype = vp
    L.hg_ratings_free.argtypes = [vp]
    L.hg_ratings_read_train.argtypes = [vp, C.c_char_p]
    L.hg_ratings_read_heldout.argtypes = [vp, C.c_char_p, C.c_int]
    L.hg_ratings_read_fold_in.argtypes = [vp, C.c_char_p, C.POINTER(C.c_uint64), C.POINTER(C.c_int)]
    L.hg_ratings_read_fold_in.restype = vp
    L.hg_ratings_read_fold_in_items.argtypes = [vp, C.c_char_p, C.POINTER(C.c_uint64), C.POINTER(C.c_int)]
    L.hg_ratings_read_fold_in_items.restype = vp
    L.hg_ratings_n.argtypes = [vp]; L.hg_ratings_n.restype = C.c_uint32
    L.hg_ratings_m.argtypes = [vp]; L.hg_ratings_m.restype = C.c_uint32
    L.hg_ratings_nnz.argtypes = [vp]; L.hg_ratings_nnz.restype = C.c_uint64
    L.hg_ratings_rowptr.argtypes = [vp]; L.hg_ratings_rowptr.restype = C.POINTER(C.c_int64)
    L.hg_ratings_col.argtypes = [vp]; L.hg_ratings_col.restype = u32p
    L.hg_ratings_val.argtypes = [vp]; L.hg_ratings_val.restype = C.POINTER(C.c_uint8)
    L.hg_ratings_seq2user.argtypes = [vp]; L.hg_ratings_seq2user.restype = u32p
    L.hg_ratings_seq2item.argtypes = [vp]; L.hg_ratings_seq2item.restype = u32p
    L.hg_ratings_heldout_count.argtypes = [vp, C.c_int]; L.hg_ratings_heldout_count.restype = C.c_uint64
    L.hg_ratings_heldout_u.argtypes = [vp, C.c_int]; L.hg_ratings_heldout_u.restype = u32p
    L.hg_ratings_heldout_i.argtypes = [vp, C.c_int]; L.hg_ratings_heldout_i.restype = u32p
    L.hg_ratings_heldout_y.argtypes = [vp, C.c_int]; L.hg_ratings_heldout_y.restype = C.POINTER(C.c_int32)
    L.hg_ratings_write_marginals.argtypes = [vp, C.c_char_p, C.c_char_p]
    L.hg_ratings_save_cache.argtypes = [vp, C.c_char_p]
    L.hg_ratings_load_cache.argtypes = [vp, C.c_char_p]
    L.hg_ratings_test_users.argtypes = [vp, C.c_char_p, u32p, C.c_uint32]
    L.hg_mt_u32.argtypes = [C.c_double, C.c_uint32, u32p]
    L.hg_digamma.argtypes = [C.c_double]; L.hg_digamma.restype = C.c_double
    L.hg_state_new.argtypes = [C.c_double, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int]
    L.hg_state_new.restype = vp
    L.hg_state_new_range.argtypes = [C.c_double, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_uint32, C.c_uint32,
                                     C.POINTER(C.c_uint32)]
    L.hg_state_new_range.restype = vp
    L.hg_state_free.argtypes = [vp]
    L.hg_state_get.argtypes = [vp, C.c_int, C.POINTER(dp)]; L.hg_state_get.restype = C.c_size_t
    L.hg_save_matrix.argtypes = [C.c_char_p, dp, C.c_uint32, C.c_uint32, u32p, C.c_uint32]
    L.hg_save_vector.argtypes = [C.c_char_p, dp, C.c_uint32, u32p, C.c_uint32]
    L.hg_load_matrix.argtypes = [C.c_char_p, dp, C.c_uint32, C.c_uint32, u32p, C.c_uint32, C.c_char_p, C.c_size_t]
    L.hg_load_vector.argtypes = [C.c_char_p, dp, C.c_uint32, u32p, C.c_uint32, C.c_char_p, C.c_size_t]
    L.hg_shape_over_rate.argtypes = [dp, C.c_uint32, C.c_uint32, dp, C.c_char_p, C.c_char_p, C.c_size_t]
    L.hg_format_fixed8.argtypes = [dp, C.c_size_t, C.c_char_p]
    L.hg_format_fixed8.restype = C.c_size_t
    L.hg_partition_users.argtypes = [C.POINTER(C.c_int64), C.c_uint32, C.c_int, u32p]
    L.hg_partition_users.restype = None
    L.hg_stop_rule.argtypes = [u32p, dp, C.c_uint32, C.POINTER(C.c_int)]
    u64p = C.POINTER(C.c_uint64)
    L.hg_eval_from_ranks.argtypes = [u64p, u32p, u32p, C.c_uint64, u64p, dp]
    L.hg_eval_from_ranks.restype = None
    L.hg_gamma_expectations.argtypes = [dp, dp, dp, C.c_uint64, C.c_uint64, C.c_int, C.c_char_p, C.c_char_p, C.c_size_t]
    L.hg_ratings_r.argtypes = [vp, C.c_uint32, C.c_uint32]; L.hg_ratings_r.restype = C.c_uint32
    L.hg_ratings_ranked_items.argtypes = [vp, C.c_uint32]; L.hg_ratings_ranked_items.restype = C.c_uint32
    L.hg_ratings_item_degrees.argtypes = [vp]; L.hg_ratings_item_degrees.restype = u32p
    L.hg_chunk_walk.argtypes = [C.c_uint64, C.c_uint64, u64p, C.c_uint64]; L.hg_chunk_walk.restype = C.c_uint64
    L.hg_chunk_offsets.argtypes = [u64p, C.c_uint64, C.c_uint64, u64p]; L.hg_chunk_offsets.restype = None
    L.hg_mask_lists_new.argtypes = [vp, C.c_int, u32p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32]
    L.hg_mask_lists_new.restype = vp
    L.hg_mask_lists_free.argtypes = [vp]; L.hg_mask_lists_free.restype = None
    L.hg_mask_lists_get.argtypes = [vp, C.c_int, C.POINTER(vp)]; L.hg_mask_lists_get.restype = C.c_uint64
    L.hg_item_mask_lists_new.argtypes = [vp, C.c_int, C.c_uint32, C.c_uint32]
    L.hg_item_mask_lists_new.restype = vp
    L.hg_item_mask_lists_free.argtypes = [vp]; L.hg_item_mask_lists_free.restype = None
    L.hg_item_mask_lists_get.argtypes = [vp, C.c_int, C.POINTER(vp)]; L.hg_item_mask_lists_get.restype = C.c_uint64
    L.hg_write_topn.argtypes = [C.c_char_p, vp, u32p, C.c_uint64, u32p, dp, C.c_uint32, C.c_uint32, u32p, u32p]
    L.hg_write_topn.restype = C.c_int64
    if hasattr(L, "hg_write_thompson"):
        L.hg_write_thompson.argtypes = [C.c_char_p, vp, u32p, C.c_uint64, u32p, dp, C.c_uint32, C.c_uint32, C.c_uint32, u32p, u32p]
        L.hg_write_thompson.restype = C.c_int64
    if hasattr(L, "hg_write_diverse"):
        L.hg_write_diverse.argtypes = [C.c_char_p, vp, u32p, C.c_uint64, u32p, dp, dp, C.c_uint32, u32p, u32p, dp]
        L.hg_write_diverse.restype = C.c_int64
    _lib = L
    return L


def _argv(args):
    arr = (C.c_char_p * len(args))(*[str(a).encode() for a in args])
    return len(args), arr


def prefix(args) -> str:
    """output-directory name for a CLI argument list (Env::prefix)"""
    n, arr = _argv(args)
    out, bad = C.create_string_buffer(4096), C.create_string_buffer(256)
    rc = lib().hg_prefix(n, arr, out, 4096, bad, 256)
    if rc:
        raise ValueError(f"unknown option {bad.value.decode()}")
    return out.value.decode()


def open_output(args) -> str:
    n, arr = _argv(args)
    out = C.create_string_buffer(4096)
    rc = lib().hg_open_output(n, arr, out, 4096)
    if rc:
        raise RuntimeError(f"open_output failed ({rc})")
    return out.value.decode()


class Ratings:
    def __init__(self, cap_n, cap_m, binary=False, rating_threshold=1):
        self.L = lib()
        self._r = C.c_void_p(self.L.hg_ratings_new(cap_n, cap_m, int(binary), rating_threshold))

    def read_train(self, path):
        return self.L.hg_ratings_read_train(self._r, str(path).encode())

    def read_heldout(self, path, which):
        return self.L.hg_ratings_read_heldout(self._r, str(path).encode(), which)

    def read_fold_in(self, path):
        """-fold-in FILE: the ratings of new users against this data set's items -> (Ratings of the new users, lines
        skipped because their item is unknown); (None, -1) when the file cannot be opened, (None, -2) when it is malformed"""
        skipped, rc = C.c_uint64(0), C.c_int(0)
        p = self.L.hg_ratings_read_fold_in(self._r, str(path).encode(), C.byref(skipped), C.byref(rc))
        if not p:
            return None, rc.value
        out = Ratings.__new__(Ratings)
        out.L, out._r = self.L, C.c_void_p(p)
        return out, skipped.value

    def read_fold_in_items(self, path):
        """-fold-in-items FILE: the ratings of new items by this data set's users -> (Ratings of the new items: m, seq2item
        and a CSR over this data set's users, lines skipped because their user is unknown); (None, -1) / (None, -2) as
        read_fold_in"""
        skipped, rc = C.c_uint64(0), C.c_int(0)
        p = self.L.hg_ratings_read_fold_in_items(self._r, str(path).encode(), C.byref(skipped), C.byref(rc))
        if not p:
            return None, rc.value
        out = Ratings.__new__(Ratings)
        out.L, out._r = self.L, C.c_void_p(p)
        return out, skipped.value

    n = property(lambda s: s.L.hg_ratings_n(s._r))
    m = property(lambda s: s.L.hg_ratings_m(s._r))
    nnz = property(lambda s: s.L.hg_ratings_nnz(s._r))

    def csr(self):
        n, nnz = self.n, self.nnz
        rp = np.ctypeslib.as_array(self.L.hg_ratings_rowptr(self._r), shape=(n + 1,)).copy()
        if nnz == 0:
            return rp, np.zeros(0, np.uint32), np.zeros(0, np.uint8)
        col = np.ctypeslib.as_array(self.L.hg_ratings_col(self._r), shape=(nnz,)).copy()
        val = np.ctypeslib.as_array(self.L.hg_ratings_val(self._r), shape=(nnz,)).copy()
        return rp, col, val

    def seq2user(self):
        return np.ctypeslib.as_array(self.L.hg_ratings_seq2user(self._r), shape=(max(self.n, 1),))[: self.n].copy()

    def seq2item(self):
        return np.ctypeslib.as_array(self.L.hg_ratings_seq2item(self._r), shape=(max(self.m, 1),))[: self.m].copy()

    def heldout(self, which):
        c = self.L.hg_ratings_heldout_count(self._r, which)
        if c == 0:
            return np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.int32)
        return (np.ctypeslib.as_array(self.L.hg_ratings_heldout_u(self._r, which), shape=(c,)).copy(),
                np.ctypeslib.as_array(self.L.hg_ratings_heldout_i(self._r, which), shape=(c,)).copy(),
                np.ctypeslib.as_array(self.L.hg_ratings_heldout_y(self._r, which), shape=(c,)).copy())

    def write_marginals(self, byusers, byitems):
        return self.L.hg_ratings_write_marginals(self._r, str(byusers).encode(), str(byitems).encode())

    def save_cache(self, data_dir):
        """-cache: binary image of the parsed dataset in <data_dir>/hgaprec.cache.bin"""
        return self.L.hg_ratings_save_cache(self._r, str(data_dir).encode())

    def load_cache(self, data_dir):
        """0 = loaded; 1 = absent, stale (TSV size/mtime), other parameters or damaged"""
        return self.L.hg_ratings_load_cache(self._r, str(data_dir).encode())

    def test_users(self, path):
        out = np.empty(max(self.n, 1), np.uint32)
        c = self.L.hg_ratings_test_users(self._r, str(path).encode(), out.ctypes.data_as(C.POINTER(C.c_uint32)), out.size)
        return None if c < 0 else out[:c].copy()

    def r(self, u, item) -> int:
        """the training rating stored for (u, item), 0 if absent; of a duplicated pair the last one (Ratings::r)"""
        return self.L.hg_ratings_r(self._r, int(u), int(item))

    def ranked_items(self, u) -> int:
        """m minus the distinct training items of u with a rating > 0"""
        return self.L.hg_ratings_ranked_items(self._r, int(u))

    def item_degrees(self):
        return np.ctypeslib.as_array(self.L.hg_ratings_item_degrees(self._r), shape=(max(self.m, 1),))[: self.m].copy()

    def mask_lists(self, which=0, users=None, lo=0, hi=None, rebase=0):
        """MaskLists::fill over the validation (which = 0) or test pairs: of `users` those inside [lo, hi) -- users None:
        the whole range -- -> (users - rebase, mask_ptr, mask_items)"""
        hi = self.n if hi is None else hi
        lst = None if users is None else np.ascontiguousarray(users, np.uint32)
        ml = C.c_void_p(self.L.hg_mask_lists_new(self._r, which, None if lst is None else lst.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                 0 if lst is None else lst.size, lo, hi, rebase))
        try:
            out = []
            for part, dt in enumerate((np.uint32, np.uint64, np.uint32)):
                p = C.c_void_p()
                cnt = self.L.hg_mask_lists_get(ml, part, C.byref(p))
                out.append(np.ctypeslib.as_array(C.cast(p, C.POINTER(np.ctypeslib.as_ctypes_type(dt))), shape=(cnt,)).copy()
                           if cnt else np.zeros(0, dt))
            return tuple(out)
        finally:
            self.L.hg_mask_lists_free(ml)

    def item_mask_lists(self, which=0, lo=0, hi=None):
        """ItemMaskLists::fill over the validation (which = 0) or test pairs: the held-out users of the items [lo, hi)
        -> (items, mask_ptr, mask_users)"""
        hi = self.m if hi is None else hi
        ml = C.c_void_p(self.L.hg_item_mask_lists_new(self._r, which, lo, hi))
        try:
            out = []
            for part, dt in enumerate((np.uint32, np.uint64, np.uint32)):
                p = C.c_void_p()
                cnt = self.L.hg_item_mask_lists_get(ml, part, C.byref(p))
                out.append(np.ctypeslib.as_array(C.cast(p, C.POINTER(np.ctypeslib.as_ctypes_type(dt))), shape=(cnt,)).copy()
                           if cnt else np.zeros(0, dt))
            return tuple(out)
        finally:
            self.L.hg_item_mask_lists_free(ml)

    def __del__(self):
        try:
            self.L.hg_ratings_free(self._r)
        except Exception:
            pass


def mt_u32(seed, count):
    out = np.empty(count, np.uint32)
    lib().hg_mt_u32(float(seed), count, out.ctypes.data_as(C.POINTER(C.c_uint32)))
    return out


def digamma(x):
    L = lib()
    return np.array([L.hg_digamma(float(v)) for v in np.atleast_1d(x)])


def initial_state(seed, n, m, k, hier, bias, rows=None) -> dict:
    """HGAPRec::initialize on the host -> {state name: array} (hpf_set_state layout).
    rows = (lo, hi): the user-side arrays of that range only, as one rank of several keeps them;
    the dict then also holds "_word_after", the generator's next 32-bit word."""
    from .capi import STATE_NAMES
    L = lib()
    out = {}
    if rows is None:
        s = C.c_void_p(L.hg_state_new(float(seed), n, m, k, int(hier), int(bias)))
    else:
        w = C.c_uint32(0)
        s = C.c_void_p(L.hg_state_new_range(float(seed), n, m, k, int(hier), int(bias), int(rows[0]), int(rows[1]), C.byref(w)))
        out["_word_after"] = int(w.value)
        n = int(rows[1]) - int(rows[0])
    try:
        for idx, name in enumerate(STATE_NAMES):
            p = C.POINTER(C.c_double)()
            cnt = L.hg_state_get(s, idx, C.byref(p))
            if cnt:
                a = np.ctypeslib.as_array(p, shape=(cnt,)).copy()
                obj, kind = idx // 4, idx % 4
                if obj <= 1 and not (kind == 1 and not hier):
                    a = a.reshape((n if obj == 0 else m), k)
                out[name] = a
    finally:
        L.hg_state_free(s)
    return out


def save_matrix(path, a, ids=None):
    a = np.ascontiguousarray(a, np.float64)
    i = None if ids is None else np.ascontiguousarray(ids, np.uint32)
    return lib().hg_save_matrix(str(path).encode(), a.ctypes.data_as(C.POINTER(C.c_double)), a.shape[0],
                                a.shape[1], None if i is None else i.ctypes.data_as(C.POINTER(C.c_uint32)),
                                0 if i is None else i.size)


def save_vector(path, a, ids=None):
    a = np.ascontiguousarray(a, np.float64)
    i = None if ids is None else np.ascontiguousarray(ids, np.uint32)
    return lib().hg_save_vector(str(path).encode(), a.ctypes.data_as(C.POINTER(C.c_double)), a.shape[0],
                                None if i is None else i.ctypes.data_as(C.POINTER(C.c_uint32)),
                                0 if i is None else i.size)


def load_matrix(path, rows, cols, ids=None) -> np.ndarray:
    """read back what save_matrix wrote: (rows, cols) float64.  ids: the id expected in the second column of each row
    (the ratings' seq2user / seq2item); None: the column is not compared.  Raises ValueError with the reader's message
    ("<path>: line N: ...") for a missing or short file, a short row or an id that differs."""
    out = np.empty((int(rows), int(cols)), np.float64)
    i = None if ids is None else np.ascontiguousarray(ids, np.uint32)
    err = C.create_string_buffer(1024)
    rc = lib().hg_load_matrix(str(path).encode(), out.ctypes.data_as(C.POINTER(C.c_double)), int(rows), int(cols),
                              None if i is None else i.ctypes.data_as(C.POINTER(C.c_uint32)), 0 if i is None else i.size,
                              err, 1024)
    if rc:
        raise ValueError(err.value.decode())
    return out


def load_vector(path, rows, ids=None) -> np.ndarray:
    """read back what save_vector wrote (or a one-column matrix such as thetabias.tsv): (rows,) float64"""
    out = np.empty(int(rows), np.float64)
    i = None if ids is None else np.ascontiguousarray(ids, np.uint32)
    err = C.create_string_buffer(1024)
    rc = lib().hg_load_vector(str(path).encode(), out.ctypes.data_as(C.POINTER(C.c_double)), int(rows),
                              None if i is None else i.ctypes.data_as(C.POINTER(C.c_uint32)), 0 if i is None else i.size,
                              err, 1024)
    if rc:
        raise ValueError(err.value.decode())
    return out


def shape_over_rate(shape, rate, rate_path="rate.tsv") -> np.ndarray:
    """the expectations of a model saved without -hier, as the CLI forms them: shape / rate[None, :].  Raises ValueError
    ("<rate_path>: line c+1: ...") for a rate that is not finite and > 0"""
    E = np.array(shape, np.float64, order="C", ndmin=2)
    r = np.ascontiguousarray(rate, np.float64)
    if r.shape != (E.shape[1],):
        raise ValueError("rate: one value per column of shape")
    err = C.create_string_buffer(1024)
    dp = C.POINTER(C.c_double)
    if lib().hg_shape_over_rate(E.ctypes.data_as(dp), E.shape[0], E.shape[1], r.ctypes.data_as(dp), str(rate_path).encode(), err, 1024):
        raise ValueError(err.value.decode())
    return E


def gamma_expectations(shape, rate, rate_path="rate.tsv"):
    """-fold-in's item side as the CLI forms it: (shape / rate, digamma(shape) - log(rate)); rate shaped like shape, or one
    value per column.  Raises ValueError ("<rate_path>: ... (row r)") for a shape or a rate that is not > 0"""
    E = np.array(shape, np.float64, order="C", ndmin=2)
    r = np.ascontiguousarray(rate, np.float64)
    if r.shape != E.shape and r.shape != (E.shape[1],):
        raise ValueError("rate: shaped like shape, or one value per column")
    L = np.empty_like(E)
    err = C.create_string_buffer(1024)
    dp = C.POINTER(C.c_double)
    if lib().hg_gamma_expectations(E.ctypes.data_as(dp), L.ctypes.data_as(dp), r.ctypes.data_as(dp), E.shape[0], E.shape[1],
                                   int(r.ndim == 1), str(rate_path).encode(), err, 1024):
        raise ValueError(err.value.decode())
    return E, L


def chunk_walk(rows, chunk=0):
    """the reports' walk over [0, rows) in chunks (chunk 0: the default size) -> [(r0, r1), ...]"""
    cnt = lib().hg_chunk_walk(rows, chunk, None, 0)
    out = np.zeros(2 * max(cnt, 1), np.uint64)
    lib().hg_chunk_walk(rows, chunk, out.ctypes.data_as(C.POINTER(C.c_uint64)), cnt)
    return [(int(out[2 * j]), int(out[2 * j + 1])) for j in range(cnt)]


def chunk_offsets(ptr, b0, b1):
    """ptr[b0 .. b1] counted from ptr[b0]"""
    p = np.ascontiguousarray(ptr, np.uint64)
    out = np.empty(b1 - b0 + 1, np.uint64)
    lib().hg_chunk_offsets(p.ctypes.data_as(C.POINTER(C.c_uint64)), b0, b1, out.ctypes.data_as(C.POINTER(C.c_uint64)))
    return out


def write_topn(path, sel, items, scores, real, row_ids, item_ids, given=None) -> int:
    """the reports' list writer: items / scores are (len(sel), N), the first `real` entries of a list exist; given: a
    Ratings whose r(row, item) == 0 an entry must meet to be written.  Returns the number of lines"""
    s = np.ascontiguousarray(sel, np.uint32)
    it = np.ascontiguousarray(items, np.uint32).reshape(s.size, -1)
    sc = np.ascontiguousarray(scores, np.float64).reshape(s.size, -1)
    ri, ii = np.ascontiguousarray(row_ids, np.uint32), np.ascontiguousarray(item_ids, np.uint32)
    u32p = C.POINTER(C.c_uint32)
    n = lib().hg_write_topn(str(path).encode(), None if given is None else given._r, s.ctypes.data_as(u32p), s.size,
                            it.ctypes.data_as(u32p), sc.ctypes.data_as(C.POINTER(C.c_double)), it.shape[1], int(real),
                            ri.ctypes.data_as(u32p), ii.ctypes.data_as(u32p))
    if n < 0:
        raise OSError(f"cannot write {path}")
    return n


def write_thompson(path, sel, items, scores, real, row_ids, item_ids, given=None) -> int:
    """the writer of recommend_thompson.tsv: items / scores are (D, len(sel), N), draw t's lists of the selected rows; the
    lines are user id, item id, draw, score -- rows in the order of sel, within a row the draws ascending, under
    write_topn's rule.  Returns the number of lines"""
    s = np.ascontiguousarray(sel, np.uint32)
    it = np.ascontiguousarray(items, np.uint32)
    sc = np.ascontiguousarray(scores, np.float64)
    if it.ndim != 3 or it.shape[1] != s.size or sc.shape != it.shape:
        raise ValueError("items and scores: (draws, len(sel), N)")
    ri, ii = np.ascontiguousarray(row_ids, np.uint32), np.ascontiguousarray(item_ids, np.uint32)
    u32p = C.POINTER(C.c_uint32)
    n = lib().hg_write_thompson(str(path).encode(), None if given is None else given._r, s.ctypes.data_as(u32p), s.size,
                                it.ctypes.data_as(u32p), sc.ctypes.data_as(C.POINTER(C.c_double)), it.shape[0], it.shape[2], int(real),
                                ri.ctypes.data_as(u32p), ii.ctypes.data_as(u32p))
    if n < 0:
        raise OSError(f"cannot write {path}")
    return n


def write_diverse(path, sel, items, scores, maxsim, row_ids, item_ids, given=None):
    """the writer of recommend_diverse.tsv: items / scores / maxsim are (len(sel), N) as Hpf.recommend_diverse returns
    them; the lines are user id, item id, score, maxsim -- rows in the order of sel, each list in pick order up to its
    first padding entry, under write_topn's rule for given items.  Returns (the number of lines, the sum of the maxsim
    column)"""
    s = np.ascontiguousarray(sel, np.uint32)
    it = np.ascontiguousarray(items, np.uint32)
    sc = np.ascontiguousarray(scores, np.float64)
    ms = np.ascontiguousarray(maxsim, np.float64)
    if it.ndim != 2 or it.shape[0] != s.size or sc.shape != it.shape or ms.shape != it.shape:
        raise ValueError("items, scores and maxsim: (len(sel), N)")
    ri, ii = np.ascontiguousarray(row_ids, np.uint32), np.ascontiguousarray(item_ids, np.uint32)
    u32p, dp = C.POINTER(C.c_uint32), C.POINTER(C.c_double)
    total = C.c_double(0.0)
    n = lib().hg_write_diverse(str(path).encode(), None if given is None else given._r, s.ctypes.data_as(u32p), s.size,
                               it.ctypes.data_as(u32p), sc.ctypes.data_as(dp), ms.ctypes.data_as(dp), it.shape[1],
                               ri.ctypes.data_as(u32p), ii.ctypes.data_as(u32p), C.byref(total))
    if n < 0:
        raise OSError(f"cannot write {path}")
    return n, total.value


def format_fixed8(values):
    """the writers' "%.8f" (exact, printf-compatible) for an array -> list of str"""
    a = np.ascontiguousarray(values, np.float64)
    buf = C.create_string_buffer(a.size * 420 + 16)
    n = lib().hg_format_fixed8(a.ctypes.data_as(C.POINTER(C.c_double)), a.size, buf)
    return buf.raw[:n].decode().split("\n")[:-1]


def partition_users(rowptr, world):
    """the C++ host's user sharding (same rule as hgaprec_amd.dist.partition_users)"""
    rp = np.ascontiguousarray(rowptr, np.int64)
    out = np.empty(2 * world, np.uint32)
    lib().hg_partition_users(rp.ctypes.data_as(C.POINTER(C.c_int64)), rp.size - 1, world,
                             out.ctypes.data_as(C.POINTER(C.c_uint32)))
    return [(int(out[2 * r]), int(out[2 * r + 1])) for r in range(world)]


def stop_rule(iters, series):
    it = np.ascontiguousarray(iters, np.uint32)
    a = np.ascontiguousarray(series, np.float64)
    why = (C.c_int * it.size)()
    at = lib().hg_stop_rule(it.ctypes.data_as(C.POINTER(C.c_uint32)), a.ctypes.data_as(C.POINTER(C.c_double)),
                            it.size, why)
    return at, list(why)


EVAL_USER_FIELDS = ("ntest", "hits10", "hits100", "best_rank", "sum_rank", "nranked")
EVAL_MEAN_FIELDS = ("users", "pairs", "precision10", "precision100", "recall100", "mrr", "meanrank")


def eval_from_ranks(q_ptr, rank, nranked):
    """-eval-all's arithmetic (eval_from_ranks, hgaprec_host.hpp): user b's ranks are rank[q_ptr[b]:q_ptr[b + 1]], nranked[b]
    the items counted as ranked for it -> (per_user: (users, 6) uint64 in the order of EVAL_USER_FIELDS,
    means: dict over EVAL_MEAN_FIELDS; users and pairs are ints)"""
    qp = np.ascontiguousarray(q_ptr, np.uint64)
    rk = np.ascontiguousarray(rank, np.uint32)
    nr = np.ascontiguousarray(nranked, np.uint32)
    nu = qp.size - 1
    if nu < 0 or nr.size != nu or (nu and int(qp[-1]) > rk.size):
        raise ValueError("q_ptr: len(nranked) + 1 entries, the last one at most len(rank)")
    per = np.zeros((nu, 6), np.uint64)
    means = np.zeros(7, np.float64)
    lib().hg_eval_from_ranks(qp.ctypes.data_as(C.POINTER(C.c_uint64)), rk.ctypes.data_as(C.POINTER(C.c_uint32)),
                             nr.ctypes.data_as(C.POINTER(C.c_uint32)), nu, per.ctypes.data_as(C.POINTER(C.c_uint64)),
                             means.ctypes.data_as(C.POINTER(C.c_double)))
    out = dict(zip(EVAL_MEAN_FIELDS, means.tolist()))
    out["users"], out["pairs"] = int(out["users"]), int(out["pairs"])
    return per, out
