"""-m gpu: hpf_factor_top -- the topn heaviest rows of every factor column of one side: transpose_cols_kernel (a batch of
columns through LDS into contiguous rows) and then hpf_rank_topn's selection, topn_kernel, a workgroup per column.

The reference is a stable argsort of -E[:, k] per column; ids and the bit patterns of the values are compared for equality."""
import ctypes as C

import numpy as np
import pytest

from hgaprec_amd import capi

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF
OTHER = 7                                   # rows of the side that is not asked


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _gamma(rows, K, seed):
    rng = np.random.default_rng(seed)
    E = rng.gamma(0.3, 1.0, (rows, K)) / rng.gamma(3.0, 1.0, (rows, 1))
    E[rng.random((rows, K)) < 0.02] = 0.0
    return E


def _reference(E, topn):
    rows, K = E.shape
    ids = np.full((K, topn), NONE, np.uint32)
    vals = np.zeros((K, topn), np.float64)
    order = np.argsort(-E, axis=0, kind="stable")[:topn].T          # [K, min(topn, rows)]
    ids[:, :order.shape[1]] = order
    vals[:, :order.shape[1]] = np.take_along_axis(E, order.T, axis=0).T
    return ids, vals


def _handle(E, side, bias, hier=False):
    """E on the side asked for, a few random rows on the other; with bias, bias columns far larger than any factor"""
    rows, K = E.shape
    D = capi.Hpf(OTHER if side else rows, rows if side else OTHER, K, hier=hier, bias=bias)
    D.set_state("BETA_E" if side else "THETA_E", E)
    D.set_state("THETA_E" if side else "BETA_E", _gamma(OTHER, K, 99))
    if bias:
        D.set_state("UBIAS_E", np.full(D.n_users, 1e30))
        D.set_state("IBIAS_E", np.full(D.n_items, 1e30))
    return D


def _check(D, E, side, topn, what):
    ids, vals = D.factor_top(side, topn)
    wi, wv = _reference(E, topn)
    assert ids.shape == wi.shape and ids.dtype == np.uint32 and vals.dtype == np.float64, what
    assert np.array_equal(ids, wi), f"{what}: ids, first bad factor {np.argwhere((ids != wi).any(axis=1))[:1]}"
    assert np.array_equal(_bits(vals), _bits(wv)), what + ": values"
    return ids, vals


@pytest.mark.parametrize("rows", [1, 255, 256, 257, 5000])
@pytest.mark.parametrize("K", [1, 100, 129])
def test_lists_are_the_stable_argsort_of_each_column(rows, K):
    E = _gamma(rows, K, rows + K)
    for side, bias in ((1, False), (0, True)):
        D = _handle(E, side, bias, hier=bool(side))
        try:
            before = _bits(D.get_state("BETA_E" if side else "THETA_E")).copy()
            for topn in (1, 100, 1024):                             # topn > rows: the padding
                ids, vals = _check(D, E, side, topn, f"rows={rows} K={K} side={side} bias={bias} topn={topn}")
                real = min(topn, rows)
                assert np.all(ids[:, real:] == NONE) and np.all(_bits(vals[:, real:]) == 0)
                assert np.all(vals < 1e29)                          # a bias column never shows
            assert np.array_equal(before, _bits(D.get_state("BETA_E" if side else "THETA_E"))), "the state was written"
        finally:
            D.close()


def test_ties_by_id_across_transpose_tiles():
    """identical rows: every column is one value, the list is 0, 1, 2, ... across the 32-row tiles of the transpose and the
    256-entry strides of the selection; then two values, the larger on every third row"""
    rows, K = 1100, 70
    E = np.tile(_gamma(1, K, 1) + 0.5, (rows, 1))
    D = _handle(E, 1, False)
    try:
        for topn in (31, 33, 1024):
            ids, _ = _check(D, E, 1, topn, f"identical rows topn={topn}")
            assert np.array_equal(ids, np.tile(np.arange(topn, dtype=np.uint32), (K, 1)))
    finally:
        D.close()
    E[::3] *= 2.0
    E[:, 5] = 0.0                                                    # and a column of zeros
    D = _handle(E, 0, True)
    try:
        ids, _ = _check(D, E, 0, 1024, "two values")
        assert np.array_equal(ids[0, :367], np.arange(0, 1100, 3, dtype=np.uint32)) and ids[0, 367] == 1
        assert np.array_equal(ids[5], np.arange(1024, dtype=np.uint32))
    finally:
        D.close()


def test_column_batches_smaller_than_k(monkeypatch):
    """HPF_FACTOR_TOP_BATCH (read under HPF_EXPERIMENTAL when the handle is created): 129 columns in batches of 7, the last
    of 3; of 32 and 33, at the tile edge of the transpose"""
    rows, K = 300, 129
    E = _gamma(rows, K, 17)
    monkeypatch.setenv("HPF_EXPERIMENTAL", "1")
    for batch in ("7", "32", "33", "1"):
        monkeypatch.setenv("HPF_FACTOR_TOP_BATCH", batch)
        D = _handle(E, 1, True)
        try:
            _check(D, E, 1, 100, f"batch={batch}")
        finally:
            D.close()
    # the knob is ignored outside HPF_EXPERIMENTAL (and the result cannot tell)
    monkeypatch.delenv("HPF_EXPERIMENTAL")
    D = _handle(E, 0, False)
    try:
        _check(D, E, 0, 100, "knob ignored")
    finally:
        D.close()


def test_refusals_launch_nothing():
    rows, K = 50, 12
    E = _gamma(rows, K, 3)
    D = _handle(E, 1, False)
    try:
        lib, h = D.lib, D._h
        u32p, dp = C.POINTER(C.c_uint32), C.POINTER(C.c_double)
        ids, vals = np.zeros((K, 1024), np.uint32), np.zeros((K, 1024), np.float64)
        pi, pv = ids.ctypes.data_as(u32p), vals.ctypes.data_as(dp)
        for side in (-1, 2):
            assert lib.hpf_factor_top(h, side, 10, pi, pv) == -1, side
        for topn in (0, 1025, 0xFFFFFFFF):
            assert lib.hpf_factor_top(h, 1, topn, pi, pv) == -1, topn
            with pytest.raises(capi.HpfError):
                D.factor_top(1, topn)
        assert lib.hpf_factor_top(h, 1, 10, None, pv) == -1 and lib.hpf_factor_top(h, 1, 10, pi, None) == -1
        assert not ids.any() and not vals.any()                       # nothing was written
        assert np.array_equal(_bits(D.get_state("BETA_E")), _bits(E))
        _check(D, E, 1, 10, "a good call after the refusals")
    finally:
        D.close()
    # no E on the side asked for: HPF_ERR_STATE; the other side is served
    D = capi.Hpf(OTHER, rows, K, hier=False, bias=False)
    try:
        D.set_state("BETA_E", E)
        with pytest.raises(capi.HpfError, match=r"\(-6\)"):
            D.factor_top(0, 10)
        _check(D, E, 1, 10, "items without a user side")
    finally:
        D.close()
