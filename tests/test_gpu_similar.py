"""-m gpu: hpf_similar -- the nearest other rows of E[beta] (E[theta]) to a row, by dot product or cosine over the K factor
columns: unit_rows_kernel, similar_sweep_kernel (topn_sweep_kernel's body with query rows and swept rows from one matrix and
the row itself left out), topn_merge_kernel.

The dot product is held bit for bit to hpf_scores + numpy's stable sort; the normalisation alone to mpmath through
libhpf_probe.so; the cosine route to the dot route on the probe's unit rows; and the whole to the exact cosine."""
import ctypes as C
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from hgaprec_amd import capi
from tests.test_gpu_rank_edges import _train

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
NONE = 0xFFFFFFFF
U53 = 2.0 ** -53
TOPNS = [1, 10, 64, 65, 100, 256]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(got, want, what):
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape, what
    assert np.array_equal(got[0], want[0]), what + ": ids"
    assert np.array_equal(_bits(got[1]), _bits(want[1])), what + ": scores"


# ---------------------------------------------------------------------------------------------------------------------
# the probe: unit_rows_kernel on a host matrix (libhpf_probe.so; test infrastructure, the package never loads it)
# ---------------------------------------------------------------------------------------------------------------------
_probe = None


def _probe_lib():
    global _probe
    if _probe is None:
        import torch  # noqa: F401  one HIP runtime per process: torch first, as hgaprec_amd.capi.load_library does
        lib = C.CDLL(str(ROOT / "hgaprec_amd" / "libhpf_probe.so"))
        dp = C.POINTER(C.c_double)
        lib.probe_unit_rows.argtypes = [dp, C.c_uint32, C.c_uint32, C.c_uint32, dp]
        _probe = lib
    return _probe


def unit_rows(E, K=None, junk=None):
    """U of the rows of E[:, :K] as unit_rows_kernel makes them, in a matrix of even stride ld > K whose columns from K on
    hold `junk` on the way in (they take no part) and must be zeros on the way out -> U[:, :K]"""
    E = np.ascontiguousarray(E, np.float64)
    rows, K = E.shape[0], K or E.shape[1]
    ld = (K + 3) & ~1
    buf = np.full((rows, ld), 0.0 if junk is None else junk, np.float64)
    buf[:, :K] = E[:, :K]
    out = np.empty_like(buf)
    dp = C.POINTER(C.c_double)
    rc = _probe_lib().probe_unit_rows(buf.ctypes.data_as(dp), rows, ld, K, out.ctypes.data_as(dp))
    assert rc == 0, f"probe_unit_rows: HIP error {rc}"
    assert np.all(_bits(out[:, K:]) == 0), "columns >= K of U are zeros"
    return out[:, :K].copy()


# ---------------------------------------------------------------------------------------------------------------------
# handles and references
# ---------------------------------------------------------------------------------------------------------------------
def _gamma(rows, K, seed):
    """expectations of a Gamma(0.3, .) factor matrix: positive, wide in magnitude, and a few exact zeros"""
    rng = np.random.default_rng(seed)
    E = rng.gamma(0.3, 1.0, (rows, K)) / rng.gamma(3.0, 1.0, (rows, 1))
    E[rng.random((rows, K)) < 0.02] = 0.0
    return E


def _item_handle(E):
    """handle A: holds E[beta] and nothing else (no CSR, no user side)"""
    from hgaprec_amd.capi import Hpf
    D = Hpf(3, E.shape[0], E.shape[1], hier=False, bias=False)
    D.set_state("BETA_E", E)
    return D


def _square_scores(E, ids):
    """handle B: n_users = n_items = m, THETA_E = BETA_E = E, no bias, a tiny CSR -> hpf_scores of the rows ids"""
    from hgaprec_amd.capi import Hpf
    m, K = E.shape
    B = Hpf(m, m, K, hier=False, bias=False)
    try:
        rowptr, col, val, _ = _train(m, m)
        B.upload_csr(rowptr, col, val)
        B.set_state("THETA_E", E)
        B.set_state("BETA_E", E)
        return B.scores(ids)
    finally:
        B.close()


def _lists(S, ids, N):
    """what hpf_similar returns for score rows S[b] of the rows ids[b]: column ids[b] removed, a stable sort on (-score, id),
    the first N, padded"""
    m = S.shape[1]
    out = np.full((len(ids), N), NONE, np.uint32)
    sc = np.zeros((len(ids), N), np.float64)
    for b, a in enumerate(ids):
        cand = np.delete(np.arange(m), a)
        order = cand[np.argsort(-S[b, cand], kind="stable")][:N]
        out[b, :order.size] = order
        sc[b, :order.size] = S[b, order]
    return out, sc


def _ids(m, seed=5):
    """every row up to 130 (three workgroups of 64 query rows, the last ragged); of 1000 rows a hundred, the tile edges among them"""
    if m <= 130:
        return np.arange(m, dtype=np.uint32)
    rng = np.random.default_rng(seed)
    return np.concatenate([[0, 63, 64, m - 1], rng.permutation(m)[:96]]).astype(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the dot product, bit for bit against hpf_scores + numpy
# ---------------------------------------------------------------------------------------------------------------------
# every m with at least two K, every K with two m; K = 129, 200 take the NCH == 0 route
DOT_SHAPES = [(1, 1), (65, 1), (2, 3), (130, 3), (63, 4), (1000, 4), (64, 5), (1, 5), (65, 32), (2, 32), (130, 33), (63, 33),
              (1000, 100), (64, 100), (130, 128), (1000, 128), (65, 129), (1000, 129), (64, 200), (130, 200)]


@pytest.mark.parametrize("m,K", DOT_SHAPES)
def test_dot_equals_scores_and_a_stable_sort_bit_for_bit(m, K):
    E = _gamma(m, K, 1000 * K + m)
    ids = _ids(m)
    S = _square_scores(E, ids)
    A = _item_handle(E)
    try:
        for N in TOPNS:
            got = A.similar(1, ids, N, "dot")
            _same(got, _lists(S, ids, N), f"m={m} K={K} N={N}")
            Ne = min(N, m - 1)
            assert np.all(got[0][:, Ne:] == NONE) and np.all(_bits(got[1][:, Ne:]) == 0)        # the padding
            assert np.all(got[0][:, :Ne] < m) and not np.any(got[0] == ids[:, None])
    finally:
        A.close()


def test_shapes_cover_the_issue():
    ms, Ks = [s[0] for s in DOT_SHAPES], [s[1] for s in DOT_SHAPES]
    assert all(ms.count(m) >= 2 for m in (1, 2, 63, 64, 65, 130, 1000)) and set(ms) == {1, 2, 63, 64, 65, 130, 1000}
    assert all(Ks.count(K) == 2 for K in (1, 3, 4, 5, 32, 33, 100, 128, 129, 200)) and len(set(Ks)) == 10
    assert any(N >= m - 1 for m in ms for N in TOPNS)


def test_user_side_ignores_large_biases():
    """side 0 on a -hier -bias handle whose bias expectations are large: the lists are those of the same theta without bias"""
    from hgaprec_amd.capi import Hpf
    n, m, K = 130, 40, 5
    Et, Eb = _gamma(n, K, 77), _gamma(m, K, 78)
    rng = np.random.default_rng(79)
    Hb = Hpf(n, m, K, hier=True, bias=True)
    Pl = Hpf(n, m, K, hier=False, bias=False)
    try:
        Hb.set_state("THETA_E", Et)
        Hb.set_state("BETA_E", Eb)
        Hb.set_state("UBIAS_E", 1e6 * (1.0 + rng.random(n)))
        Hb.set_state("IBIAS_E", 1e6 * (1.0 + rng.random(m)))
        Pl.set_state("THETA_E", Et)
        ids = _ids(n)
        S = _square_scores(Et, ids)
        for metric in ("dot", "cosine"):
            for N in (10, 129, 200):
                got = Hb.similar(0, ids, N, metric)
                _same(got, Pl.similar(0, ids, N, metric), f"side 0, {metric}, N={N}")
                if metric == "dot":
                    _same(got, _lists(S, ids, N), f"side 0 against hpf_scores, N={N}")
    finally:
        Hb.close()
        Pl.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the normalisation alone, against mpmath at 60 digits
# ---------------------------------------------------------------------------------------------------------------------
def _norm_rows(K, seed):
    rng = np.random.default_rng(seed)
    rows = [r for r in _gamma(12, K, seed)]
    base = rng.gamma(0.3, 1.0, K) + 2.0 ** -30                       # no zero: the scaled copies stay in the normal range
    what = {"base": len(rows)}
    rows.append(base)
    what["down"] = len(rows)
    rows.append(base * 2.0 ** -900)
    what["up"] = len(rows)
    rows.append(base * 2.0 ** 900)
    what["one"] = len(rows)
    one = np.zeros(K)
    one[K // 2] = 3.7e-5
    rows.append(one)
    what["zero"] = len(rows)
    rows.append(np.zeros(K))
    if K >= 3:
        what["345"] = len(rows)
        for a in (-500, 0, 300):
            r = np.zeros(K)
            r[0], r[K - 1] = 3.0 * 2.0 ** a, 4.0 * 2.0 ** a
            rows.append(r)
        what["tiny"] = len(rows)
        r = np.full(K, 2.0 ** -600)
        r[1] = 1.0
        rows.append(r)
    return np.array(rows), what


@pytest.mark.parametrize("K", [1, 3, 100, 129])
def test_unit_rows_against_mpmath(K, capsys):
    """|U_k - exact| <= (K/2 + 3) 2^-53 exact: K roundings in a sum of positive squares, halved by the root, plus the root,
    the division and slack for second order.  The largest observed ratio is printed (DESIGN.md section 4e has the figures)."""
    import mpmath
    E, what = _norm_rows(K, 300 + K)
    U = unit_rows(E, K, junk=7.0)
    worst = 0.0
    with mpmath.workdps(60):
        for r in range(E.shape[0]):
            x = [mpmath.mpf(float(v)) for v in E[r]]
            nrm = mpmath.sqrt(mpmath.fsum(v * v for v in x))
            for k in range(K):
                if nrm == 0 or x[k] == 0:
                    assert _bits(U[r, k]) == 0, (r, k)
                    continue
                exact = x[k] / nrm
                ratio = float(abs(mpmath.mpf(float(U[r, k])) - exact) / (exact * mpmath.mpf(2) ** -53))
                worst = max(worst, ratio)
                assert ratio <= K / 2 + 3, (K, r, k, ratio)
    with capsys.disabled():
        print(f"\nunit_rows_kernel K={K}: largest |U - exact| / (2^-53 exact) = {worst:.3f} (bound {K / 2 + 3})")
    assert np.all(np.isfinite(U))
    # a row times 2^-900 and times 2^+900: bit-equal to the unscaled row's U
    assert np.array_equal(_bits(U[what["down"]]), _bits(U[what["base"]]))
    assert np.array_equal(_bits(U[what["up"]]), _bits(U[what["base"]]))
    # one nonzero entry: exactly 1.0 there; an all-zero row: zeros
    one = np.zeros(K)
    one[K // 2] = 1.0
    assert np.array_equal(_bits(U[what["one"]]), _bits(one))
    assert np.all(_bits(U[what["zero"]]) == 0)
    if K >= 3:
        for j in range(3):                                            # (3, 4, 0, ...) 2^a: exactly fl(0.6), fl(0.8)
            r = U[what["345"] + j]
            assert r[0] == 0.6 and r[K - 1] == 0.8 and np.all(_bits(r[1:K - 1]) == 0)
        t = U[what["tiny"]]                                           # 2^-600 beside 1.0: the squares underflow, U does not
        assert t[1] == 1.0 and np.all(t[[0] + list(range(2, K))] == 2.0 ** -600)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the cosine is the dot product of the unit rows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,K", [(64, 1), (130, 100), (65, 129), (1000, 33)])
def test_cosine_equals_dot_on_the_probes_unit_rows(m, K):
    E = _gamma(m, K, 2000 * K + m)
    E[m // 2] = 0.0                                                   # an all-zero row: cosine +0.0 with every row, no NaN
    ids = np.unique(np.concatenate([_ids(m), [m // 2]])).astype(np.uint32)
    A, Cc = _item_handle(E), _item_handle(unit_rows(E))
    try:
        for N in (1, 10, 100, 256):
            got = A.similar(1, ids, N, "cosine")
            _same(got, Cc.similar(1, ids, N, "dot"), f"m={m} K={K} N={N}")
            assert np.all(np.isfinite(got[1]))
        z = list(ids).index(m // 2)
        Ne = min(10, m - 1)
        got = A.similar(1, ids, 10, "cosine")
        assert np.all(_bits(got[1][z]) == 0) and np.array_equal(got[0][z, :Ne], np.delete(np.arange(m), m // 2)[:Ne])
    finally:
        A.close()
        Cc.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. the accuracy contract, end to end
# ---------------------------------------------------------------------------------------------------------------------
def test_cosine_against_mpmath_end_to_end(capsys):
    """K = 100, m = 1000, N = 10: every returned cosine is within (2K + 8) 2^-53 of the exact one -- per element of U the
    error is (K/2 + 2) u, twice, and the product chain adds (K + 3) u (tests/test_gpu_rank_edges.py's bound for it); all
    terms are positive and the cosine is <= 1 -- and a row that is not returned has an exact cosine <= that of the last
    one returned + twice the bound.  The largest observed error is printed (DESIGN.md section 4e has the figure)."""
    import mpmath
    m, K, N = 1000, 100, 10
    E = _gamma(m, K, 4242)
    ids = np.array([0, 63, 64, m - 1], np.uint32)
    A = _item_handle(E)
    try:
        got_i, got_s = A.similar(1, ids, N, "cosine")
    finally:
        A.close()
    bound = (2 * K + 8) * U53
    worst = 0.0
    with mpmath.workdps(60):
        X = [[mpmath.mpf(float(v)) for v in row] for row in E]
        nrm = [mpmath.sqrt(mpmath.fdot(x, x)) for x in X]
        for b, a in enumerate(ids):
            exact = [mpmath.fdot(X[a], X[j]) / (nrm[a] * nrm[j]) for j in range(m)]
            for j, s in zip(got_i[b], got_s[b]):
                err = float(abs(mpmath.mpf(float(s)) - exact[j]))
                worst = max(worst, err)
                assert err <= bound, (a, j, err / U53)
            last = exact[got_i[b][-1]]
            taken = set(int(j) for j in got_i[b]) | {int(a)}
            assert len(taken) == N + 1
            assert all(exact[j] <= last + 2 * bound for j in range(m) if j not in taken), a
            assert all(got_s[b][j] >= got_s[b][j + 1] for j in range(N - 1))
    with capsys.disabled():
        print(f"\nhpf_similar cosine K={K} m={m}: largest |dev - exact| = {worst / U53:.2f} x 2^-53 (bound {2 * K + 8})")


# ---------------------------------------------------------------------------------------------------------------------
# 5. ties and the self entry
# ---------------------------------------------------------------------------------------------------------------------
def test_ties_come_in_ascending_id_and_the_row_itself_never_does():
    m, K = 130, 5                                                     # 130 rows: the last tile and the last workgroup are ragged
    E = _gamma(m, K, 55) + 2.0 ** -20
    copies = {0: 0, 7: 3, 63: -7, 64: 0, 65: 40, 100: -300, 129: 1}   # row -> the power of two its copy of row 0 is scaled by
    for r, p in copies.items():
        E[r] = E[0] * 2.0 ** p
    sel = np.array([0, 63, 64, 129], np.uint32)
    A = _item_handle(E)
    try:
        ci, cs = A.similar(1, sel, 20, "cosine")
        di, ds = A.similar(1, sel, 129, "dot")
    finally:
        A.close()
    U = unit_rows(E)
    assert all(np.array_equal(_bits(U[r]), _bits(U[0])) for r in copies)
    for b, a in enumerate(sel):
        others = [r for r in sorted(copies) if r != a]
        # identical unit rows tie -- with the score the row would get against itself -- and come in ascending id
        assert list(ci[b, :len(others)]) == others, a
        assert np.all(_bits(cs[b, :len(others)]) == _bits(cs[b, 0])) and abs(cs[b, 0] - 1.0) < 1e-14
        assert cs[b, len(others)] < cs[b, 0] and a not in ci[b]
        # dot: the exact copies of the selected row (scale 2^0 against 2^0) are listed with the score they get
        assert a not in di[b] and sorted(di[b]) == [r for r in range(m) if r != a]
    b0, b64 = 0, 2
    assert 64 in di[b0] and 0 in di[b64]
    assert _bits(ds[b0][list(di[b0]).index(64)]) == _bits(ds[b64][list(di[b64]).index(0)])


# ---------------------------------------------------------------------------------------------------------------------
# 6. compaction, the threshold rule and splits: K = 1, exact scores, 5000 rows
# ---------------------------------------------------------------------------------------------------------------------
EDGE_M = 5000


def _edge_values(kind):
    i = np.arange(EDGE_M, dtype=np.int64)
    if kind == "ascending":                  # every row beats all before it: everything is accepted, a compaction every few tiles
        return i + 1
    if kind == "descending":                 # nothing is accepted after the first fill
        return EDGE_M - i
    if kind == "equal":                      # the strict > keeps later ties out
        return np.full(EDGE_M, 3, np.int64)
    half = EDGE_M // 2                       # plateaus of 600 equal scores that fall, then rise: ties straddle tiles and split ends
    fall = 100 - i[:half] // 600
    return np.concatenate([fall, fall.min() + (i[half:] - half) // 600])


@pytest.fixture(scope="module", params=["ascending", "descending", "equal", "plateaus"])
def edge(request):
    v = _edge_values(request.param).astype(np.float64)
    assert v.min() >= 1 and v.max() ** 2 < 2 ** 53                    # every product is exact in a double
    A = _item_handle(v[:, None].copy())
    yield request.param, A, v
    A.close()


@pytest.mark.parametrize("N", [10, 150])
def test_compaction_threshold_and_splits(edge, N):
    kind, A, v = edge
    sel = np.unique(np.concatenate([[0, 63, 64, 599, 600, 2499, 2500, EDGE_M - 1], np.arange(17, EDGE_M, 79)])).astype(np.uint32)
    # the case is what it is meant to be: two workgroups, several splits, each longer than a candidate buffer
    blocks, splits, tps = capi.recommend_grid(sel.size, EDGE_M, N)
    cap = capi.recommend_cap(N)
    assert blocks == 2 and splits > 1 and tps * 64 > cap and 64 < sel.size <= 128
    got = A.similar(1, sel, N, "dot")
    S = v[sel][:, None] * v[None, :]
    _same(got, _lists(S, sel, N), f"{kind} N={N}")
    if kind == "equal":
        assert np.array_equal(got[0][0], np.arange(1, N + 1, dtype=np.uint32))       # row 0 selected: 1 .. N


# ---------------------------------------------------------------------------------------------------------------------
# 7. batches
# ---------------------------------------------------------------------------------------------------------------------
def _batch_case():
    m, K = 130, 33
    E = _gamma(m, K, 909)
    sel = np.concatenate([np.arange(0, 117, 3), [6]]).astype(np.uint32)        # 40 rows; row 6 twice, in batches 0 and 2
    assert sel.size == 40 and sel[2] == 6 and sel[39] == 6
    return E, sel


_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from tests.test_gpu_similar import _batch_case, _item_handle
E, sel = _batch_case()
A = _item_handle(E)
out = []
for metric in ("dot", "cosine"):
    for N in (10, 100, 256):
        ids, sc = A.similar(1, sel, N, metric)
        out.append([ids.tolist(), sc.view(np.uint64).tolist()])
A.close()
print("RESULT " + json.dumps(out))
"""


def test_batches_give_the_same_lists():
    """HPF_LOO_BATCH=16: the 40 selected rows go through the kernels in three batches (16, 16, 8).  The library reads the
    variable when a handle is created, hence a fresh process."""
    env = dict(os.environ, HPF_LOO_BATCH="16")
    r = subprocess.run([sys.executable, "-c", _CHILD, str(ROOT)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][0][7:])
    E, sel = _batch_case()
    A = _item_handle(E)
    try:
        k = 0
        for metric in ("dot", "cosine"):
            for N in (10, 100, 256):
                i1, s1 = A.similar(1, sel, N, metric)
                assert np.array_equal(np.array(got[k][0], np.uint32), i1), (metric, N)
                assert np.array_equal(np.array(got[k][1], np.uint64), _bits(s1)), (metric, N)
                # a row selected twice: equal output rows
                assert np.array_equal(i1[2], i1[39]) and np.array_equal(_bits(s1[2]), _bits(s1[39]))
                k += 1
    finally:
        A.close()


# ---------------------------------------------------------------------------------------------------------------------
# 8. errors
# ---------------------------------------------------------------------------------------------------------------------
def test_errors():
    """every refusal of include/hpf.h's comment, each before anything is launched and with a message.  (An odd row stride --
    HPF_ERR_UNSUPPORTED, as for the other fused calls -- cannot be produced through hpf_create: every planned stride is a
    multiple of four.)"""
    from hgaprec_amd.capi import Hpf, HpfError
    m, K = 70, 4
    E = _gamma(m, K, 8)
    A = _item_handle(E)
    ids = np.arange(m, dtype=np.uint32)
    u32p, dp = C.POINTER(C.c_uint32), C.POINTER(C.c_double)
    try:
        want = A.similar(1, ids, 10, "dot")
        bad = ids.copy()
        bad[5] = m
        for args, msg in (((2, ids, 10, "dot"), "side"), ((-1, ids, 10, "dot"), "side"), ((1, ids, 10, 2), "metric"),
                          ((1, ids, 10, -1), "metric"), ((1, ids, 0, "dot"), "topn"), ((1, ids, 257, "cosine"), "topn"),
                          ((1, bad, 10, "dot"), "item index out of range"), ((1, bad, 10, "cosine"), "item index out of range")):
            with pytest.raises(HpfError, match=r"\(-1\).*" + msg):       # HPF_ERR_INVALID
                A.similar(*args)
        with pytest.raises(ValueError):
            A.similar(1, ids, 10, "euclid")
        # a null pointer with n_sel > 0
        out_i, out_s = np.empty((m, 10), np.uint32), np.empty((m, 10), np.float64)
        pi, po, ps = ids.ctypes.data_as(u32p), out_i.ctypes.data_as(u32p), out_s.ctypes.data_as(dp)
        for a in ((None, po, ps), (pi, None, ps), (pi, po, None)):
            assert A.lib.hpf_similar(A._h, 1, a[0], m, 10, 1, a[1], a[2]) == -1
            assert b"null pointer" in A.lib.hpf_last_error(A._h)
        # n_sel = 0 is fine, also with null pointers
        got = A.similar(1, np.zeros(0, np.uint32), 10)
        assert got[0].shape == (0, 10) and got[1].shape == (0, 10)
        assert A.lib.hpf_similar(A._h, 1, None, 0, 10, 0, None, None) == 0
        # no E on the user side of this handle: HPF_ERR_STATE; an id is judged against the side that was asked for
        with pytest.raises(HpfError, match=r"\(-6\).*E state not set"):
            A.similar(0, np.arange(3, dtype=np.uint32), 2, "dot")
        _same(A.similar(1, ids, 10, "dot"), want, "after the refused calls")
    finally:
        A.close()
    F = Hpf(5, 6, 3, hier=False, bias=False)
    try:
        for side in (0, 1):
            with pytest.raises(HpfError, match=r"\(-6\).*E state not set"):
                F.similar(side, np.arange(2, dtype=np.uint32), 2)
        F.set_state("THETA_E", _gamma(5, 3, 1))
        with pytest.raises(HpfError, match=r"\(-1\).*user index out of range"):
            F.similar(0, np.array([5], np.uint32), 2)
        got = F.similar(0, np.array([4, 4], np.uint32), 6)
        assert np.array_equal(got[0][0], got[0][1]) and sorted(got[0][0][:4]) == [0, 1, 2, 3] and np.all(got[0][:, 4:] == NONE)
    finally:
        F.close()
