"""-m gpu: hpf_recommend -- the top-N of every selected user from one sweep over the items (topn_sweep_kernel: streaming
selection into per-(user, split) candidate buffers, compacted when they fill; topn_merge_kernel) -- and `hgaprec -recommend N`.
Its contract: items and scores equal hpf_rank_topn's bit for bit."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from hgaprec_amd import capi
from tests.test_gpu_eval_all import allusers  # noqa: F401
from tests.test_gpu_loo_ranks import SHAPES, _case
from tests.test_gpu_score_modes import N as FX_N, _outdir, _run, _score_args, fx  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
NONE = 0xFFFFFFFF
TOPNS = [1, 10, 64, 100, 255, 256]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(got, want, what):
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape, what
    assert np.array_equal(got[0], want[0]), what + ": items"
    assert np.array_equal(_bits(got[1]), _bits(want[1])), what + ": scores"


# ---------------------------------------------------------------------------------------------------------------------
# 1. bit for bit against hpf_rank_topn
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,bias,m", SHAPES)
def test_recommend_equals_rank_topn_bit_for_bit(K, bias, m):
    D, rowptr, col, val, users, mask, mptr, mitems, q = _case(K, bias, m)
    try:
        for topn in TOPNS:
            want = D.rank_topn(users, topn, mptr, mitems)
            got = D.recommend(users, topn, mptr, mitems)
            _same(got, want, f"K={K} m={m} topn={topn}, mask list")
            Ne = min(topn, m)
            # user 3 has every item masked: items 0 .. Ne - 1 with zero bits; beyond m the padding
            assert np.array_equal(got[0][3, :Ne], np.arange(Ne, dtype=np.uint32)) and np.all(_bits(got[1][3]) == 0)
            assert np.all(got[0][:, Ne:] == NONE) and np.all(_bits(got[1][:, Ne:]) == 0)
            assert np.all(got[0][:, :Ne] < m)
            _same(D.recommend(users, topn), D.rank_topn(users, topn), f"K={K} m={m} topn={topn}, no mask list")
        assert m >= max(TOPNS) or m in (200, 70, 64)                # m < topn is among the cases
    finally:
        D.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. compaction and the threshold rule: K = 1, exact scores, 391 tiles
# ---------------------------------------------------------------------------------------------------------------------
EDGE_M, EDGE_N = 25000, 150


def _edge_beta(kind):
    i = np.arange(EDGE_M, dtype=np.int64)
    if kind == "ascending":                  # every item beats all before it: everything is accepted
        return i + 1
    if kind == "descending":                 # nothing is accepted after the first fill
        return EDGE_M - i
    if kind == "equal":                      # the strict > keeps later ties out
        return np.full(EDGE_M, 3, np.int64)
    # plateaus of 600 equal scores whose value falls, then a copy whose value rises: ties straddle tiles, compactions,
    # split ends and the two halves
    half = EDGE_M // 2
    fall = 100 - i[:half] // 600
    rise = fall.min() + (i[half:] - half) // 600
    return np.concatenate([fall, rise])


@pytest.fixture(scope="module", params=["ascending", "descending", "equal", "plateaus"])
def edge(request):
    """a handle as tests/test_gpu_rank_edges.py's _k1_state builds it: no -hier, its tiny training matrix (1 to 3 items per
    user, one stored with rating 0), THETA_E / BETA_E set directly.  theta_u is a power of two and beta_i a small integer:
    every score is exact in a double"""
    from hgaprec_amd.capi import Hpf
    from tests.test_gpu_rank_edges import _train
    beta = _edge_beta(request.param)
    theta = 2.0 ** (np.arange(EDGE_N) % 5 - 2)
    assert beta.min() >= 1 and beta.max() < 2 ** 40
    rowptr, col, val, zeroed = _train(EDGE_N, EDGE_M)
    D = Hpf(EDGE_N, EDGE_M, 1, hier=False, bias=False)
    D.upload_csr(rowptr, col, val)
    D.set_state("THETA_E", theta[:, None].copy())
    D.set_state("BETA_E", beta.astype(np.float64)[:, None].copy())
    users = np.arange(EDGE_N, dtype=np.uint32)
    # every fourth user masks items in the first tile, around a plateau end, a split end and the last item
    masks = [[0, 1, 63, 64, 599, 600, 601, 12499, 12500, 16 * 64 * 3, EDGE_M - 1, EDGE_M - 1] if u % 4 == 3 else [] for u in users]
    mptr = np.zeros(EDGE_N + 1, np.uint64)
    mptr[1:] = np.cumsum([len(x) for x in masks])
    mitems = np.array([i for x in masks for i in x], np.uint32)
    yield request.param, D, users, mptr, mitems, zeroed, theta, beta
    D.close()


@pytest.mark.parametrize("topn", [1, 100, 256])
def test_compaction_and_the_threshold_rule(edge, topn):
    kind, D, users, mptr, mitems, zeroed, theta, beta = edge
    # the case is what it is meant to be: 3 blocks, several splits, each long enough to fill and compact its buffers
    blocks, splits, tps = capi.recommend_grid(EDGE_N, EDGE_M, topn)
    cap = capi.recommend_cap(topn)
    assert blocks == 3 and splits > 1 and tps > cap // 64 and tps * 16 >= cap and (EDGE_M + 63) // 64 == 391
    want = D.rank_topn(users, topn, mptr, mitems)
    got = D.recommend(users, topn, mptr, mitems)
    _same(got, want, f"{kind} topn={topn}")
    # ... and what the exact scores say for the users without a mask list
    for u in (0, 1, 2, 64, 149):
        s = theta[u] * beta.astype(np.float64)
        s[sorted(zeroed[u])] = 0.0
        order = np.argsort(-s, kind="stable")[:topn]
        assert np.array_equal(got[0][u], order.astype(np.uint32)), f"{kind} topn={topn} user {u}"
        assert np.array_equal(_bits(got[1][u]), _bits(s[order]))
    if kind == "equal":
        assert not zeroed[0] and np.array_equal(got[0][0], np.arange(topn, dtype=np.uint32))


# ---------------------------------------------------------------------------------------------------------------------
# 3. batch boundary
# ---------------------------------------------------------------------------------------------------------------------
_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from tests.test_gpu_loo_ranks import _case, SHAPES
out = []
for K, bias, m in SHAPES:
    D, rowptr, col, val, users, mask, mptr, mitems, q = _case(K, bias, m)
    row = []
    for topn in (10, 100, 256):
        items, sc = D.recommend(users, topn, mptr, mitems)
        row.append([items.tolist(), sc.view(np.uint64).tolist()])
    out.append(row)
    D.close()
print("RESULT " + json.dumps(out))
"""


def test_batch_boundary_gives_the_same_lists():
    """HPF_LOO_BATCH=16: the 37 users go through the kernels in three batches (16, 16, 5), each with bit rows and candidate
    buffers of its own.  The library reads the variable, hence a fresh process."""
    env = dict(os.environ, HPF_LOO_BATCH="16")
    r = subprocess.run([sys.executable, "-c", _CHILD, str(ROOT)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][0][7:])
    for (K, bias, m), row in zip(SHAPES, got):
        D, rowptr, col, val, users, mask, mptr, mitems, q = _case(K, bias, m)
        for topn, (items, scbits) in zip((10, 100, 256), row):
            i1, s1 = D.recommend(users, topn, mptr, mitems)
            assert np.array_equal(np.array(items, np.uint32), i1), (K, m, topn)
            assert np.array_equal(np.array(scbits, np.uint64), _bits(s1)), (K, m, topn)
        D.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. routing and errors
# ---------------------------------------------------------------------------------------------------------------------
def test_routing_above_the_fused_range_and_errors():
    from hgaprec_amd.capi import HpfError
    K, bias, m = SHAPES[2]
    D, rowptr, col, val, users, mask, mptr, mitems, q = _case(K, bias, m)
    try:
        assert capi.RECOMMEND_FUSED_MAX == 256
        for topn in (257, 1024):
            _same(D.recommend(users, topn, mptr, mitems), D.rank_topn(users, topn, mptr, mitems), f"topn={topn}")
        bad_users, bad_items, bad_ptr = users.copy(), mitems.copy(), mptr.copy()
        bad_users[5] = D.n_users
        bad_items[-1] = m
        bad_ptr[0] = 1
        for args in ((users, 0, mptr, mitems), (users, 1025, mptr, mitems), (bad_users, 10, mptr, mitems),
                     (users, 10, mptr, bad_items), (users, 10, bad_ptr, mitems)):
            with pytest.raises(HpfError, match=r"\(-1\)"):            # HPF_ERR_INVALID
                D.recommend(*args)
        items, sc = D.recommend(np.zeros(0, np.uint32), 10)
        assert items.shape == (0, 10) and sc.shape == (0, 10)
        _same(D.recommend(users, 10, mptr, mitems), D.rank_topn(users, 10, mptr, mitems), "after the refused calls")
    finally:
        D.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. the CLI
# ---------------------------------------------------------------------------------------------------------------------
def _args(f, d, tag, mode, label):
    a = _score_args(f, tag, "MODE", label=label)
    k = a.index("MODE")
    return ["-dir", d] + a[2:k] + list(mode) + a[k + 1:]


@pytest.mark.parametrize("tag", ["hier", "flat"])
def test_cli_recommend_is_the_front_of_ranking_tsv(fx, allusers, tag):
    f = fx
    ga = _args(f, allusers, tag, ["-gen-ranking"], "genall_r")
    ra = _args(f, allusers, tag, ["-recommend", 100], "recall")
    _run(f.tmp, ga)
    _run(f.tmp, ra)
    gout, rout = _outdir(f, ga), _outdir(f, ra)
    want = ["\t".join(l.split("\t")[:3]) for l in (gout / "ranking.tsv").read_text().splitlines()]
    got = (rout / "recommend.tsv").read_text().splitlines()
    assert len(want) > 90 * FX_N and got == want
    assert (rout / "recommend.txt").read_text() == "%d\t%d\t%d\n" % (FX_N, len(got), 100)
    assert not (rout / "ranking.tsv").exists()


def test_cli_recommend_is_refused_with_ngpus(fx, allusers):
    f = fx
    args = _args(f, allusers, "hier", ["-recommend", 100], "recall2") + ["-ngpus", 2]
    r = _run(f.tmp, args, ok=False)
    assert r.returncode != 0 and "-recommend" in r.stderr and "without -ngpus" in r.stderr
    assert not (_outdir(f, args) / "recommend.tsv").exists()
