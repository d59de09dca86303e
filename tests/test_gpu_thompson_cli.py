"""-m gpu: `hgaprec -recommend N -thompson D -thompson-seed S` on a trained model, with and without -bias:
recommend_thompson.tsv is the binding's hpf_recommend_thompson(seed = S, draw = t), t < D, on the state the run loads -- E
from the expectation files as every score mode loads it, the shapes from the shape files -- printed by the writer's rule,
line for line; recommend.tsv is byte for byte what the run without the flag writes; the same behind -fold-in."""
import numpy as np
import pytest

from hgaprec_amd import hostlib
from hgaprec_amd.capi import Hpf
from tests.test_gpu_fold_in_cli import _item_side, _write_new_users
from tests.test_gpu_moments_cli import _shapes
from tests.test_gpu_recommend import _args
from tests.test_gpu_score_modes import K, M, N, _device, _outdir, _run, fx  # noqa: F401

pytestmark = pytest.mark.gpu
REC, DRAWS, SEED = 10, 3, 5


def _lines(uids, iids, users, lists, given):
    """the writer's rule: users in order, within a user the draws ascending, each list best first, no given item"""
    return ["%d\t%d\t%d\t%.5f" % (uids[u], iids[it], t, s) for b, u in enumerate(users) for t, (items, scores) in enumerate(lists)
            for it, s in zip(items[b], scores[b]) if not given(u, it)]


@pytest.mark.parametrize("tag", ["hier", "flat"])
def test_cli_thompson_is_the_binding_and_leaves_recommend_tsv_alone(fx, tag):  # noqa: F811
    f = fx
    plain = _args(f, f.data, tag, ["-recommend", REC], "thompson_plain")
    _run(f.tmp, plain)
    args = _args(f, f.data, tag, ["-recommend", REC, "-thompson", DRAWS, "-thompson-seed", SEED], "thompson")
    _run(f.tmp, args)
    out, out0 = _outdir(f, args), _outdir(f, plain)
    assert (out / "recommend.tsv").read_bytes() == (out0 / "recommend.tsv").read_bytes()
    assert (out / "recommend.txt").read_bytes() == (out0 / "recommend.txt").read_bytes()
    assert not (out0 / "recommend_thompson.tsv").exists()
    got = (out / "recommend_thompson.tsv").read_text().splitlines()

    users = np.arange(N, dtype=np.uint32)
    mlists = [np.sort(f.valid[1][f.valid[0] == u]) for u in users]
    mptr = np.zeros(N + 1, np.uint64)
    mptr[1:] = np.cumsum([len(x) for x in mlists])
    D = _device(f, tag)
    try:
        for w, a in _shapes(f, tag).items():
            D.set_state(w, a)
        lists = [D.recommend_thompson(users, REC, SEED, t, mptr, np.concatenate(mlists).astype(np.uint32)) for t in range(DRAWS)]
    finally:
        D.close()
    want = _lines(f.s2u, f.s2i, users, lists, lambda u, it: f.train_r[u, it] != 0)
    assert len(want) > N * DRAWS and got == want
    assert (out / "recommend_thompson.txt").read_text() == "%d\t%d\t%d\t%d\t%d\n" % (N, len(got), REC, DRAWS, SEED)
    # the draws differ from each other, and a user's list is best first within a draw
    assert not np.array_equal(lists[0][0], lists[1][0])
    last = {}
    for ln in got:
        u, _, t, s = ln.split("\t")
        assert (u, t) not in last or float(s) <= last[(u, t)], ln
        last[(u, t)] = float(s)
    # without -thompson-seed the seed is 0
    args0 = _args(f, f.data, tag, ["-recommend", REC, "-thompson", 1], "thompson_seed0")
    _run(f.tmp, args0)
    assert (_outdir(f, args0) / "recommend_thompson.txt").read_text().split("\t")[3:] == ["1", "0\n"]


def test_cli_thompson_behind_fold_in(fx):  # noqa: F811
    f = fx
    new = f.tmp / "new_users_thompson.tsv"
    _write_new_users(f, new)
    common = f.base + f.flags["hier"] + ["-model-dir", f.model["hier"], "-fold-in", new, "-fold-iters", 5, "-recommend", REC]
    plain, args = common + ["-label", "fold_thompson_plain"], common + ["-label", "fold_thompson", "-thompson", DRAWS, "-thompson-seed", SEED]
    _run(f.tmp, plain)
    _run(f.tmp, args)
    out, out0 = _outdir(f, args), _outdir(f, plain)
    for name in ("foldin_recommend.tsv", "foldin_recommend.txt", "foldin_htheta.tsv", "foldin_htheta_shape.tsv", "foldin.txt"):
        assert (out / name).read_bytes() == (out0 / name).read_bytes(), name
    assert not (out0 / "foldin_recommend_thompson.tsv").exists() and not (out / "recommend_thompson.tsv").exists()
    got = (out / "foldin_recommend_thompson.tsv").read_text().splitlines()
    # the binding on a handle folded in the same way, the item side's shapes handed in behind the fold-in as the run does
    nu, _ = f.R.read_fold_in(new)
    ids = nu.seq2user()
    rowptr, col, val = nu.csr()
    shapes = _shapes(f, "hier")
    D = Hpf(nu.n, M, K, hier=True, bias=True)
    try:
        D.upload_csr(rowptr, col, val)
        for w, a in _item_side(f, "hier").items():
            D.set_state(w, a)
        D.fold_in(5)
        for w in ("BETA_SHAPE", "IBIAS_SHAPE"):
            D.set_state(w, shapes[w])
        users = np.arange(nu.n, dtype=np.uint32)
        lists = [D.recommend_thompson(users, REC, SEED, t) for t in range(DRAWS)]
    finally:
        D.close()
    mine = [set(col[rowptr[b]:rowptr[b + 1]].tolist()) for b in range(nu.n)]
    want = _lines(ids, f.s2i, users, lists, lambda u, it: int(it) in mine[u])
    assert len(want) > 0 and got == want
    assert (out / "foldin_recommend_thompson.txt").read_text() == "%d\t%d\t%d\t%d\t%d\n" % (nu.n, len(got), REC, DRAWS, SEED)


@pytest.mark.parametrize("tail,msg", [
    (["-thompson", "2"], "-thompson goes with -recommend N"),
    (["-recommend", "300", "-thompson", "2"], "-thompson needs -recommend N with N <= 256"),
    (["-recommend", "5", "-thompson", "65"], "-thompson needs the number of posterior draws"),
    (["-recommend", "5", "-thompson-seed", "1"], "-thompson-seed goes with -thompson D"),
    (["-audience", "5", "-thompson", "2"], "-thompson goes with -recommend N, not with -audience")])
def test_cli_refusals(fx, tail, msg):  # noqa: F811
    f = fx
    r = _run(f.tmp, f.base + ["-model-dir", f.model["flat"], "-label", "thompson_refused"] + tail, ok=False)
    assert r.returncode != 0 and msg in r.stdout + r.stderr, (r.returncode, r.stdout[-500:], r.stderr[-500:])
