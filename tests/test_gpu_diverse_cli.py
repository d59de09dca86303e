"""-m gpu: `hgaprec -recommend N -diverse L [-diverse-pool P]` on a saved model: recommend_diverse.tsv is the binding's
hpf_recommend_diverse(topn = N, pool = P, lambda = L) on the state the run loads, printed by the writer's rule, line for line;
recommend.tsv is byte for byte what the run without the flag writes; the same behind -fold-in.  On a model whose item side
is clustered (the saved -hier model with its htheta / hbeta replaced) the mean maxsim of the lists at -diverse 0.7 is below
that at -diverse 1."""
import shutil

import numpy as np
import pytest

from hgaprec_amd import hostlib
from hgaprec_amd.capi import Hpf
from tests.test_gpu_diverse import PAD, clustered
from tests.test_gpu_fold_in_cli import _item_side, _write_new_users
from tests.test_gpu_recommend import _args
from tests.test_gpu_score_modes import K, M, N, _device, _outdir, _run, fx  # noqa: F401

pytestmark = pytest.mark.gpu
REC, POOL, LAM = 10, 40, 0.7


def _lines(uids, iids, users, out, given):
    """the writer's rule: users in order, each list in pick order up to its padding, no given item"""
    items, scores, maxsim, _ = out
    lines, total = [], 0.0
    for b, u in enumerate(users):
        for it, s, ms in zip(items[b], scores[b], maxsim[b]):
            if it == PAD:
                break
            if not given(u, it):
                lines.append("%d\t%d\t%.5f\t%.5f" % (uids[u], iids[it], s, ms))
                total += ms
    return lines, total


def _masks(f, users):
    mlists = [np.sort(f.valid[1][f.valid[0] == u]) for u in users]
    mptr = np.zeros(len(users) + 1, np.uint64)
    mptr[1:] = np.cumsum([len(x) for x in mlists])
    return mptr, np.concatenate(mlists).astype(np.uint32)


def _txt(n_users, lines, total, rec, pool, lam):
    return "%d\t%d\t%d\t%d\t%g\t%.5f\n" % (n_users, len(lines), rec, pool, lam, total / len(lines) if lines else 0.0)


@pytest.mark.parametrize("tag", ["hier", "flat"])
def test_cli_diverse_is_the_binding_and_leaves_recommend_tsv_alone(fx, tag):  # noqa: F811
    f = fx
    plain = _args(f, f.data, tag, ["-recommend", REC], "diverse_plain")
    _run(f.tmp, plain)
    args = _args(f, f.data, tag, ["-recommend", REC, "-diverse", LAM, "-diverse-pool", POOL], "diverse")
    _run(f.tmp, args)
    out, out0 = _outdir(f, args), _outdir(f, plain)
    assert (out / "recommend.tsv").read_bytes() == (out0 / "recommend.tsv").read_bytes()
    assert (out / "recommend.txt").read_bytes() == (out0 / "recommend.txt").read_bytes()
    assert not (out0 / "recommend_diverse.tsv").exists()
    got = (out / "recommend_diverse.tsv").read_text().splitlines()

    users = np.arange(N, dtype=np.uint32)
    mptr, mitems = _masks(f, users)
    D = _device(f, tag)
    try:
        lists = D.recommend_diverse(users, REC, pool=POOL, lam=LAM, mask_ptr=mptr, mask_items=mitems)
        dflt = D.recommend_diverse(users, REC, lam=LAM, mask_ptr=mptr, mask_items=mitems)
    finally:
        D.close()
    want, total = _lines(f.s2u, f.s2i, users, lists, lambda u, it: f.train_r[u, it] != 0)
    assert len(want) > N and got == want
    assert (out / "recommend_diverse.txt").read_text() == _txt(N, want, total, REC, POOL, LAM)
    # without -diverse-pool the pool is min(256, 4 N) -- the binding's default too
    args0 = _args(f, f.data, tag, ["-recommend", REC, "-diverse", LAM], "diverse_default_pool")
    _run(f.tmp, args0)
    want0, total0 = _lines(f.s2u, f.s2i, users, dflt, lambda u, it: f.train_r[u, it] != 0)
    assert (_outdir(f, args0) / "recommend_diverse.tsv").read_text().splitlines() == want0
    assert (_outdir(f, args0) / "recommend_diverse.txt").read_text() == _txt(N, want0, total0, REC, 4 * REC, LAM)
    # -explain and -because keep describing recommend.tsv
    both = _args(f, f.data, tag, ["-recommend", REC, "-explain", 2], "diverse_explain_plain")
    both_d = _args(f, f.data, tag, ["-recommend", REC, "-explain", 2, "-diverse", LAM], "diverse_explain")
    _run(f.tmp, both)
    _run(f.tmp, both_d)
    assert (_outdir(f, both_d) / "recommend_explain.tsv").read_bytes() == (_outdir(f, both) / "recommend_explain.tsv").read_bytes()


def test_cli_diverse_lowers_the_mean_maxsim_on_a_clustered_model(fx):  # noqa: F811
    f = fx
    d = f.tmp / "clustered_model"
    if not d.exists():
        shutil.copytree(f.model["hier"], d)
    theta, beta, _ = clustered(N, M, K, 2026)
    assert hostlib.save_matrix(d / "htheta.tsv", theta, f.s2u) == 0 and hostlib.save_matrix(d / "hbeta.tsv", beta, f.s2i) == 0
    common = f.base + f.flags["hier"] + ["-model-dir", d, "-recommend", REC, "-diverse-pool", POOL]
    mean = {}
    for lam in (0.7, 1):
        args = common + ["-diverse", lam, "-label", f"clustered_{lam}"]
        _run(f.tmp, args)
        out = _outdir(f, args)
        fields = (out / "recommend_diverse.txt").read_text().split("\t")
        assert fields[:5] == [str(N), fields[1], str(REC), str(POOL), "%g" % lam] and int(fields[1]) > N
        rows = [ln.split("\t") for ln in (out / "recommend_diverse.tsv").read_text().splitlines()]
        assert len(rows) == int(fields[1])
        mean[lam] = float(fields[5])
        assert abs(mean[lam] - np.mean([float(r[3]) for r in rows])) < 1e-4          # the txt's mean is the column's (printed at 5 digits)
        if lam == 1:                              # lambda = 1: recommend.tsv's lines (with the biases every unmasked score is > 0)
            rec = [ln.split("\t") for ln in (out / "recommend.tsv").read_text().splitlines()]
            assert [r[:3] for r in rows] == rec
    print(f"mean maxsim: -diverse 0.7 {mean[0.7]:.5f}, -diverse 1 {mean[1]:.5f}")
    assert mean[0.7] < mean[1]


def test_cli_diverse_behind_fold_in(fx):  # noqa: F811
    f = fx
    new = f.tmp / "new_users_diverse.tsv"
    _write_new_users(f, new)
    common = f.base + f.flags["hier"] + ["-model-dir", f.model["hier"], "-fold-in", new, "-fold-iters", 5, "-recommend", REC]
    plain, args = common + ["-label", "fold_diverse_plain"], common + ["-label", "fold_diverse", "-diverse", LAM, "-diverse-pool", POOL]
    _run(f.tmp, plain)
    _run(f.tmp, args)
    out, out0 = _outdir(f, args), _outdir(f, plain)
    for name in ("foldin_recommend.tsv", "foldin_recommend.txt", "foldin_htheta.tsv", "foldin_htheta_shape.tsv", "foldin.txt"):
        assert (out / name).read_bytes() == (out0 / name).read_bytes(), name
    assert not (out0 / "foldin_recommend_diverse.tsv").exists() and not (out / "recommend_diverse.tsv").exists()
    got = (out / "foldin_recommend_diverse.tsv").read_text().splitlines()
    # the binding on a handle folded in the same way
    nu, _ = f.R.read_fold_in(new)
    ids = nu.seq2user()
    rowptr, col, val = nu.csr()
    D = Hpf(nu.n, M, K, hier=True, bias=True)
    try:
        D.upload_csr(rowptr, col, val)
        for w, a in _item_side(f, "hier").items():
            D.set_state(w, a)
        D.fold_in(5)
        users = np.arange(nu.n, dtype=np.uint32)
        lists = D.recommend_diverse(users, REC, pool=POOL, lam=LAM)
    finally:
        D.close()
    mine = [set(col[rowptr[b]:rowptr[b + 1]].tolist()) for b in range(nu.n)]
    want, total = _lines(ids, f.s2i, users, lists, lambda u, it: int(it) in mine[u])
    assert len(want) > 0 and got == want
    assert (out / "foldin_recommend_diverse.txt").read_text() == _txt(nu.n, want, total, REC, POOL, LAM)


@pytest.mark.parametrize("tail,msg", [
    (["-diverse", "0.5"], "-diverse goes with -recommend N"),
    (["-recommend", "300", "-diverse", "0.5"], "-diverse needs -recommend N with N <= 256"),
    (["-recommend", "5", "-diverse", "1.5"], "-diverse needs the weight of relevance against similarity"),
    (["-recommend", "5", "-diverse-pool", "20"], "-diverse-pool goes with -diverse L"),
    (["-recommend", "50", "-diverse", "0.5", "-diverse-pool", "20"], "-diverse-pool needs the number of candidates per user, N .. 256"),
    (["-audience", "5", "-diverse", "0.5"], "-diverse goes with -recommend N, not with -audience")])
def test_cli_refusals(fx, tail, msg):  # noqa: F811
    f = fx
    r = _run(f.tmp, f.base + ["-model-dir", f.model["flat"], "-label", "diverse_refused"] + tail, ok=False)
    assert r.returncode != 0 and msg in r.stdout + r.stderr, (r.returncode, r.stdout[-500:], r.stderr[-500:])
