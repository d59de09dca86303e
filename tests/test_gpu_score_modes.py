"""-m gpu: the CLI's score modes -- train, then `hgaprec ... -gen-ranking | -rmse | -msr -model-dir <trained dir>` --
against Python on the same factor files: once through the library (hostlib.load_* -> Hpf.set_state(*_E) ->
rank_topn / item_ranks, formatted like the driver: text-identical) and once through numpy alone."""
import math
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from hgaprec_amd import hostlib
from tests.util import make_problem

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "hgaprec_amd" / "hgaprec"
N, M, K = 150, 200, 5
SEED = 31


def _write_dataset(d, seed):
    """train.tsv = a make_problem matrix (every user and item is registered by it); per user 0-2 validation and
    1-3 test items outside the training row: every user has a test pair"""
    rng = np.random.default_rng(seed)
    rowptr, col, val = make_problem(N, M, 4000, seed)
    uid = rng.permutation(10 * N)[:N] + 1
    iid = rng.permutation(10 * M)[:M] + 1
    u = np.repeat(np.arange(N), np.diff(rowptr))
    d.mkdir(parents=True)
    with open(d / "train.tsv", "w") as f:
        for j in rng.permutation(u.size):
            f.write(f"{uid[u[j]]}\t{iid[col[j]]}\t{val[j]}\n")
    lines = {"validation.tsv": [], "test.tsv": []}
    for b in range(N):
        free = np.setdiff1d(np.arange(M), col[rowptr[b]:rowptr[b + 1]])
        pick = rng.permutation(free)[: 5]
        nv, nt = int(rng.integers(0, 3)), int(rng.integers(1, 4))
        for it in pick[:nv]:
            lines["validation.tsv"].append(f"{uid[b]}\t{iid[it]}\t{rng.integers(1, 6)}\n")
        for it in pick[nv:nv + nt]:
            lines["test.tsv"].append(f"{uid[b]}\t{iid[it]}\t{rng.integers(1, 6)}\n")
    for name, ls in lines.items():
        (d / name).write_text("".join(ls[j] for j in rng.permutation(len(ls))))
    (d / "test_users.tsv").write_text("".join(f"{x}\n" for x in rng.permutation(uid)[:40]))


def _run(cwd, args, ok=True):
    r = subprocess.run([str(EXE)] + [str(a) for a in args], cwd=cwd, capture_output=True, text=True, timeout=300)
    if ok:
        assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
    return r


class Fix:
    pass


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    """the data set, what the CLI's reader makes of it, and two trained models (-hier -bias, and plain)"""
    f = Fix()
    f.tmp = tmp_path_factory.mktemp("score_modes")
    f.data = f.tmp / "data"
    _write_dataset(f.data, SEED)
    f.base = ["-dir", f.data, "-n", N, "-m", M, "-k", K, "-rfreq", 2]
    f.flags = {"hier": ["-hier", "-bias", "-max-iterations", 3], "flat": []}
    f.model = {}
    for tag, fl in f.flags.items():
        _run(f.tmp, f.base + fl)
        f.model[tag] = f.tmp / hostlib.prefix([str(a) for a in f.base + fl])
        assert (f.model[tag] / ("hbeta.tsv" if tag == "hier" else "beta_shape.tsv")).exists()
    R = hostlib.Ratings(N, M)
    assert R.read_train(f.data / "train.tsv") == 0
    assert R.read_heldout(f.data / "validation.tsv", 0) == 0 and R.read_heldout(f.data / "test.tsv", 1) == 0
    assert R.n == N and R.m == M
    f.R = R
    f.rowptr, f.col, f.val = R.csr()
    f.s2u, f.s2i = R.seq2user(), R.seq2item()
    f.valid, f.test = R.heldout(0), R.heldout(1)
    assert np.unique(f.test[0]).size == N                       # every user has a test pair
    f.sampled = R.test_users(f.data / "test_users.tsv")
    assert f.sampled.size == 40
    f.train_r = np.zeros((N, M), np.int64)
    for b in range(N):
        js = np.arange(f.rowptr[b], f.rowptr[b + 1])
        f.train_r[b, f.col[js]] = f.val[js]
    f.vmask = np.zeros((N, M), bool)
    f.vmask[f.valid[0], f.valid[1]] = True
    f.item_deg = np.bincount(f.col, minlength=M)
    return f


def _load(f, tag):
    """the expectations of a trained directory, as the score modes load them"""
    d = f.model[tag]
    if tag == "hier":
        Et = hostlib.load_matrix(d / "htheta.tsv", N, K, f.s2u)
        Eb = hostlib.load_matrix(d / "hbeta.tsv", M, K, f.s2i)
        return Et, Eb, hostlib.load_vector(d / "thetabias.tsv", N, f.s2u), hostlib.load_vector(d / "betabias.tsv", M, f.s2i)
    Et = hostlib.load_matrix(d / "theta_shape.tsv", N, K, f.s2u) / hostlib.load_vector(d / "theta_rate.tsv", K)[None, :]
    Eb = hostlib.load_matrix(d / "beta_shape.tsv", M, K, f.s2i) / hostlib.load_vector(d / "beta_rate.tsv", K)[None, :]
    return Et, Eb, None, None


def _numpy_scores(f, tag):
    Et, Eb, ub, ib = _load(f, tag)
    s = Et @ Eb.T
    if ub is not None:
        s = s + (ub[:, None] + ib[None, :])
    return s


def _masked(f, s):
    s = s.copy()
    s[(f.train_r > 0) | f.vmask] = 0.0
    return s


def _device(f, tag):
    from hgaprec_amd.capi import Hpf
    Et, Eb, ub, ib = _load(f, tag)
    D = Hpf(N, M, K, hier=tag == "hier", bias=ub is not None)
    D.upload_csr(f.rowptr, f.col, f.val)
    D.set_state("THETA_E", Et)
    D.set_state("BETA_E", Eb)
    if ub is not None:
        D.set_state("UBIAS_E", ub)
        D.set_state("IBIAS_E", ib)
    return D


def _mask_lists(f, users):
    mask = [np.flatnonzero(f.vmask[u]).astype(np.uint32) for u in users]
    mptr = np.zeros(len(users) + 1, np.uint64)
    mptr[1:] = np.cumsum([x.size for x in mask])
    return mptr, np.concatenate(mask).astype(np.uint32) if mptr[-1] else np.zeros(0, np.uint32)


def _test_rating(f):
    t = np.zeros((N, M), np.int64)
    t[f.test[0], f.test[1]] = f.test[2]
    return t


def _score_args(f, tag, mode, label="score"):
    fl = [a for a in f.flags[tag] if a not in ("-max-iterations", 3)]
    return f.base + fl + [mode, "-model-dir", f.model[tag], "-label", label]


def _outdir(f, args):
    return f.tmp / hostlib.prefix([str(a) for a in args])


def test_fixture_has_no_near_ties(fx):
    """the order checks below compare numpy's order with the device's: positive scores of one user must not be
    closer than 1e-12 relative (the seed of the fixture was chosen so; this does not hide ties, it rules them out)"""
    for tag in ("hier", "flat"):
        s = _masked(fx, _numpy_scores(fx, tag))
        for b in range(N):
            v = np.sort(s[b][s[b] > 0])
            assert v.size > 1 and np.min(np.diff(v) / v[1:]) > 1e-12, (tag, b)


@pytest.mark.parametrize("tag", ["hier", "flat"])
def test_gen_ranking_is_what_the_library_gives_on_the_loaded_files(fx, tag):
    f = fx
    args = _score_args(f, tag, "-gen-ranking")
    _run(f.tmp, args)
    out = _outdir(f, args)
    D = _device(f, tag)
    users = f.sampled
    mptr, mitems = _mask_lists(f, users)
    items, sc = D.rank_topn(users, 100, mptr, mitems)
    tr = _test_rating(f)
    ranking, h10, h100 = [], 0.0, 0.0
    for b, u in enumerate(users):
        hits10 = hits100 = 0
        for j in range(100):
            it = int(items[b, j])
            v = 1 if tr[u, it] >= 1 else 0
            hits10 += v if j < 10 else 0
            hits100 += v
            if f.train_r[u, it] == 0:
                ranking.append("%d\t%d\t%.5f\t%d\n" % (f.s2u[u], f.s2i[it], sc[b, j], v))
        h10 += hits10 / 10
        h100 += hits100 / 100
    assert (out / "ranking.tsv").read_text() == "".join(ranking)
    assert (out / "precision.txt").read_text() == "%d\t%.5f\t%.5f\n" % (users.size, h10 / users.size, h100 / users.size)

    qs = np.concatenate([np.full(np.count_nonzero(f.test[0] == u), b) for b, u in enumerate(users)]).astype(np.uint32)
    qi = np.concatenate([f.test[1][f.test[0] == u] for u in users]).astype(np.uint32)
    rank, pred = D.item_ranks(users, qs, qi, mptr, mitems)
    lines, a0, a1, a2 = [], 0.0, 0.0, 0
    for b, u in enumerate(users):
        q = np.flatnonzero(qs == b)
        q = q[np.argsort(rank[q], kind="stable")]
        nranked = M - np.count_nonzero(f.train_r[u] > 0)
        rank_ui, rr = 0.0, 0.0
        for x in q:
            lines.append("%d\t%d\t%.5f\t%d\t%d\n" % (u, qi[x], pred[x], rank[x], f.item_deg[qi[x]]))
            rank_ui += rank[x] + 1
            rr += 1 // (int(rank[x]) + 1)
        if q.size and nranked:
            a0 += (rank_ui / nranked) / q.size
            a1 += rr / q.size
            a2 += 1
    assert (out / "itemrank.tsv").read_text() == "".join(lines)
    assert (out / "meanrank.txt").read_text() == "%d\t%.5f\t%.5f\n" % (a2, a0 / a2, a1 / a2)
    assert not (out / "hbeta.tsv").exists() and not (out / "beta.tsv").exists()       # no save_model in a score mode
    D.close()


@pytest.mark.parametrize("tag", ["hier", "flat"])
def test_gen_ranking_against_numpy_alone(fx, tag):
    f = fx
    args = _score_args(f, tag, "-gen-ranking")
    out = _outdir(f, args)
    if not (out / "ranking.tsv").exists():
        _run(f.tmp, args)
    s = _masked(f, _numpy_scores(f, tag))
    u2s = {int(x): j for j, x in enumerate(f.s2u)}
    i2s = {int(x): j for j, x in enumerate(f.s2i)}
    got = {}
    for l in (out / "ranking.tsv").read_text().splitlines():
        a = l.split("\t")
        u, it = u2s[int(a[0])], i2s[int(a[1])]
        assert a[2] == "%.5f" % s[u, it], l                      # the printed score, to its 5 decimals
        got.setdefault(u, []).append(it)
    assert sorted(got) == sorted(int(u) for u in f.sampled)
    for u, its in got.items():
        order = np.argsort(-s[u], kind="stable")[:100]           # score descending, item ascending
        assert its == [int(i) for i in order if f.train_r[u, i] == 0]


@pytest.mark.parametrize("tag", ["hier", "flat"])
def test_rmse_against_numpy(fx, tag):
    f = fx
    args = _score_args(f, tag, "-rmse", label="rmse")
    _run(f.tmp, args)
    out = _outdir(f, args)
    s = _numpy_scores(f, tag)
    tu, ti, ty = f.test
    acc, lines = 0.0, []
    for u, i, y in zip(tu, ti, ty):                              # map order, summed serially
        p = float(s[u, i])
        acc += (p - int(y)) * (p - int(y))
        lines.append("%d\t%.5f\n" % (y, p))
    assert (out / "test_scores.tsv").read_text() == "".join(lines)
    assert (out / "rmse.txt").read_text() == "%.5f\n" % math.sqrt(acc / tu.size)


def _msr_expected(f, tag):
    s = _masked(f, _numpy_scores(f, tag))
    lim = M - 1
    vcount = np.bincount(f.valid[1], minlength=M)
    lines = ["User\tHeldOutItem\tHeldOutItemIndex\tUserNegatives\tUserCount\tItemCount\n"]
    for u in range(N):
        t = int(f.test[1][f.test[0] == u][-1])                   # the last test pair in (user, item) order
        masked = int(np.count_nonzero(((f.train_r[u] > 0) | f.vmask[u])[:lim]))
        rank = 0
        if t < lim:
            order = np.argsort(-s[u, :lim], kind="stable")
            rank = int(np.flatnonzero(order == t)[0])
        lines.append("%d\t%d\t%d\t%d\t%d\t%d\n" % (f.s2u[u], f.s2i[t], rank, lim - masked, masked, vcount[t] + f.item_deg[t]))
    return "".join(lines)


def test_msr_against_numpy(fx):
    f = fx
    args = _score_args(f, "hier", "-msr", label="msr")
    _run(f.tmp, args)
    assert (_outdir(f, args) / "pred.csv").read_text() == _msr_expected(f, "hier")


def test_msr_stops_on_a_user_without_test_pair(fx):
    f = fx
    d2 = f.tmp / "data_nopair"
    shutil.copytree(f.data, d2)
    victim = int(f.s2u[17])
    (d2 / "test.tsv").write_text("".join(l for l in (f.data / "test.tsv").read_text().splitlines(True)
                                         if int(l.split("\t")[0]) != victim))
    args = ["-dir", d2] + _score_args(f, "hier", "-msr", label="nopair")[2:]
    r = _run(f.tmp, args, ok=False)
    assert r.returncode != 0 and f"user {victim} " in r.stderr
    assert not (_outdir(f, args) / "pred.csv").exists()


def test_refusals(fx):
    f = fx
    # the output directory the run would create is the model directory: nothing is touched
    before = (f.model["hier"] / "validation.txt").read_text()
    assert before
    fl = [a for a in f.flags["hier"] if a not in ("-max-iterations", 3)]
    r = _run(f.tmp, f.base + fl + ["-gen-ranking", "-model-dir", f.model["hier"]], ok=False)
    assert r.returncode not in (0, 2) and "is the model directory" in r.stderr
    assert (f.model["hier"] / "validation.txt").read_text() == before
    # a missing model file is named
    empty = f.tmp / "no_model"
    empty.mkdir()
    args = f.base + fl + ["-rmse", "-model-dir", empty, "-label", "nomodel"]
    r = _run(f.tmp, args, ok=False)
    assert r.returncode != 0 and "hbeta.tsv" in r.stderr and "cannot open" in r.stderr
    assert not (_outdir(f, args) / "test_scores.tsv").exists()
    # the model of another data set (an id that is not the ratings') is refused with file and line
    other = f.tmp / "other_model"
    other.mkdir()
    for name in ("htheta.tsv", "hbeta.tsv", "thetabias.tsv", "betabias.tsv"):
        shutil.copy(f.model["hier"] / name, other / name)
    lines = (other / "hbeta.tsv").read_text().splitlines()
    lines[2] = "2\t999999\t" + "\t".join(lines[2].split("\t")[2:])
    (other / "hbeta.tsv").write_text("\n".join(lines) + "\n")
    r = _run(f.tmp, f.base + fl + ["-rmse", "-model-dir", other, "-label", "othermodel"], ok=False)
    assert r.returncode != 0 and "hbeta.tsv: line 3:" in r.stderr and "999999" in r.stderr
    # the bridges stay refused as before
    r = _run(f.tmp, ["-dir", f.data, "-nmf"], ok=False)
    assert r.returncode == 2 and "outside the MI355X hot-path build" in r.stderr
