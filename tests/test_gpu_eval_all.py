"""-m gpu: `hgaprec ... -eval-all -model-dir <trained dir>` -- every user's every test item through hpf_rank_queries --
against the -gen-ranking report of the same model with every user listed in test_users.tsv (compute_itemrank through
hpf_item_ranks), and against Python on the loaded factor files."""
import shutil

import numpy as np
import pytest

from hgaprec_amd import hostlib
from tests.test_gpu_score_modes import K, M, N, _device, _load, _mask_lists, _outdir, _run, _score_args, fx  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def allusers(fx):
    """the fixture's data set with a test_users.tsv that lists every user (the fixture's own lists 40)"""
    f = fx
    d = f.tmp / "data_all_users"
    if not d.exists():
        shutil.copytree(f.data, d)
        (d / "test_users.tsv").write_text("".join(f"{x}\n" for x in f.s2u))
    # every test pair is a hit under the default -rating-threshold 1, and every user has one: nobody is left out
    assert np.all(f.test[2] >= 1) and np.unique(f.test[0]).size == N
    return d


def _args(f, d, tag, mode, label):
    return ["-dir", d] + _score_args(f, tag, mode, label=label)[2:]


@pytest.mark.parametrize("tag", ["hier", "flat"])
def test_eval_all_against_gen_ranking_and_the_library(fx, allusers, tag):
    f = fx
    ga = _args(f, allusers, tag, "-gen-ranking", "genall")
    ea = _args(f, allusers, tag, "-eval-all", "evalall")
    _run(f.tmp, ga)
    _run(f.tmp, ea)
    gout, eout = _outdir(f, ga), _outdir(f, ea)

    # itemrank_all.tsv: the lines of itemrank.tsv, users ascending and ranks ascending within a user
    def key(l):
        a = l.split("\t")
        return int(a[0]), int(a[3])
    got = (eout / "itemrank_all.tsv").read_text().splitlines()
    want = (gout / "itemrank.tsv").read_text().splitlines()
    assert len(got) == f.test[0].size and got == sorted(got, key=key)
    assert got == sorted(want, key=key)

    # meanrank: the second field of meanrank.txt, as printed
    ev = (eout / "eval_all.txt").read_text().rstrip("\n").split("\t")
    mr = (gout / "meanrank.txt").read_text().rstrip("\n").split("\t")
    assert len(ev) == 7 and ev[6] == mr[1] and ev[0] == mr[0] == str(N)

    # eval_users.tsv: the integers Python derives from hpf_item_ranks on the loaded factor files
    D = _device(f, tag)
    users = np.arange(N, dtype=np.uint32)
    mptr, mitems = _mask_lists(f, users)
    tu, ti = f.test[0].astype(np.uint32), f.test[1].astype(np.uint32)      # sorted by (user, item)
    rank, _ = D.item_ranks(users, tu, ti, mptr, mitems)
    D.close()
    rows = []
    for u in range(N):
        r = rank[tu == u].astype(np.int64)
        rows.append([u, int(f.s2u[u]), r.size, int(np.count_nonzero(r < 10)), int(np.count_nonzero(r < 100)), int(r.min()),
                     int((r + 1).sum())])
    text = (eout / "eval_users.tsv").read_text()
    assert text == "".join("\t".join(str(x) for x in row) + "\n" for row in rows)

    # eval_all.txt: the numpy means of those integers, to the printed digits
    a = np.array(rows, np.float64)
    nranked = np.array([M - np.count_nonzero(f.train_r[u] > 0) for u in range(N)], np.float64)
    per_user = np.stack([a[:, 3] / 10, a[:, 4] / 100, a[:, 4] / a[:, 2], 1.0 / (a[:, 5] + 1), (a[:, 6] / nranked) / a[:, 2]])
    means = np.add.accumulate(per_user, axis=1)[:, -1] / N             # summed in seq order, like the report
    assert ev[1] == str(f.test[0].size)
    assert ev[2:] == ["%.5f" % w for w in means]
    assert np.allclose(means, per_user.mean(axis=1), rtol=1e-12)
    assert float(ev[5]) > 0.0 and np.any(a[:, 5] > 0)                  # real division: 1 / (j + 1) in integers is 0 for j > 0
    assert not (eout / "itemrank.tsv").exists() and not (eout / "ranking.tsv").exists()


def test_eval_all_is_refused_with_ngpus(fx, allusers):
    f = fx
    args = _args(f, allusers, "hier", "-eval-all", "evalall2") + ["-ngpus", 2]
    r = _run(f.tmp, args, ok=False)
    assert r.returncode == 1 and "-eval-all" in r.stderr and "without -ngpus" in r.stderr
    out = _outdir(f, args)
    assert not (out / "eval_all.txt").exists() and not (out / "itemrank_all.tsv").exists()
