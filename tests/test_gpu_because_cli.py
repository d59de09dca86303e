"""-m gpu: `hgaprec -recommend N -because T` on a trained model against the reference of tests/because_ref.py (mpmath) on the
state the run loads -- E from the expectation files as every score mode loads it, Elog = psi(shape) - log(rate) from the
shape and rate files --: the same (user, item, rated item) lines in the same order, the values within 2e-8 (the file prints
eight decimals); recommend.tsv byte for byte what the run without the flag writes; the same behind -fold-in (there against
the binding on the folded-in handle) and beside -explain."""
import math

import numpy as np
import pytest

from hgaprec_amd import hostlib
from hgaprec_amd.capi import Hpf
from tests import because_ref as R
from tests.test_gpu_fold_in_cli import _item_side, _write_new_users
from tests.test_gpu_recommend import _args
from tests.test_gpu_score_modes import K, M, N, _load, _outdir, _run, fx  # noqa: F401

pytestmark = pytest.mark.gpu
REC, T = 5, 3


def _loaded_state(f, tag):
    """E and Elog of both sides as `-because` puts them into the handle"""
    d = f.model[tag]
    psi = lambda a: hostlib.digamma(a.ravel()).reshape(a.shape)                              # noqa: E731
    log = lambda a: np.array([math.log(v) for v in a.ravel()]).reshape(a.shape)              # noqa: E731  (libm's log, as the CLI's host)
    Et, Eb, ub, ib = _load(f, tag)
    if tag == "hier":
        L = [psi(hostlib.load_matrix(d / (b + "_shape.tsv"), r, K, ids)) - log(hostlib.load_matrix(d / (b + "_rate.tsv"), r, K, ids))
             for b, r, ids in (("htheta", N, f.s2u), ("hbeta", M, f.s2i))]
        bl = [psi(hostlib.load_matrix(d / (b + "_shape.tsv"), r, 1, ids)[:, 0]) - log(hostlib.load_matrix(d / (b + "_rate.tsv"), r, 1, ids)[:, 0])
              for b, r, ids in (("thetabias", N, f.s2u), ("betabias", M, f.s2i))]
        return R.State(Et, L[0], Eb, L[1], ub, bl[0], ib, bl[1])
    L = [psi(hostlib.load_matrix(d / (b + "_shape.tsv"), r, K, ids)) - log(hostlib.load_vector(d / (b + "_rate.tsv"), K))[None, :]
         for b, r, ids in (("theta", N, f.s2u), ("beta", M, f.s2i))]
    return R.State(Et, L[0], Eb, L[1])


def _pairs_of(f, path):
    """the (user, item) lines of a recommend file, back in seq numbers"""
    u_of = {int(x): s for s, x in enumerate(f.s2u)}
    i_of = {int(x): s for s, x in enumerate(f.s2i)}
    rec = [ln.split("\t") for ln in path.read_text().splitlines()]
    return [(u_of[int(ln[0])], i_of[int(ln[1])]) for ln in rec]


@pytest.mark.parametrize("tag", ["hier", "flat"])
def test_cli_because_is_the_reference_and_leaves_recommend_tsv_alone(fx, tag):  # noqa: F811
    f = fx
    plain = _args(f, f.data, tag, ["-recommend", REC], "because_plain")
    _run(f.tmp, plain)
    args = _args(f, f.data, tag, ["-recommend", REC, "-because", T], "because")
    _run(f.tmp, args)
    out, out0 = _outdir(f, args), _outdir(f, plain)
    assert (out / "recommend.tsv").read_bytes() == (out0 / "recommend.tsv").read_bytes()
    assert (out / "recommend.txt").read_bytes() == (out0 / "recommend.txt").read_bytes()
    assert not (out0 / "recommend_because.tsv").exists() and not (out / "recommend_explain.tsv").exists()
    pairs = _pairs_of(f, out / "recommend.tsv")
    assert len(pairs) > N
    st = _loaded_state(f, tag)
    got = [ln.split("\t") for ln in (out / "recommend_because.tsv").read_text().splitlines()]
    want = []
    by_user = {}
    for u, j in pairs:
        by_user.setdefault(u, []).append(j)
    exact = {}
    for u, ts in by_user.items():
        hist = f.col[f.rowptr[u]:f.rowptr[u + 1]]
        yy = np.where(f.val[f.rowptr[u]:f.rowptr[u + 1]] > 1, f.val[f.rowptr[u]:f.rowptr[u + 1]], 1).astype(np.float64)
        for j, (con, _, _) in zip(ts, R.exact(st, hist, yy, u, ts)):
            exact[(u, j)] = (hist, con)
    for u, j in pairs:                                              # recommend.tsv's order
        hist, con = exact[(u, j)]
        _, order = R.top(con, hist, T)
        want += [(int(f.s2u[u]), int(f.s2i[j]), int(f.s2i[hist[r]]), float(con[r])) for r in order]
    assert len(got) == len(want)
    worst = 0.0
    for g, w in zip(got, want):
        assert (int(g[0]), int(g[1]), int(g[2])) == w[:3], (g, w)
        worst = max(worst, abs(float(g[3]) - w[3]))
        assert abs(float(g[3]) - w[3]) <= 2e-8, (g, w)
    assert all(len(g[3].split(".")[1]) == 8 for g in got)           # %.8f
    print(f"{tag}: {len(got)} lines, the values within {worst:.2e} of mpmath")
    assert (out / "recommend_because.txt").read_text() == "%d\t%d\t%d\n" % (len(pairs), len(got), T)


def test_cli_because_beside_explain(fx):  # noqa: F811
    f = fx
    alone = _args(f, f.data, "hier", ["-recommend", REC, "-because", T], "because")
    both = _args(f, f.data, "hier", ["-recommend", REC, "-explain", 2, "-because", T], "because_explain")
    _run(f.tmp, alone)
    _run(f.tmp, both)
    a, b = _outdir(f, alone), _outdir(f, both)
    for name in ("recommend.tsv", "recommend.txt", "recommend_because.tsv", "recommend_because.txt"):
        assert (a / name).read_bytes() == (b / name).read_bytes(), name
    n_pairs = len((b / "recommend.tsv").read_text().splitlines())
    assert (b / "recommend_explain.txt").read_text() == "%d\t%d\t%d\n" % (n_pairs, n_pairs * 2, 2)


def test_cli_because_behind_fold_in(fx):  # noqa: F811
    f = fx
    new = f.tmp / "new_users_because.tsv"
    _write_new_users(f, new)
    args = f.base + f.flags["hier"] + ["-model-dir", f.model["hier"], "-label", "fold_because", "-fold-in", new, "-fold-iters", 3,
                                       "-recommend", REC, "-because", T]
    _run(f.tmp, args)
    out = f.tmp / hostlib.prefix([str(a) for a in args])
    rec = [ln.split("\t")[:2] for ln in (out / "foldin_recommend.tsv").read_text().splitlines()]
    got = (out / "foldin_recommend_because.tsv").read_text().splitlines()
    assert len(rec) > 0 and not (out / "recommend_because.tsv").exists()
    # the binding on a handle folded in the same way
    nu, _ = f.R.read_fold_in(new)
    ids = nu.seq2user()
    rowptr, col, val = nu.csr()
    u_of = {int(x): s for s, x in enumerate(ids)}
    i_of = {int(x): s for s, x in enumerate(f.s2i)}
    D = Hpf(nu.n, M, K, hier=True, bias=True)
    try:
        D.upload_csr(rowptr, col, val)
        for w, a in _item_side(f, "hier").items():
            D.set_state(w, a)
        D.fold_in(3)
        groups = {}
        for u, i in rec:
            groups.setdefault(u_of[int(u)], []).append(i_of[int(i)])
        users = np.array(list(groups), np.uint32)                   # foldin_recommend.tsv's order: users in seq order
        assert np.all(np.diff(users.astype(np.int64)) > 0)
        t_ptr = np.concatenate([[0], np.cumsum([len(t) for t in groups.values()])]).astype(np.uint64)
        t_items = np.array([j for t in groups.values() for j in t], np.uint32)
        items, con, _, _ = D.because(users, t_ptr, t_items, T)
    finally:
        D.close()
    want = ["%d\t%d\t%d\t%.8f" % (ids[u], f.s2i[j], f.s2i[r], c)
            for (u, j), ir, cr in zip([(u, j) for u, t in groups.items() for j in t], items, con) for r, c in zip(ir, cr) if r != R.NONE]
    assert got == want
    given = {int(ids[u]): set(int(f.s2i[c]) for c in col[rowptr[u]:rowptr[u + 1]]) for u in range(nu.n)}
    assert all(int(ln.split("\t")[2]) in given[int(ln.split("\t")[0])] for ln in got)      # a rated item is one the user was given
    assert (out / "foldin_recommend_because.txt").read_text() == "%d\t%d\t%d\n" % (len(rec), len(got), T)
