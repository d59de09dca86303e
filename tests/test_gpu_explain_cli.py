"""-m gpu: `hgaprec -topic-items N -topic-users N` and `hgaprec -recommend N -explain T` on a trained model against
Hpf.factor_top / Hpf.explain on a handle given the expectations the model files hold: the same text, line for line; and
recommend.tsv byte for byte what the run without -explain writes."""
import numpy as np
import pytest

from hgaprec_amd import hostlib
from tests.test_gpu_fold_in_cli import _write_new_users
from tests.test_gpu_recommend import _args
from tests.test_gpu_score_modes import K as FX_K, M as FX_M, N as FX_N, _load, _outdir, _run, fx  # noqa: F401

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF
TOPN, REC, T = 7, 10, 3


@pytest.fixture(scope="module")
def models(fx):  # noqa: F811
    """the fixture's -hier -bias model, and a flat model WITH bias trained beside it"""
    f = fx
    if "flatbias" not in f.model:
        fl = ["-bias", "-max-iterations", 3]
        _run(f.tmp, f.base + fl)
        f.flags["flatbias"] = fl
        f.model["flatbias"] = f.tmp / hostlib.prefix([str(a) for a in f.base + fl])
        assert (f.model["flatbias"] / "betabias.tsv").exists() and (f.model["flatbias"] / "beta_shape.tsv").exists()
    return f


def _expectations(f, tag):
    if tag != "flatbias":
        return _load(f, tag)
    d = f.model[tag]
    Et = hostlib.load_matrix(d / "theta_shape.tsv", FX_N, FX_K, f.s2u) / hostlib.load_vector(d / "theta_rate.tsv", FX_K)[None, :]
    Eb = hostlib.load_matrix(d / "beta_shape.tsv", FX_M, FX_K, f.s2i) / hostlib.load_vector(d / "beta_rate.tsv", FX_K)[None, :]
    return Et, Eb, hostlib.load_vector(d / "thetabias.tsv", FX_N, f.s2u), hostlib.load_vector(d / "betabias.tsv", FX_M, f.s2i)


def _handle(f, tag):
    from hgaprec_amd.capi import Hpf
    Et, Eb, ub, ib = _expectations(f, tag)
    assert ub is not None
    D = Hpf(FX_N, FX_M, FX_K, hier=tag == "hier", bias=True)
    D.set_state("THETA_E", Et)
    D.set_state("BETA_E", Eb)
    D.set_state("UBIAS_E", ub)
    D.set_state("IBIAS_E", ib)
    return D


@pytest.mark.parametrize("tag", ["hier", "flatbias"])
def test_cli_topics_are_what_the_library_gives_on_the_loaded_files(models, tag):
    f = models
    args = _args(f, f.data, tag, ["-topic-items", TOPN, "-topic-users", TOPN], "topic")
    _run(f.tmp, args)
    out = _outdir(f, args)
    D = _handle(f, tag)
    try:
        for side, name, ext in ((1, "topic_items", f.s2i), (0, "topic_users", f.s2u)):
            ids, vals = D.factor_top(side, TOPN)
            assert not np.any(ids == NONE)
            want = ["%d\t%d\t%.8f" % (k, ext[r], v) for k in range(FX_K) for r, v in zip(ids[k], vals[k])]
            got = (out / (name + ".tsv")).read_text().splitlines()
            assert got == want, name
            assert (out / (name + ".txt")).read_text() == "%d\t%d\t%d\n" % (FX_K, FX_K * TOPN, TOPN)
            assert [int(l.split("\t")[0]) for l in got] == [k for k in range(FX_K) for _ in range(TOPN)]    # factors ascend, N lines each
    finally:
        D.close()
    assert not (out / "ranking.tsv").exists() and not (out / "recommend.tsv").exists()


@pytest.mark.parametrize("tag", ["hier", "flatbias"])
def test_cli_explain_is_what_the_library_gives_and_leaves_recommend_tsv_alone(models, tag):
    f = models
    plain = _args(f, f.data, tag, ["-recommend", REC], "rec_plain")
    _run(f.tmp, plain)
    args = _args(f, f.data, tag, ["-recommend", REC, "-explain", T], "rec_explain")
    _run(f.tmp, args)
    out, out0 = _outdir(f, args), _outdir(f, plain)
    assert (out / "recommend.tsv").read_bytes() == (out0 / "recommend.tsv").read_bytes()
    assert (out / "recommend.txt").read_bytes() == (out0 / "recommend.txt").read_bytes()
    assert not (out0 / "recommend_explain.tsv").exists()
    # the pairs of recommend.tsv, in its order, back in seq numbers
    u_of = {int(x): s for s, x in enumerate(f.s2u)}
    i_of = {int(x): s for s, x in enumerate(f.s2i)}
    rec = [l.split("\t") for l in (out / "recommend.tsv").read_text().splitlines()]
    u = np.array([u_of[int(l[0])] for l in rec], np.uint32)
    i = np.array([i_of[int(l[1])] for l in rec], np.uint32)
    assert u.size > FX_N
    D = _handle(f, tag)
    try:
        fac, con = D.explain(u, i, T)
    finally:
        D.close()
    assert not np.any(fac == NONE)                                  # K + 2 = 7 terms >= T
    want = ["%d\t%d\t%d\t%.8f" % (f.s2u[a], f.s2i[b], k, c) for a, b, fr, cr in zip(u, i, fac, con) for k, c in zip(fr, cr)]
    got = (out / "recommend_explain.tsv").read_text().splitlines()
    assert got == want
    assert (out / "recommend_explain.txt").read_text() == "%d\t%d\t%d\n" % (u.size, u.size * T, T)
    vals = np.array([float(l.split("\t")[3]) for l in got]).reshape(-1, T)
    assert np.all(vals[:, :-1] >= vals[:, 1:])                      # each pair's terms best first


def test_cli_explain_behind_fold_in(models):
    f = models
    new = f.tmp / "new_users_explain.tsv"
    _write_new_users(f, new)
    args = f.base + f.flags["hier"] + ["-model-dir", f.model["hier"], "-label", "fold_explain", "-fold-in", new, "-fold-iters", 3,
                                       "-recommend", REC, "-explain", T]
    _run(f.tmp, args)
    out = f.tmp / hostlib.prefix([str(a) for a in args])
    rec = [l.split("\t")[:2] for l in (out / "foldin_recommend.tsv").read_text().splitlines()]
    exp = [l.split("\t") for l in (out / "foldin_recommend_explain.tsv").read_text().splitlines()]
    assert len(rec) > 0 and len(exp) == len(rec) * T
    assert [e[:2] for e in exp[::T]] == rec                         # the pairs of foldin_recommend.tsv, in its order
    assert all(0 <= int(e[2]) < FX_K + 2 for e in exp)
    assert (out / "foldin_recommend_explain.txt").read_text() == "%d\t%d\t%d\n" % (len(rec), len(exp), T)
    assert not (out / "recommend_explain.tsv").exists()
