"""-m gpu: `hgaprec -similar-items N -similar-users N [-similar-metric dot]` on a trained model against Hpf.similar on a
handle given the expectations the model files hold: the same text, line for line."""
import numpy as np
import pytest

from tests.test_gpu_recommend import _args
from tests.test_gpu_score_modes import M as FX_M, N as FX_N, _load, _outdir, _run, fx  # noqa: F401

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF
TOPN = 5


def _want(f, tag, side, metric):
    """the lines of similar_items.tsv (side 1) or similar_users.tsv (side 0), as the driver formats them"""
    from hgaprec_amd.capi import Hpf
    Et, Eb, ub, ib = _load(f, tag)
    E, ext = (Eb, f.s2i) if side else (Et, f.s2u)
    D = Hpf(FX_N, FX_M, E.shape[1], hier=tag == "hier", bias=ub is not None)
    try:
        D.set_state("BETA_E" if side else "THETA_E", E)
        ids, sc = D.similar(side, np.arange(E.shape[0], dtype=np.uint32), TOPN, metric)
    finally:
        D.close()
    assert not np.any(ids == NONE) and not np.any(ids == np.arange(E.shape[0])[:, None])     # no padding, no row in its own list
    return ["%d\t%d\t%.5f" % (ext[a], ext[b], s) for a in range(E.shape[0]) for b, s in zip(ids[a], sc[a])]


@pytest.mark.parametrize("tag,metric", [("hier", "cosine"), ("flat", "dot")])
def test_cli_similar_is_what_the_library_gives_on_the_loaded_files(fx, tag, metric):
    f = fx
    mode = ["-similar-items", TOPN, "-similar-users", TOPN] + ([] if metric == "cosine" else ["-similar-metric", metric])
    args = _args(f, f.data, tag, mode, "sim_" + metric)
    _run(f.tmp, args)
    out = _outdir(f, args)
    for side, name, rows, ext in ((1, "similar_items", FX_M, f.s2i), (0, "similar_users", FX_N, f.s2u)):
        got = (out / (name + ".tsv")).read_text().splitlines()
        assert got == _want(f, tag, side, metric), name
        assert (out / (name + ".txt")).read_text() == "%d\t%d\t%d\t%s\n" % (rows, rows * TOPN, TOPN, metric)
        first = [int(l.split("\t")[0]) for l in got]
        assert first == [int(ext[r]) for r in range(rows) for _ in range(TOPN)]                # rows in seq order, N lines each
        assert all(l.split("\t")[0] != l.split("\t")[1] for l in got)                         # no list contains its own id
    assert not (out / "ranking.tsv").exists() and not (out / "recommend.tsv").exists()


def test_cli_similar_is_refused_with_ngpus(fx):
    f = fx
    args = _args(f, f.data, "hier", ["-similar-items", TOPN], "sim_two") + ["-ngpus", 2]
    r = _run(f.tmp, args, ok=False)
    assert r.returncode != 0 and "-similar-items" in r.stderr and "without -ngpus" in r.stderr
    assert not (_outdir(f, args) / "similar_items.tsv").exists()
