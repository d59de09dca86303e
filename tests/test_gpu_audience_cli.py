"""-m gpu: `hgaprec -audience N [-explain T]` on a trained model, and `-fold-in-items FILE -audience N`, against Hpf.audience
(and Hpf.explain) on a handle given what the run reads: the same text, line for line."""
import numpy as np
import pytest

from hgaprec_amd import hostlib
from hgaprec_amd.capi import Hpf
from tests.test_gpu_fold_in_items_cli import _user_side, _write_new_items
from tests.test_gpu_recommend import _args
from tests.test_gpu_score_modes import K, M, N, _device, _outdir, _run, fx  # noqa: F401

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF
TOPN, T = 7, 3


def _lines(users, scores, item_ids, user_ids, rated):
    """audience.tsv as the driver writes it: items in the order given, each list best first, no padding, no user with a
    given rating for the item (rated[u, i] != 0) -> (lines, the (user, item) pairs of the lines)"""
    lines, pairs = [], []
    for b in range(users.shape[0]):
        for u, s in zip(users[b], scores[b]):
            if u == NONE or rated[u, b]:
                continue
            lines.append("%d\t%d\t%.5f" % (item_ids[b], user_ids[u], s))
            pairs.append((int(u), b))
    return lines, pairs


def _validation_by_item(f):
    lists = [np.flatnonzero(f.vmask[:, i]).astype(np.uint32) for i in range(M)]
    mptr = np.zeros(M + 1, np.uint64)
    mptr[1:] = np.cumsum([x.size for x in lists])
    return mptr, np.concatenate(lists).astype(np.uint32)


@pytest.mark.parametrize("tag", ["hier", "flat"])
def test_cli_audience_is_what_the_library_gives_on_the_loaded_files(fx, tag):  # noqa: F811
    f = fx
    args = _args(f, f.data, tag, ["-audience", TOPN], "aud")
    eargs = _args(f, f.data, tag, ["-audience", TOPN, "-explain", T], "aud_explain")
    _run(f.tmp, args)
    _run(f.tmp, eargs)
    out, eout = _outdir(f, args), _outdir(f, eargs)
    D = _device(f, tag)
    try:
        mptr, musers = _validation_by_item(f)
        assert musers.size == f.valid[0].size > 50
        im, ip, iu = f.R.item_mask_lists(0)
        assert np.array_equal(ip, mptr) and np.array_equal(iu, musers)             # the run's own regrouping
        users, sc = D.audience(np.arange(M, dtype=np.uint32), TOPN, mptr, musers)
        want, pairs = _lines(users, sc, f.s2i, f.s2u, f.train_r)
        got = (out / "audience.tsv").read_text().splitlines()
        assert got == want and len(want) > 0.9 * M * TOPN
        assert (out / "audience.txt").read_text() == "%d\t%d\t%d\n" % (M, len(want), TOPN)
        assert [int(l.split("\t")[0]) for l in got] == [int(f.s2i[i]) for _, i in pairs]     # items in seq order
        assert not (out / "audience_explain.tsv").exists() and not (out / "recommend.tsv").exists()
        # -explain T: the same lists, and the terms of their pairs
        assert (eout / "audience.tsv").read_bytes() == (out / "audience.tsv").read_bytes()
        assert (eout / "audience.txt").read_bytes() == (out / "audience.txt").read_bytes()
        pu, pi = np.array([p[0] for p in pairs], np.uint32), np.array([p[1] for p in pairs], np.uint32)
        fac, con = D.explain(pu, pi, T)
        ewant = ["%d\t%d\t%d\t%.8f" % (f.s2i[i], f.s2u[u], k, c) for (u, i), fr, cr in zip(pairs, fac, con)
                 for k, c in zip(fr, cr) if k != NONE]
        assert (eout / "audience_explain.tsv").read_text().splitlines() == ewant
        assert (eout / "audience_explain.txt").read_text() == "%d\t%d\t%d\n" % (len(pairs), len(ewant), T)
    finally:
        D.close()


@pytest.mark.parametrize("tag", ["hier", "flat"])
def test_audience_behind_fold_in_items(fx, tag):  # noqa: F811
    f = fx
    hier = bias = tag == "hier"
    new = f.tmp / f"aud_new_items_{tag}.tsv"
    _write_new_items(f, new)
    base = f.base + f.flags[tag] + ["-model-dir", f.model[tag], "-fold-in-items", new, "-fold-iters", 5]
    plain, withaud = base + ["-label", "audfold0"], base + ["-label", "audfold1", "-audience", TOPN]
    _run(f.tmp, plain)
    _run(f.tmp, withaud)
    out0, out1 = (f.tmp / hostlib.prefix([str(a) for a in a_]) for a_ in (plain, withaud))
    names0 = sorted(p.name for p in out0.glob("foldin_*"))
    names1 = sorted(p.name for p in out1.glob("foldin_*"))
    assert names1 == sorted(names0 + ["foldin_audience.tsv", "foldin_audience.txt"]) and len(names0) >= 4
    for name in names0:
        assert (out1 / name).read_bytes() == (out0 / name).read_bytes(), name

    ni, _ = f.R.read_fold_in_items(new)
    m, ids = ni.m, ni.seq2item()
    rowptr, col, val = ni.csr()
    rated = np.zeros((N, m), np.int64)
    rated[np.repeat(np.arange(N), np.diff(rowptr)), col] = val
    D = Hpf(N, m, K, hier=hier, bias=bias)
    try:
        D.upload_csr(rowptr, col, val)
        for w, a in _user_side(f, tag).items():
            D.set_state(w, a)
        D.fold_in_items(5)
        users, sc = D.audience(np.arange(m, dtype=np.uint32), TOPN)                # no list beyond the given ratings
        want, _ = _lines(users, sc, ids, f.s2u, rated)
        assert (out1 / "foldin_audience.tsv").read_text().splitlines() == want and len(want) > 0.5 * m * TOPN
        assert (out1 / "foldin_audience.txt").read_text() == "%d\t%d\t%d\n" % (m, len(want), TOPN)
    finally:
        D.close()
