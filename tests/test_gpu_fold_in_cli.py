"""-m gpu: `hgaprec ... -fold-in FILE -fold-iters 5 -recommend 10 -model-dir <trained dir>` against the Python binding on
the same inputs: the item side read from the trained directory as shape and rate, E = shape / rate and
Elog = psi(shape) - log(rate) formed on the host, the users of FILE folded in by hpf_fold_in.  The files the run writes
must be, byte for byte, what the same writers make of the binding's arrays."""
import math

import numpy as np
import pytest

from hgaprec_amd import hostlib
from hgaprec_amd.capi import Hpf
from tests.test_gpu_score_modes import K, M, N, _run, fx  # noqa: F401

pytestmark = pytest.mark.gpu
NEW_ID = 1000000          # the training users' ratings come back under ids the data set does not have
UNKNOWN_ITEM = 9999999


def _write_new_users(f, path):
    """20 training users' rows under new ids, in an order that is not the training set's, with lines for unknown items
    in between and one user who has nothing else"""
    rng = np.random.default_rng(7)
    picked = rng.permutation(N)[:20]
    lines, given = [], {}
    for b in picked:
        uid = int(f.s2u[b]) + NEW_ID
        js = np.arange(f.rowptr[b], f.rowptr[b + 1])
        given[uid] = set(int(f.s2i[c]) for c in f.col[js])
        for j in js:
            lines.append(f"{uid}\t{f.s2i[f.col[j]]}\t{f.val[j]}\n")
            if rng.random() < 0.1:
                lines.append(f"{uid}\t{UNKNOWN_ITEM + int(rng.integers(5))}\t3\n")
    lines.insert(3, f"{NEW_ID - 1}\t{UNKNOWN_ITEM}\t5\n")
    path.write_text("".join(lines))
    return [int(f.s2u[b]) + NEW_ID for b in picked], given, sum(1 for ln in lines if int(ln.split()[1]) >= UNKNOWN_ITEM)


def _item_side(f, tag):
    d = f.model[tag]
    psi = lambda a: hostlib.digamma(a.ravel()).reshape(a.shape)                              # noqa: E731
    log = lambda a: np.array([math.log(v) for v in a.ravel()]).reshape(a.shape)              # noqa: E731  (libm's log, as the CLI's host)
    if tag == "hier":
        sh = hostlib.load_matrix(d / "hbeta_shape.tsv", M, K, f.s2i)
        rt = hostlib.load_matrix(d / "hbeta_rate.tsv", M, K, f.s2i)
        bs = hostlib.load_matrix(d / "betabias_shape.tsv", M, 1, f.s2i)[:, 0]
        br = hostlib.load_matrix(d / "betabias_rate.tsv", M, 1, f.s2i)[:, 0]
        return {"BETA_E": sh / rt, "BETA_ELOG": psi(sh) - log(rt), "IBIAS_E": bs / br, "IBIAS_ELOG": psi(bs) - log(br)}
    sh = hostlib.load_matrix(d / "beta_shape.tsv", M, K, f.s2i)
    rt = hostlib.load_vector(d / "beta_rate.tsv", K)[None, :] * np.ones((M, 1))
    return {"BETA_E": sh / rt, "BETA_ELOG": psi(sh) - log(rt)}


@pytest.mark.parametrize("tag", ["hier", "flat"])
def test_fold_in_cli_equals_the_binding(fx, tag):  # noqa: F811
    f = fx
    hier = bias = tag == "hier"
    new = f.tmp / f"new_users_{tag}.tsv"
    order, given, n_unknown = _write_new_users(f, new)
    args = f.base + f.flags[tag] + ["-model-dir", f.model[tag], "-label", "fold", "-fold-in", new, "-fold-iters", 5, "-recommend", 10]
    _run(f.tmp, args)
    out = f.tmp / hostlib.prefix([str(a) for a in args])
    assert out != f.model[tag]

    nu, skipped = f.R.read_fold_in(new)
    n = nu.n
    ids = nu.seq2user()
    assert n == 20 and list(ids) == order and skipped == n_unknown > 2
    rowptr, col, val = nu.csr()
    item = _item_side(f, tag)
    D = Hpf(n, M, K, hier=hier, bias=bias)
    try:
        D.upload_csr(rowptr, col, val)
        for w, a in item.items():
            D.set_state(w, a)
        iters = D.fold_in(5)
        assert np.all(iters == 5)
        base = "htheta" if hier else "theta"
        files = [(base + "_shape.tsv", "THETA_SHAPE", "m"), (base + ".tsv", "THETA_E", "m")]
        files.append((base + "_rate.tsv", "THETA_RATE", "m" if hier else "k"))
        if hier:
            files += [("thetarate_shape.tsv", "XI_SHAPE", "v"), ("thetarate_rate.tsv", "XI_RATE", "v"), ("thetarate.tsv", "XI_E", "v")]
        if bias:
            files += [("thetabias_shape.tsv", "UBIAS_SHAPE", "m"), ("thetabias_rate.tsv", "UBIAS_RATE", "m"), ("thetabias.tsv", "UBIAS_E", "m")]
        for name, w, kind in files:
            a = D.get_state(w)
            ref = f.tmp / f"ref_{tag}_{name}"
            if kind == "m":
                assert hostlib.save_matrix(ref, a.reshape(n, -1), ids) == 0
            else:
                assert hostlib.save_vector(ref, a, ids) == 0          # (the K-vector: its id column is seq2user[k], as save_model has it)
            got = (out / ("foldin_" + name)).read_text()
            assert got == ref.read_text(), name
            assert len(got.splitlines()) == (K if kind == "k" else n), name
            assert [int(ln.split("\t")[1]) for ln in got.splitlines()] == list(ids[: len(got.splitlines())]), name
        assert (out / "foldin.txt").read_text() == f"{n}\t{col.size}\t{skipped}\t5\t0\t5\t5.00000\t5\n"
        # the recommendations: the binding's, and never an item the user was given
        items, scores = D.recommend(np.arange(n, dtype=np.uint32), 10)
        want = []
        for b in range(n):
            mine = set(col[rowptr[b]:rowptr[b + 1]].tolist())
            want += [f"{ids[b]}\t{f.s2i[it]}\t{s:.5f}\n" for it, s in zip(items[b], scores[b]) if int(it) not in mine]
        got = (out / "foldin_recommend.tsv").read_text()
        assert got == "".join(want)
        for ln in got.splitlines():
            u, it, _ = ln.split("\t")
            assert int(it) not in given[int(u)]
        assert (out / "foldin_recommend.txt").read_text() == f"{n}\t{len(want)}\t10\n"
        assert len(want) > 0
    finally:
        D.close()
