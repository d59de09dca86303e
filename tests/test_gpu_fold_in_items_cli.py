"""-m gpu: `hgaprec ... -fold-in-items FILE -fold-iters 5 -model-dir <trained dir>` against the Python binding on the same
inputs: the user side read from the trained directory as shape and rate, E = shape / rate and Elog = psi(shape) - log(rate)
formed on the host, the items of FILE folded in by hpf_fold_in_items.  The files the run writes must be, byte for byte,
what the same writers make of the binding's arrays."""
import math

import numpy as np
import pytest

from hgaprec_amd import hostlib
from hgaprec_amd.capi import Hpf
from tests.test_gpu_score_modes import K, M, N, _run, fx  # noqa: F401

pytestmark = pytest.mark.gpu
NEW_ID = 1000000          # the training items' ratings come back under ids the data set does not have
UNKNOWN_USER = 9999999


def _write_new_items(f, path):
    """15 training items' columns under new ids, in an order that is not the training set's, with lines of unknown users
    in between and one item that has nothing else"""
    rng = np.random.default_rng(7)
    picked = rng.permutation(M)[:15]
    user_of = np.repeat(np.arange(N), np.diff(f.rowptr))
    lines = []
    for c in picked:
        iid = int(f.s2i[c]) + NEW_ID
        for j in np.flatnonzero(f.col == c):
            lines.append(f"{f.s2u[user_of[j]]}\t{iid}\t{f.val[j]}\n")
            if rng.random() < 0.1:
                lines.append(f"{UNKNOWN_USER + int(rng.integers(5))}\t{iid}\t3\n")
    lines.insert(3, f"{UNKNOWN_USER}\t{NEW_ID - 1}\t5\n")
    path.write_text("".join(lines))
    order = []
    for ln in lines:
        u, i, _ = ln.split("\t")
        if int(u) < UNKNOWN_USER and int(i) not in order:
            order.append(int(i))
    return order, sum(1 for ln in lines if int(ln.split()[0]) >= UNKNOWN_USER)


def _user_side(f, tag):
    d = f.model[tag]
    psi = lambda a: hostlib.digamma(a.ravel()).reshape(a.shape)                              # noqa: E731
    log = lambda a: np.array([math.log(v) for v in a.ravel()]).reshape(a.shape)              # noqa: E731  (libm's log, as the CLI's host)
    if tag == "hier":
        sh = hostlib.load_matrix(d / "htheta_shape.tsv", N, K, f.s2u)
        rt = hostlib.load_matrix(d / "htheta_rate.tsv", N, K, f.s2u)
        bs = hostlib.load_matrix(d / "thetabias_shape.tsv", N, 1, f.s2u)[:, 0]
        br = hostlib.load_matrix(d / "thetabias_rate.tsv", N, 1, f.s2u)[:, 0]
        return {"THETA_E": sh / rt, "THETA_ELOG": psi(sh) - log(rt), "UBIAS_E": bs / br, "UBIAS_ELOG": psi(bs) - log(br)}
    sh = hostlib.load_matrix(d / "theta_shape.tsv", N, K, f.s2u)
    rt = hostlib.load_vector(d / "theta_rate.tsv", K)[None, :] * np.ones((N, 1))
    return {"THETA_E": sh / rt, "THETA_ELOG": psi(sh) - log(rt)}


@pytest.mark.parametrize("tag", ["hier", "flat"])
def test_fold_in_items_cli_equals_the_binding(fx, tag):  # noqa: F811
    f = fx
    hier = bias = tag == "hier"
    new = f.tmp / f"new_items_{tag}.tsv"
    order, n_unknown = _write_new_items(f, new)
    args = f.base + f.flags[tag] + ["-model-dir", f.model[tag], "-label", "folditems", "-fold-in-items", new, "-fold-iters", 5]
    _run(f.tmp, args)
    out = f.tmp / hostlib.prefix([str(a) for a in args])
    assert out != f.model[tag]

    ni, skipped = f.R.read_fold_in_items(new)
    m = ni.m
    ids = ni.seq2item()
    assert ni.n == N and m == len(order) and list(ids) == order and skipped == n_unknown > 2
    rowptr, col, val = ni.csr()
    D = Hpf(N, m, K, hier=hier, bias=bias)
    try:
        D.upload_csr(rowptr, col, val)
        for w, a in _user_side(f, tag).items():
            D.set_state(w, a)
        iters = D.fold_in_items(5)
        assert iters.shape == (m,) and np.all(iters == 5)
        base = "hbeta" if hier else "beta"
        files = [(base + "_shape.tsv", "BETA_SHAPE", "m"), (base + ".tsv", "BETA_E", "m")]
        files.append((base + "_rate.tsv", "BETA_RATE", "m" if hier else "k"))
        if hier:
            files += [("betarate_shape.tsv", "ETA_SHAPE", "v"), ("betarate_rate.tsv", "ETA_RATE", "v"), ("betarate.tsv", "ETA_E", "v")]
        if bias:
            files += [("betabias_shape.tsv", "IBIAS_SHAPE", "m"), ("betabias_rate.tsv", "IBIAS_RATE", "m"), ("betabias.tsv", "IBIAS_E", "m")]
        for name, w, kind in files:
            a = D.get_state(w)
            ref = f.tmp / f"ref_items_{tag}_{name}"
            if kind == "m":
                assert hostlib.save_matrix(ref, a.reshape(m, -1), ids) == 0
            else:
                assert hostlib.save_vector(ref, a, ids) == 0          # (the K-vector: its id column is seq2item[k], as save_model has it)
            got = (out / ("foldin_" + name)).read_text()
            assert got == ref.read_text(), name
            assert len(got.splitlines()) == (K if kind == "k" else m), name
            assert [int(ln.split("\t")[1]) for ln in got.splitlines()] == list(ids[: len(got.splitlines())]), name
        assert (out / "foldin_items.txt").read_text() == f"{m}\t{col.size}\t{skipped}\t5\t0\t5\t5.00000\t5\n"
        assert not (out / "foldin.txt").exists()
    finally:
        D.close()
