"""-m gpu: `hgaprec -recommend N -ucb Z` on a trained model, with and without -bias: recommend_ucb.tsv is the binding's
hpf_recommend_ucb on the state the run loads -- E from the expectation files as every score mode loads it, the shapes from
the shape files -- line for line, and numpy's moments of the same files within the five printed decimals; recommend.tsv is
byte for byte what the run without the flag writes; behind -fold-in a user with one rating is less sure than one with
fifty; the refusals."""
import numpy as np
import pytest

from hgaprec_amd import hostlib
from tests import moments_ref as ref
from tests.test_gpu_recommend import _args
from tests.test_gpu_score_modes import K, M, N, _device, _load, _outdir, _run, fx  # noqa: F401

pytestmark = pytest.mark.gpu
REC, Z = 5, 2


def _shapes(f, tag):
    d = f.model[tag]
    if tag == "hier":
        return {"THETA_SHAPE": hostlib.load_matrix(d / "htheta_shape.tsv", N, K, f.s2u), "BETA_SHAPE": hostlib.load_matrix(d / "hbeta_shape.tsv", M, K, f.s2i),
                "UBIAS_SHAPE": hostlib.load_matrix(d / "thetabias_shape.tsv", N, 1, f.s2u)[:, 0].copy(),
                "IBIAS_SHAPE": hostlib.load_matrix(d / "betabias_shape.tsv", M, 1, f.s2i)[:, 0].copy()}
    return {"THETA_SHAPE": hostlib.load_matrix(d / "theta_shape.tsv", N, K, f.s2u), "BETA_SHAPE": hostlib.load_matrix(d / "beta_shape.tsv", M, K, f.s2i)}


@pytest.mark.parametrize("tag", ["hier", "flat"])
def test_cli_ucb_is_the_reference_and_leaves_recommend_tsv_alone(fx, tag):  # noqa: F811
    f = fx
    plain = _args(f, f.data, tag, ["-recommend", REC], "ucb_plain")
    _run(f.tmp, plain)
    args = _args(f, f.data, tag, ["-recommend", REC, "-ucb", Z], "ucb")
    _run(f.tmp, args)
    out, out0 = _outdir(f, args), _outdir(f, plain)
    assert (out / "recommend.tsv").read_bytes() == (out0 / "recommend.tsv").read_bytes()
    assert (out / "recommend.txt").read_bytes() == (out0 / "recommend.txt").read_bytes()
    assert not (out0 / "recommend_ucb.tsv").exists()
    got = (out / "recommend_ucb.tsv").read_text().splitlines()

    # the binding on the state the run loads, the users' validation items as the mask list
    users = np.arange(N, dtype=np.uint32)
    lists = [np.sort(f.valid[1][f.valid[0] == u]) for u in users]
    mptr = np.zeros(N + 1, np.uint64)
    mptr[1:] = np.cumsum([len(x) for x in lists])
    shapes = _shapes(f, tag)
    D = _device(f, tag)
    try:
        for w, a in shapes.items():
            D.set_state(w, a)
        items, ucb, mean, var = D.recommend_ucb(users, REC, float(Z), mptr, np.concatenate(lists).astype(np.uint32))
    finally:
        D.close()
    want = ["%d\t%d\t%.5f\t%.5f\t%.5f" % (f.s2u[u], f.s2i[it], ucb[u, j], mean[u, j], np.sqrt(var[u, j]))
            for u in users for j, it in enumerate(items[u]) if f.train_r[u, it] == 0]
    assert len(want) > N and got == want
    assert (out / "recommend_ucb.txt").read_text() == "%d\t%d\t%d\t%g\n" % (N, len(got), REC, Z)

    # numpy alone on the same files: the printed moments, the expression, the order
    Et, Eb, ub, ib = _load(f, tag)
    st = {"THETA_E": Et, "BETA_E": Eb, **shapes}
    if ub is not None:
        st.update(UBIAS_E=ub, IBIAS_E=ib)
    X, Y = ref.derived_rows(st, ub is not None)
    S = Et @ Eb.T + (0.0 if ub is None else ub[:, None] + ib[None, :])
    V = X @ Y.T
    u_of = {int(x): s for s, x in enumerate(f.s2u)}
    i_of = {int(x): s for s, x in enumerate(f.s2i)}
    last = {}
    for ln in got:
        a = ln.split("\t")
        u, i, c, mu, sd = u_of[int(a[0])], i_of[int(a[1])], float(a[2]), float(a[3]), float(a[4])
        assert abs(mu - S[u, i]) <= 1e-5 + 1e-9 * S[u, i] and abs(sd - np.sqrt(V[u, i])) <= 1e-5 + 1e-9 * np.sqrt(V[u, i]), ln
        assert abs(c - (mu + Z * sd)) <= 4e-5 and not f.vmask[u, i] and f.train_r[u, i] == 0, ln
        assert u not in last or c <= last[u] + 1e-5, ln                # best first
        last[u] = c
    assert len(last) == N


def test_cli_ucb_behind_fold_in(fx):  # noqa: F811
    """two planted new users beside a few others: one with a single rating, one with fifty"""
    f = fx
    rng = np.random.default_rng(5)
    new = f.tmp / "new_users_ucb.tsv"
    lines, n_new = [], 0
    for uid, cnt in ((900001, 1), (900002, 50), (900003, 7), (900004, 12), (900005, 3)):
        for it in rng.permutation(M)[:cnt]:
            lines.append(f"{uid}\t{f.s2i[it]}\t{rng.integers(1, 6)}\n")
        n_new += 1
    new.write_text("".join(lines))
    common = f.base + f.flags["hier"] + ["-model-dir", f.model["hier"], "-fold-in", new, "-fold-iters", 5, "-recommend", REC]
    plain, args = common + ["-label", "fold_ucb_plain"], common + ["-label", "fold_ucb", "-ucb", Z]
    _run(f.tmp, plain)
    _run(f.tmp, args)
    out, out0 = _outdir(f, args), _outdir(f, plain)
    for name in ("foldin_recommend.tsv", "foldin_recommend.txt", "foldin_htheta.tsv", "foldin_htheta_shape.tsv", "foldin.txt"):
        assert (out / name).read_bytes() == (out0 / name).read_bytes(), name
    assert not (out0 / "foldin_recommend_ucb.tsv").exists() and not (out / "recommend_ucb.tsv").exists()
    got = [ln.split("\t") for ln in (out / "foldin_recommend_ucb.tsv").read_text().splitlines()]
    assert len(got) == REC * n_new and all(len(g) == 5 for g in got)           # M - 50 items are left to the fullest user
    assert (out / "foldin_recommend_ucb.txt").read_text() == "%d\t%d\t%d\t%g\n" % (n_new, len(got), REC, Z)
    cv = {uid: np.mean([float(g[4]) / float(g[3]) for g in got if int(g[0]) == uid]) for uid in (900001, 900002)}
    print("mean sd / mean over the list: one rating %.3f, fifty ratings %.3f" % (cv[900001], cv[900002]))
    assert cv[900001] > cv[900002]


@pytest.mark.parametrize("tail,msg", [
    (["-ucb", "2"], "-ucb goes with -recommend N"),
    (["-recommend", "300", "-ucb", "2"], "-ucb needs -recommend N with N <= 256"),
    (["-recommend", "5", "-ucb", "-1"], "-ucb needs the number of standard deviations"),
    (["-recommend", "5", "-ucb", "two"], "-ucb needs the number of standard deviations"),
    (["-recommend", "5", "-ucb"], "-ucb needs the number of standard deviations"),
    (["-audience", "5", "-ucb", "2"], "-ucb goes with -recommend N, not with -audience")])
def test_cli_refusals(fx, tail, msg):  # noqa: F811
    f = fx
    r = _run(f.tmp, f.base + ["-model-dir", f.model["flat"], "-label", "ucb_refused"] + tail, ok=False)
    assert r.returncode != 0 and msg in r.stdout + r.stderr, (r.returncode, r.stdout[-500:], r.stderr[-500:])
