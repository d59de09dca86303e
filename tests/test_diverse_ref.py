"""CPU: tests/diverse_ref.py, the numpy statement of hpf_recommend_diverse's greedy selection, against the properties the
definition implies and against the hand-checked fixture."""
import numpy as np
import pytest

from tests import diverse_ref as R


def _random_case(rng, P, K=6):
    X = rng.gamma(0.5, 1.0, (P, K)) + 1e-3
    U = X / np.linalg.norm(X, axis=1, keepdims=True)
    G = U @ U.T
    G = np.maximum(G, G.T)                                            # symmetric bit for bit, as the kernel's is
    r = np.sort(rng.gamma(1.0, 1.0, P) + 1e-6)[::-1].copy()
    c = rng.permutation(10 * P)[:P].astype(np.uint32)
    return c, r, G


@pytest.mark.parametrize("P,topn,lam", [(1, 1, 0.5), (7, 7, 0.0), (16, 5, 0.3), (33, 33, 0.7), (40, 64, 0.5), (64, 20, 1.0)])
def test_every_pick_maximises_the_key_among_the_unpicked(P, topn, lam):
    rng = np.random.default_rng(P * 131 + topn)
    c, r, G = _random_case(rng, P)
    items, scores, maxsim, key = R.mmr(c, r, G, topn, lam)
    n = min(topn, P)
    assert items[0] == c[0] and scores[0] == r[0] and maxsim[0] == 0.0 and key[0] == np.float64(lam) * 1.0   # the first pick is c_0
    pos = {int(v): j for j, v in enumerate(c)}
    picked = []
    rel = r / r[0]
    for t in range(n):
        j = pos[int(items[t])]
        assert j not in picked and scores[t] == r[j]
        pen = np.array([max([0.0] + [G[q, p] for p in picked]) for q in range(P)])
        keys = np.float64(lam) * rel - (np.float64(1.0) - np.float64(lam)) * pen
        rest = [q for q in range(P) if q not in picked]
        assert maxsim[t] == pen[j] and key[t] == keys[j]
        assert all(keys[j] > keys[q] or (keys[j] == keys[q] and j <= q) for q in rest)       # the largest, ties to the smaller j
        picked.append(j)
    assert (items[n:] == R.PAD).all() and not scores[n:].any() and not maxsim[n:].any() and not key[n:].any()


@pytest.mark.parametrize("P,topn", [(1, 1), (9, 4), (20, 20), (20, 30)])
def test_lambda_one_is_the_identity(P, topn):
    c, r, G = _random_case(np.random.default_rng(P + topn), P)
    r[P // 2:] = r[P // 2]                                            # a run of equal scores: the order of the list holds
    items, scores, maxsim, key = R.mmr(c, r, G, topn, 1.0)
    n = min(topn, P)
    assert (items[:n] == c[:n]).all() and (scores[:n] == r[:n]).all() and (key[:n] == r[:n] / r[0]).all()
    assert (items[n:] == R.PAD).all()


def test_ties_go_to_the_earlier_pool_position():
    c = np.array([5, 9, 2, 7], np.uint32)
    r = np.array([2.0, 1.0, 1.0, 1.0])
    G = np.zeros((4, 4)); np.fill_diagonal(G, 1.0)
    items, _, _, key = R.mmr(c, r, G, 4, 0.5)
    assert items.tolist() == [5, 9, 2, 7] and key.tolist() == [0.5, 0.25, 0.25, 0.25]
    # -0.0 and +0.0 are equal as values: lambda = 0 and a zero cosine give keys of either sign, the smaller j wins
    items, _, _, key = R.mmr(c, r, G, 4, 0.0)
    assert items.tolist() == [5, 9, 2, 7] and not key.any()


def test_pool_is_the_positive_prefix():
    it = np.array([3, 1, 4, 0, R.PAD], np.uint32)
    sc = np.array([2.0, 1.0, 0.5, 0.0, 0.0])
    c, r = R.pool_of(it, sc)
    assert c.tolist() == [3, 1, 4] and r.tolist() == [2.0, 1.0, 0.5]
    c, r = R.pool_of(it[3:], sc[3:])
    assert c.size == 0 and R.mmr(c, r, np.zeros((0, 0)), 3, 0.5)[0].tolist() == [R.PAD] * 3


def test_hand_checked_fixture():
    theta, beta, topn, want = R.fixture()
    s = (theta @ beta.T)[0]
    order = np.lexsort((np.arange(7), -s))[:6]                        # hpf_recommend's order: score descending, ties by item
    nrm = np.linalg.norm(beta, axis=1, keepdims=True)
    U = np.divide(beta, nrm, out=np.zeros_like(beta), where=nrm > 0)
    c, r = R.pool_of(order.astype(np.uint32), s[order])
    items, scores, maxsim, key = R.mmr(c, r, (U @ U.T)[np.ix_(c, c)], topn, 0.5)
    assert items.tolist() == want["items"].tolist() == [0, 3, 1, 2, 4, 5]
    assert scores.tolist() == want["scores"].tolist()
    assert maxsim.tolist() == want["maxsim"].tolist() == [0, 0, 1, 1, 1, 1]
    assert key.tolist() == want["mmr"].tolist() == [.5, .125, -.25, -.375, -.4375, -.46875]
