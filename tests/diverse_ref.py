"""The definition of hpf_recommend_diverse's greedy selection in numpy (include/hpf.h): plain fp64 operations in the
stated order, given a pool, a Gram matrix and lambda.  numpy's scalar and array arithmetic on float64 is IEEE: one rounding
per operation, nothing contracted.

    rel_j = r_j / r_0;  om = 1.0 - lambda;  pen_j = 0.0
    for t = 0 .. min(topn, P) - 1:
        key_j = lambda * rel_j - om * pen_j          over the entries not yet picked
        j*    = the largest key, compared as values; among equal keys the smallest j
        out[t] = (c_j*, r_j*, pen_j*, key_j*)
        pen_j = max(pen_j, G[j, j*])                 over the entries still unpicked
    positions from min(topn, P) on: (0xffffffff, 0.0, 0.0, 0.0)
"""
import numpy as np

PAD = 0xFFFFFFFF


def pool_of(items, scores):
    """the pool of one user from a list hpf_recommend returned at topn = pool: the prefix whose score is > +0.0"""
    items = np.asarray(items, np.uint32)
    scores = np.asarray(scores, np.float64)
    ok = (scores > 0.0) & (items != PAD)
    P = int(ok.size if ok.all() else np.argmin(ok))
    return items[:P].copy(), scores[:P].copy()


def mmr(pool_items, pool_scores, G, topn, lam):
    """pool_items / pool_scores: [P] in list order (every score > 0); G: [P, P], G[j, k] the cosine of pool entries j and k.
    -> (items, scores, maxsim, mmr), each [topn]"""
    c = np.asarray(pool_items, np.uint32)
    r = np.asarray(pool_scores, np.float64)
    G = np.asarray(G, np.float64)
    P = c.size
    assert r.shape == (P,) and G.shape == (P, P)
    lam = np.float64(lam)
    out_i = np.full(topn, PAD, np.uint32)
    out_s, out_m, out_k = np.zeros(topn), np.zeros(topn), np.zeros(topn)
    if P == 0:
        return out_i, out_s, out_m, out_k
    rel = r / r[0]
    om = np.float64(1.0) - lam
    pen = np.zeros(P, np.float64)
    alive = np.ones(P, bool)
    for t in range(min(topn, P)):
        key = lam * rel - om * pen
        best = -1
        for j in range(P):                                          # by value, ties to the smaller j
            if alive[j] and (best < 0 or key[j] > key[best]):
                best = j
        out_i[t], out_s[t], out_m[t], out_k[t] = c[best], r[best], pen[best], key[best]
        alive[best] = False
        pen = np.where(alive, np.maximum(pen, G[:, best]), pen)
    return out_i, out_s, out_m, out_k


def mmr_lists(lists_items, lists_scores, gram_of, topn, lam):
    """mmr over the lists hpf_recommend returned at topn = pool for several users; gram_of(items) -> the Gram matrix of a pool"""
    outs = []
    for it, sc in zip(lists_items, lists_scores):
        c, r = pool_of(it, sc)
        outs.append(mmr(c, r, gram_of(c), topn, lam))
    return tuple(np.stack([o[k] for o in outs]) for k in range(4))


def fixture():
    """The hand-checkable model, every number exact in binary: K = 2, no bias, one user with E[theta] = (1, 0.25); items
    0, 1, 2 with rows (4, 0), (2, 0), (1, 0), items 3, 4, 5 with rows (0, 4), (0, 2), (0, 1), item 6 with row (0, 0), the
    user's one training item.  Scores 4, 2, 1, 1, .5, .25 (items 0 .. 5); the cosine is 1 inside a group and 0 across.
    With lambda = 0.5, pool = topn = 6: rel = 1, .5, .25, .25, .125, .0625; round 0 picks item 0 (key .5); round 1 the keys
    are .25 - .5, .125 - .5, and .125, .0625, .03125 for the other group: item 3; from then on every pen is 1:
    .25 - .5 = -.25 (item 1), .125 - .5 = -.375 (item 2), -.4375 (item 4), -.46875 (item 5)."""
    theta = np.array([[1.0, 0.25]])
    beta = np.array([[4.0, 0.0], [2.0, 0.0], [1.0, 0.0], [0.0, 4.0], [0.0, 2.0], [0.0, 1.0], [0.0, 0.0]])
    want = dict(items=np.array([0, 3, 1, 2, 4, 5], np.uint32), scores=np.array([4.0, 1.0, 2.0, 1.0, 0.5, 0.25]),
                maxsim=np.array([0.0, 0.0, 1.0, 1.0, 1.0, 1.0]), mmr=np.array([0.5, 0.125, -0.25, -0.375, -0.4375, -0.46875]))
    return theta, beta, 6, want
