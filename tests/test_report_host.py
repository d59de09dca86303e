"""No GPU: the loops the CLI's reports on a saved model share (hgaprec_host.hpp: for_chunks, chunk_offsets, MaskLists,
Ratings::r / ranked_items / item_degrees, write_topn, gamma_expectations) through the host library, against numpy on a
seeded random data set."""
import math

import numpy as np
import pytest

from hgaprec_amd import hostlib

N_USERS, N_ITEMS = 37, 23


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """ids 1-based in the files; some users without a validation pair, duplicated training pairs with two ratings"""
    tmp = tmp_path_factory.mktemp("report_host")
    g = np.random.default_rng(11)
    train = [(u, int(i), int(g.integers(1, 6))) for u in range(N_USERS) for i in g.choice(N_ITEMS, int(g.integers(1, 9)), replace=False)]
    train += [(u, i, y % 5 + 1) for (u, i, y) in train[::7]]                       # the same pair again, another rating
    order = g.permutation(len(train))
    # every user and every item first appears in seq order: seq id == file id - 1
    head = [(u, u % N_ITEMS, 3) for u in range(N_USERS)] + [(0, i, 2) for i in range(N_ITEMS)]
    train = head + [train[j] for j in order]
    valid = sorted({(int(u), int(i)) for u, i in zip(g.integers(0, N_USERS, 90), g.integers(0, N_ITEMS, 90)) if u % 5 != 3})
    (tmp / "train.tsv").write_text("".join(f"{u + 1}\t{i + 1}\t{y}\n" for u, i, y in train))
    (tmp / "validation.tsv").write_text("".join(f"{u + 1}\t{i + 1}\t1\n" for u, i in valid))
    rt = hostlib.Ratings(N_USERS, N_ITEMS)
    assert rt.read_train(tmp / "train.tsv") == 0 and rt.read_heldout(tmp / "validation.tsv", 0) == 0
    assert rt.n == N_USERS and rt.m == N_ITEMS
    assert (rt.seq2user() == np.arange(1, N_USERS + 1)).all() and (rt.seq2item() == np.arange(1, N_ITEMS + 1)).all()
    dense = np.zeros((N_USERS, N_ITEMS), np.int64)
    for u, i, y in train:
        dense[u, i] = y                                                             # the last one stays
    vlists = [[i for (v, i) in valid if v == u] for u in range(N_USERS)]
    assert any(not l for l in vlists) and any(len(l) > 2 for l in vlists)
    return rt, dense, vlists, tmp


def test_training_rating_ranked_items_and_degrees(data):
    rt, dense, _, _ = data
    for u in range(N_USERS):
        assert [rt.r(u, i) for i in range(N_ITEMS)] == dense[u].tolist()
        assert rt.ranked_items(u) == N_ITEMS - int((dense[u] > 0).sum())
    _, col, _ = rt.csr()
    assert (rt.item_degrees() == np.bincount(col, minlength=N_ITEMS)).all()


@pytest.mark.parametrize("rows", [0, 1, 12, 13, 65536, 65537, 200000])
@pytest.mark.parametrize("chunk", [0, 1, 3, 5, 12, 10 ** 6])
def test_chunk_walk_visits_every_row_once_in_order(rows, chunk):
    ch = chunk or 65536
    assert hostlib.chunk_walk(rows, chunk) == [(r0, min(rows, r0 + ch)) for r0 in range(0, rows, ch)]


@pytest.mark.parametrize("chunk", [1, 3, 5, 64])
@pytest.mark.parametrize("scattered", [False, True])
def test_mask_lists_and_query_offsets_across_chunk_boundaries(data, chunk, scattered):
    rt, _, vlists, _ = data
    g = np.random.default_rng(5)
    users = g.integers(0, N_USERS, 29).astype(np.uint32) if scattered else np.arange(N_USERS, dtype=np.uint32)
    qptr = np.concatenate([[0], np.cumsum(g.integers(0, 4, users.size))]).astype(np.uint64)
    one_u, one_p, one_i = rt.mask_lists(0, users) if scattered else rt.mask_lists(0)
    assert (one_u == users).all()
    assert one_p.tolist() == np.concatenate([[0], np.cumsum([len(vlists[u]) for u in users])]).tolist()
    assert one_i.tolist() == [i for u in users for i in vlists[u]]
    cat_u, cat_p, cat_i, cat_q = [], [0], [], [0]
    for b0, b1 in hostlib.chunk_walk(users.size, chunk):
        u, p, i = rt.mask_lists(0, users[b0:b1]) if scattered else rt.mask_lists(0, None, b0, b1)
        assert p[0] == 0 and p.size == b1 - b0 + 1 and p[-1] == i.size
        cq = hostlib.chunk_offsets(qptr, b0, b1)
        assert cq[0] == 0 and cq.size == b1 - b0 + 1
        cat_p += (len(cat_i) + p[1:].astype(np.int64)).tolist()
        cat_u += u.tolist(); cat_i += i.tolist()
        cat_q += (int(qptr[b0]) + cq[1:].astype(np.int64)).tolist()
    assert cat_u == one_u.tolist() and cat_p == one_p.tolist() and cat_i == one_i.tolist() and cat_q == qptr.tolist()


def test_mask_lists_of_a_rank_are_local_and_inside_its_range(data):
    rt, _, vlists, _ = data
    sample = np.array([30, 2, 11, 17, 10, 29, 18, 11], np.uint32)
    u, p, i = rt.mask_lists(0, sample, 10, 18, 10)
    kept = [int(s) for s in sample if 10 <= s < 18]
    assert u.tolist() == [s - 10 for s in kept] and i.tolist() == [x for s in kept for x in vlists[s]]
    assert p.tolist() == np.concatenate([[0], np.cumsum([len(vlists[s]) for s in kept])]).tolist()


@pytest.mark.parametrize("real", [0, 3, 6, 40])
@pytest.mark.parametrize("keep", [False, True])
def test_list_writer_prints_the_kept_real_entries(data, real, keep):
    rt, dense, _, tmp = data
    N = 6
    g = np.random.default_rng(7)
    sel = np.array([5, 36, 0, 17], np.uint32)
    items = g.integers(0, N_ITEMS, (sel.size, N)).astype(np.uint32)
    scores = g.random((sel.size, N)) * 3
    shown = min(real, N)
    items[:, shown:] = 0xffffffff                                                   # padding: an index nobody may follow
    uid, iid = rt.seq2user(), rt.seq2item()
    want = [f"{uid[u]}\t{iid[it]}\t{scores[b, j]:.5f}\n"
            for b, u in enumerate(sel) for j, it in enumerate(items[b, :shown]) if not (keep and dense[u, it] != 0)]
    path = tmp / f"topn_{real}_{int(keep)}.tsv"
    lines = hostlib.write_topn(path, sel, items, scores, real, uid, iid, rt if keep else None)
    assert lines == len(want) and path.read_text() == "".join(want)
    if keep and real >= N:
        assert lines < sel.size * N                                                 # the predicate did reject something


@pytest.mark.parametrize("per_column", [False, True])
def test_gamma_expectations_are_the_formula(per_column):
    g = np.random.default_rng(3)
    sh = g.gamma(0.3, 1.0, (19, 5)) + 1e-12
    rt = g.gamma(2.0, 1.0, 5 if per_column else (19, 5)) + 1e-12
    E, L = hostlib.gamma_expectations(sh, rt, "m/hbeta_rate.tsv")
    full = np.broadcast_to(rt, sh.shape)
    assert (E == sh / full).all()
    psi = hostlib.digamma(sh.ravel()).reshape(sh.shape)
    assert L.tolist() == [[psi[r, c] - math.log(full[r, c]) for c in range(5)] for r in range(19)]


@pytest.mark.parametrize("bad", [0.0, -0.5, float("nan")])
@pytest.mark.parametrize("where", ["shape", "rate", "rate vector"])
def test_gamma_expectations_refuse_what_is_not_positive(bad, where):
    sh = np.full((4, 3), 0.7)
    rt = np.full(3 if where == "rate vector" else (4, 3), 1.3)
    (sh if where == "shape" else rt)[(1,) if where == "rate vector" else (2, 1)] = bad
    row = 0 if where == "rate vector" else 2
    with pytest.raises(ValueError, match=rf"^m/beta_rate\.tsv: a shape or a rate that is not > 0 \(row {row}\)$"):
        hostlib.gamma_expectations(sh, rt, "m/beta_rate.tsv")
