"""-m gpu: the user pass that writes W in its segment epilogue (phi_pass_fused_kernel, row_sums_kernel) against
the two kernels apart (phi_pass_packed_kernel, row_sweep_kernel): HPF_FUSED_SWEEP=2 -- the fused route wherever an instance
exists, not only for the shape the library takes it for by default -- and =0 in one build.

The split keeps every array bit-identical: the epilogue computes W of a single-segment row with the sweep's own device
functions on the sums it holds in registers, and the sums kernel keeps the sweep's grid, its group -> rows mapping and the
order of csum / rsum / red[] / colsum_part.  So every test runs both routes for 4 iterations and compares EVERY state array
and work_info() with np.array_equal -- over the column counts that give 4, 8 and 16 lanes per nonzero and odd and even
element counts (K = 20 keeps plain rows and K = 200's shape spills with the epilogue: hpf_plan::fused_sweep leaves both
unfused, and the two routes are then the same kernels), row-major and tiled work lists, -bias, -hier, -novb, the three
pieces of a rank of two, hipGraph replay, user sides of one row and of 65, and a first user pass whose epilogue meets an
element the p59 rows cannot hold (the fall-back protocol: one fall-back, the bits of a w_storage = 3 run).

The problem is the tiled tests': make_problem(900, 600, 40000, 5, heavy_user, heavy_item, singles) -- long rows cut into
segments, users with one rating -- with three users without any rating appended.
"""
import numpy as np
import pytest

from tests.util import compare_states, init_states, make_problem

pytestmark = pytest.mark.gpu

ITERS = 4
N, M_ITEMS, N_EMPTY = 900, 600, 3
_cache = {}


def _problem():
    if "prob" not in _cache:
        rowptr, col, val = make_problem(N, M_ITEMS, 40000, 5, heavy_user=True, heavy_item=True, singles=True)
        rowptr = np.concatenate([rowptr, np.full(N_EMPTY, rowptr[-1], np.int64)])      # users without a rating
        _cache["prob"] = (rowptr, col, val)
    return _cache["prob"]


def _start_state(n, m, K, hier, bias, seed=11, s_prior=0.3):
    """a random valid state, shared by the runs of a case (and left unchanged): Elog spread 12 inside a row"""
    key = ("st", n, m, K, hier, bias, seed)
    if key not in _cache:
        rng = np.random.default_rng(seed + K)
        st = {}
        for name, rows in (("THETA", n), ("BETA", m)):
            st[f"{name}_SHAPE"] = rng.uniform(0.3, 2.0, (rows, K))
            st[f"{name}_E"] = rng.uniform(0.05, 1.5, (rows, K))
            st[f"{name}_ELOG"] = rng.uniform(-12.0, 0.0, (rows, K))
        if hier:
            for name, rows in (("XI", n), ("ETA", m)):
                rate = rng.uniform(0.5, 3.0, rows)
                shape = np.full(rows, s_prior + K * s_prior)
                st[f"{name}_SHAPE"], st[f"{name}_RATE"] = shape, rate
                st[f"{name}_E"], st[f"{name}_ELOG"] = shape / rate, rng.uniform(-2.0, 2.0, rows)
        if bias:
            for name, rows in (("UBIAS", n), ("IBIAS", m)):
                st[f"{name}_SHAPE"] = rng.uniform(0.3, 2.0, rows)
                st[f"{name}_E"] = rng.uniform(0.05, 1.5, rows)
                st[f"{name}_ELOG"] = rng.uniform(-12.0, 0.0, rows)
        assert set(st) == set(init_states(hier, bias))
        _cache[key] = st
    return _cache[key]


def _run(monkeypatch, route, prob, K, hier, bias, state=None, step=None, **hpf_kw):
    """one handle under HPF_FUSED_SWEEP=route: ITERS iterations -> ({state: array}, work_info)"""
    from hgaprec_amd.capi import Hpf
    monkeypatch.setenv("HPF_FUSED_SWEEP", route)
    rowptr, col, val = prob
    n = rowptr.size - 1
    m = hpf_kw.pop("m", M_ITEMS)
    D = Hpf(n, m, K, hier=hier, bias=bias, **hpf_kw)
    D.upload_csr(rowptr, col, val)
    for w, a in (state or _start_state(n, m, K, hier, bias)).items():
        D.set_state(w, a)
    if step is None:
        D.iterate(ITERS)                                    # one call, no synchronisation inside
    else:
        for _ in range(ITERS):
            step(D)
    out = {w: D.get_state(w) for w in compare_states(hier, bias)}
    wi = D.work_info()
    D.close()
    return out, wi


def _same(a, b, hier, bias, what=""):
    for w in compare_states(hier, bias):
        assert np.array_equal(a[0][w], b[0][w]), (what, w)
        assert np.all(np.isfinite(a[0][w])), (what, w)
    assert a[1] == b[1], (what, a[1], b[1])


def _both(monkeypatch, prob, K, hier, bias, **kw):
    on = _run(monkeypatch, "2", prob, K, hier, bias, **kw)
    off = _run(monkeypatch, "0", prob, K, hier, bias, **kw)
    _same(on, off, hier, bias)
    return on, off


@pytest.mark.parametrize("hier", [True, False])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("K", [20, 50, 100, 200])
def test_row_major_lists(monkeypatch, K, bias, hier):
    """(4, 6) at K = 50, (8, 6) at K = 100: 13 elements per lane, two or four totals per lane after the reduce-scatter; rows of
    several segments (the heavy user, the heavy item's side is the other one), single ratings, empty rows"""
    on, _ = _both(monkeypatch, _problem(), K, hier, bias)
    wi = on[1]
    assert wi["w_fallbacks"] == 0 and wi["w_layout"] == (0 if K == 20 else 3), wi
    assert wi["tiles_user"] == 0 and wi["tiles_item"] == 0, wi


@pytest.mark.parametrize("hier,bias", [(True, False), (False, True)])
@pytest.mark.parametrize("K", [20, 50, 100, 200])
def test_tiled_lists(monkeypatch, K, hier, bias):
    """every row regrouped by tile: a user whose ratings fall into one tile is one segment of a one-wave workgroup, the others
    are combined from their partials and keep the full sweep body"""
    monkeypatch.setenv("HPF_EXPERIMENTAL", "1")
    monkeypatch.setenv("HPF_TILE", "1")
    monkeypatch.setenv("HPF_TILE_BYTES", "8192")
    on, _ = _both(monkeypatch, _problem(), K, hier, bias)
    assert on[1]["tiles_user"] > 1 and on[1]["tiles_item"] > 1 and on[1]["w_fallbacks"] == 0, on[1]


@pytest.mark.parametrize("n_users", [1, 65])
def test_one_user_and_one_past_a_wave(monkeypatch, n_users):
    """a user side of exactly one row (more waves than rows, a sweep group alone in its wave) and of 65: one past the 64 rows
    of four sweep workgroups, the last done word with a single bit in use"""
    m, K = 80, 100
    rowptr, col, val = make_problem(n_users, m, 30 * n_users, 3)
    _both(monkeypatch, (rowptr, col, val), K, True, False, m=m)
    _both(monkeypatch, (rowptr, col, val), K, False, True, m=m)


def test_novb(monkeypatch):
    """-novb with -bias and without -hier: the item rate is built from the column sums of before this iteration's user sweep"""
    _both(monkeypatch, _problem(), 100, False, True, novb=True)
    _both(monkeypatch, _problem(), 50, True, False, novb=True)


@pytest.mark.parametrize("graph", ["0", "1"])
def test_graph_replay_and_eager(monkeypatch, graph):
    monkeypatch.setenv("HPF_EXPERIMENTAL", "1")
    monkeypatch.setenv("HPF_GRAPH", graph)
    on, _ = _both(monkeypatch, _problem(), 100, True, False)
    assert on[1]["graph_replay"] == int(graph), on[1]


@pytest.mark.parametrize("graph", ["0", "1"])
def test_the_three_pieces_of_a_rank_of_two(monkeypatch, graph):
    """rank 0 of two with the first half of the users, through hpf_iterate_local_items / _users / hpf_iterate_global (eager and
    as three graph replays); nothing is exchanged, so the buffer holds this rank's part -- the same in both routes"""
    from hgaprec_amd import dist as hd
    monkeypatch.setenv("HPF_EXPERIMENTAL", "1")
    monkeypatch.setenv("HPF_GRAPH", graph)
    rowptr, col, val = _problem()
    n = rowptr.size - 1
    b = n // 2
    shard = hd.shard_csr(rowptr, col, val, 0, b)

    def step(D):
        D.iterate_local_items(); D.iterate_local_users(); D.iterate_global()

    for K, hier, bias in ((100, True, False), (50, True, True)):
        _both(monkeypatch, shard, K, hier, bias, step=step, n_ranks=2, rank=0, n_users_total=n)


def test_an_epilogue_that_cannot_pack_its_row(monkeypatch):
    """A column of E[beta] of 1e40 makes the first user rate in that column ~1e42: W there is e^-97 of the row maximum, which a
    p59 row cannot hold.  With the fused route it is the PASS that meets it, in the epilogue of an early segment, while most
    of its 5 000 users' workgroups have not started: they must not skip (the flag it raises is the pending bit; the sums kernel
    turns it into bit 1).  Four iterations in one call complete, with one fall-back, where a w_storage = 3 run ends and where
    the unfused route ends, bit for bit.  Legal input throughout: the library's own flags, nothing provoked."""
    n, m, K = 5000, 300, 100
    prob = make_problem(n, m, 60000, 7, heavy_item=True)
    st = dict(_start_state(n, m, K, True, False, seed=23))
    be = st["BETA_E"].copy()
    be[:, 0] = 1e40
    st["BETA_E"] = be
    on = _run(monkeypatch, "1", prob, K, True, False, state=st, m=m)            # the default route: K = 100 is fused
    off = _run(monkeypatch, "0", prob, K, True, False, state=st, m=m)
    plain = _run(monkeypatch, "2", prob, K, True, False, state=st, m=m, w_storage=3)
    assert on[1]["w_layout"] == 4 and on[1]["w_fallbacks"] == 1, on[1]
    assert off[1]["w_layout"] == 4 and off[1]["w_fallbacks"] == 1, off[1]
    assert plain[1]["w_layout"] == 4 and plain[1]["w_fallbacks"] == 0, plain[1]
    _same(on, off, True, False, "fused against unfused")
    for w in compare_states(True, False):
        assert np.array_equal(on[0][w], plain[0][w]), w
