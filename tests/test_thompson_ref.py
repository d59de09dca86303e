"""CPU: tests/thompson_ref.py alone -- the numpy statement of the sampler that the GPU tests hold gamma_rows_kernel to must
itself draw from the Gamma distribution, with independent streams per element, and must take no decision near its edge
on the inputs of the GPU value test (the precondition under which a device that evaluates log, log1p and cos within 2 ulp
takes the same decisions)."""
import numpy as np
import pytest

from tests import thompson_ref as ref

N = ref.KS_DRAWS


def test_the_cap_is_the_dkw_massart_bound():
    assert abs(ref.KS_CAP - 0.0421) < 5e-5 and ref.KS_CAP == np.sqrt(np.log(2.0 / 1e-6) / 2.0) / np.sqrt(N)
    assert ref.KS_SHAPES == [0.05, 0.3, float(np.nextafter(1.0, 0.0)), 1.0, 3.7, 100.0, 1e4, 1e8]


@pytest.fixture(scope="module")
def columns():
    """one column of 4096 rows per shape, as the GPU distribution test draws them"""
    shapes = np.array(ref.KS_SHAPES)
    rows = np.broadcast_to(np.arange(N, dtype=np.uint64)[:, None], (N, shapes.size))
    cols = np.broadcast_to(np.arange(shapes.size, dtype=np.uint64)[None, :], (N, shapes.size))
    g, tr = ref.gamma_unit(99, 3, 0, rows, cols, np.broadcast_to(shapes, (N, shapes.size)))
    return shapes, g, tr


def test_ks_distance_from_the_gamma_distribution(columns):
    shapes, g, tr = columns
    assert np.all(tr["attempt"] >= 0) and np.all(np.isfinite(g)) and np.all(g > 0)
    for j, a in enumerate(shapes):
        d = ref.ks_distance(g[:, j], a)
        print(f"shape {a:g}: KS distance {d:.4f} (cap {ref.KS_CAP:.4f}), attempts per element {tr['tries'][:, j].mean():.4f}")
        assert d <= ref.KS_CAP, (a, d)


def test_sample_mean(columns):
    shapes, g, _ = columns
    for j, a in enumerate(shapes):
        assert abs(g[:, j].mean() / a - 1.0) <= 6.0 / np.sqrt(a * N), (a, g[:, j].mean() / a)


def test_adjacent_columns_and_rows_are_uncorrelated(columns):
    _, g, _ = columns
    # (the product of two independent standardised variables has variance 1 whatever their skew: the scale is 1 / sqrt(n))
    z = (g - g.mean(0)) / g.std(0)
    for j in range(g.shape[1] - 1):
        assert abs(np.mean(z[:, j] * z[:, j + 1])) <= 6.0 / np.sqrt(N), j
    for j in range(g.shape[1]):
        assert abs(np.mean(z[:-1, j] * z[1:, j])) <= 6.0 / np.sqrt(N), j
    # one shape in every element: neighbours in a row and in a column of the handle's layout, both sides
    for obj in (0, 1):
        rows = np.broadcast_to(np.arange(64, dtype=np.uint64)[:, None], (64, 64))
        cols = np.broadcast_to(np.arange(64, dtype=np.uint64)[None, :], (64, 64))
        x, _ = ref.gamma_unit(1, 0, obj, rows, cols, np.full((64, 64), 3.7))
        z = (x - x.mean()) / x.std()
        assert abs(np.mean(z[:, :-1] * z[:, 1:])) <= 6.0 / np.sqrt(64 * 63) and abs(np.mean(z[:-1] * z[1:])) <= 6.0 / np.sqrt(64 * 63)
    # and the two sides do not share a stream, nor two draws, nor two seeds
    base, _ = ref.gamma_unit(1, 0, 0, rows, cols, np.full((64, 64), 3.7))
    for seed, draw, obj in ((1, 0, 1), (1, 1, 0), (2, 0, 0), (1 + (1 << 32), 0, 0)):
        other, _ = ref.gamma_unit(seed, draw, obj, rows, cols, np.full((64, 64), 3.7))
        assert np.mean(other == base) < 0.01
        z1, z2 = (base - base.mean()) / base.std(), (other - other.mean()) / other.std()
        assert abs(np.mean(z1 * z2)) <= 6.0 / 64


@pytest.mark.parametrize("K,bias", [(5, True), (100, False)])
def test_precondition_of_the_gpu_value_test(K, bias):
    """seed 20261021, draw 0 on the GPU test's inputs: every decision has margin >= 2^-44 A and every |1 + w| >= 2^-40.  (Had
    the seed failed this, another would have been chosen and named here: the condition itself is not loosened.)"""
    st = ref.value_case(K, bias)
    for want, tr, shapes in ref.reference_sides(st, K, bias, ref.SEED, ref.DRAW):
        assert shapes.min() >= 0.05 and shapes.max() <= 1e8
        assert np.all(tr["attempt"] >= 0)
        print(f"K={K} bias={bias}: smallest margin / A {tr['ratio'].min():.3g}, smallest |1 + w| {np.abs(tr['t']).min():.3g}, "
              f"attempts per element {tr['tries'].mean():.4f}")
        assert tr["ratio"].min() >= ref.MARGIN_MIN and np.abs(tr["t"]).min() >= ref.T_MIN
        assert np.all(np.isfinite(want)) and np.all(want >= 0.0) and np.all(want[want > 0] >= 2.0 ** -1000)
    flat = np.concatenate([st[w].ravel() for w in st if w.endswith("_SHAPE")])
    for planted in (0.3, 1.0, np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0)):
        assert (flat == planted).sum() >= 2                         # on both sides
    assert sum((st[w] == 0.0).sum() for w in st if w.endswith("_E")) >= 10


def test_sample_side_ids_and_layout():
    """a row's sample depends on its id, not on its place in the selection; the bias sits at the side's bias column"""
    st = ref.value_case(5, True, 40, 30)
    (theta, _, _), (beta, _, _) = ref.reference_sides(st, 5, True, 7, 1)
    ids = np.array([33, 0, 5, 5], np.uint64)
    (t2, _, _), (b2, _, _) = ref.reference_sides(st, 5, True, 7, 1, ids, ids[1:])
    assert np.array_equal(ref.bits(t2), ref.bits(theta[ids.astype(np.int64)])) and np.array_equal(ref.bits(b2), ref.bits(beta[ids[1:].astype(np.int64)]))
    # the user bias is column K = 5 of the counter, the item bias column K + 1 = 6
    g, _ = ref.gamma_unit(7, 1, 0, np.arange(40), np.full(40, 5), st["UBIAS_SHAPE"])
    assert np.array_equal(ref.bits(theta[:, 5]), ref.bits(g * (st["UBIAS_E"] / st["UBIAS_SHAPE"])))
    g, _ = ref.gamma_unit(7, 1, 1, np.arange(30), np.full(30, 6), st["IBIAS_SHAPE"])
    assert np.array_equal(ref.bits(beta[:, 5]), ref.bits(g * (st["IBIAS_E"] / st["IBIAS_SHAPE"])))
