"""The mpmath references of tests/report_ref.py held against the CPU oracle, so that the references -- and the magnitudes
A their bounds are stated in -- are validated without a GPU before tests/test_gpu_report_terms.py holds the kernels to them.

A small model (30 users, 20 items, K = 5) runs two iterations in the oracle: hier, flat, bias, binary.  From the oracle's
exported state the references evaluate every held-out pair and every term of the ELBO; the oracle's own totals
(orc.Model.heldout_sum, .elbo()) must lie within the bound a kernel is held to -- sum of c u A over the terms plus
n u sum |term| for the additions, c = 4 max(1, c_ref) -- with the oracle in the device's place.  c_ref is measured here,
on these inputs, from the plain-double restatement of the same formulas, and printed.

c_ref seen (glibc, x86-64): pair likelihood 1.6 .. 4.7 (the serial sum of log i in log y!), nonzero term 1.3 .. 3.4,
Gamma term 1.4 .. 2.2.
"""
import numpy as np
import pytest

from oracle import orc
from tests import report_ref as rr
from tests.util import heldout_pairs, make_problem

N, M, K = 30, 20, 5

CASES = [
    pytest.param((True, False, False), id="hier"),
    pytest.param((False, False, False), id="flat"),
    pytest.param((True, True, False), id="hier-bias"),
    pytest.param((False, True, False), id="flat-bias"),
    pytest.param((True, False, True), id="hier-binary"),
]


def _state(Mo, hier, bias):
    names = ["THETA", "BETA"] + (["XI", "ETA"] if hier else []) + (["UBIAS", "IBIAS"] if bias else [])
    return {f"{o}_{k}": Mo.state(f"{o}_{k}") for o in names for k in ("SHAPE", "RATE", "E", "ELOG")}


@pytest.fixture(scope="module", params=CASES)
def model(request):
    hier, bias, binary = request.param
    rowptr, col, val = make_problem(N, M, 150, seed=3)
    if binary:
        val = np.ones_like(val)
    Mo = orc.Model(N, M, K, hier, bias, binary)
    Mo.set_csr(rowptr, col, val)
    Mo.initialize(0)
    Mo.iterate(1)
    used = {o: (Mo.state(f"{o}_E"), Mo.state(f"{o}_ELOG")) for o in ("XI", "ETA")} if hier else None
    Mo.iterate(1)
    return Mo, _state(Mo, hier, bias), used, (rowptr, col, val), (hier, bias, binary)


def test_pair_likelihood_reference_agrees_with_the_oracle(model):
    Mo, st, _, _, (hier, bias, binary) = model
    hu, hi, hy = heldout_pairs(N, M, 200, seed=4)
    if binary:
        hy = (np.arange(hy.size) % 3 > 0).astype(np.int32)            # zeros and ones
    else:
        hy[:8] = [0, 255, 256, 300, -1, 44, 2, 2 ** 31 - 1]          # the yval_t wrap
    terms, plain = [], []
    for u, i, y in zip(hu, hi, hy):
        ub, ib = (st["UBIAS_E"][u], st["IBIAS_E"][i]) if bias else (None, None)
        terms.append(rr.pair_ll(st["THETA_E"][u], st["BETA_E"][i], y, ub, ib, binary))
        plain.append(rr.plain_pair_ll(st["THETA_E"][u], st["BETA_E"][i], y, ub, ib, binary))
    c_ref = rr.c_ref(plain, terms)
    exact, bound = rr.sum_bound(terms, rr.c_for(c_ref))
    got = Mo.heldout_sum(hu, hi, hy)
    print(f"\npair likelihood: c_ref {c_ref:.2f}; oracle sum {got!r}, |error| / bound {abs(got - float(exact)) / bound:.3f}")
    assert rr.abs_err(got, exact) <= bound


def test_elbo_reference_agrees_with_the_oracle(model):
    Mo, st, used, (rowptr, col, val), (hier, bias, binary) = model
    rows = np.repeat(np.arange(N), np.diff(rowptr))
    pairs = [(int(u), int(i), int(y), 1) for u, i, y in zip(rows, col, val)]
    nnz, gamma = rr.elbo_terms(st, used, pairs, K, hier, bias, 0.3, 0.3)
    c_nnz = rr.c_ref([t[2] for t in nnz], [t[:2] for t in nnz])
    c_gamma = rr.c_ref([t[2] for t in gamma], [t[:2] for t in gamma])
    exact, bound = rr.elbo_bound(nnz, gamma, rr.c_for(c_nnz), rr.c_for(c_gamma))
    got = Mo.elbo()
    print(f"\nELBO: c_ref nonzero term {c_nnz:.2f}, Gamma term {c_gamma:.2f}; oracle {got!r}, "
          f"|error| / bound {abs(got - float(exact)) / bound:.3f}, bound / |ELBO| {bound / abs(got):.1e}")
    assert rr.abs_err(got, exact) <= bound


def test_references_on_values_known_in_closed_form():
    """the formulas themselves, where the answer is known without them"""
    import mpmath as mp
    with mp.workdps(rr.DPS):
        # one factor, E = 2 and 3, y = 2: 2 log 6 - 6 - log 2
        e, A = rr.pair_ll([2.0], [3.0], 2)
        assert abs(e - (2 * mp.log(6) - 6 - mp.log(2))) < mp.mpf(10) ** -40 and A == pytest.approx(2 * np.log(6) + 6 + np.log(2))
        # the wrap: 256 is 0, 257 is 1, -1 is 255
        assert rr.pair_ll([2.0], [3.0], 256)[0] == rr.pair_ll([2.0], [3.0], 0)[0] == -6
        assert rr.pair_ll([2.0], [3.0], -1)[0] == rr.pair_ll([2.0], [3.0], 255)[0]
        # the clamp from both sides
        assert rr.pair_ll([0.0], [3.0], 0, binary=True)[0] == -mp.mpf(1e-30)
        assert rr.pair_ll([1e-20], [1e-20], 0, binary=True)[0] == -mp.mpf(1e-30)
        assert rr.pair_ll([2e-15], [1e-15], 0, binary=True)[0] == -(mp.mpf(2e-15) * mp.mpf(1e-15))
        # two equal columns: logsumexp = x + log 2; y = 3: 9 (x + log 2 - log 3) - dot
        e, _ = rr.nnz_term([0.5, 0.25], [0.25, 0.5], [1.0, 2.0], [3.0, 4.0], 3)
        assert abs(e - (9 * (mp.mpf(0.75) + mp.log(2) - mp.log(3)) - 11)) < mp.mpf(10) ** -40
        # the W form of the same rows
        w = float(mp.exp(mp.mpf(-0.25)))
        e2, _ = rr.nnz_term_w([1.0, w], [w, 1.0], 0.5, 0.5, [1.0, 2.0], [3.0, 4.0], 3)
        assert abs(e2 - e) < 1e-14
        # a Gamma(1, 1) element under a Gamma(1, 1) prior with its exact E = 1: every addend cancels but the two b E
        e, A = rr.gamma_term(1.0, 1.0, 1.0, -0.5772156649015329, 1.0, 1.0)
        assert abs(e) < mp.mpf(10) ** -40 and A == pytest.approx(2.0)
        # the clamps
        assert rr.gamma_term(0.0, 2.0, 1.0, 0.0, 0.3, 0.3)[0] == rr.gamma_term(-1.0, 2.0, 1.0, 0.0, 0.3, 0.3)[0] \
            == rr.gamma_term(1e-30, 2.0, 1.0, 0.0, 0.3, 0.3)[0]
        assert rr.gamma_term(2.0, 0.0, 1.0, 0.0, 0.3, 0.3)[0] == rr.gamma_term(2.0, 1e-30, 1.0, 0.0, 0.3, 0.3)[0]
