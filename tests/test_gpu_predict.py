"""-m gpu: hpf_predict -- the rate of a list of (user, item) pairs, E_theta[u] . E_beta[i] (+ both biases) --
against the oracle state's serial dot product."""
import numpy as np
import pytest

from tests.test_gpu_ranking import _setup
from tests.util import heldout_pairs

pytestmark = pytest.mark.gpu

SHAPES = [(5, False, 200), (7, True, 70), (100, False, 1000), (260, True, 64)]
N = 150


def _serial(M, u, i, bias):
    """prediction_score_hier: s += E_theta[u][k] * E_beta[i][k] for k ascending, then the biases"""
    Et, Eb = M.state("THETA_E"), M.state("BETA_E")
    s = np.zeros(u.size)
    for k in range(Et.shape[1]):
        s += Et[u, k] * Eb[i, k]
    if bias:
        s = s + (M.state("UBIAS_E")[u] + M.state("IBIAS_E")[i])
    return s


@pytest.mark.parametrize("K,bias,m", SHAPES)
def test_predict_matches_serial_dot_product(orc, K, bias, m):
    from hgaprec_amd.capi import Hpf, HpfError
    M, D, *_ = _setup(orc, N, m, K, 4000, bias, seed=K)
    u, i, _ = heldout_pairs(N, m, 3000, seed=K + 1)
    want = _serial(M, u, i, bias)
    got = D.predict(u, i)
    assert got.shape == want.shape
    assert np.max(np.abs(got - want) / want) < 1e-12

    # a handle with only the expectations and no CSR gives the same numbers
    with Hpf(N, m, K, hier=True, bias=bias) as E:
        E.set_state("THETA_E", D.get_state("THETA_E"))
        E.set_state("BETA_E", D.get_state("BETA_E"))
        if bias:
            E.set_state("UBIAS_E", D.get_state("UBIAS_E"))
            E.set_state("IBIAS_E", D.get_state("IBIAS_E"))
        assert np.array_equal(E.predict(u, i), got)
        assert E.predict(np.zeros(0, np.uint32), np.zeros(0, np.uint32)).size == 0        # cnt = 0
        for bu, bi in (([0, N], [0, 0]), ([0, 1], [m, 0])):
            with pytest.raises(HpfError):
                E.predict(np.array(bu, np.uint32), np.array(bi, np.uint32))
    D.close()


def test_predict_needs_expectations():
    from hgaprec_amd.capi import Hpf, HpfError
    with Hpf(10, 10, 4) as D:
        with pytest.raises(HpfError):
            D.predict(np.array([1], np.uint32), np.array([1], np.uint32))
