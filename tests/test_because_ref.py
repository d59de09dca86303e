"""CPU: the reference of hpf_because (tests/because_ref.py) on the inputs tests/test_gpu_because.py runs.

- the identity sum_i c(i -> j) + prior(j) + E[ibias_j] = score holds in mpmath (60 digits);
- plain numpy float64 stays within the bound the GPU test holds the kernels to, (4 S + H + 64) 2^-53 relative, with S <= 80;
- no two neighbours of an exact contribution list are closer than twice that bound, so the GPU test's order check needs
  none of its exemptions.
"""
import numpy as np
import pytest

from tests import because_ref as R


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_identity_float64_distance_and_gaps(case):
    inp, st, res = R.reference(case)
    assert sorted(int(inp.rowptr[u + 1] - inp.rowptr[u]) for u in inp.users[:len(R.HISTORIES)]) == sorted(R.HISTORIES)
    worst_np, least_gap, lists = 0.0, float("inf"), 0
    for q, (b, u, j) in enumerate(inp.pairs()):
        items, yy = inp.history(u)
        con, prior, score = res[q]
        H = len(items)
        S = st.spread(u, items)
        assert S <= 80.0, (case, u, S)
        bnd = R.bound(S, H)
        # the identity, exactly
        whole = R.MP.fsum(con) + prior + (R.MP.mpf(float(st.ib[j])) if st.bias else 0)
        assert abs(whole - score) <= score * R.MP.mpf(10) ** -50, (case, u, j)
        # float64 against it
        (ncon, nprior), = R.numpy64(st, items, yy, u, [j])
        errs = [R.ulps(a, e) for a, e in zip(ncon, con)] + [R.ulps(nprior, prior)]
        worst_np = max(worst_np, max(errs))
        assert max(errs) * R.U53 <= bnd, (case, u, j, max(errs), bnd / R.U53)
        # neighbours of the sorted exact list
        if H > 1:
            lists += 1
            srt = sorted(con, reverse=True)
            gap = min(float((a - c) / a) for a, c in zip(srt, srt[1:]))
            least_gap = min(least_gap, gap / bnd)
            assert gap >= 2.0 * bnd, (case, u, j, gap, bnd)
    print(f"{R.case_id(case)}: numpy within {worst_np:.1f} u; least relative gap {least_gap:.3g} bounds over {lists} lists")


def test_cases_cover_what_the_gpu_test_promises():
    assert {(c[0], c[1], c[2]) for c in R.CASES} == {(b, h, v) for b in (False, True) for h in (False, True) for v in (False, True)}
    assert {c[3] for c in R.CASES} == {1, 5, 64, 65, 100, 130} and {c[4] for c in R.CASES} == {1, 5, 32}
    assert 700 in R.HISTORIES and set(R.HISTORIES) == {0, 1, 2, 63, 64, 65, 129, 700}
    x = np.array([0.018, 0.3, 1.0, 7.5, 40.0])
    want = [float(R.MP.digamma(float(v))) for v in x]
    assert np.allclose(R.digamma(x), want, rtol=1e-12, atol=1e-12)
