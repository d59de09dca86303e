"""CPU: tests/toplist.py forgives what a reference at a relative tolerance cannot decide, and nothing else."""
import numpy as np

from tests.toplist import NONE, tolerant_rank, tolerant_top

RTOL = 1e-9


def _case():
    """40 scores well apart (at least 1e-3 relative), except 7 and 23, which differ by 5e-10 relative"""
    ref = 1.0 + 0.01 * np.random.default_rng(3).permutation(40).astype(np.float64)
    ref[23] = ref[7] * (1.0 + 5e-10)
    order = np.lexsort((np.arange(40), -ref))
    return ref, order


def test_the_exact_list_and_a_near_tie_swap_are_accepted():
    ref, order = _case()
    a = int(np.flatnonzero(order == 23)[0])
    assert order[a + 1] == 7
    for topn in (a + 2, a + 1, 10, 40):                     # the pair inside the list, the pair at the cut, elsewhere
        ids = order[:topn].copy()
        assert tolerant_top(ids, ref[ids], ref, RTOL) is None
        if topn >= a + 2:
            ids[[a, a + 1]] = ids[[a + 1, a]]               # the device saw them the other way round, each within rtol
            vals = ref[ids]
            vals[a], vals[a + 1] = ref[23], ref[7]          # ... so that its values still descend
            assert tolerant_top(ids, vals, ref, RTOL) is None
    ids = order[:a + 1].copy()
    ids[a] = 7                                              # at the cut the other one of the pair got in
    assert tolerant_top(ids, ref[ids] * (1 + 3e-10), ref, RTOL) is None
    # values within rtol of the reference, padded beyond the candidates
    ids = np.concatenate([order, [NONE, NONE]])
    vals = np.concatenate([ref[order] * (1.0 - 4e-10), [0.0, 0.0]])
    assert tolerant_top(ids, vals, ref, RTOL) is None


def test_a_masked_candidate_stands_at_zero():
    ref, order = _case()
    masked = [int(order[0]), int(order[3])]
    kept = np.array([i for i in order if i not in masked])
    assert tolerant_top(kept[:10], ref[kept[:10]], ref, RTOL, masked=masked) is None
    # every proper candidate listed: the masked ones follow at +0.0
    ids = np.concatenate([kept, sorted(masked)])
    vals = np.concatenate([ref[kept], [0.0, 0.0]])
    assert tolerant_top(ids, vals, ref, RTOL, masked=masked) is None
    # listed with its score, or in front of a proper candidate that was left out
    bad = order[:10]
    assert "masked" in tolerant_top(bad, ref[bad], ref, RTOL, masked=masked)
    ids, vals = np.concatenate([kept[:9], masked[:1]]), np.concatenate([ref[kept[:9]], [0.0]])
    assert "left out" in tolerant_top(ids, vals, ref, RTOL, masked=masked)


def test_what_is_rejected():
    ref, order = _case()
    ids = order[:10].copy()
    good = ref[ids]
    assert tolerant_top(ids, good, ref, RTOL) is None
    # one entry replaced by a candidate worse by 1e-6 than the one it pushes out
    worse = ref.copy()
    worse[order[10]] = ref[order[9]] * (1.0 - 1e-6)
    swapped = ids.copy()
    swapped[9] = order[10]
    assert tolerant_top(ids, worse[ids], worse, RTOL) is None
    assert "left out" in tolerant_top(swapped, worse[swapped], worse, RTOL)
    # a duplicate
    dup = ids.copy()
    dup[5] = dup[4]
    assert "twice" in tolerant_top(dup, ref[dup], ref, RTOL)
    # a value off by 1e-6
    off = good.copy()
    off[2] *= 1.0 + 1e-6
    assert "reference" in tolerant_top(ids, off, ref, RTOL)
    # values that increase, a short list, a row that lists itself
    up = ids.copy()
    up[[1, 2]] = up[[2, 1]]
    assert "increase" in tolerant_top(up, ref[up], ref, RTOL)
    short = np.concatenate([ids[:9], [NONE]])
    assert "candidates exist" in tolerant_top(short, np.concatenate([good[:9], [0.0]]), ref, RTOL)
    assert "no candidate" in tolerant_top(ids, good, ref, RTOL, exclude=[int(ids[0])])
    assert tolerant_top(ids[1:], good[1:], ref, RTOL, exclude=[int(ids[0])]) is None


def test_ranks():
    ref, order = _case()
    for pos in (0, 5, 39):
        q = int(order[pos])
        others = np.delete(ref, q)
        assert tolerant_rank(pos, ref[q], others, RTOL) is None
        # off by one where no tie excuses it
        assert tolerant_rank(pos + 1, ref[q], others, RTOL) is not None
        if pos:
            assert tolerant_rank(pos - 1, ref[q], others, RTOL) is not None
    a = int(np.flatnonzero(order == 23)[0])                 # 23 stands right in front of 7, 5e-10 above it
    assert tolerant_rank(a, ref[23], np.delete(ref, 23), RTOL) is None
    assert tolerant_rank(a + 1, ref[23], np.delete(ref, 23), RTOL) is None       # the near tie may fall either way
    assert tolerant_rank(a + 1, ref[7], np.delete(ref, 7), RTOL) is None
    assert tolerant_rank(a, ref[7], np.delete(ref, 7), RTOL) is None
    assert tolerant_rank(a + 2, ref[23], np.delete(ref, 23), RTOL) is not None
    assert tolerant_rank(a - 1, ref[7], np.delete(ref, 7), RTOL) is not None
