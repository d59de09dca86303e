"""Ranked lists against a reference that agrees only to a relative tolerance.

A top-N list or a rank computed from scores that are each within rtol of the reference's cannot be compared id by id:
two entries whose reference values lie closer than the tolerance may come out in either order, and at the cut of the
list either may be the one that is left out.  Two values each within rtol of the truth can swap only inside a band of
2 rtol, so that is all the helpers forgive.  Scores are the ranking calls' domain: finite and >= +0.0.

    tolerant_top(ids, vals, ref_all, rtol, masked=(), exclude=())  -> None, or what is wrong with the list
    tolerant_rank(rank, s_q, ref_all, rtol)                        -> None, or what is wrong with the rank
"""
import numpy as np

NONE = 0xFFFFFFFF


def _close(v, r, rtol):
    return abs(v - r) <= rtol * abs(r)


def tolerant_top(ids, vals, ref_all, rtol, masked=(), exclude=()):
    """ids, vals: a returned list, best first, padded with (NONE, 0.0) beyond the candidates.  ref_all[i]: the reference
    value of candidate i.  masked: candidates the call must not list with a score (it replaces their score by +0.0: they may
    appear, at 0.0, once every proper candidate is listed); exclude: ids that are no candidates at all (hpf_similar: the row
    itself).  Accepts the list iff the ids are distinct and none is masked with a score, vals[j] is within rtol of
    ref_all[ids[j]], vals does not increase, and no left-out candidate's reference exceeds the smallest returned value by
    more than 2 rtol relative."""
    ids, vals = np.asarray(ids).astype(np.int64), np.asarray(vals, np.float64)
    ref_all = np.asarray(ref_all, np.float64)
    masked, exclude = set(int(x) for x in masked), set(int(x) for x in exclude)
    cand = ref_all.size - len(exclude)
    real = ids != NONE
    n_real = int(real.sum())
    if n_real != min(ids.size, cand):
        return f"{n_real} entries listed, {min(ids.size, cand)} candidates exist"
    if not np.all(real[:n_real]):
        return "padding in front of an entry"
    if np.any(vals[n_real:] != 0.0):
        return "a padding entry carries a value"
    got = ids[:n_real]
    if len(set(got.tolist())) != n_real:
        return "an id is listed twice"
    if np.any(got < 0) or np.any(got >= ref_all.size):
        return "an id out of range"
    for j, i in enumerate(got.tolist()):
        if i in exclude:
            return f"entry {j}: id {i} is no candidate"
        want = 0.0 if i in masked else ref_all[i]
        if i in masked and vals[j] != 0.0:
            return f"entry {j}: masked id {i} listed with the score {vals[j]!r}"
        if not _close(vals[j], want, rtol):
            return f"entry {j}: id {i} has {vals[j]!r}, the reference {want!r}"
    if np.any(np.diff(vals[:n_real]) > 0):
        return "the values increase"
    if n_real:
        least = vals[n_real - 1]
        out = np.ones(ref_all.size, bool)
        out[got] = False
        for i in exclude:
            out[i] = False
        for i in masked:
            out[i] = False                      # a left-out masked candidate stands at +0.0: never above a listed one
        worst = ref_all[out].max() if out.any() else -np.inf
        if worst > least + 2.0 * rtol * abs(worst):
            return f"left out: a candidate with the reference {worst!r}, the smallest listed value is {least!r}"
    return None


def tolerant_rank(rank, s_q, ref_all, rtol):
    """rank: how many OTHER candidates come before the queried one; s_q: its (returned) score; ref_all: the reference
    scores of the others (masked ones already 0.0).  Accepts a rank between the count of references above s_q (1 + 2 rtol)
    and the count at or above s_q (1 - 2 rtol)."""
    ref_all = np.asarray(ref_all, np.float64)
    lo = int(np.sum(ref_all > s_q * (1.0 + 2.0 * rtol)))
    hi = int(np.sum(ref_all >= s_q * (1.0 - 2.0 * rtol)))
    if not lo <= int(rank) <= hi:
        return f"rank {int(rank)} outside [{lo}, {hi}] for the score {s_q!r}"
    return None
