"""The CPU reference of the two fold-in calls, on the oracle: no GPU import, so that tests/statemodel.py can run it in a
sequence and tests/test_gpu_fold_in.py / tests/test_gpu_fold_in_items.py share it.

oracle_fold: oracle.orc.Model on the same CSR, the user side at the prior, the item side as given; per iteration
iterate(1), then every item-side array is put back.  The oracle's user half reads only the OLD item side, so that is one
fold-in iteration (test_gpu_fold_in.py::test_oracle_loop_is_the_fold_in_equations checks the claim against a numpy
restatement of the equations of include/hpf.h).  novb is never passed on: include/hpf.h, "novb changes nothing here".

oracle_items: item fold-in of (R, user side U) IS user fold-in of (R^T, item side := U) with the names exchanged, so it is
oracle_fold on the item-major lists (users ascending inside an item, as the upload builds them) with THETA <-> BETA,
XI <-> ETA, UBIAS <-> IBIAS swapped."""
import numpy as np

from oracle import orc
from tests.util import compare_states

S0 = R0 = 0.3
SWAP = {"THETA": "BETA", "BETA": "THETA", "XI": "ETA", "ETA": "XI", "UBIAS": "IBIAS", "IBIAS": "UBIAS"}


def psi(x):
    x = np.asarray(x, np.float64)
    return orc.psi(x.ravel()).reshape(x.shape)


def user_states(hier, bias):
    return [w for w in compare_states(hier, bias) if w.split("_")[0] in ("THETA", "XI", "UBIAS")]


def item_states(hier, bias):
    return [w for w in compare_states(hier, bias) if w.split("_")[0] in ("BETA", "ETA", "IBIAS")]


def swap(w):
    o, _, rest = w.partition("_")
    return SWAP[o] + "_" + rest


def oracle_fold(n, m, K, hier, bias, rowptr, col, val, item, T, trace=False, kept=None):
    """T fold-in iterations on the oracle -> the user-side states (trace: THETA_E after every iteration as well; kept: a list
    that receives what theta kept of its rate prior for the ELBO, oracle.orc.Model.prior_kept -- state beside the arrays)"""
    M = orc.Model(n, m, K, hier, bias, val is None)
    M.set_csr(rowptr, col, val)
    M.initialize(0)                                            # (the accumulators at their priors)
    e0, l0 = S0 / R0, float(psi(S0)) - np.log(R0)
    objs = [("THETA", (n, K), (n, K) if hier else (K,))] + ([("XI", (n,), (n,))] if hier else []) + ([("UBIAS", (n,), (n,))] if bias else [])
    for o, shp, rshp in objs:
        M.set_state(o + "_SHAPE", np.full(shp, S0)); M.set_state(o + "_RATE", np.full(rshp, R0))
        M.set_state(o + "_E", np.full(shp, e0)); M.set_state(o + "_ELOG", np.full(shp, l0))
    put_back = [w for w in item_states(hier, bias)]
    for w in put_back:
        M.set_state(w, item[w])
    steps = []
    for _ in range(T):
        M.iterate(1)
        for w in put_back:
            M.set_state(w, item[w])
        if trace:
            steps.append(M.state("THETA_E"))
    out = {w: M.state(w) for w in user_states(hier, bias)}
    if kept is not None:
        kept.append(M.prior_kept(0))
    return (out, steps) if trace else out


def oracle_items(n, m, K, hier, bias, imajor, users, T, trace=False, kept=None):
    """T item fold-in iterations on the oracle -> the item-side states (trace: BETA_E after every iteration as well)"""
    colptr, usr, val = imajor
    as_items = {swap(w): a for w, a in users.items()}
    r = oracle_fold(m, n, K, hier, bias, colptr, usr, val, as_items, T, trace=trace, kept=kept)
    out = {swap(w): a for w, a in (r[0] if trace else r).items()}
    return (out, r[1]) if trace else out


def item_major(n, m, rowptr, col, val):
    """the item-major view the upload builds from a CSR over n users: (colptr, users, val), users ascending inside an item"""
    usr = np.repeat(np.arange(n, dtype=np.uint32), np.diff(rowptr))
    o = np.argsort(col, kind="stable")
    colptr = np.zeros(m + 1, np.int64)
    colptr[1:] = np.cumsum(np.bincount(col, minlength=m))
    return colptr, usr[o], None if val is None else np.asarray(val)[o]
