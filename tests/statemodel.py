"""Random call orders against a handle that keeps its model lazily: the invariant is that LAZINESS IS NOT OBSERVABLE.

libhpf_hip.so defers work: after a sweep S holds raw sums until somebody asks for a shape, Elog is rebuilt on export,
W is derived from a handed-in Elog at the next iteration, a fall-back from the packed rows is repaired at the next
synchronisation point.  Which of these are pending depends on what was called before, so every consumer has to ask the
right questions before it reads a buffer -- and a mistake shows only under a call order nobody wrote down.

This module draws such call orders and runs them on three executors:

  oracle      oracle.orc.Model, whose four arrays per Gamma object are independent: that is the semantics
  lazy        one Hpf that does exactly the operations and nothing else
  eager twin  a second Hpf that does the same operations and, after every one, exports every array of
              compare_states and synchronises: nothing is ever pending on it

lazy and twin must agree bit for bit on everything an operation returns, and both with the oracle at the bars the
suite already uses.  (tests/test_state_sequences_host.py checks the generator and the oracle run without a GPU,
tests/test_gpu_state_sequences.py runs the three together.)

An operation is a small tuple that prints readably:

  ("iterate", k)                 hpf_iterate(k), k = 1..3
  ("pieces",)                    iterate_local_items, iterate_local_users, iterate_global with nothing in between
  ("get", w) / ("get_dev", w)    ONE array of compare_states(hier, bias): observation changes the lazy state
  ("set", w, how, sub)           how = "host" | "device"; the value is the ORACLE'S current array times U(0.8, 1.25)
                                 (E, SHAPE, RATE) or plus U(-0.5, 0.5) (ELOG), drawn from default_rng(sub); w among
                                 the _E and _ELOG arrays of every object and the _SHAPE arrays of THETA, BETA, UBIAS,
                                 IBIAS; THETA_RATE / BETA_RATE only before the first iteration (include/hpf.h: a rate
                                 is kept for export before iteration 0 only)
  ("heldout",) ("elbo",) ("predict",) ("synchronize",)
  ("snapshot_swap",)             snapshot(), a fresh handle with the same CSR, restore(), the old one closed
  ("refused", form)              calls the library must refuse (or, the bias rate, ignore) without a trace:
                                 "count" a set_state and a get_state with a wrong count, "absent" a state that is not
                                 part of the model, "bias_rate" hpf_set_state(UBIAS_RATE)
  ("fall_back",)                 never drawn: woven in by with_fall_back() -- BETA_E[:, 0] = 1e40 and iterate(2) in one
                                 call, so that the first user sweep cannot pack its rows and an iteration is skipped

sequence(seed) draws these and nothing else: it is what its committed seeds were chosen for, and a digest in
tests/test_state_sequences_host.py pins what it returns.  serving_sequence(seed) draws them and the serving calls, on a
small fixed query set of the Problem (four users, eight queried items, six pairs, four items; topn = 10, T = 4):

  ("fold_in", T) / ("fold_in_items", T)   T = 1..3 iterations, tol = 0, on the handle's own CSR, before or after the first
                                 iteration: a whole side is written and left "as hpf_set_state would"; the rates of that
                                 side (the bias rate among them) can then be exported before the first iteration.  The
                                 oracle runs tests/fold_ref.py on its current frozen side
  ("scores",) ("rank_topn",) ("item_ranks",)                                   need SCORES
  ("loo_ranks",) ("rank_queries",) ("recommend",) ("audience",) ("explain",)   need SCORING
  ("similar", side) ("factor_top", side)                                       need FACTORS (users by cosine, items by dot)
  ("because",)                                                                 need BECAUSE, once the sequence has iterated
  ("score_moments",) ("recommend_ucb", z)   z of {0, 1.5}                       need MOMENTS, once the sequence has iterated

Everything a read-only call returns is the same bits on lazy and twin, and within RTOL of plain numpy on the ORACLE'S
arrays (oracle_read_error; lists and ranks through tests/toplist.py).  What because and the moments need before the first
sweep is the directed snapshot test's.  A config of serving_sequence() also draws fold_long_min (HPF_FOLD_LONG_MIN unset
or 32: at these shapes no item has the 256 ratings at which fold_in_long_kernel takes a row by itself).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from tests.util import compare_states, copy_state, heldout_pairs, make_problem, rel_err

RTOL = 1e-9                     # tests/test_gpu_parity.py: states against the oracle

# (n, m, K, nnz): K = 5 plain rows, K = 21 (+ bias) a padded stride, K = 100 packed (p59) rows and a fused user sweep
SHAPES = ((60, 40, 5, 1000), (150, 120, 21, 3000), (200, 150, 100, 4000))

# the kinds of operation the coverage conditions are stated over
KINDS = ("iterate", "pieces", "get_sel", "get_rate", "get_prior", "set_e", "set_elog", "set_shape",
         "heldout", "elbo", "predict", "snapshot_swap", "refused")
REFUSED_FORMS = ("count", "absent", "bias_rate")


def kind_of(op):
    """the coverage kind of an operation (None for synchronize, a rate set and the injected fall-back)"""
    name = op[0]
    if name in ("get", "get_dev"):
        w = op[1]
        if w.startswith(("XI_", "ETA_")):
            return "get_prior"
        return "get_rate" if w.endswith("_RATE") else "get_sel"
    if name == "set":
        suffix = op[1].rsplit("_", 1)[1]
        return {"E": "set_e", "ELOG": "set_elog", "SHAPE": "set_shape"}.get(suffix)
    return name if name in KINDS else None


def _objects(hier, bias, prior=True):
    o = ["THETA", "BETA"]
    if hier and prior:
        o += ["XI", "ETA"]
    if bias:
        o += ["UBIAS", "IBIAS"]
    return o


def sequence(seed):
    """-> (config, ops), from the seed alone"""
    rng = np.random.default_rng([int(seed), 20251])
    shape = int(rng.integers(len(SHAPES)))
    n, m, K, nnz = SHAPES[shape]
    hier = bool(rng.integers(2))
    bias = True if shape == 1 else bool(rng.integers(2))
    novb = bool(rng.integers(2)) if (bias and not hier) else False
    config = dict(n=n, m=m, K=K, nnz=nnz, hier=hier, bias=bias, novb=novb,
                  w_storage=int(rng.choice([0, 3])),
                  graph=[None, "0", "1"][int(rng.integers(3))],
                  fused_sweep=[None, "0"][int(rng.integers(2))],
                  data_seed=int(rng.integers(1, 1000)))
    ops = []
    iterated = False
    rate_set = set()
    length = int(rng.integers(25, 36))
    while len(ops) < length:
        if not iterated and len(ops) >= 3:          # the start state is the less interesting half
            kind = "iterate"
        else:
            r = rng.random()
            kind = "synchronize" if r < 0.03 else "set_rate" if r < 0.06 else KINDS[int(rng.integers(len(KINDS)))]
        how = "device" if rng.random() < 0.3 else "host"
        sub = int(rng.integers(1 << 30))
        if kind == "iterate":
            op = ("iterate", int(rng.integers(1, 4)))
        elif kind in ("pieces", "heldout", "predict", "synchronize", "snapshot_swap"):
            op = (kind,)
        elif kind == "elbo":
            if not iterated:                        # hpf_elbo: defined after the first iteration
                continue
            op = ("elbo",)
        elif kind == "refused":
            op = ("refused", REFUSED_FORMS[int(rng.integers(len(REFUSED_FORMS)))])
        elif kind == "get_sel":
            objs = _objects(hier, bias, prior=False)
            w = objs[int(rng.integers(len(objs)))] + ["_SHAPE", "_E", "_ELOG"][int(rng.integers(3))]
            op = ("get_dev" if how == "device" else "get", w)
        elif kind == "get_rate":
            objs = _objects(hier, bias, prior=False)
            w = objs[int(rng.integers(len(objs)))] + "_RATE"
            if not iterated and w not in rate_set:  # nothing to export yet
                continue
            op = ("get_dev" if how == "device" else "get", w)
        elif kind == "get_prior":
            if not hier:
                continue
            w = ["XI", "ETA"][int(rng.integers(2))] + ["_SHAPE", "_RATE", "_E", "_ELOG"][int(rng.integers(4))]
            op = ("get_dev" if how == "device" else "get", w)
        elif kind in ("set_e", "set_elog"):
            objs = _objects(hier, bias)
            op = ("set", objs[int(rng.integers(len(objs)))] + ("_E" if kind == "set_e" else "_ELOG"), how, sub)
        elif kind == "set_shape":
            objs = _objects(hier, bias, prior=False)
            op = ("set", objs[int(rng.integers(len(objs)))] + "_SHAPE", how, sub)
        else:                                       # set_rate
            if iterated:
                continue
            w = ["THETA_RATE", "BETA_RATE"][int(rng.integers(2))]
            rate_set.add(w)
            op = ("set", w, how, sub)
        if op[0] in ("iterate", "pieces"):
            iterated = True
        ops.append(op)
    return config, ops


# ---- the serving calls ---------------------------------------------------------------------------------------------------
# what serving_sequence() draws beside KINDS: the two fold-ins, which write a whole side, and the read-only calls grouped by
# the need they ask of hpf_lazy::State::ask
SERVING_READS = {
    "scores": (("scores",), ("rank_topn",), ("item_ranks",)),                                        # SCORES
    "scoring": (("loo_ranks",), ("rank_queries",), ("recommend",), ("audience",), ("explain",)),     # SCORING
    "factors": (("similar", 0), ("similar", 1), ("factor_top", 0), ("factor_top", 1)),               # FACTORS
    "because": (("because",),),                                                                      # BECAUSE
    "moments": (("score_moments",), ("recommend_ucb",)),                                             # MOMENTS (recommend_ucb: + z)
}
FOLDS = ("fold_in", "fold_in_items")
NEW_KINDS = FOLDS + tuple(SERVING_READS)
SERVING_KINDS = KINDS + NEW_KINDS
READ_CALLS = tuple(call for calls in SERVING_READS.values() for call in calls)
_KIND_OF_READ = {call[0]: kind for kind, calls in SERVING_READS.items() for call in calls}
# after these a consumer finds something pending (or a whole side replaced): every read-only call is somewhere the first
# operation after each of them
CONTEXTS = ("iteration", "set_e", "set_elog", "set_shape", "fold_in", "fold_in_items", "snapshot_swap")
TOPN, TERMS, UCB_Z = 10, 4, (0.0, 1.5)


def serving_kind_of(op):
    """kind_of over SERVING_KINDS"""
    return _KIND_OF_READ.get(op[0]) or (op[0] if op[0] in FOLDS else kind_of(op))


def read_call_of(op):
    """the entry of READ_CALLS an operation is (None for every other operation)"""
    if op[0] not in _KIND_OF_READ:
        return None
    return op[:2] if op[0] in ("similar", "factor_top") else op[:1]


def context_of(op):
    k = serving_kind_of(op)
    return "iteration" if k in ("iterate", "pieces") else k if k in CONTEXTS else None


def _weight(prev, kind):
    """How often `kind` is drawn after `prev`, in proportion to what the coverage conditions of
    tests/test_state_sequences_host.py ask of that transition: two occurrences of every kind after every other, and one per
    call of the kind where a read-only call follows a context."""
    if prev is None:
        return 1.0
    if kind in SERVING_READS and (prev in CONTEXTS or prev in ("iterate", "pieces")):
        return 1.0 + len(SERVING_READS[kind])
    return 2.0


def serving_sequence(seed):
    """-> (config, ops), from the seed alone: sequence()'s operations and the serving calls.  The kind of the next operation
    is drawn with _weight(), and a transition that has occurred in this sequence is put back once: thirty operations are
    thirty different questions."""
    rng = np.random.default_rng([int(seed), 20252])
    shape = int(rng.integers(len(SHAPES)))
    n, m, K, nnz = SHAPES[shape]
    hier = bool(rng.integers(2))
    bias = True if shape == 1 else bool(rng.integers(2))
    novb = bool(rng.integers(2)) if (bias and not hier) else False
    config = dict(n=n, m=m, K=K, nnz=nnz, hier=hier, bias=bias, novb=novb,
                  w_storage=int(rng.choice([0, 3])),
                  graph=[None, "0", "1"][int(rng.integers(3))],
                  fused_sweep=[None, "0"][int(rng.integers(2))],
                  fold_long_min=[None, "32"][int(rng.integers(2))],
                  data_seed=int(rng.integers(1, 1000)))
    ops, seen = [], set()
    iterated = False
    rate_set = set()                # the rates that can be exported before the first iteration: handed in, or a fold-in's
    prev = None
    length = int(rng.integers(25, 36))
    while len(ops) < length:
        if not iterated and len(ops) >= 4:          # the start state is the less interesting half
            kind = "iterate"
        else:
            r = rng.random()
            if r < 0.02:
                kind = "synchronize"
            elif r < 0.04:
                kind = "set_rate"
            else:
                w = np.array([_weight(prev, k) for k in SERVING_KINDS])
                kind = SERVING_KINDS[int(rng.choice(len(SERVING_KINDS), p=w / w.sum()))]
                if (prev, kind) in seen and rng.random() < 0.9:
                    continue
        how = "device" if rng.random() < 0.3 else "host"
        sub = int(rng.integers(1 << 30))
        if kind == "iterate":
            op = ("iterate", int(rng.integers(1, 4)))
        elif kind in ("pieces", "heldout", "predict", "synchronize", "snapshot_swap"):
            op = (kind,)
        elif kind == "elbo":
            if not iterated:                        # hpf_elbo: defined after the first iteration
                continue
            op = ("elbo",)
        elif kind == "refused":
            op = ("refused", REFUSED_FORMS[int(rng.integers(len(REFUSED_FORMS)))])
        elif kind == "get_sel":
            objs = _objects(hier, bias, prior=False)
            w = objs[int(rng.integers(len(objs)))] + ["_SHAPE", "_E", "_ELOG"][int(rng.integers(3))]
            op = ("get_dev" if how == "device" else "get", w)
        elif kind == "get_rate":
            objs = _objects(hier, bias, prior=False)
            w = objs[int(rng.integers(len(objs)))] + "_RATE"
            if not iterated and w not in rate_set:  # nothing to export yet
                continue
            op = ("get_dev" if how == "device" else "get", w)
        elif kind == "get_prior":
            if not hier:
                continue
            w = ["XI", "ETA"][int(rng.integers(2))] + ["_SHAPE", "_RATE", "_E", "_ELOG"][int(rng.integers(4))]
            op = ("get_dev" if how == "device" else "get", w)
        elif kind in ("set_e", "set_elog"):
            objs = _objects(hier, bias)
            op = ("set", objs[int(rng.integers(len(objs)))] + ("_E" if kind == "set_e" else "_ELOG"), how, sub)
        elif kind == "set_shape":
            objs = _objects(hier, bias, prior=False)
            op = ("set", objs[int(rng.integers(len(objs)))] + "_SHAPE", how, sub)
        elif kind == "set_rate":
            if iterated:
                continue
            w = ["THETA_RATE", "BETA_RATE"][int(rng.integers(2))]
            rate_set.add(w)
            op = ("set", w, how, sub)
        elif kind in FOLDS:                          # tol = 0: every row runs T iterations
            op = (kind, int(rng.integers(1, 4)))
            rate_set |= {"THETA_RATE", "UBIAS_RATE"} if kind == "fold_in" else {"BETA_RATE", "IBIAS_RATE"}
        else:                                       # a read-only call
            if kind in ("because", "moments") and not iterated:     # before the first sweep: the directed snapshot test
                continue
            calls = SERVING_READS[kind]
            op = calls[int(rng.integers(len(calls)))]
            if op[0] == "recommend_ucb":
                op = op + (UCB_Z[int(rng.integers(len(UCB_Z)))],)
        if op[0] in ("iterate", "pieces"):
            iterated = True
        seen.add((prev, serving_kind_of(op)))
        prev = serving_kind_of(op)
        ops.append(op)
    return config, ops


def with_fall_back(seed, ops):
    """ops with ("fall_back",) woven in at a seeded position, leaving at least three operations behind it"""
    rng = np.random.default_rng([int(seed), 77])
    at = int(rng.integers(2, len(ops) - 3))
    return ops[:at] + [("fall_back",)] + ops[at:]


def first_exports(ops):
    """the arrays that are, somewhere in ops, the first export after an iteration"""
    out, armed = set(), False
    for op in ops:
        if op[0] in ("iterate", "pieces"):
            armed = True
        elif op[0] in ("get", "get_dev") and armed:
            out.add(op[1])
            armed = False
    return out


def set_env(monkeypatch, config):
    """the knobs of a config, under HPF_EXPERIMENTAL=1; the library reads them when a handle is created"""
    monkeypatch.setenv("HPF_EXPERIMENTAL", "1")
    for key, name in (("graph", "HPF_GRAPH"), ("fused_sweep", "HPF_FUSED_SWEEP"), ("fold_long_min", "HPF_FOLD_LONG_MIN")):
        if config.get(key) is None:                 # (a config of sequence() has no fold_long_min)
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, config[key])


class Problem:
    """the ratings of a config, its 200 held-out pairs, its 50 pairs to predict and the fixed queries of the serving calls:
    four users (the first and the last among them), two queried items for each, six pairs, four items"""

    def __init__(self, config):
        n, m = config["n"], config["m"]
        self.n, self.m = n, m
        self.csr = make_problem(n, m, config["nnz"], config["data_seed"])
        self.held = heldout_pairs(n, m, 200, seed=config["data_seed"] + 1)
        pu, pi, _ = heldout_pairs(n, m, 50, seed=config["data_seed"] + 2)
        self.pairs = (pu, pi)
        self.users = np.array([0, 7, n // 2, n - 1], dtype=np.uint32)
        self.q_ptr = np.arange(0, 9, 2, dtype=np.uint64)
        self.q_items = ((np.arange(8, dtype=np.uint32) * 37 + 5) % m).astype(np.uint32)
        self.q_sel = np.repeat(np.arange(4, dtype=np.uint32), 2)
        rng = np.random.default_rng(config["data_seed"] + 3)
        self.six = (rng.integers(0, n, 6).astype(np.uint32), rng.integers(0, m, 6).astype(np.uint32))
        self.six[0][0], self.six[1][0], self.six[0][1], self.six[1][1] = 0, 0, n - 1, m - 1
        self.items = np.array([0, 3, m // 2, m - 1], dtype=np.uint32)
        # a top-N list of a query user holds proper scores only (hpf_audience's may run into the masked users)
        assert all(m - np.unique(self.rated_by(u)).size >= TOPN for u in self.users), config

    def history(self, u):
        """the items of user u in CSR order and the factor yy of the phi pass"""
        rowptr, col, val = self.csr
        a, b = int(rowptr[u]), int(rowptr[u + 1])
        return col[a:b], np.where(val[a:b] > 1, val[a:b], 1).astype(np.float64)

    def rated_by(self, u):
        """the items user u has a stored rating > 0 for: what the ranking calls mask"""
        rowptr, col, val = self.csr
        a, b = int(rowptr[u]), int(rowptr[u + 1])
        return col[a:b][val[a:b] > 0]

    def raters_of(self, i):
        """the users with a stored rating > 0 for item i: what hpf_audience masks"""
        rowptr, col, val = self.csr
        usr = np.repeat(np.arange(self.n), np.diff(rowptr))
        return usr[(col == i) & (val > 0)]


def perturbed(current, w, sub):
    rng = np.random.default_rng(sub)
    cur = np.asarray(current, np.float64)
    if w.endswith("_ELOG"):
        return cur + rng.uniform(-0.5, 0.5, size=cur.shape)
    return cur * rng.uniform(0.8, 1.25, size=cur.shape)


def oracle_predict(M, bias, pu, pi):
    s = np.einsum("ij,ij->i", M.state("THETA_E")[pu], M.state("BETA_E")[pi])
    if bias:
        s = s + M.state("UBIAS_E")[pu] + M.state("IBIAS_E")[pi]
    return s


def oracle_fold_into(M, n, m, K, hier, bias, csr, items, T):
    """hpf_fold_in (items: hpf_fold_in_items) on the model's own CSR, in the oracle: tests/fold_ref.py against the
    oracle's current frozen side, every array of the folded side put in place as hpf_set_state would (the inner model is
    built without novb: include/hpf.h, "novb changes nothing here").  With hier the E and Elog of xi / eta that the last
    rate of the fold-in was built from go along: the reference keeps them beside the arrays for the ELBO
    (GPMatrix::set_prior_rate), the library in the same buffers a sweep leaves them in."""
    from tests import fold_ref
    rowptr, col, val = csr
    kept = []
    if items:
        frozen = {w: M.state(w) for w in fold_ref.user_states(hier, bias)}
        new = fold_ref.oracle_items(n, m, K, hier, bias, fold_ref.item_major(n, m, rowptr, col, val), frozen, T, kept=kept)
    else:
        frozen = {w: M.state(w) for w in fold_ref.item_states(hier, bias)}
        new = fold_ref.oracle_fold(n, m, K, hier, bias, rowptr, col, val, frozen, T, kept=kept)
    for w, v in new.items():
        M.set_state(w, v)
    if hier:
        M.set_prior_kept(1 if items else 0, kept[0])


class OracleRun:
    def __init__(self, orc, config, prob):
        c = config
        self.c, self.prob = c, prob
        self.M = orc.Model(c["n"], c["m"], c["K"], c["hier"], c["bias"], False, novb=c["novb"])
        self.M.set_csr(*prob.csr)
        self.M.initialize(c["data_seed"])

    def step(self, op):
        """-> what the operation returns in the oracle (for a set: the value to hand to the device models)"""
        M, name = self.M, op[0]
        if name == "iterate":
            M.iterate(op[1])
        elif name == "pieces":
            M.iterate(1)
        elif name in ("get", "get_dev"):
            return M.state(op[1])
        elif name == "set":
            v = perturbed(M.state(op[1]), op[1], op[3])
            M.set_state(op[1], v)
            return v
        elif name == "heldout":
            return M.heldout_sum(*self.prob.held)
        elif name == "elbo":
            return M.elbo()
        elif name == "predict":
            return oracle_predict(M, self.c["bias"], *self.prob.pairs)
        elif name == "fall_back":
            be = M.state("BETA_E").copy()
            be[:, 0] = 1e40
            M.set_state("BETA_E", be)
            M.iterate(2)
            return be
        elif name in FOLDS:
            self.fold(name == "fold_in_items", op[1])
        return None

    def fold(self, items, T):
        c = self.c
        oracle_fold_into(self.M, c["n"], c["m"], c["K"], c["hier"], c["bias"], self.prob.csr, items, T)

    def row_spread(self):
        """the widest Elog spread inside a row of either side (the columns one softmax sees)"""
        worst = 0.0
        for obj, b in (("THETA", "UBIAS"), ("BETA", "IBIAS")):
            L = self.M.state(obj + "_ELOG")
            if self.c["bias"]:
                L = np.concatenate([L, self.M.state(b + "_ELOG")[:, None]], axis=1)
            worst = max(worst, float(np.max(L.max(axis=1) - L.min(axis=1))))
        return worst

    def check_valid(self, where):
        for w in compare_states(self.c["hier"], self.c["bias"]):
            v = self.M.state(w)
            assert np.all(np.isfinite(v)), (where, w)
            if w.endswith(("_E", "_SHAPE")):
                assert np.all(v > 0), (where, w)
        assert self.row_spread() <= 40.0, (where, self.row_spread())


class DeviceRun:
    """one Hpf driven by operations; eager: export everything and synchronise after every one"""

    def __init__(self, config, prob, oracle_model, eager, w_storage=None):
        self.c, self.prob, self.eager = config, prob, eager
        self.ws = config["w_storage"] if w_storage is None else w_storage
        self.iterated = False
        self.D = self._fresh()
        copy_state(oracle_model, self.D, config["hier"], config["bias"])
        self._flush()

    def _fresh(self):
        from hgaprec_amd.capi import Hpf
        c = self.c
        D = Hpf(c["n"], c["m"], c["K"], hier=c["hier"], bias=c["bias"], novb=c["novb"], w_storage=self.ws)
        D.upload_csr(*self.prob.csr)
        D.heldout_bind(0, *self.prob.held)
        return D

    def close(self):
        self.D.close()

    def _flush(self):
        if not self.eager:
            return
        from hgaprec_amd.capi import HpfError
        for w in compare_states(self.c["hier"], self.c["bias"]):
            try:
                self.D.get_state(w)
            except HpfError:
                if self.iterated or not w.endswith("_RATE"):     # before iteration 0 a rate exists only if it was set
                    raise
        self.D.synchronize()

    def export_all(self):
        return {w: self.D.get_state(w) for w in compare_states(self.c["hier"], self.c["bias"])}

    def refused(self, form):
        """-> the statuses; everything here must leave the handle as it was"""
        D, c = self.D, self.c
        lib, h = D.lib, D._h
        from hgaprec_amd.capi import STATE
        dp = C.POINTER(C.c_double)
        big = np.full(max(c["n"], c["m"]) * c["K"] + 8, 0.5)
        out = np.full(big.size, -7.0)
        pb, po = big.ctypes.data_as(dp), out.ctypes.data_as(dp)
        if form == "count":
            good = c["n"] * c["K"]
            got = (lib.hpf_set_state(h, STATE["THETA_E"], pb, good + 1), lib.hpf_get_state(h, STATE["THETA_E"], po, good - 1),
                   lib.hpf_set_state(h, STATE["BETA_RATE"], pb, 1 if c["K"] > 1 else 2),
                   lib.hpf_get_state(h, STATE["BETA_RATE"], po, 1 if c["K"] > 1 else 2))
            want = (-1, -1, -1, -1)
        elif form == "absent":
            w = "XI_E" if not c["hier"] else "UBIAS_E" if not c["bias"] else None
            if w is None:                           # every object is part of this model: an id beyond the last one
                got = (lib.hpf_set_state(h, len(STATE), pb, c["n"]), lib.hpf_get_state(h, len(STATE), po, c["n"]))
            else:
                got = (lib.hpf_set_state(h, STATE[w], pb, c["n"]), lib.hpf_get_state(h, STATE[w], po, c["n"]))
            want = (-1, -1)
        else:                                       # the bias rate is the constant r_prior + m: a no-op with bias, no state without
            got = (lib.hpf_set_state(h, STATE["UBIAS_RATE"], pb, c["n"]),)
            want = (0,) if c["bias"] else (-1,)
        assert got == want, (form, got, want)
        assert np.all(out == -7.0), form            # a refused export wrote nothing
        return got

    def step(self, op, value=None):
        D, name, res = self.D, op[0], None
        if name == "iterate":
            D.iterate(op[1])
            self.iterated = True
        elif name == "pieces":
            D.iterate_local_items()
            D.iterate_local_users()
            D.iterate_global()
            self.iterated = True
        elif name == "get":
            res = D.get_state(op[1])
        elif name == "get_dev":
            res = D.get_state_device(op[1]).cpu().numpy()
        elif name == "set":
            if op[2] == "device":
                import torch
                D.set_state_device(op[1], torch.from_numpy(np.ascontiguousarray(value)).to(f"cuda:{D.device}"))
            else:
                D.set_state(op[1], value)
        elif name == "heldout":
            res = D.heldout_ll(*self.prob.held)
            assert D.heldout_ll_bound(0) == res
        elif name == "elbo":
            res = D.elbo()
        elif name == "predict":
            res = D.predict(*self.prob.pairs)
        elif name == "synchronize":
            D.synchronize()
        elif name == "snapshot_swap":
            blob = D.snapshot()
            new = self._fresh()
            new.restore(blob)
            D.close()
            self.D = new
        elif name == "refused":
            res = self.refused(op[1])
        elif name == "fall_back":
            D.set_state("BETA_E", value)
            D.iterate(2)
            self.iterated = True
        elif name == "fold_in":
            res = (D.fold_in(op[1], 0.0),)
        elif name == "fold_in_items":
            res = (D.fold_in_items(op[1], 0.0),)
        elif read_call_of(op) is not None:
            res = device_read(D, self.prob, op)
        else:
            raise ValueError(op)
        self._flush()
        return res


def device_read(D, prob, op):
    """a read-only serving call on the fixed queries of the problem -> the tuple of arrays it returns"""
    name, p = op[0], prob
    if name == "scores":
        return (D.scores(p.users),)
    if name == "rank_topn":
        return D.rank_topn(p.users, topn=TOPN)
    if name == "item_ranks":
        return D.item_ranks(p.users, p.q_sel, p.q_items)
    if name == "loo_ranks":
        return D.loo_ranks(p.users, p.q_items[::2])
    if name == "rank_queries":
        return D.rank_queries(p.users, p.q_ptr, p.q_items)
    if name == "recommend":
        return D.recommend(p.users, topn=TOPN)
    if name == "audience":
        return D.audience(p.items, topn=TOPN)
    if name == "explain":
        return D.explain(*p.six, TERMS)
    if name == "similar":                           # the users by cosine, the items by dot product
        return D.similar(op[1], p.items if op[1] else p.users, TOPN, metric="dot" if op[1] else "cosine")
    if name == "factor_top":
        return D.factor_top(op[1], TOPN)
    if name == "because":
        return D.because(p.users, p.q_ptr, p.q_items, TERMS)
    if name == "score_moments":
        return D.score_moments(*p.six)
    if name == "recommend_ucb":
        return D.recommend_ucb(p.users, topn=TOPN, z=op[1])
    raise ValueError(op)


def _rel(got, want):
    """element-wise relative error; a reference of exactly 0.0 (a masked score) asks for exactly 0.0"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if not got.size:
        return 0.0
    zero = want == 0.0
    if np.any(got[zero] != 0.0):
        return np.inf
    return float(np.max(np.abs(got - want)[~zero] / np.abs(want[~zero]))) if np.any(~zero) else 0.0


def oracle_read_error(M, config, prob, op, res):
    """A serving call's result against plain numpy on the ORACLE'S arrays -> the worst relative error of the values it
    returns.  Lists and ranks go through tests/toplist.py at RTOL: what is wrong with one raises AssertionError."""
    from tests import because_ref, moments_ref
    from tests.toplist import NONE, tolerant_rank, tolerant_top
    name, p, bias, K = op[0], prob, config["bias"], config["K"]
    Et, Eb = M.state("THETA_E"), M.state("BETA_E")
    ub, ib = (M.state("UBIAS_E"), M.state("IBIAS_E")) if bias else (np.zeros(p.n), np.zeros(p.m))

    def row(u):                                     # the scores of user u for every item
        return Et[u] @ Eb.T + (ub[u] + ib)

    def listed(ids, vals, ref, masked=(), exclude=()):
        bad = tolerant_top(ids, vals, ref, RTOL, masked=masked, exclude=exclude)
        assert bad is None, f"{op}: {bad}"
        real = np.asarray(ids) != NONE
        want = np.where(np.isin(ids[real], np.asarray(list(masked), np.int64)), 0.0, np.asarray(ref)[ids[real].astype(np.int64)])
        return _rel(np.asarray(vals)[real], want)

    def ranked(rank, sc, u, q):
        ref = row(u)
        ref[p.rated_by(u)] = 0.0
        bad = tolerant_rank(rank, sc, np.delete(ref, q), RTOL)
        assert bad is None, f"{op}: user {u} item {q}: {bad}"
        return _rel(sc, ref[q])

    if name == "scores":
        return _rel(res[0], np.stack([row(u) for u in p.users]))
    if name in ("rank_topn", "recommend"):
        return max(listed(res[0][b], res[1][b], row(u), masked=p.rated_by(u)) for b, u in enumerate(p.users))
    if name in ("item_ranks", "rank_queries"):
        return max(ranked(res[0][q], res[1][q], p.users[p.q_sel[q]], p.q_items[q]) for q in range(p.q_items.size))
    if name == "loo_ranks":
        err = max(ranked(res[0][b], res[1][b], u, p.q_items[2 * b]) for b, u in enumerate(p.users))
        assert np.array_equal(res[2], [np.unique(p.rated_by(u)).size for u in p.users]), f"{op}: masked counts {res[2]}"
        return err
    if name == "audience":
        return max(listed(res[0][b], res[1][b], Et @ Eb[i] + (ub + ib[i]), masked=p.raters_of(i)) for b, i in enumerate(p.items))
    if name == "explain":
        err = 0.0
        for q, (u, i) in enumerate(zip(*p.six)):
            terms = np.concatenate([Et[u] * Eb[i], [ub[u], ib[i]]]) if bias else Et[u] * Eb[i]
            err = max(err, listed(res[0][q], res[1][q], terms))
        return err
    if name == "similar":
        E, ids = (Eb, p.items) if op[1] else (Et, p.users)
        if not op[1]:
            E = E / np.sqrt((E * E).sum(1))[:, None]
        return max(listed(res[0][b], res[1][b], E @ E[r], exclude=[r]) for b, r in enumerate(ids))
    if name == "factor_top":
        E = Eb if op[1] else Et
        return max(listed(res[0][k], res[1][k], E[:, k]) for k in range(K))
    if name == "because":
        st = because_ref.State(Et, M.state("THETA_ELOG"), Eb, M.state("BETA_ELOG"),
                               *((ub, M.state("UBIAS_ELOG"), ib, M.state("IBIAS_ELOG")) if bias else ()))
        items, contrib, sums, priors = res
        err, q = 0.0, 0
        for b, u in enumerate(p.users):
            hist, yy = p.history(u)
            targets = p.q_items[int(p.q_ptr[b]):int(p.q_ptr[b + 1])]
            for con, prior in because_ref.numpy64(st, hist, yy, int(u), targets):
                pos = {int(i): r for r, i in enumerate(hist)}
                assert all(int(i) == NONE or int(i) in pos for i in items[q]), f"{op}: target {q}: an item outside the history"
                ids = np.array([NONE if int(i) == NONE else pos[int(i)] for i in items[q]], np.int64)
                err = max(err, listed(ids, contrib[q], con), _rel(sums[q], con.sum()), _rel(priors[q], prior))
                q += 1
        return err
    # the moments: the mean as a score, the variance against exact arithmetic on the oracle's E and shapes
    st = {w: M.state(w) for w in ("THETA_E", "THETA_SHAPE", "BETA_E", "BETA_SHAPE") + (("UBIAS_E", "UBIAS_SHAPE", "IBIAS_E", "IBIAS_SHAPE") if bias else ())}
    if name == "score_moments":
        u, i = p.six
        mean = np.einsum("ij,ij->i", Et[u], Eb[i]) + ub[u] + ib[i]
        var = [float(moments_ref.exact_var(st, bias, int(a), int(b))) for a, b in zip(u, i)]
        return max(_rel(res[0], mean), _rel(res[1], var))
    if name == "recommend_ucb":
        items, ucb, mean, var = res
        X, Y = moments_ref.derived_rows(st, bias)
        err = 0.0
        for b, u in enumerate(p.users):
            ref_mean, ref_var = row(u), X[u] @ Y.T                  # float64 for the whole row: which items belong in the list
            # (every query user has at least TOPN items without a rating: a masked item, which would be listed with the ucb it
            # would have scored, never gets into a list)
            assert not np.isin(items[b], p.rated_by(u)).any(), f"{op}: user {u}: a masked item is listed"
            err = max(err, listed(items[b], ucb[b], moments_ref.ucb(ref_mean, ref_var, op[1]), masked=p.rated_by(u)))
            exact = [float(moments_ref.exact_var(st, bias, int(u), int(i))) for i in items[b]]
            err = max(err, _rel(mean[b], ref_mean[items[b].astype(np.int64)]), _rel(var[b], exact))
        return err
    raise ValueError(op)


def same_results(a, b):
    """everything two handles returned from one call, bit for bit"""
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def oracle_error(w, dv, rf):
    """the suite's measure of an exported array against the oracle's: element-wise relative, except Elog, which may pass
    arbitrarily close to zero and is held to max(|Elog|, 1) (test_random_configurations_match_the_oracle)"""
    dv, rf = np.asarray(dv, np.float64), np.asarray(rf, np.float64)
    if w.endswith("ELOG"):
        return float(np.max(np.abs(dv - rf) / np.maximum(np.abs(rf), 1.0))) if rf.size else 0.0
    return rel_err(dv, rf)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def run_three(orc, config, ops, label):
    """the operations on oracle, lazy and twin in lock step, every result compared -> (lazy, twin, oracle), still open
    (the caller closes them).  label goes in front of every assertion message together with the operations so far."""
    prob = Problem(config)
    O = OracleRun(orc, config, prob)
    lazy = DeviceRun(config, prob, O.M, eager=False)
    twin = DeviceRun(config, prob, O.M, eager=True)
    worst = {}
    try:
        for k, op in enumerate(ops):
            where = f"{label} {config}: op {k} of {ops[:k + 1]}"
            ref = O.step(op)
            value = ref if op[0] in ("set", "fall_back") else None
            a, b = lazy.step(op, value), twin.step(op, value)
            name = op[0]
            if name in ("get", "get_dev"):
                assert same_bits(a, b), f"{where}: lazy and twin differ in {int(np.sum(a != b))} entries"
                e = oracle_error(op[1], a, ref)
                assert e < RTOL, f"{where}: against the oracle {e:.3e}"
            elif name == "heldout":
                assert a == b, f"{where}: lazy {a} twin {b}"
                assert a[1] == prob.held[0].size and abs(a[0] - ref) / a[1] < 1e-9, f"{where}: {a} oracle {ref}"
            elif name == "elbo":
                assert a == b, f"{where}: lazy {a!r} twin {b!r}"
                assert abs(a - ref) <= 1e-10 * abs(ref), f"{where}: {a!r} oracle {ref!r}"
            elif name == "predict":
                assert same_bits(a, b), f"{where}: lazy and twin differ"
                assert rel_err(a, ref) < 1e-9, f"{where}: against numpy over the oracle's E {rel_err(a, ref):.3e}"
            elif name == "refused":
                assert a == b, where
            elif name in FOLDS:
                assert same_results(a, b) and np.all(a[0] == op[1]), f"{where}: iterations run {a[0]} (lazy) {b[0]} (twin)"
            elif read_call_of(op) is not None:
                assert same_results(a, b), f"{where}: lazy and twin differ in output(s) {[k for k, (x, y) in enumerate(zip(a, b)) if x.tobytes() != y.tobytes()]}"
                e = oracle_read_error(O.M, config, prob, op, a)
                worst[name] = max(worst.get(name, 0.0), e)
                assert e < RTOL, f"{where}: against numpy over the oracle's arrays {e:.3e}"
        if worst:
            print(f"{label}: worst error against the oracle per call: " + ", ".join(f"{k} {v:.2e}" for k, v in sorted(worst.items())))
        where = f"{label} {config}: after {ops}"
        fa, fb = lazy.export_all(), twin.export_all()
        for w in fa:
            assert same_bits(fa[w], fb[w]), f"{where}: {w}: lazy and twin differ"
            e = oracle_error(w, fa[w], O.M.state(w))
            assert e < RTOL, f"{where}: {w} against the oracle {e:.3e}"
    except BaseException:
        lazy.close(); twin.close()
        raise
    return lazy, twin, O
