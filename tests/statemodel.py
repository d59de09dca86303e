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
    for key, name in (("graph", "HPF_GRAPH"), ("fused_sweep", "HPF_FUSED_SWEEP")):
        if config[key] is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, config[key])


class Problem:
    """the ratings of a config, its 200 held-out pairs and its 50 pairs to predict"""

    def __init__(self, config):
        n, m = config["n"], config["m"]
        self.csr = make_problem(n, m, config["nnz"], config["data_seed"])
        self.held = heldout_pairs(n, m, 200, seed=config["data_seed"] + 1)
        pu, pi, _ = heldout_pairs(n, m, 50, seed=config["data_seed"] + 2)
        self.pairs = (pu, pi)


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
        return None

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
        else:
            raise ValueError(op)
        self._flush()
        return res


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
