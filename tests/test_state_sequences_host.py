"""The random call orders of tests/statemodel.py, without a GPU: the generators are repeatable, sequence() still draws
what it drew when its seeds were chosen, the committed seeds cover what they are meant to cover, and the oracle stays a
valid HPF state through every sequence -- the fold-ins of serving_sequence() included -- so a fall-back from the packed rows
in tests/test_gpu_state_sequences.py is always an injected one."""
import hashlib

import pytest

from tests import statemodel as sm
from tests.util import compare_states

# the random sequences of test_gpu_state_sequences.py::test_random_call_orders
STATE_SEEDS = [1, 3, 4, 16, 160, 189, 194, 227, 274, 288, 326, 365, 369, 427, 433, 436, 458, 470, 511, 522,
               549, 598, 611, 704, 979, 996, 1051, 1059, 1076, 1095, 1103, 1241, 1267, 1295, 1308, 1337, 1344, 1345, 1386, 1459]
# further seeds whose config is K = 100 with w_storage = 0 (p59 rows): a fall-back is woven into their sequences
PACKED_SEEDS = [2, 8, 10, 22, 24, 25, 28, 30]
# sha256 over repr(sequence(seed)) of the 48 seeds above, taken before serving_sequence() was written beside it
SEQUENCE_DIGEST = "49e63c04a4df4b9b5266465729781248a5c4c2293c5e7c3f339eacd592b968f5"
# the sequences of serving_sequence() in test_gpu_state_sequences.py::test_random_serving_call_orders: chosen greedily, out
# of the seeds 1 .. 25000, for the conditions asserted below
SERVING_SEEDS = [90, 370, 812, 944, 1199, 1244, 1552, 2407, 2458, 2787, 3089, 3110, 3125, 3289, 3471, 4540, 4749, 5872, 6026, 7114,
                 7187, 8241, 8721, 9208, 10132, 10398, 11077, 11253, 12085, 13407, 14372, 14923, 16275, 16749, 16765, 17470, 22325,
                 22472, 24467, 24544]
# those of them whose config is K = 100 with w_storage = 0: a second test weaves a fall-back into their sequences
SERVING_PACKED = [s for s in SERVING_SEEDS if (lambda c: c["K"] == 100 and c["w_storage"] == 0)(sm.serving_sequence(s)[0])]


def test_the_generator_is_repeatable():
    for seed in STATE_SEEDS[:5] + PACKED_SEEDS[:2]:
        assert sm.sequence(seed) == sm.sequence(seed)
        c, ops = sm.sequence(seed)
        assert 25 <= len(ops) <= 35
        assert sm.with_fall_back(seed, ops) == sm.with_fall_back(seed, ops)
    assert sm.sequence(STATE_SEEDS[0]) != sm.sequence(STATE_SEEDS[1])


def test_the_seed_lists_are_what_they_say():
    assert len(STATE_SEEDS) == 40 and len(set(STATE_SEEDS)) == 40
    assert len(PACKED_SEEDS) == 8 and not set(PACKED_SEEDS) & set(STATE_SEEDS)
    for seed in PACKED_SEEDS:
        c, ops = sm.sequence(seed)
        assert c["K"] == 100 and c["w_storage"] == 0, (seed, c)
        woven = sm.with_fall_back(seed, ops)
        at = woven.index(("fall_back",))
        assert len(woven) == len(ops) + 1 and woven[:at] + woven[at + 1:] == ops and len(woven) - at > 3


def test_operations_are_well_formed():
    for seed in STATE_SEEDS + PACKED_SEEDS:
        c, ops = sm.sequence(seed)
        arrays = set(compare_states(c["hier"], c["bias"]))
        iterated = False
        rates = set()
        assert not c["novb"] or (c["bias"] and not c["hier"])
        for op in ops:
            if op[0] in ("get", "get_dev"):
                assert op[1] in arrays, (seed, op)
                if op[1].endswith("_RATE") and not op[1].startswith(("XI_", "ETA_")):
                    assert iterated or op[1] in rates, (seed, op)        # nothing else can be exported before iteration 0
            elif op[0] == "set":
                assert op[1] in arrays and op[2] in ("host", "device"), (seed, op)
                obj, kind = op[1].rsplit("_", 1)
                if kind == "RATE":
                    assert not iterated and obj in ("THETA", "BETA"), (seed, op)
                    rates.add(op[1])
                elif kind == "SHAPE":
                    assert obj in ("THETA", "BETA", "UBIAS", "IBIAS"), (seed, op)
            elif op[0] == "elbo":
                assert iterated, seed
            elif op[0] == "iterate":
                assert 1 <= op[1] <= 3
            elif op[0] == "refused":
                assert op[1] in sm.REFUSED_FORMS
            else:
                assert op in (("pieces",), ("heldout",), ("predict",), ("synchronize",), ("snapshot_swap",)), (seed, op)
            iterated = iterated or op[0] in ("iterate", "pieces")


def test_every_kind_of_operation_follows_every_other_at_least_twice():
    count = {(a, b): 0 for a in sm.KINDS for b in sm.KINDS}
    for seed in STATE_SEEDS:
        kinds = [sm.kind_of(op) for op in sm.sequence(seed)[1]]
        for a, b in zip(kinds, kinds[1:]):
            if a is not None and b is not None:
                count[(a, b)] += 1
    rare = {p: k for p, k in count.items() if k < 2}
    assert not rare, rare


def test_every_array_is_somewhere_the_first_export_after_an_iteration():
    first = set()
    for seed in STATE_SEEDS:
        first |= sm.first_exports(sm.sequence(seed)[1])
    assert first == set(compare_states(True, True)), set(compare_states(True, True)) - first


def test_every_config_value_is_drawn_at_least_three_times():
    drawn = {}
    for seed in STATE_SEEDS:
        c = sm.sequence(seed)[0]
        for key in ("K", "hier", "bias", "novb", "w_storage", "graph", "fused_sweep"):
            drawn[(key, c[key])] = drawn.get((key, c[key]), 0) + 1
    want = ([("K", s[2]) for s in sm.SHAPES] + [(k, v) for k in ("hier", "bias", "novb") for v in (False, True)] +
            [("w_storage", 0), ("w_storage", 3), ("graph", None), ("graph", "0"), ("graph", "1"),
             ("fused_sweep", None), ("fused_sweep", "0")])
    assert all(drawn.get(k, 0) >= 3 for k in want), {k: drawn.get(k, 0) for k in want}


def test_sequence_draws_what_it_drew_when_its_seeds_were_chosen():
    h = hashlib.sha256()
    for seed in STATE_SEEDS + PACKED_SEEDS:
        h.update(repr(sm.sequence(seed)).encode())
    assert h.hexdigest() == SEQUENCE_DIGEST


# ---- serving_sequence() -------------------------------------------------------------------------------------------------

def _serving():
    return [(seed,) + sm.serving_sequence(seed) for seed in SERVING_SEEDS]


def test_the_serving_generator_is_repeatable():
    assert len(SERVING_SEEDS) <= 40 and len(set(SERVING_SEEDS)) == len(SERVING_SEEDS)
    for seed in SERVING_SEEDS[:6]:
        assert sm.serving_sequence(seed) == sm.serving_sequence(seed)
        c, ops = sm.serving_sequence(seed)
        assert 25 <= len(ops) <= 35
        assert sm.with_fall_back(seed, ops) == sm.with_fall_back(seed, ops)
    assert sm.serving_sequence(SERVING_SEEDS[0]) != sm.serving_sequence(SERVING_SEEDS[1])
    assert len(SERVING_PACKED) >= 3, SERVING_PACKED
    for seed in SERVING_PACKED:
        ops = sm.serving_sequence(seed)[1]
        woven = sm.with_fall_back(seed, ops)
        at = woven.index(("fall_back",))
        assert len(woven) == len(ops) + 1 and woven[:at] + woven[at + 1:] == ops and len(woven) - at > 3


def test_serving_operations_are_well_formed():
    reads = {c[0] for c in sm.READ_CALLS}
    for seed, c, ops in _serving():
        arrays = set(compare_states(c["hier"], c["bias"]))
        iterated = False
        rates = set()
        assert not c["novb"] or (c["bias"] and not c["hier"])
        assert c["fold_long_min"] in (None, "32")
        for op in ops:
            if op[0] in ("get", "get_dev"):
                assert op[1] in arrays, (seed, op)
                if op[1].endswith("_RATE") and not op[1].startswith(("XI_", "ETA_")):
                    assert iterated or op[1] in rates, (seed, op)        # handed in, or left by a fold-in of that side
            elif op[0] == "set":
                assert op[1] in arrays and op[2] in ("host", "device"), (seed, op)
                obj, kind = op[1].rsplit("_", 1)
                if kind == "RATE":
                    assert not iterated and obj in ("THETA", "BETA"), (seed, op)
                    rates.add(op[1])
                elif kind == "SHAPE":
                    assert obj in ("THETA", "BETA", "UBIAS", "IBIAS"), (seed, op)
            elif op[0] == "elbo":
                assert iterated, seed
            elif op[0] == "iterate":
                assert 1 <= op[1] <= 3
            elif op[0] == "refused":
                assert op[1] in sm.REFUSED_FORMS
            elif op[0] in sm.FOLDS:
                assert len(op) == 2 and 1 <= op[1] <= 3, (seed, op)
                rates |= {"THETA_RATE", "UBIAS_RATE"} if op[0] == "fold_in" else {"BETA_RATE", "IBIAS_RATE"}
            elif op[0] in reads:
                assert sm.read_call_of(op) in sm.READ_CALLS, (seed, op)
                assert op[0] != "recommend_ucb" or (len(op) == 2 and op[1] in sm.UCB_Z), (seed, op)
                assert len(op) == (2 if op[0] in ("similar", "factor_top", "recommend_ucb") else 1), (seed, op)
                assert iterated or sm.serving_kind_of(op) not in ("because", "moments"), (seed, op)
            else:
                assert op in (("pieces",), ("heldout",), ("predict",), ("synchronize",), ("snapshot_swap",)), (seed, op)
            iterated = iterated or op[0] in ("iterate", "pieces")


def test_every_serving_kind_follows_every_other_at_least_twice():
    """over all of SERVING_KINDS: the thirteen kinds of sequence(), the two fold-ins and the five kinds of read-only call"""
    count = {(a, b): 0 for a in sm.SERVING_KINDS for b in sm.SERVING_KINDS}
    for seed, c, ops in _serving():
        kinds = [sm.serving_kind_of(op) for op in ops]
        for a, b in zip(kinds, kinds[1:]):
            if a is not None and b is not None:
                count[(a, b)] += 1
    rare = {p: k for p, k in count.items() if k < 2}
    assert len(count) == 400 and not rare, rare


def test_every_serving_call_is_drawn_and_is_the_first_after_every_context():
    """every individual call at least four times; every read-only call at least once the first operation after an
    iteration, a set of an E, of an Elog and of a shape, either fold-in and a snapshot swap (no call needed a shorter list
    of contexts); z of recommend_ucb both ways"""
    drawn = {c: 0 for c in sm.READ_CALLS + tuple((f,) for f in sm.FOLDS)}
    first = {(ctx, c): 0 for ctx in sm.CONTEXTS for c in sm.READ_CALLS}
    zs = set()
    for seed, c, ops in _serving():
        for k, op in enumerate(ops):
            call = sm.read_call_of(op) or (op[:1] if op[0] in sm.FOLDS else None)
            if call is None:
                continue
            drawn[call] += 1
            if op[0] == "recommend_ucb":
                zs.add(op[1])
            if k and op[0] not in sm.FOLDS and sm.context_of(ops[k - 1]):
                first[(sm.context_of(ops[k - 1]), call)] += 1
    assert len(drawn) == 17 and len(first) == 7 * 15
    assert all(v >= 4 for v in drawn.values()), {k: v for k, v in drawn.items() if v < 4}
    assert all(first.values()), [k for k, v in first.items() if not v]
    assert zs == set(sm.UCB_Z)


def test_the_fold_ins_come_before_the_first_iteration_and_before_what_reads_their_side():
    """each fold-in at least twice before the first iteration, and at least twice directly followed by each of iterate,
    pieces and snapshot_swap"""
    early = {f: 0 for f in sm.FOLDS}
    then = {(f, nxt): 0 for f in sm.FOLDS for nxt in ("iterate", "pieces", "snapshot_swap")}
    for seed, c, ops in _serving():
        iterated = False
        for k, op in enumerate(ops):
            if op[0] in sm.FOLDS:
                early[op[0]] += not iterated
                if k + 1 < len(ops) and (op[0], ops[k + 1][0]) in then:
                    then[(op[0], ops[k + 1][0])] += 1
            iterated = iterated or op[0] in ("iterate", "pieces")
    assert all(v >= 2 for v in early.values()), early
    assert all(v >= 2 for v in then.values()), then


def test_every_serving_config_value_is_drawn_at_least_three_times():
    drawn = {}
    keys = ("K", "hier", "bias", "novb", "w_storage", "graph", "fused_sweep", "fold_long_min")
    for seed, c, ops in _serving():
        for key in keys:
            drawn[(key, c[key])] = drawn.get((key, c[key]), 0) + 1
    want = ([("K", s[2]) for s in sm.SHAPES] + [(k, v) for k in ("hier", "bias", "novb") for v in (False, True)] +
            [("w_storage", 0), ("w_storage", 3), ("graph", None), ("graph", "0"), ("graph", "1"),
             ("fused_sweep", None), ("fused_sweep", "0"), ("fold_long_min", None), ("fold_long_min", "32")])
    assert all(drawn.get(k, 0) >= 3 for k in want), {k: drawn.get(k, 0) for k in want}


@pytest.mark.parametrize("seed", STATE_SEEDS + PACKED_SEEDS + [-s for s in SERVING_SEEDS])
def test_the_oracle_stays_a_valid_state(orc, seed):
    """all values finite, E and SHAPE positive, the Elog spread inside a row at most 40 -- far from the 88 at which the
    packed rows give up -- after every operation of every sequence (without the woven-in fall-back); a negative seed is
    one of SERVING_SEEDS"""
    config, ops = sm.sequence(seed) if seed > 0 else sm.serving_sequence(-seed)
    O = sm.OracleRun(orc, config, sm.Problem(config))
    O.check_valid((seed, "start"))
    for k, op in enumerate(ops):
        O.step(op)
        O.check_valid((seed, k, op))
