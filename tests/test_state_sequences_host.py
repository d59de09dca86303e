"""The random call orders of tests/statemodel.py, without a GPU: the generator is repeatable, the committed seeds cover
what they are meant to cover, and the oracle stays a valid HPF state through every sequence -- so a fall-back from the
packed rows in tests/test_gpu_state_sequences.py is always an injected one."""
import pytest

from tests import statemodel as sm
from tests.util import compare_states

# the random sequences of test_gpu_state_sequences.py::test_random_call_orders
STATE_SEEDS = [1, 3, 4, 16, 160, 189, 194, 227, 274, 288, 326, 365, 369, 427, 433, 436, 458, 470, 511, 522,
               549, 598, 611, 704, 979, 996, 1051, 1059, 1076, 1095, 1103, 1241, 1267, 1295, 1308, 1337, 1344, 1345, 1386, 1459]
# further seeds whose config is K = 100 with w_storage = 0 (p59 rows): a fall-back is woven into their sequences
PACKED_SEEDS = [2, 8, 10, 22, 24, 25, 28, 30]


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


@pytest.mark.parametrize("seed", STATE_SEEDS + PACKED_SEEDS)
def test_the_oracle_stays_a_valid_state(orc, seed):
    """all values finite, E and SHAPE positive, the Elog spread inside a row at most 40 -- far from the 88 at which the
    packed rows give up -- after every operation of every sequence (without the woven-in fall-back)"""
    config, ops = sm.sequence(seed)
    O = sm.OracleRun(orc, config, sm.Problem(config))
    O.check_valid((seed, "start"))
    for k, op in enumerate(ops):
        O.step(op)
        O.check_valid((seed, k, op))
