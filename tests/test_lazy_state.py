"""CPU: the handle's lazy state, hgaprec_amd/csrc/hpf_lazy.hpp.

`make -C hgaprec_amd/csrc lazy` builds host/lazy_selftest.cpp -- a stand-alone program, under ASan/UBSan -- which drives
the flags the way hpf_capi.hip does (ask what a call needs, run the jobs in the order given, report the event) next to a
naive model of the buffers, over seeded random orders of every set kind on every object, both sweeps, both folds, a
reported flush, a snapshot round trip and every request kind, with all four of hier / bias, -novb, one and several ranks,
with and without a communicator.  It checks that after the jobs of a request everything the request named is current and
nothing was refreshed while a fall-back was due, that a twin which exports everything after every event ends in the same
state as the lazy handle, that a refused request changes no flag, and that the snapshot words round-trip for every
combination of bits.  What it cannot show is that the jobs do what the model assumes: tests/test_gpu_state_sequences.py.
"""
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "hgaprec_amd" / "csrc"


def test_lazy_state_selftest():
    r = subprocess.run(["make", "-C", str(CSRC), "lazy"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    env = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=1:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}
    r = subprocess.run([str(ROOT / "hgaprec_amd" / "lazy_selftest_asan")], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    m = re.search(r"lazy_selftest ok: (\d+) sequences, (\d+) events, (\d+) \(event, request\) pairs, (\d+) of (\d+) event kinds, "
                  r"(\d+) of (\d+) request kinds, (\d+) snapshot words", r.stdout)
    assert m, r.stdout[-2000:]
    seqs, events, pairs, ev_seen, ev_all, need_seen, need_all, words = map(int, m.groups())
    assert seqs >= 3000 and 20 * seqs <= events, (seqs, events)
    assert ev_seen == ev_all and need_seen == need_all, m.group(0)      # every event kind and every request kind occurred
    # fourteen side bits x the two handle words, and the 512 side words of a blob from before bits 9 .. 14 existed
    assert pairs >= 400 and words == 16384 * 4 * 2 + 512, m.group(0)


def test_the_flags_are_out_of_reach_of_the_library():
    """hpf_capi.hip names no flag: it reports events and asks (the private members of hpf_lazy::State enforce it; this
    keeps the names out of new code paths and comments that would suggest otherwise)"""
    text = (CSRC / "hpf_capi.hip").read_text()
    code = "\n".join(ln.split("//")[0] for ln in text.splitlines())
    for name in ("have_E", "have_L", "have_prior", "have_bias_E", "have_bias_L", "bias_rate_known", "w_dirty", "w_from_sweep",
                 "l_stale", "es_stale", "derived_dirty", "sums_dirty", "start_sums_done", "tail_partial"):
        assert not re.search(rf"\b{name}\b", code), name
    for gone in ("need_e", "refresh_e", "scoring_ready", "recover_between_iterations"):
        assert not re.search(rf"\b{gone}\(", text), gone
