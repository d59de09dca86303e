"""No GPU: `-explain T`, `-topic-items N` and `-topic-users N` through the CLI's parser, and the hpf_explain and
hpf_factor_top symbols with their argument types."""
import ctypes as C
import subprocess
from pathlib import Path

import pytest

from hgaprec_amd import capi, hostlib

ROOT = Path(__file__).resolve().parent.parent
EXE = str(ROOT / "hgaprec_amd" / "hgaprec")
BASE = ["-dir", "x", "-n", "5", "-m", "5", "-k", "2"]

EXPLAIN_N = "-explain needs the number of terms per recommended item, 1 .. 32"
EXPLAIN_ALONE = "-explain goes with -recommend N: it explains the recommended items"
TOPIC_ITEMS = "-topic-items needs the number of items per factor, 1 .. 1024"
TOPIC_USERS = "-topic-users needs the number of users per factor, 1 .. 1024"


def test_binding_has_both_calls_once_with_their_argtypes():
    assert capi.EXPORTS.count("hpf_explain") == 1 and capi.EXPORTS.count("hpf_factor_top") == 1
    lib = capi.load_library()
    u32p, dp = C.POINTER(C.c_uint32), C.POINTER(C.c_double)
    assert lib.hpf_explain.argtypes == [C.c_void_p, u32p, u32p, C.c_size_t, C.c_uint32, u32p, dp]
    assert lib.hpf_factor_top.argtypes == [C.c_void_p, C.c_int, C.c_uint32, u32p, dp]
    out = subprocess.run(["nm", "-D", "--defined-only", str(ROOT / "hgaprec_amd" / "libhpf_hip.so")], capture_output=True, text=True)
    assert out.returncode == 0 and " T hpf_explain" in out.stdout and " T hpf_factor_top" in out.stdout
    assert capi.EXPLAIN_MAX == 32 and capi.FACTOR_TOP_MAX == 1024
    hdr = (ROOT / "include" / "hpf.h").read_text()
    assert "#define HPF_EXPLAIN_MAX 32" in hdr and "#define HPF_ABI_VERSION 8" in hdr
    # a null handle is refused before anything else is looked at
    assert lib.hpf_explain(None, None, None, 0, 5, None, None) == -1
    assert lib.hpf_factor_top(None, 1, 10, None, None) == -1


def test_parser_takes_the_counts_and_leaves_the_prefix_alone():
    # a score mode changes nothing in the name of the output directory
    assert hostlib.prefix(BASE + ["-topic-items", "5", "-topic-users", "7"]) == hostlib.prefix(BASE)
    assert hostlib.prefix(BASE + ["-recommend", "5", "-explain", "3"]) == hostlib.prefix(BASE)
    assert hostlib.prefix(BASE + ["-explain", "3", "-recommend", "5"]) == hostlib.prefix(BASE)     # in either order
    for n in ("1", "1024"):
        hostlib.prefix(BASE + ["-topic-items", n])
        hostlib.prefix(BASE + ["-topic-users", n])
    for t in ("1", "32"):
        hostlib.prefix(BASE + ["-recommend", "5", "-explain", t])
        hostlib.prefix(BASE + ["-fold-in", "new.tsv", "-recommend", "5", "-explain", t])


@pytest.mark.parametrize("tail,msg", [
    (["-recommend", "5", "-explain", "0"], EXPLAIN_N),
    (["-recommend", "5", "-explain", "33"], EXPLAIN_N),
    (["-recommend", "5", "-explain", "5x"], EXPLAIN_N),
    (["-recommend", "5", "-explain"], EXPLAIN_N),
    (["-explain", "5"], EXPLAIN_ALONE),
    (["-explain", "5", "-topic-items", "5"], EXPLAIN_ALONE),
    (["-topic-items", "0"], TOPIC_ITEMS),
    (["-topic-items", "1025"], TOPIC_ITEMS),
    (["-topic-items"], TOPIC_ITEMS),
    (["-topic-users", "0"], TOPIC_USERS),
    (["-topic-users", "-hier"], TOPIC_USERS),
])
def test_cli_refuses_at_parse_time(tmp_path, tail, msg):
    with pytest.raises(ValueError, match="-explain|-topic"):
        hostlib.prefix(BASE + tail)
    r = subprocess.run([EXE] + BASE + tail, cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 2 and msg in r.stderr
    assert not list(tmp_path.iterdir())                              # refused before the output directory exists


def test_cli_takes_the_flags_and_refuses_them_with_ngpus(tmp_path):
    head = [EXE, "-dir", str(tmp_path / "missing"), "-n", "5", "-m", "5", "-k", "2"]
    for mode in (["-topic-items", "5", "-topic-users", "5"], ["-recommend", "5", "-explain", "3"]):
        r = subprocess.run(head + mode, cwd=tmp_path, capture_output=True, text=True)
        assert r.returncode != 0
        assert "unknown option" not in r.stdout and "outside the MI355X hot-path build" not in r.stderr
        assert "ONE GPU" not in r.stderr and "needs the number" not in r.stderr      # accepted: fails later, no GPU or no data
        assert "no CPU fallback" in r.stderr or "cannot open file" in r.stdout + r.stderr
    for mode in (["-topic-items", "5"], ["-topic-users", "5"], ["-recommend", "5", "-explain", "3"]):
        r = subprocess.run(head + mode + ["-ngpus", "2", "-label", "two"], cwd=tmp_path, capture_output=True, text=True)
        assert r.returncode == 1 and "ONE GPU" in r.stderr and "without -ngpus" in r.stderr
    assert not list(tmp_path.glob("*two*"))
