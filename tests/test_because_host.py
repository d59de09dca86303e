"""No GPU: `-because T` through the CLI's parser, and the hpf_because symbol with its argument types."""
import ctypes as C
import subprocess
from pathlib import Path

import pytest

from hgaprec_amd import capi, hostlib

ROOT = Path(__file__).resolve().parent.parent
EXE = str(ROOT / "hgaprec_amd" / "hgaprec")
BASE = ["-dir", "x", "-n", "5", "-m", "5", "-k", "2"]

BECAUSE_N = "-because needs the number of rated items per recommended item, 1 .. 32"
BECAUSE_ALONE = "-because goes with -recommend N: it traces the recommended items to the user's ratings"


def test_binding_has_the_call_once_with_its_argtypes():
    assert capi.EXPORTS.count("hpf_because") == 1
    lib = capi.load_library()
    u32p, u64p, dp = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_double)
    assert lib.hpf_because.argtypes == [C.c_void_p, u32p, C.c_uint32, u64p, u32p, C.c_uint32, u32p, dp, dp, dp]
    out = subprocess.run(["nm", "-D", "--defined-only", str(ROOT / "hgaprec_amd" / "libhpf_hip.so")], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.count(" T hpf_because\n") == 1
    assert capi.BECAUSE_MAX == 32
    hdr = (ROOT / "include" / "hpf.h").read_text()
    assert "#define HPF_BECAUSE_MAX %d\n" % capi.BECAUSE_MAX in hdr and "#define HPF_ABI_VERSION 8" in hdr
    assert hdr.count("hpf_because(hpf_handle *h") == 1
    # a null handle is refused before anything else is looked at
    assert lib.hpf_because(None, None, 0, None, None, 5, None, None, None, None) == -1


def test_parser_takes_the_count_and_leaves_the_prefix_alone():
    assert hostlib.prefix(BASE + ["-recommend", "5", "-because", "3"]) == hostlib.prefix(BASE)
    assert hostlib.prefix(BASE + ["-because", "3", "-recommend", "5"]) == hostlib.prefix(BASE)     # in either order
    assert hostlib.prefix(BASE + ["-recommend", "5", "-explain", "2", "-because", "3"]) == hostlib.prefix(BASE)
    for t in ("1", "32"):
        hostlib.prefix(BASE + ["-recommend", "5", "-because", t])
        hostlib.prefix(BASE + ["-fold-in", "new.tsv", "-recommend", "5", "-because", t])


@pytest.mark.parametrize("tail,msg", [
    (["-recommend", "5", "-because", "0"], BECAUSE_N),
    (["-recommend", "5", "-because", "33"], BECAUSE_N),
    (["-recommend", "5", "-because", "5x"], BECAUSE_N),
    (["-recommend", "5", "-because"], BECAUSE_N),
    (["-because", "5"], BECAUSE_ALONE),
    (["-because", "5", "-topic-items", "5"], BECAUSE_ALONE),
    (["-fold-in", "new.tsv", "-because", "5"], BECAUSE_ALONE),
])
def test_cli_refuses_at_parse_time(tmp_path, tail, msg):
    with pytest.raises(ValueError, match="-because"):
        hostlib.prefix(BASE + tail)
    r = subprocess.run([EXE] + BASE + tail, cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 2 and msg in r.stderr
    assert not list(tmp_path.iterdir())                              # refused before the output directory exists


def test_cli_takes_the_flag_and_refuses_it_with_ngpus(tmp_path):
    head = [EXE, "-dir", str(tmp_path / "missing"), "-n", "5", "-m", "5", "-k", "2"]
    mode = ["-recommend", "5", "-because", "3"]
    r = subprocess.run(head + mode, cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode != 0
    assert "unknown option" not in r.stdout and "outside the MI355X hot-path build" not in r.stderr
    assert "ONE GPU" not in r.stderr and "needs the number" not in r.stderr      # accepted: fails later, no GPU or no data
    assert "no CPU fallback" in r.stderr or "cannot open file" in r.stdout + r.stderr
    r = subprocess.run(head + mode + ["-ngpus", "2", "-label", "two"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 1 and "ONE GPU" in r.stderr and "without -ngpus" in r.stderr
    assert not list(tmp_path.glob("*two*"))
