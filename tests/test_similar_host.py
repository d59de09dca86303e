"""No GPU: `-similar-items N`, `-similar-users N` and `-similar-metric` through the CLI's parser, and the hpf_similar symbol
with its argument types."""
import ctypes as C
import subprocess
from pathlib import Path

import pytest

from hgaprec_amd import capi, hostlib

ROOT = Path(__file__).resolve().parent.parent
EXE = str(ROOT / "hgaprec_amd" / "hgaprec")
BASE = ["-dir", "x", "-n", "5", "-m", "5", "-k", "2"]


def test_binding_has_hpf_similar_once_with_its_argtypes():
    assert capi.EXPORTS.count("hpf_similar") == 1
    lib = capi.load_library()
    u32p, dp = C.POINTER(C.c_uint32), C.POINTER(C.c_double)
    assert lib.hpf_similar.argtypes == [C.c_void_p, C.c_int, u32p, C.c_uint32, C.c_uint32, C.c_int, u32p, dp]
    out = subprocess.run(["nm", "-D", "--defined-only", str(ROOT / "hgaprec_amd" / "libhpf_hip.so")], capture_output=True, text=True)
    assert out.returncode == 0 and " T hpf_similar" in out.stdout
    assert capi.SIMILARITY == {"cosine": 0, "dot": 1} and capi.SIMILAR_MAX == capi.RECOMMEND_FUSED_MAX == 256
    hdr = (ROOT / "include" / "hpf.h").read_text()
    assert "typedef enum { HPF_SIM_COSINE = 0, HPF_SIM_DOT = 1 } hpf_similarity;" in hdr
    # a null handle is refused before anything else is looked at
    assert lib.hpf_similar(None, 1, None, 0, 10, 0, None, None) == -1


def test_parser_takes_the_counts_and_the_metric():
    # a score mode changes nothing in the name of the output directory
    assert hostlib.prefix(BASE + ["-similar-items", "5", "-similar-users", "7", "-similar-metric", "dot"]) == hostlib.prefix(BASE)
    for n in ("1", "100", "256"):
        hostlib.prefix(BASE + ["-similar-items", n])
        hostlib.prefix(BASE + ["-similar-users", n, "-similar-metric", "cosine"])


@pytest.mark.parametrize("tail,msg", [
    (["-similar-items", "0"], "-similar-items needs the number of neighbours per item, 1 .. 256"),
    (["-similar-items", "257"], "-similar-items needs the number of neighbours per item, 1 .. 256"),
    (["-similar-items"], "-similar-items needs the number of neighbours per item, 1 .. 256"),
    (["-similar-items", "5x"], "-similar-items needs the number of neighbours per item, 1 .. 256"),
    (["-similar-users", "0"], "-similar-users needs the number of neighbours per user, 1 .. 256"),
    (["-similar-users", "257"], "-similar-users needs the number of neighbours per user, 1 .. 256"),
    (["-similar-users", "-hier"], "-similar-users needs the number of neighbours per user, 1 .. 256"),
    (["-similar-items", "5", "-similar-metric", "bogus"], "-similar-metric is cosine (the default) or dot"),
    (["-similar-metric"], "-similar-metric is cosine (the default) or dot"),
])
def test_cli_refuses_at_parse_time(tmp_path, tail, msg):
    with pytest.raises(ValueError, match="-similar"):
        hostlib.prefix(BASE + tail)
    r = subprocess.run([EXE] + BASE + tail, cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 2 and msg in r.stderr
    assert not list(tmp_path.iterdir())                              # refused before the output directory exists


def test_cli_takes_both_flags_and_refuses_them_with_ngpus(tmp_path):
    base = [EXE, "-dir", str(tmp_path / "missing"), "-n", "5", "-m", "5", "-k", "2", "-similar-items", "5", "-similar-users", "5"]
    r = subprocess.run(base, cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode != 0
    assert "unknown option" not in r.stdout and "outside the MI355X hot-path build" not in r.stderr
    assert "ONE GPU" not in r.stderr and "needs the number" not in r.stderr      # accepted: fails later, no GPU or no data
    assert "no CPU fallback" in r.stderr or "cannot open file" in r.stdout + r.stderr
    for mode in (["-similar-items", "5"], ["-similar-users", "5"]):
        r = subprocess.run([EXE, "-dir", str(tmp_path / "missing"), "-n", "5", "-m", "5", "-k", "2"] + mode +
                           ["-ngpus", "2", "-label", "two"], cwd=tmp_path, capture_output=True, text=True)
        assert r.returncode == 1 and "-similar-items" in r.stderr and "ONE GPU" in r.stderr and "without -ngpus" in r.stderr
    assert not list(tmp_path.glob("*two*"))
