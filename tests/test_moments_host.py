"""No GPU: libhpf_hip.so exports hpf_score_moments and hpf_recommend_ucb and capi.py binds them with the header's signatures;
`-ucb Z` through the CLI's parser with its refusals."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest

from hgaprec_amd import capi, hostlib

ROOT = Path(__file__).resolve().parent.parent
EXE = str(ROOT / "hgaprec_amd" / "hgaprec")
BASE = ["-dir", "x", "-n", "5", "-m", "5", "-k", "2"]


def test_binding_has_both_calls_once_with_their_argtypes():
    assert capi.EXPORTS.count("hpf_score_moments") == 1 and capi.EXPORTS.count("hpf_recommend_ucb") == 1
    assert callable(capi.Hpf.score_moments) and callable(capi.Hpf.recommend_ucb)
    lib = capi.load_library()
    u32p, u64p, dp = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_double)
    assert lib.hpf_score_moments.argtypes == [C.c_void_p, u32p, u32p, C.c_size_t, dp, dp]
    assert lib.hpf_recommend_ucb.argtypes == [C.c_void_p, u32p, C.c_uint32, u64p, u32p, C.c_uint32, C.c_double, u32p, dp, dp, dp]
    out = subprocess.run(["nm", "-D", "--defined-only", str(ROOT / "hgaprec_amd" / "libhpf_hip.so")], capture_output=True, text=True)
    assert out.returncode == 0 and " T hpf_score_moments" in out.stdout and " T hpf_recommend_ucb" in out.stdout
    # a null handle is refused before anything else
    assert lib.hpf_score_moments(None, None, None, 0, None, None) == -1
    assert lib.hpf_recommend_ucb(None, None, 0, None, None, 10, 1.0, None, None, None, None) == -1
    assert lib.hpf_abi_version() == 8                                            # new functions only
    assert "#define HPF_ABI_VERSION 8" in (ROOT / "include" / "hpf.h").read_text()


def test_the_header_declares_what_is_bound():
    text = re.sub(r"/\*.*?\*/", " ", (ROOT / "include" / "hpf.h").read_text(), flags=re.S)
    flat = " ".join(text.split())
    assert ("int hpf_score_moments(hpf_handle *h, const uint32_t *u, const uint32_t *i, size_t cnt, double *out_mean, "
            "double *out_var);") in flat
    assert ("int hpf_recommend_ucb(hpf_handle *h, const uint32_t *users, uint32_t n_sel, const uint64_t *mask_ptr, "
            "const uint32_t *mask_items, uint32_t topn, double z, uint32_t *out_items , double *out_ucb , double *out_mean , "
            "double *out_var );") in flat


# ---- the parser ------------------------------------------------------------------------------------------------------------
def test_parser_takes_z_and_leaves_the_prefix_alone():
    assert hostlib.prefix(BASE + ["-recommend", "5", "-ucb", "2"]) == hostlib.prefix(BASE)      # a score mode: the same directory name
    for z in ("0", "0.5", "3", "1e1"):
        hostlib.prefix(BASE + ["-recommend", "256", "-ucb", z])
    hostlib.prefix(BASE + ["-ucb", "2", "-recommend", "5"])                                     # in either order
    hostlib.prefix(BASE + ["-fold-in", "new.tsv", "-recommend", "5", "-ucb", "2", "-explain", "3"])


@pytest.mark.parametrize("tail,msg", [
    (["-ucb", "2"], "-ucb goes with -recommend N: it orders the recommended items by mean + Z sd"),
    (["-recommend", "257", "-ucb", "2"], "-ucb needs -recommend N with N <= 256"),
    (["-recommend", "5", "-ucb", "-1"], "-ucb needs the number of standard deviations added to the mean, a number >= 0"),
    (["-recommend", "5", "-ucb", "nan"], "-ucb needs the number of standard deviations"),
    (["-recommend", "5", "-ucb", "inf"], "-ucb needs the number of standard deviations"),
    (["-recommend", "5", "-ucb", "2x"], "-ucb needs the number of standard deviations"),
    (["-recommend", "5", "-ucb"], "-ucb needs the number of standard deviations"),
    (["-audience", "5", "-ucb", "2"], "-ucb goes with -recommend N, not with -audience"),
    (["-fold-in-items", "f", "-audience", "5", "-ucb", "2"], "-ucb goes with -recommend N, not with -audience")])
def test_refusals_exit_before_anything_is_read(tail, msg):
    r = subprocess.run([EXE] + BASE + tail, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and msg in r.stderr, (r.returncode, r.stderr[-500:])
