"""CPU: hpf_plan::because_plan, the shape of hpf_because's two kernels (hgaprec_amd/csrc/hpf_plan.hpp).

`make -C hgaprec_amd/csrc because` builds host/because_selftest.cpp, a stand-alone program that walks K = 1..1024 with and
without bias and a seeded list of user and pair counts and checks: the row stride of the gathered copy holds the K + 2 * bias
live columns in whole 128-byte lines and is the fold-in's, R * 64 >= the stride with a kernel instance for R, and launch
grids that are non-zero, within their cap and leave nobody without a wave.  Its fixed cases must be
tests/data/because_plan_table.txt, and capi.because_plan / capi.because_grid must agree with every line.
"""
import subprocess
from pathlib import Path

import pytest

from hgaprec_amd import capi

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "hgaprec_amd" / "csrc"
TABLE = ROOT / "tests" / "data" / "because_plan_table.txt"


def table_rows(text):
    return [tuple(ln.split()) for ln in text.splitlines() if ln.strip() and not ln.startswith("#")]


def test_because_selftest_invariants_and_recorded_table():
    r = subprocess.run(["make", "-C", str(CSRC), "because"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    r = subprocess.run([str(ROOT / "hgaprec_amd" / "because_selftest")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    assert "because_selftest ok: 2048 points" in r.stdout
    got = [row for row in table_rows(r.stdout) if row[0] == "bp"]
    want = table_rows(TABLE.read_text())
    assert len(want) == 48 and all(len(row) in (4, 11) for row in want)
    assert got == want, [(g, w) for g, w in zip(got, want) if g != w][:5]


def test_python_mirror_matches_the_table():
    for row in table_rows(TABLE.read_text()):
        K, bias = int(row[1]), bool(int(row[2]))
        if row[3] == "none":
            with pytest.raises(ValueError):
                capi.because_plan(K, bias)
            continue
        p = capi.because_plan(K, bias)
        assert (p["ld"], p["R"]) == (int(row[3]), int(row[4])), row
        assert tuple(capi.because_grid(n, 1)[0] for n in (1, 40, 16384)) == tuple(int(x) for x in row[5:8]), row
        assert tuple(capi.because_grid(1, nt)[1] for nt in (1, 4099, 1638400)) == tuple(int(x) for x in row[8:11]), row
    # one and several columns per lane among the GPU test's column counts
    assert [capi.because_plan(K, b)["R"] for K, b in ((1, True), (5, False), (64, False), (65, False), (100, True), (130, False))] == [1, 1, 1, 2, 2, 3]
