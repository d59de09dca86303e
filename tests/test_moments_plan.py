"""CPU: hpf_plan::moments_plan, the shape of hpf_score_moments' and hpf_recommend_ucb's kernels (hgaprec_amd/csrc/hpf_plan.hpp).

`make -C hgaprec_amd/csrc moments` builds host/moments_selftest.cpp, a stand-alone program that walks K = 1..1024 with and
without bias and a seeded list of pair, row, item and user counts and checks: C = 2 K + 2 * bias fits HPF_MAX_COLUMNS or
there is no plan, the derived rows and the mean chain end on whole MFMA steps (the two chains are those hpf_scores issues
for K and for C columns), a 16-byte piece of the staged concatenation lies in one part, X is built for exactly the users of
a batch of the top-N sweep, and launch grids that are non-zero, within their cap and leave nothing without a thread.  Its
fixed cases must be tests/data/moments_plan_table.txt, and capi.moments_plan / capi.moments_grid must agree with every line.
"""
import subprocess
from pathlib import Path

import pytest

from hgaprec_amd import capi

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "hgaprec_amd" / "csrc"
TABLE = ROOT / "tests" / "data" / "moments_plan_table.txt"


def table_rows(text):
    return [tuple(ln.split()) for ln in text.splitlines() if ln.strip() and not ln.startswith("#")]


def test_moments_selftest_invariants_and_recorded_table():
    r = subprocess.run(["make", "-C", str(CSRC), "moments"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    r = subprocess.run([str(ROOT / "hgaprec_amd" / "moments_selftest")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    assert "moments_selftest ok: 2048 points" in r.stdout
    got = [row for row in table_rows(r.stdout) if row[0] == "mp"]
    want = table_rows(TABLE.read_text())
    assert len(want) == 44 and all(len(row) in (4, 13) for row in want)
    assert got == want, [(g, w) for g, w in zip(got, want) if g != w][:5]


def test_python_mirror_matches_the_table():
    for row in table_rows(TABLE.read_text()):
        K, bias = int(row[1]), bool(int(row[2]))
        if row[3] == "none":
            with pytest.raises(ValueError):
                capi.moments_plan(K, bias)
            continue
        p = capi.moments_plan(K, bias)
        assert (p["C"], p["ldx"], p["mean_cols"], p["mean_steps"], p["var_steps"]) == tuple(int(x) for x in row[3:8]), row
        assert tuple(capi.moments_grid(c, 1, p["ldx"])[0] for c in (1, 4099, 1638400)) == tuple(int(x) for x in row[8:11]), row
        assert capi.moments_grid(1, 70, p["ldx"])[1] == int(row[11]), row
    # the limit: K <= 511 with bias, K <= 512 without
    assert capi.moments_plan(511, True)["C"] == 1024 and capi.moments_plan(512, False)["C"] == 1024
    for K, bias in ((512, True), (513, False), (0, False)):
        with pytest.raises(ValueError):
            capi.moments_plan(K, bias)
    # among the GPU test's column counts: both chains end inside an MFMA step (K = 5), the mean chain exactly on one (16)
    assert capi.moments_plan(5, False)["mean_cols"] == 8 and capi.moments_plan(5, False)["ldx"] == 12
    assert capi.moments_plan(16, True)["mean_cols"] == 16 and capi.moments_plan(16, True)["ldx"] == 36
