"""CPU: hpf_plan::fold_plan, the shape of hpf_fold_in's kernel (hgaprec_amd/csrc/hpf_plan.hpp).

`make -C hgaprec_amd/csrc fold` builds host/fold_selftest.cpp, a stand-alone program that walks K = 1..1024 with and
without bias and a seeded list of user counts and checks: R * 64 >= ld >= K + 2 * bias with a kernel instance for R, the LDS
of a workgroup within what a launch may ask for, 1 <= rows_held with rows_held * ld * 8 inside a wave's slice, and a launch
grid that is non-zero for n >= 1 and leaves no user without a wave.  Its fixed cases must be tests/data/fold_plan_table.txt,
and capi.fold_plan / capi.fold_grid -- the mirror the GPU tests take rows_held from -- must agree with every line.
"""
import subprocess
from pathlib import Path

from hgaprec_amd import capi

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "hgaprec_amd" / "csrc"


def table_rows(text):
    return [tuple(ln.split()) for ln in text.splitlines() if ln.strip() and not ln.startswith("#")]


def run_selftest():
    r = subprocess.run(["make", "-C", str(CSRC), "fold"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    r = subprocess.run([str(ROOT / "hgaprec_amd" / "fold_selftest")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    return r.stdout


def test_fold_selftest_invariants_and_recorded_table():
    out = run_selftest()
    assert "fold_selftest ok: 2048 points" in out
    got = [row for row in table_rows(out) if row[0] == "fp"]
    want = table_rows((ROOT / "tests" / "data" / "fold_plan_table.txt").read_text())
    assert len(want) == 50 and all(row[0] == "fp" and len(row) in (4, 11) for row in want)
    assert got == want, [(g, w) for g, w in zip(got, want) if g != w][:5]


def test_python_mirror_matches_the_table():
    want = table_rows((ROOT / "tests" / "data" / "fold_plan_table.txt").read_text())
    for row in want:
        K, bias = int(row[1]), bool(int(row[2]))
        if row[3] == "none":
            try:
                capi.fold_plan(K, bias)
            except ValueError:
                continue
            raise AssertionError(f"capi.fold_plan({K}, {bias}) has a plan where the library has none")
        p = capi.fold_plan(K, bias)
        assert (p["ld"], p["R"], p["lds_wave_bytes"], p["rows_held"]) == tuple(int(x) for x in row[3:7]), row
        assert tuple(capi.fold_grid(n) for n in (1, 5, 100000, 4000000)) == tuple(int(x) for x in row[7:11]), row
    # the case the GPU tests lean on: K = 100 keeps 13 rows of 112 doubles in a 12 KiB slice, two columns per lane
    assert capi.fold_plan(100) == {"ld": 112, "R": 2, "lds_wave_bytes": 12288, "rows_held": 13}
