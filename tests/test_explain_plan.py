"""CPU: hpf_plan::explain_plan, the shape of hpf_explain's kernel, and hpf_plan::factor_top_batch, the column batches of
hpf_factor_top (hgaprec_amd/csrc/hpf_plan.hpp).

`make -C hgaprec_amd/csrc explain` builds host/explain_selftest.cpp, a stand-alone program that walks K = 1..1024 with and
without bias and a seeded list of pair and row counts and checks: terms = K + 2 * bias, R * 64 >= terms with a kernel
instance for R, a launch grid that is non-zero, within its cap and leaves no pair without a wave, and column batches of at
least one column, at most K, within 512 MB and within the knob.  Its fixed cases must be tests/data/explain_plan_table.txt,
and capi.explain_plan / capi.explain_grid -- the mirror the GPU tests take the pairs of a grid-stride trip from -- must
agree with every line.
"""
import subprocess
from pathlib import Path

from hgaprec_amd import capi

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "hgaprec_amd" / "csrc"
TABLE = ROOT / "tests" / "data" / "explain_plan_table.txt"


def table_rows(text):
    return [tuple(ln.split()) for ln in text.splitlines() if ln.strip() and not ln.startswith("#")]


def run_selftest():
    r = subprocess.run(["make", "-C", str(CSRC), "explain"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    r = subprocess.run([str(ROOT / "hgaprec_amd" / "explain_selftest")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    return r.stdout


def test_explain_selftest_invariants_and_recorded_table():
    out = run_selftest()
    assert "explain_selftest ok: 2048 points" in out
    got = [row for row in table_rows(out) if row[0] in ("ep", "ft")]
    want = table_rows(TABLE.read_text())
    assert len([r for r in want if r[0] == "ep"]) == 52 and len([r for r in want if r[0] == "ft"]) == 11
    assert all(len(r) in (4, 10) for r in want if r[0] == "ep") and all(len(r) == 5 for r in want if r[0] == "ft")
    assert got == want, [(g, w) for g, w in zip(got, want) if g != w][:5]


def test_python_mirror_matches_the_table():
    for row in table_rows(TABLE.read_text()):
        if row[0] != "ep":
            continue
        K, bias = int(row[1]), bool(int(row[2]))
        if row[3] == "none":
            try:
                capi.explain_plan(K, bias)
            except ValueError:
                continue
            raise AssertionError(f"capi.explain_plan({K}, {bias}) has a plan where the library has none")
        p = capi.explain_plan(K, bias)
        assert (p["terms"], p["R"]) == (int(row[3]), int(row[4])), row
        assert tuple(capi.explain_grid(c) for c in (1, 5, 4099, 10000000)) == tuple(int(x) for x in row[5:9]), row
        assert capi.explain_grid(10000000) * capi.EXPLAIN_WAVES * capi.EXPLAIN_RUN == int(row[9]), row
    # every R from 1 to 16 has a column count among the GPU tests' shapes (K = 1022 with bias fills the last)
    assert capi.explain_plan(100) == {"terms": 100, "R": 2} and capi.explain_plan(1022, True) == {"terms": 1024, "R": 16}
