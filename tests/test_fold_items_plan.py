"""CPU: what hpf_fold_in_items decides on the host (hgaprec_amd/csrc/hpf_plan.hpp, fold_items_plan and fold_part) and the
reader of `-fold-in-items FILE`, under ASan/UBSan.

`make -C hgaprec_amd/csrc fold_items` builds host/fold_items_selftest.cpp, a stand-alone program with the sanitizers linked
in.  It walks K = 1..1024 with and without bias and checks: R * 64 >= ld; an instance of fold_in_long_kernel for (R, WAVES);
the workgroup's LDS (WAVES partial rows + the shared stop word) within the launch limit; the parts of the WAVES waves cover
[0, len) exactly once, in order and in whole 64-blocks, for a seeded list of lengths with 0, 1 and WAVES * 64 +- 1 among
them; a grid that is non-zero and leaves no long row without a workgroup.  Its fixed cases must be
tests/data/fold_items_plan_table.txt, and the mirror in capi.py must agree with every line.  The same program runs
Ratings::read_fold_in_items on the cases of host_selftest.cpp's fold-in block, transposed.
"""
import subprocess
from pathlib import Path

from hgaprec_amd import capi

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "hgaprec_amd" / "csrc"
TABLE = ROOT / "tests" / "data" / "fold_items_plan_table.txt"


def table_rows(text):
    return [tuple(ln.split()) for ln in text.splitlines() if ln.strip() and not ln.startswith("#")]


def test_selftest_invariants_reader_and_recorded_table():
    r = subprocess.run(["make", "-C", str(CSRC), "fold_items"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    r = subprocess.run([str(ROOT / "hgaprec_amd" / "fold_items_selftest_asan")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    assert "fold_items_selftest ok: 2048 points" in r.stdout
    got = [row for row in table_rows(r.stdout) if row[0] == "fip"]
    want = table_rows(TABLE.read_text())
    assert len(want) == 56 and all(row[0] == "fip" for row in want)
    assert got == want, [(g, w) for g, w in zip(got, want) if g != w][:5]


def test_python_mirror_matches_the_table():
    for row in table_rows(TABLE.read_text()):
        K, bias = int(row[1]), bool(int(row[2]))
        if row[3] == "none":
            try:
                capi.fold_items_plan(K, bias)
            except ValueError:
                continue
            raise AssertionError(f"capi.fold_items_plan({K}, {bias}) has a plan where the library has none")
        p = capi.fold_items_plan(K, bias)
        assert (p["ld"], p["R"], p["waves"], p["lds_long_bytes"], p["long_min"]) == tuple(int(x) for x in row[3:8]), row
        assert (capi.fold_long_grid(1), capi.fold_long_grid(5000)) == (int(row[8]), int(row[9])), row
        assert row[10] == "|"
        parts = [capi.fold_part(p["waves"] * 64 + 1, p["waves"], w) for w in range(p["waves"])]
        assert [f"{a}-{b}" for a, b in parts] == list(row[11:]), row
    assert capi.fold_long_grid(0) == 0
    # the cases the GPU tests lean on
    assert capi.fold_items_plan(100)["waves"] == 8 and capi.fold_items_plan(520)["R"] == 9 and capi.fold_items_plan(520)["waves"] == 4
    assert capi.fold_items_plan(5, True)["long_min"] == capi.FOLD_LONG_MIN


def test_parts_cover_a_row_once():
    for waves in (4, 8):
        for length in (0, 1, 63, 64, 65, waves * 64 - 1, waves * 64, waves * 64 + 1, 7924, 100000, 2 ** 32 - 1):
            at = 0
            for w in range(waves):
                a, b = capi.fold_part(length, waves, w)
                assert a == at and a <= b <= length and (a % 64 == 0 or a == length) and (b % 64 == 0 or b == length)
                at = b
            assert at == length
