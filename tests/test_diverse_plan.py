"""CPU: hpf_plan::diverse_plan, the shape of hpf_recommend_diverse's mmr_kernel (hgaprec_amd/csrc/hpf_plan.hpp).

`make -C hgaprec_amd/csrc diverse` builds host/diverse_selftest.cpp, a stand-alone program that walks pool = 1..256 over a
list of K and a seeded list of user and compute-unit counts and checks: the pool padded to whole 16 x 16 tiles, the MFMA
steps of a tile, the strips of the four waves covering every tile exactly once, a slab of Pp x Pp doubles of at most 512 KB,
and a grid that is non-zero, no larger than the users, the compute units or 256 MB of slabs allow, and no smaller either.
Its fixed cases must be tests/data/diverse_plan_table.txt.
"""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "hgaprec_amd" / "csrc"
TABLE = ROOT / "tests" / "data" / "diverse_plan_table.txt"


def table_rows(text):
    return [tuple(ln.split()) for ln in text.splitlines() if ln.strip() and not ln.startswith("#")]


def test_diverse_selftest_invariants_and_recorded_table():
    r = subprocess.run(["make", "-C", str(CSRC), "diverse"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    r = subprocess.run([str(ROOT / "hgaprec_amd" / "diverse_selftest")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    assert "diverse_selftest ok: 1792 points" in r.stdout
    got = [row for row in table_rows(r.stdout) if row[0] == "dp"]
    want = table_rows(TABLE.read_text())
    assert len(want) == 60 and all(len(row) == 14 for row in want)
    assert got == want, [(g, w) for g, w in zip(got, want) if g != w][:5]


def test_the_table_states_the_shapes_the_issue_names():
    """independent of the program: the arithmetic of a few lines by hand"""
    rows = {(int(r[1]), int(r[2])): [int(x) for x in r[3:]] for r in table_rows(TABLE.read_text())}
    # pool K -> Pp side tiles steps strips tiles_per_wave slab_bytes lds_bytes wg(1) wg(100) wg(100000)
    assert rows[(256, 100)][:7] == [256, 16, 256, 25, 64, 64, 512 << 10]
    assert rows[(256, 100)][8:] == [1, 100, 512]                      # 256 MB of 512 KB slabs
    assert rows[(128, 100)][:7] == [128, 8, 64, 25, 16, 16, 128 << 10]
    assert rows[(128, 100)][8:] == [1, 100, 2048]                     # 256 compute units x 8 before 256 MB / 128 KB = 2048
    assert rows[(17, 3)][:7] == [32, 2, 4, 1, 2, 2, 8192]
    assert rows[(1, 1)][:7] == [16, 1, 1, 1, 1, 1, 2048]
    assert rows[(100, 129)][:6] == [112, 7, 49, 33, 14, 14]
