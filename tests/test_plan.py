"""CPU: the shape planner and the kernel-instance predicates of hgaprec_amd/csrc/hpf_plan.hpp.

`make -C hgaprec_amd/csrc plan` builds host/plan_selftest.cpp -- a stand-alone program, under ASan/UBSan -- which plans
every column count 1..HPF_MAX_COLUMNS x w_storage 0..3 x HPF_W_PACK off/on, checks each plan (ld >= C, the packed and the
plain row arithmetic, a kernel instance for the phi pass, the gather-only probe and the sweep, the fall-back to plain
doubles equal to the w_storage = 3 plan) and the shapes the knobs HPF_PHI_CFG / HPF_SWEEP_CFG force, pins the batches, the
launch grid and the chunk counts of the fused rank kernels (rank_batch_users, rank_grid, rank_chunks), and prints the mapping
as runs.  The runs must be tests/data/plan_table.txt, which was recorded from the library's hpf_get_work_info on a GPU
before the planner became a header of its own.

The same program pins the tile policy (tile_policy, tiling_fits) to DESIGN.md section 5, checks the invariants of the queue
plan of a tiled pass (plan_tile_queues) over a seeded sweep and, run as `plan_selftest_asan tile-queues`, prints
`tq case-id chunks chunk_segs fnv64` for a fixed list of cases.  Those lines must be tests/data/tile_queue_table.txt, recorded from the queue arithmetic as it stood inside
hpf_capi.hip before it moved into the header.
"""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "hgaprec_amd" / "csrc"


def table_rows(text):
    return [tuple(ln.split()) for ln in text.splitlines() if ln.strip() and not ln.startswith("#")]


def test_planner_selftest_and_recorded_table():
    r = subprocess.run(["make", "-C", str(CSRC), "plan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    env = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=1:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}
    r = subprocess.run([str(ROOT / "hgaprec_amd" / "plan_selftest_asan")], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    assert "plan_selftest ok: 8192 points" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    got, want = table_rows(r.stdout), table_rows((ROOT / "tests" / "data" / "plan_table.txt").read_text())
    assert len(want) > 100 and all(len(row) in (5, 11) for row in want)
    assert got == want, [(g, w) for g, w in zip(got, want) if g != w][:5]
    r = subprocess.run([str(ROOT / "hgaprec_amd" / "plan_selftest_asan"), "tile-queues"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    got_tq, want_tq = table_rows(r.stdout), table_rows((ROOT / "tests" / "data" / "tile_queue_table.txt").read_text())
    assert len(want_tq) >= 16 and all(len(row) == 5 and row[0] == "tq" for row in want_tq)
    assert got_tq == want_tq, [(g, w) for g, w in zip(got_tq, want_tq) if g != w][:5]
