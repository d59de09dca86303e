"""CPU: the planner of hpf_recommend (topn_fused, topn_cap, topn_grid, topn_batch_users in hgaprec_amd/csrc/hpf_plan.hpp).

`make -C hgaprec_amd/csrc plan` builds host/plan_selftest.cpp, a stand-alone program under ASan/UBSan.  Its default run
checks, over a seeded sweep of item counts, selections, list lengths and HPF_LOO_BATCH values: no empty split; a split of
at least four candidate buffers' worth of items (cap / 16 tiles) or a single split; cap >= topn + 64; at most 512 MB of
candidate buffers per batch; batches a multiple of 64 users or the 16-rounded selection; and C2's arithmetic at topn = 100
(21 440 users x 4 splits x 256 entries x 12 B = 263 MB).  Run as `plan_selftest_asan topn-grid` it prints
    tg case-id m n_sel topn fused cap batch blocks splits tiles_per_split candidate-bytes
for a fixed list of cases, which must be tests/data/topn_grid_table.txt."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "hgaprec_amd" / "csrc"
ENV = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=1:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}


def _rows(text):
    return [tuple(ln.split()) for ln in text.splitlines() if ln.strip() and not ln.startswith("#")]


def _selftest(*args):
    r = subprocess.run(["make", "-C", str(CSRC), "plan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    r = subprocess.run([str(ROOT / "hgaprec_amd" / "plan_selftest_asan"), *args], capture_output=True, text=True, env=ENV, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "FAIL" not in r.stderr
    return r.stdout


def test_invariants_hold_and_the_default_output_is_unchanged():
    out = _selftest()
    assert "plan_selftest ok: 8192 points" in out
    assert not any(ln.startswith(("tg ", "tq ")) for ln in out.splitlines())


def test_recorded_grid_table():
    got = _rows(_selftest("topn-grid"))
    want = _rows((ROOT / "tests" / "data" / "topn_grid_table.txt").read_text())
    assert len(want) >= 16 and all(len(row) == 12 and row[0] == "tg" for row in want)
    assert got == want, [(g, w) for g, w in zip(got, want) if g != w][:5]
    by_id = {row[1]: [int(x) for x in row[2:]] for row in got}
    # C2 at topn = 100: 21 440 users x 4 splits x 256 entries x 12 B
    m, n_sel, topn, fused, cap, batch, blocks, splits, tps, nbytes = by_id["c2_top100"]
    assert (cap, batch, splits, tps) == (256, 21440, 4, 391) and nbytes == 21440 * 4 * 256 * 12 == 263454720
    for cid, (m, n_sel, topn, fused, cap, batch, blocks, splits, tps, nbytes) in by_id.items():
        ntiles = (m + 63) // 64
        assert cap >= topn + 64 and blocks == (batch + 63) // 64, cid
        assert splits * tps >= ntiles > (splits - 1) * tps, cid                       # every tile swept, no empty split
        assert tps >= cap // 16 or splits == 1, cid
        assert nbytes == batch * splits * cap * 12 <= 512 << 20, cid
        assert batch % 64 == 0 or batch == (n_sel + 15) // 16 * 16 or cid.endswith("knob16"), cid
