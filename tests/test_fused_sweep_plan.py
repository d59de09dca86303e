"""CPU: which (side, layout, shape) runs the fused sweep epilogue -- hpf_plan::fused_sweep, has_phi_fused, has_sums.

`make -C hgaprec_amd/csrc plan` builds host/plan_selftest.cpp, a stand-alone program under ASan/UBSan.  Run as
`plan_selftest_asan fused-sweep` it walks every column count x w_storage (only the user side of p59 rows, only with the knob
on, only the shapes whose build keeps three waves per SIMD without scratch, never after the fall-back to plain doubles) and
prints, for the column counts of the benchmark's configurations and of tests/test_gpu_fused_sweep.py,
    fs C w_layout phi_G phi_R fused_user fused_item fused_user_under_HPF_FUSED_SWEEP=2
The default (knob 1) fuses only the shape measured to pay, (8, 6); the knob 2 every shape with an instance.
"""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "hgaprec_amd" / "csrc"

# K = 20: plain rows; 50: (4, 6), measured slower fused; 100: (8, 6) -- the benchmark's C2; 200: (16, 6), whose fused build spills; 800: 64 lanes
WANT = """
fs 20 0 4 5 0 0 0
fs 22 0 4 3 0 0 0
fs 50 3 4 6 0 0 1
fs 52 3 4 6 0 0 1
fs 100 3 8 6 1 0 1
fs 102 3 8 6 1 0 1
fs 200 3 16 6 0 0 0
fs 202 3 16 6 0 0 0
fs 800 3 64 6 0 0 0
"""


def test_fused_sweep_policy():
    r = subprocess.run(["make", "-C", str(CSRC), "plan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    env = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=1:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}
    r = subprocess.run([str(ROOT / "hgaprec_amd" / "plan_selftest_asan"), "fused-sweep"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    assert r.stdout.split() == WANT.split(), r.stdout
