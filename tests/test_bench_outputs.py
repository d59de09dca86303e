"""bench.py's plain run and --dump-outputs: the line of a run without --full carries the contract's fields and none of the
side blocks, and the dump holds the state the timed steps left -- every array of the model, rows of a large side sampled
the same way every time, under 64 MB in all."""
import importlib.util
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


def _bench():
    spec = importlib.util.spec_from_file_location("bench_module", ROOT / "bench.py")
    m = importlib.util.module_from_spec(spec)
    sys.modules["bench_module"] = m
    spec.loader.exec_module(m)
    return m


class _Handle:
    """what dump_outputs reads of a handle, on the CPU: the library's state shapes, each array filled with its index"""

    def __init__(self, n, m, K, hier, bias):
        self.n_users, self.n_items, self.K, self.hier, self.bias = n, m, K, hier, bias

    def state_shape(self, which):
        from hgaprec_amd.capi import Hpf
        return Hpf.state_shape(self, which)

    def get_state_device(self, which):
        import torch
        from hgaprec_amd.capi import STATE
        shp = self.state_shape(which)
        return torch.arange(int(np.prod(shp)), dtype=torch.float64).reshape(shp) + 1000.0 * STATE[which]


@pytest.mark.parametrize("n,m,K,hier,bias", [(1_000_000, 100_000, 100, True, False),     # C2: both sides sampled
                                             (600, 400, 20, False, True)])              # small: every row
def test_dump_is_every_state_array_sampled_the_same_way_under_64_mb(tmp_path, n, m, K, hier, bias):
    b = _bench()
    from hgaprec_amd.capi import STATE
    runs = []
    for rep in range(2):
        d = tmp_path / f"run{rep}"
        b.dump_outputs(_Handle(n, m, K, hier, bias), dict(hier=hier, bias=bias), d)
        runs.append({p.name: np.load(p) for p in sorted(d.glob("*.npy"))})
        assert sum(p.stat().st_size for p in d.iterdir()) < 64_000_000
    objs = ["theta", "beta"] + (["xi", "eta"] if hier else []) + (["ubias", "ibias"] if bias else [])
    assert sorted(runs[0]) == sorted(f"{o}_{k}.npy" for o in objs for k in ("shape", "rate", "e", "elog"))
    for name, a in runs[0].items():
        assert a.dtype == np.float64 and np.array_equal(a, runs[1][name])
    # the same rows in every array of a side, and they are rows of the array (not a reshuffle of its elements)
    te = runs[0]["theta_e.npy"]
    rows = (te[:, 0] - 1000.0 * STATE["THETA_E"]) / K
    assert np.array_equal(rows, np.round(rows)) and np.all(np.diff(rows) > 0)
    assert np.array_equal(te, (rows[:, None] * K + np.arange(K)[None, :]) + 1000.0 * STATE["THETA_E"])
    assert np.array_equal((runs[0]["theta_shape.npy"][:, 0] - 1000.0 * STATE["THETA_SHAPE"]) / K, rows)
    if hier:
        assert np.array_equal(runs[0]["xi_e.npy"] - 1000.0 * STATE["XI_E"], rows)
    else:
        assert runs[0]["theta_rate.npy"].shape == (K,)             # one K-vector without -hier: written whole
    want_rows = n if n * K * 8 * 4 < b.DUMP_BYTES // 2 else None
    if want_rows:
        assert te.shape == (n, K)
    else:
        assert 1000 < te.shape[0] < n


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_what_they_computed(tmp_path):
    """no --full: the line has the contract's fields and the kernel times of the timed steps, no check or side block;
    --steps is the number of timed steps; the dump is the model's state after them"""
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1", "--scale", "0.01",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["metric"].startswith("rating-nonzeros/sec per CAVI iter") and d["unit"] == "rating-nonzeros/s"
    assert d["higher_is_better"] is True and d["dtype"] == "f64" and d["steps"] == 4 and d["warmup"] == 1
    assert d["ms_per_step"] > 0 and abs(d["value"] - d["config"]["nnz_total"] / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    assert d["kernels_ms"]["iteration_ms"] > 0
    for k in ("self_check", "cpu_baseline", "other_configs", "w48_opt_in", "replica_check", "rccl"):
        assert k not in d, k
    assert d["roofline"]["pmc"] is None and d["roofline"]["gather_only_ms"] is None
    files = {p.name: np.load(p) for p in out.glob("*.npy")}
    assert sorted(files) == sorted(f"{o}_{k}.npy" for o in ("theta", "beta", "xi", "eta") for k in ("shape", "rate", "e", "elog"))
    assert sum(p.stat().st_size for p in out.iterdir()) < 64_000_000
    K = 100
    assert files["theta_e.npy"].shape[1] == K and files["beta_e.npy"].shape == (1000, K)
    for name, a in files.items():
        assert a.dtype == np.float64 and np.all(np.isfinite(a)), name
    assert np.all(files["theta_e.npy"] > 0) and np.all(files["beta_shape.npy"] >= 0.3)
