"""No GPU: `-recommend N` through the CLI's parser, the hpf_recommend symbol, and the binding's mirrors of the planner."""
import ctypes as C
import subprocess
from pathlib import Path

import pytest

from hgaprec_amd import capi, hostlib

ROOT = Path(__file__).resolve().parent.parent
EXE = str(ROOT / "hgaprec_amd" / "hgaprec")
CSRC = ROOT / "hgaprec_amd" / "csrc"
BASE = ["-dir", "x", "-n", "5", "-m", "5", "-k", "2"]


def _topn_grid_lines():
    r = subprocess.run(["make", "-C", str(CSRC), "plan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    r = subprocess.run([str(ROOT / "hgaprec_amd" / "plan_selftest_asan"), "topn-grid"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    return [ln.split() for ln in r.stdout.splitlines() if ln.startswith("tg ")]


def test_parser_takes_recommend_with_a_count():
    # a score mode changes nothing in the name of the output directory
    assert hostlib.prefix(BASE + ["-recommend", "100"]) == hostlib.prefix(BASE)
    for n in ("1", "256", "257", "1024"):
        hostlib.prefix(BASE + ["-recommend", n])


@pytest.mark.parametrize("tail", [["-recommend", "0"], ["-recommend", "1025"], ["-recommend"], ["-recommend", "-hier"],
                                  ["-recommend", "10x"], ["-recommend", "-3"]])
def test_parser_rejects_a_count_out_of_range_or_missing(tmp_path, tail):
    with pytest.raises(ValueError, match="-recommend"):
        hostlib.prefix(BASE + tail)
    r = subprocess.run([EXE] + BASE + tail, cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 2 and "-recommend needs the number of items per user, 1 .. 1024" in r.stderr
    assert not list(tmp_path.iterdir())                              # refused before the output directory exists


def test_cli_takes_recommend_and_refuses_it_with_ngpus(tmp_path):
    base = [EXE, "-dir", str(tmp_path / "missing"), "-n", "5", "-m", "5", "-k", "2", "-recommend", "100"]
    r = subprocess.run(base, cwd=tmp_path, capture_output=True, text=True)
    assert "unknown option" not in r.stdout and "outside the MI355X hot-path build" not in r.stderr
    assert "ONE GPU" not in r.stderr and "-recommend needs" not in r.stderr      # accepted (fails later: no data)
    r = subprocess.run(base + ["-ngpus", "2", "-label", "two"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 1 and "-recommend" in r.stderr and "ONE GPU" in r.stderr and "without -ngpus" in r.stderr
    assert not list(tmp_path.glob("*two*"))


def test_library_exports_hpf_recommend():
    assert "hpf_recommend" in capi.EXPORTS
    lib = capi.load_library()
    assert getattr(lib, "hpf_recommend") is not None
    assert lib.hpf_recommend.argtypes[5] is C.c_uint32 and len(lib.hpf_recommend.argtypes) == 8
    out = subprocess.run(["nm", "-D", "--defined-only", str(ROOT / "hgaprec_amd" / "libhpf_hip.so")], capture_output=True, text=True)
    assert out.returncode == 0 and " T hpf_recommend" in out.stdout and " T hpf_rank_topn" in out.stdout
    # a null handle is refused before anything else is looked at
    assert lib.hpf_recommend(None, None, 0, None, None, 10, None, None) == -1


def test_binding_mirrors_the_planner():
    lines = _topn_grid_lines()
    assert len(lines) >= 12
    fused = {int(l[4]): int(l[5]) for l in lines}                    # topn -> fused
    assert fused[capi.RECOMMEND_FUSED_MAX] == 1 and fused[capi.RECOMMEND_FUSED_MAX + 1] == 0
    assert all(f == (t <= capi.RECOMMEND_FUSED_MAX) for t, f in fused.items())
    for _, cid, m, n_sel, topn, f, cap, batch, blocks, splits, tps, nbytes in lines:
        m, topn, cap, batch, blocks, splits, tps = (int(x) for x in (m, topn, cap, batch, blocks, splits, tps))
        assert capi.recommend_cap(topn) == cap, cid
        assert capi.recommend_grid(batch, m, topn) == (blocks, splits, tps), cid
