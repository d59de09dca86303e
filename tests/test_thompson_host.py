"""No GPU: libhpf_hip.so exports hpf_sample_state and hpf_recommend_thompson and capi.py binds them with the header's
signatures; `-thompson D` / `-thompson-seed S` through the CLI's parser with their refusals; the writer of
recommend_thompson.tsv through the host library."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from hgaprec_amd import capi, hostlib

ROOT = Path(__file__).resolve().parent.parent
EXE = str(ROOT / "hgaprec_amd" / "hgaprec")
BASE = ["-dir", "x", "-n", "5", "-m", "5", "-k", "2"]


def test_binding_has_both_calls_once_with_their_argtypes():
    assert capi.EXPORTS.count("hpf_sample_state") == 1 and capi.EXPORTS.count("hpf_recommend_thompson") == 1
    assert callable(capi.Hpf.sample_state) and callable(capi.Hpf.recommend_thompson)
    for f in (capi.Hpf.sample_state, capi.Hpf.recommend_thompson):
        assert "(seed, draw)" in f.__doc__                                       # the contract is named where it is bound
    lib = capi.load_library()
    u32p, u64p, dp = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_double)
    assert lib.hpf_sample_state.argtypes == [C.c_void_p, C.c_int, u32p, C.c_uint32, C.c_uint64, C.c_uint32, dp]
    assert lib.hpf_recommend_thompson.argtypes == [C.c_void_p, u32p, C.c_uint32, u64p, u32p, C.c_uint32, C.c_uint64, C.c_uint32, u32p, dp]
    out = subprocess.run(["nm", "-D", "--defined-only", str(ROOT / "hgaprec_amd" / "libhpf_hip.so")], capture_output=True, text=True)
    assert out.returncode == 0 and " T hpf_sample_state" in out.stdout and " T hpf_recommend_thompson" in out.stdout
    # a null handle is refused before anything else
    assert lib.hpf_sample_state(None, 0, None, 0, 0, 0, None) == -1
    assert lib.hpf_recommend_thompson(None, None, 0, None, None, 10, 0, 0, None, None) == -1
    assert lib.hpf_abi_version() == 8                                            # new functions only
    assert "#define HPF_ABI_VERSION 8" in (ROOT / "include" / "hpf.h").read_text()


def test_the_header_declares_what_is_bound():
    text = re.sub(r"/\*.*?\*/", " ", (ROOT / "include" / "hpf.h").read_text(), flags=re.S)
    flat = " ".join(text.split())
    assert ("int hpf_sample_state(hpf_handle *h, int side, const uint32_t *ids, uint32_t n_sel, uint64_t seed, uint32_t draw, "
            "double *out );") in flat
    assert ("int hpf_recommend_thompson(hpf_handle *h, const uint32_t *users, uint32_t n_sel, const uint64_t *mask_ptr, "
            "const uint32_t *mask_items, uint32_t topn, uint64_t seed, uint32_t draw, uint32_t *out_items , double *out_scores );") in flat


# ---- the parser ------------------------------------------------------------------------------------------------------------
def test_parser_takes_d_and_seed_and_leaves_the_prefix_alone():
    assert hostlib.prefix(BASE + ["-recommend", "5", "-thompson", "3", "-thompson-seed", "5"]) == hostlib.prefix(BASE)   # a score mode: the same directory name
    for d in ("1", "3", "64"):
        hostlib.prefix(BASE + ["-recommend", "256", "-thompson", d])
    for s in ("0", "5", "20261021", "18446744073709551615"):
        hostlib.prefix(BASE + ["-recommend", "10", "-thompson", "2", "-thompson-seed", s])
    hostlib.prefix(BASE + ["-thompson-seed", "9", "-thompson", "2", "-recommend", "5"])           # in any order
    hostlib.prefix(BASE + ["-fold-in", "new.tsv", "-recommend", "5", "-thompson", "2", "-ucb", "1", "-explain", "3"])


@pytest.mark.parametrize("tail,msg", [
    (["-thompson", "2"], "-thompson goes with -recommend N: it recommends from D draws of the model from its posterior"),
    (["-recommend", "257", "-thompson", "2"], "-thompson needs -recommend N with N <= 256"),
    (["-recommend", "5", "-thompson", "0"], "-thompson needs the number of posterior draws per user, 1 .. 64"),
    (["-recommend", "5", "-thompson", "65"], "-thompson needs the number of posterior draws"),
    (["-recommend", "5", "-thompson", "-1"], "-thompson needs the number of posterior draws"),
    (["-recommend", "5", "-thompson", "2.5"], "-thompson needs the number of posterior draws"),
    (["-recommend", "5", "-thompson", "two"], "-thompson needs the number of posterior draws"),
    (["-recommend", "5", "-thompson"], "-thompson needs the number of posterior draws"),
    (["-audience", "5", "-thompson", "2"], "-thompson goes with -recommend N, not with -audience"),
    (["-fold-in-items", "f", "-audience", "5", "-thompson", "2"], "-thompson goes with -recommend N, not with -audience"),
    (["-recommend", "5", "-thompson-seed", "3"], "-thompson-seed goes with -thompson D"),
    (["-recommend", "5", "-thompson", "2", "-thompson-seed", "-1"], "-thompson-seed needs the seed of the draws"),
    (["-recommend", "5", "-thompson", "2", "-thompson-seed", "18446744073709551616"], "-thompson-seed needs the seed of the draws"),
    (["-recommend", "5", "-thompson", "2", "-thompson-seed", "1x"], "-thompson-seed needs the seed of the draws"),
    (["-recommend", "5", "-thompson", "2", "-thompson-seed"], "-thompson-seed needs the seed of the draws")])
def test_refusals_exit_before_anything_is_read(tail, msg):
    r = subprocess.run([EXE] + BASE + tail, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and msg in r.stderr, (r.returncode, r.stderr[-500:])


# ---- the writer ------------------------------------------------------------------------------------------------------------
def test_writer_orders_users_then_draws_then_rank(tmp_path):
    """user id, item id, draw, score: users in the order of the selection, within a user the draws ascending, each list
    best first; padding is never printed"""
    rng = np.random.default_rng(3)
    D, n_sel, N, m = 3, 4, 5, 4                                   # m < N: the last entry of every list is padding
    sel = np.array([2, 0, 3, 1], np.uint32)
    items = np.full((D, n_sel, N), 0xFFFFFFFF, np.uint32)
    for t in range(D):
        for b in range(n_sel):
            items[t, b, :m] = rng.permutation(m)
    scores = np.sort(rng.random((D, n_sel, N)), axis=2)[:, :, ::-1].copy()
    scores[:, :, m:] = 0.0
    uid, iid = np.array([10, 11, 12, 13], np.uint32), np.array([100, 101, 102, 103], np.uint32)
    path = tmp_path / "recommend_thompson.tsv"
    lines = hostlib.write_thompson(path, sel, items, scores, m, uid, iid)
    want = ["%d\t%d\t%d\t%.5f" % (uid[sel[b]], iid[items[t, b, j]], t, scores[t, b, j]) for b in range(n_sel) for t in range(D) for j in range(m)]
    assert lines == len(want) == D * n_sel * m and path.read_text().splitlines() == want
    # one draw: write_topn's lines with the draw's number in between
    p1, p0 = tmp_path / "one.tsv", tmp_path / "topn.tsv"
    assert hostlib.write_thompson(p1, sel, items[:1], scores[:1], m, uid, iid) == hostlib.write_topn(p0, sel, items[0], scores[0], m, uid, iid)
    assert [ln.split("\t")[:2] + ln.split("\t")[3:] for ln in p1.read_text().splitlines()] == [ln.split("\t") for ln in p0.read_text().splitlines()]
    with pytest.raises(ValueError):
        hostlib.write_thompson(p1, sel, items[0], scores[0], m, uid, iid)


def test_writer_leaves_out_given_items(tmp_path):
    """recommend.tsv's rule: an item the user has a training rating for is never printed"""
    n, m, D, N = 6, 8, 2, 8
    rng = np.random.default_rng(4)
    pairs = [(u, u % m, 3) for u in range(n)] + [(0, i, 2) for i in range(m)] + [(u, (3 * u + 1) % m, 4) for u in range(n)]
    (tmp_path / "train.tsv").write_text("".join(f"{u + 1}\t{i + 1}\t{y}\n" for u, i, y in pairs))
    rt = hostlib.Ratings(n, m)
    assert rt.read_train(tmp_path / "train.tsv") == 0
    dense = np.zeros((n, m), np.int64)
    for u, i, y in pairs:
        dense[u, i] = y
    sel = np.array([4, 0, 5], np.uint32)
    items = np.stack([np.stack([rng.permutation(m) for _ in sel]) for _ in range(D)]).astype(np.uint32)
    scores = np.sort(rng.random((D, sel.size, N)), axis=2)[:, :, ::-1].copy()
    uid, iid = rt.seq2user(), rt.seq2item()
    want = ["%d\t%d\t%d\t%.5f" % (uid[u], iid[items[t, b, j]], t, scores[t, b, j])
            for b, u in enumerate(sel) for t in range(D) for j in range(N) if dense[u, items[t, b, j]] == 0]
    path = tmp_path / "given.tsv"
    assert hostlib.write_thompson(path, sel, items, scores, m, uid, iid, rt) == len(want) < D * sel.size * N
    assert path.read_text().splitlines() == want
    assert not any(ln.startswith(f"{uid[0]}\t") for ln in want)       # user 0 was given every item
