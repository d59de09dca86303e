"""No GPU: libhpf_hip.so exports hpf_recommend_diverse and capi.py binds it with the header's signature; `-diverse L` /
`-diverse-pool P` through the CLI's parser with their refusals; the writer of recommend_diverse.tsv through the host
library."""
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


def test_binding_has_the_call_once_with_its_argtypes():
    assert capi.EXPORTS.count("hpf_recommend_diverse") == 1
    assert callable(capi.Hpf.recommend_diverse)
    doc = " ".join(capi.Hpf.recommend_diverse.__doc__.split())
    assert "lambda = 1 identity" in doc and "bit for bit" in doc                 # the identity is stated where it is bound
    lib = capi.load_library()
    u32p, u64p, dp = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_double)
    assert lib.hpf_recommend_diverse.argtypes == [C.c_void_p, u32p, C.c_uint32, u64p, u32p, C.c_uint32, C.c_uint32, C.c_double,
                                                  u32p, dp, dp, dp]
    out = subprocess.run(["nm", "-D", "--defined-only", str(ROOT / "hgaprec_amd" / "libhpf_hip.so")], capture_output=True, text=True)
    assert out.returncode == 0 and " T hpf_recommend_diverse" in out.stdout
    # a null handle is refused before anything else
    assert lib.hpf_recommend_diverse(None, None, 0, None, None, 10, 40, 0.7, None, None, None, None) == -1
    assert lib.hpf_abi_version() == 8                                            # a new function only
    text = (ROOT / "include" / "hpf.h").read_text()
    assert "#define HPF_ABI_VERSION 8" in text and "#define HPF_DIVERSE_POOL_MAX 256" in text
    assert capi.DIVERSE_POOL_MAX == 256


def test_the_header_declares_what_is_bound():
    text = re.sub(r"/\*.*?\*/", " ", (ROOT / "include" / "hpf.h").read_text(), flags=re.S)
    flat = " ".join(text.split())
    assert ("int hpf_recommend_diverse(hpf_handle *h, const uint32_t *users, uint32_t n_sel, const uint64_t *mask_ptr, "
            "const uint32_t *mask_items, uint32_t topn, uint32_t pool, double lambda, uint32_t *out_items , double *out_scores , "
            "double *out_maxsim , double *out_mmr );") in flat


_CTYPE = {"hpf_handle *": C.c_void_p, "const uint32_t *": C.POINTER(C.c_uint32), "uint32_t *": C.POINTER(C.c_uint32),
          "const uint64_t *": C.POINTER(C.c_uint64), "double *": C.POINTER(C.c_double), "uint32_t": C.c_uint32, "double": C.c_double}


def test_argtypes_are_derived_from_the_header():
    """the parameter list of the header's declaration, type by type, is what capi.py hands to ctypes"""
    text = re.sub(r"/\*.*?\*/", " ", (ROOT / "include" / "hpf.h").read_text(), flags=re.S)
    m = re.search(r"int\s+hpf_recommend_diverse\s*\(([^)]*)\)\s*;", text)
    assert m, "hpf.h declares hpf_recommend_diverse"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    types = [re.sub(r"\s*\w+$", "", p) for p in params]                                         # drop the parameter's name
    assert len(types) == 12 and all(t in _CTYPE for t in types), types
    assert capi.load_library().hpf_recommend_diverse.argtypes == [_CTYPE[t] for t in types]


# ---- the parser ------------------------------------------------------------------------------------------------------------
def test_parser_takes_l_and_pool_and_leaves_the_prefix_alone():
    assert hostlib.prefix(BASE + ["-recommend", "5", "-diverse", "0.7", "-diverse-pool", "20"]) == hostlib.prefix(BASE)   # a score mode: the same directory name
    for l in ("0", "1", "0.3", "1.0", "5e-1", "0.0"):
        hostlib.prefix(BASE + ["-recommend", "256", "-diverse", l])
    for n, p in (("1", "1"), ("10", "10"), ("10", "256"), ("256", "256"), ("100", "128")):
        hostlib.prefix(BASE + ["-recommend", n, "-diverse", "0.5", "-diverse-pool", p])
    hostlib.prefix(BASE + ["-diverse-pool", "30", "-diverse", "0.5", "-recommend", "5"])          # in any order
    hostlib.prefix(BASE + ["-fold-in", "new.tsv", "-recommend", "5", "-diverse", "0.5", "-ucb", "1", "-thompson", "2", "-explain", "3", "-because", "2"])


@pytest.mark.parametrize("tail,msg", [
    (["-diverse", "0.5"], "-diverse goes with -recommend N: it re-ranks the recommended items by relevance minus similarity to what is already picked"),
    (["-recommend", "257", "-diverse", "0.5"], "-diverse needs -recommend N with N <= 256"),
    (["-recommend", "5", "-diverse", "1.5"], "-diverse needs the weight of relevance against similarity, a number in [0, 1]"),
    (["-recommend", "5", "-diverse", "-0.1"], "-diverse needs the weight of relevance against similarity"),
    (["-recommend", "5", "-diverse", "nan"], "-diverse needs the weight of relevance against similarity"),
    (["-recommend", "5", "-diverse", "half"], "-diverse needs the weight of relevance against similarity"),
    (["-recommend", "5", "-diverse", "0.5x"], "-diverse needs the weight of relevance against similarity"),
    (["-recommend", "5", "-diverse"], "-diverse needs the weight of relevance against similarity"),
    (["-audience", "5", "-diverse", "0.5"], "-diverse goes with -recommend N, not with -audience"),
    (["-fold-in-items", "f", "-audience", "5", "-diverse", "0.5"], "-diverse goes with -recommend N, not with -audience"),
    (["-recommend", "5", "-diverse", "0.5", "-ngpus", "2"], "-diverse scores a saved model on one GPU: run it without -ngpus"),
    (["-recommend", "5", "-diverse-pool", "20"], "-diverse-pool goes with -diverse L"),
    (["-recommend", "5", "-diverse", "0.5", "-diverse-pool", "4"], "-diverse-pool needs the number of candidates per user, N .. 256"),
    (["-recommend", "5", "-diverse", "0.5", "-diverse-pool", "257"], "-diverse-pool needs the number of candidates per user, N .. 256"),
    (["-recommend", "5", "-diverse", "0.5", "-diverse-pool", "0"], "-diverse-pool needs the number of candidates per user"),
    (["-recommend", "5", "-diverse", "0.5", "-diverse-pool", "2.5"], "-diverse-pool needs the number of candidates per user"),
    (["-recommend", "5", "-diverse", "0.5", "-diverse-pool", "many"], "-diverse-pool needs the number of candidates per user"),
    (["-recommend", "5", "-diverse", "0.5", "-diverse-pool"], "-diverse-pool needs the number of candidates per user")])
def test_refusals_exit_before_anything_is_read(tail, msg):
    r = subprocess.run([EXE] + BASE + tail, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and msg in r.stderr, (r.returncode, r.stderr[-500:])


# ---- the writer ------------------------------------------------------------------------------------------------------------
def test_writer_prints_pick_order_without_padding(tmp_path):
    """user id, item id, score, maxsim: users in the order of the selection, each list in pick order (the scores are NOT
    descending) up to its first padding entry; the second value returned is the sum of the maxsim column"""
    PAD = 0xFFFFFFFF
    sel = np.array([2, 0, 3], np.uint32)
    items = np.array([[1, 3, 0, 2], [2, 0, PAD, PAD], [PAD, PAD, PAD, PAD]], np.uint32)
    scores = np.array([[4.0, 1.0, 2.0, 0.5], [0.75, 0.125, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]])
    maxsim = np.array([[0.0, 0.25, 1.0, 0.999996], [0.0, 0.5, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]])
    uid, iid = np.array([10, 11, 12, 13], np.uint32), np.array([100, 101, 102, 103], np.uint32)
    path = tmp_path / "recommend_diverse.tsv"
    lines, total = hostlib.write_diverse(path, sel, items, scores, maxsim, uid, iid)
    want = ["12\t101\t4.00000\t0.00000", "12\t103\t1.00000\t0.25000", "12\t100\t2.00000\t1.00000", "12\t102\t0.50000\t1.00000",
            "10\t102\t0.75000\t0.00000", "10\t100\t0.12500\t0.50000"]
    assert lines == 6 and path.read_text().splitlines() == want
    assert total == 0.0 + 0.25 + 1.0 + 0.999996 + 0.0 + 0.5
    with pytest.raises(ValueError):
        hostlib.write_diverse(path, sel, items[0], scores[0], maxsim[0], uid, iid)
    with pytest.raises(ValueError):
        hostlib.write_diverse(path, sel, items, scores, maxsim[:, :2], uid, iid)


def test_writer_leaves_out_given_items(tmp_path):
    """recommend.tsv's rule: an item the user has a training rating for is never printed"""
    n, m, N = 6, 8, 8
    rng = np.random.default_rng(4)
    pairs = [(u, u % m, 3) for u in range(n)] + [(0, i, 2) for i in range(m)] + [(u, (3 * u + 1) % m, 4) for u in range(n)]
    (tmp_path / "train.tsv").write_text("".join(f"{u + 1}\t{i + 1}\t{y}\n" for u, i, y in pairs))
    rt = hostlib.Ratings(n, m)
    assert rt.read_train(tmp_path / "train.tsv") == 0
    dense = np.zeros((n, m), np.int64)
    for u, i, y in pairs:
        dense[u, i] = y
    sel = np.array([4, 0, 5], np.uint32)
    items = np.stack([rng.permutation(m) for _ in sel]).astype(np.uint32)
    scores = rng.random((sel.size, N)) + 0.5
    maxsim = rng.random((sel.size, N))
    uid, iid = rt.seq2user(), rt.seq2item()
    want, wsum = [], 0.0
    for b, u in enumerate(sel):
        for j in range(N):
            if dense[u, items[b, j]] == 0:
                want.append("%d\t%d\t%.5f\t%.5f" % (uid[u], iid[items[b, j]], scores[b, j], maxsim[b, j]))
                wsum += maxsim[b, j]
    path = tmp_path / "given.tsv"
    lines, total = hostlib.write_diverse(path, sel, items, scores, maxsim, uid, iid, rt)
    assert 0 < lines == len(want) < sel.size * N and path.read_text().splitlines() == want
    assert total == wsum
    assert not any(ln.startswith(f"{uid[0]}\t") for ln in want)       # user 0 was given every item
