"""No GPU: `-audience N` through the CLI's parser with its conflicts, the transposed mask lists (ItemMaskLists: the
validation users of a chunk of items) through the host library against a numpy regrouping, and the hpf_audience symbol."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from hgaprec_amd import capi, hostlib

ROOT = Path(__file__).resolve().parent.parent
EXE = str(ROOT / "hgaprec_amd" / "hgaprec")
BASE = ["-dir", "x", "-n", "5", "-m", "5", "-k", "2"]

AUDIENCE_N = "-audience needs the number of users per item, 1 .. 256"
AUDIENCE_ALONE = "-audience runs alone or behind -fold-in-items"
EXPLAIN_ALONE = "-explain goes with -recommend N: it explains the recommended items"
BECAUSE_ALONE = "-because goes with -recommend N: it traces the recommended items to the user's ratings"
FOLD_ITEMS_ALONE = "-fold-in-items runs alone: not with -fold-in and not with another score mode"


# ---- the binding -------------------------------------------------------------------------------------------------------
def test_binding_has_the_call_once_with_its_argtypes():
    assert capi.EXPORTS.count("hpf_audience") == 1 and callable(capi.Hpf.audience)
    lib = capi.load_library()
    u32p, u64p, dp = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_double)
    assert lib.hpf_audience.argtypes == [C.c_void_p, u32p, C.c_uint32, u64p, u32p, C.c_uint32, u32p, dp]
    out = subprocess.run(["nm", "-D", "--defined-only", str(ROOT / "hgaprec_amd" / "libhpf_hip.so")], capture_output=True, text=True)
    assert out.returncode == 0 and " T hpf_audience" in out.stdout
    assert lib.hpf_audience(None, None, 0, None, None, 10, None, None) == -1     # a null handle is refused before anything else
    assert lib.hpf_abi_version() == 8                                            # a new function only
    assert "#define HPF_ABI_VERSION 8" in (ROOT / "include" / "hpf.h").read_text()


# ---- the parser ------------------------------------------------------------------------------------------------------------
def test_parser_takes_the_count_and_leaves_the_prefix_alone():
    assert hostlib.prefix(BASE + ["-audience", "5"]) == hostlib.prefix(BASE)       # a score mode: the same directory name
    for n in ("1", "256"):
        hostlib.prefix(BASE + ["-audience", n])
    hostlib.prefix(BASE + ["-audience", "5", "-explain", "3"])
    hostlib.prefix(BASE + ["-explain", "3", "-audience", "5"])                     # in either order
    hostlib.prefix(BASE + ["-fold-in-items", "new.tsv", "-audience", "5"])
    hostlib.prefix(BASE + ["-audience", "5", "-fold-in-items", "new.tsv", "-explain", "3"])


OTHER_MODES = [["-fold-in", "users.tsv"], ["-recommend", "10"], ["-rmse"], ["-msr"], ["-eval-all"], ["-gen-ranking"],
               ["-similar-items", "5"], ["-similar-users", "5"], ["-topic-items", "5"], ["-topic-users", "5"]]


@pytest.mark.parametrize("tail,msg", [
    (["-audience", "0"], AUDIENCE_N),
    (["-audience", "257"], AUDIENCE_N),
    (["-audience", "5x"], AUDIENCE_N),
    (["-audience", "-hier"], AUDIENCE_N),
    (["-audience"], AUDIENCE_N)] +
    [(["-audience", "5"] + c, AUDIENCE_ALONE) for c in OTHER_MODES] +
    [(OTHER_MODES[0] + ["-audience", "5"], AUDIENCE_ALONE), (OTHER_MODES[1] + ["-explain", "2", "-audience", "5"], AUDIENCE_ALONE),
     # -fold-in-items keeps refusing what it refuses, -audience or not
     (["-fold-in-items", "f", "-audience", "5", "-recommend", "5"], FOLD_ITEMS_ALONE),
     (["-fold-in-items", "f", "-audience", "5", "-similar-items", "5"], FOLD_ITEMS_ALONE),
     # -explain without -recommend and without -audience: today's error, word for word
     (["-explain", "5"], EXPLAIN_ALONE),
     (["-explain", "5", "-topic-items", "5"], EXPLAIN_ALONE),
     (["-fold-in-items", "f", "-explain", "5"], EXPLAIN_ALONE),
     # -because is not offered for audiences
     (["-audience", "5", "-because", "3"], BECAUSE_ALONE)])
def test_cli_refuses_at_parse_time(tmp_path, tail, msg):
    with pytest.raises(ValueError):
        hostlib.prefix(BASE + tail)
    r = subprocess.run([EXE] + BASE + tail, cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 2 and "error: " + msg in r.stderr.splitlines() and "unknown option" not in r.stdout
    assert not list(tmp_path.iterdir())                              # refused before the output directory exists


def test_cli_takes_the_flag_and_refuses_it_with_ngpus(tmp_path):
    head = [EXE, "-dir", str(tmp_path / "missing"), "-n", "5", "-m", "5", "-k", "2"]
    for mode in (["-audience", "256"], ["-audience", "5", "-explain", "3"], ["-fold-in-items", "new.tsv", "-audience", "5"]):
        r = subprocess.run(head + mode, cwd=tmp_path, capture_output=True, text=True)
        assert r.returncode != 0
        assert "unknown option" not in r.stdout and "outside the MI355X hot-path build" not in r.stderr
        assert "ONE GPU" not in r.stderr and "needs the number" not in r.stderr and "runs alone" not in r.stderr   # accepted: fails later
    r = subprocess.run(head + ["-audience", "5", "-ngpus", "2", "-label", "two"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 1 and "ONE GPU" in r.stderr and "without -ngpus" in r.stderr
    assert not list(tmp_path.glob("*two*"))


def test_usage_text_names_the_flag(tmp_path):
    r = subprocess.run([EXE] + BASE + ["-nmf"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 2 and "-audience" in r.stderr and "outside the MI355X hot-path build" in r.stderr


# ---- the transposed mask lists ------------------------------------------------------------------------------------------
N_USERS, N_ITEMS = 41, 29


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """ids 1-based in the files, seq id == file id - 1; random held-out pairs; items 3, 11 and the last without one"""
    tmp = tmp_path_factory.mktemp("audience_host")
    g = np.random.default_rng(17)
    head = [(u, u % N_ITEMS, 3) for u in range(N_USERS)] + [(0, i, 2) for i in range(N_ITEMS)]
    pairs = sorted({(int(u), int(i)) for u, i in zip(g.integers(0, N_USERS, 200), g.integers(0, N_ITEMS, 200))
                    if i not in (3, 11, N_ITEMS - 1)})
    (tmp / "train.tsv").write_text("".join(f"{u + 1}\t{i + 1}\t{y}\n" for u, i, y in head))
    (tmp / "validation.tsv").write_text("".join(f"{u + 1}\t{i + 1}\t1\n" for u, i in pairs))
    rt = hostlib.Ratings(N_USERS, N_ITEMS)
    assert rt.read_train(tmp / "train.tsv") == 0 and rt.read_heldout(tmp / "validation.tsv", 0) == 0
    assert rt.n == N_USERS and rt.m == N_ITEMS
    assert (rt.seq2user() == np.arange(1, N_USERS + 1)).all() and (rt.seq2item() == np.arange(1, N_ITEMS + 1)).all()
    return rt, np.array(pairs, np.int64)


def _regroup(pairs, lo, hi):
    """numpy: the users of the pairs whose item is in [lo, hi), by item, ascending inside an item"""
    u, i = pairs[:, 0], pairs[:, 1]
    keep = (i >= lo) & (i < hi)
    o = np.lexsort((u[keep], i[keep]))
    ptr = np.concatenate([[0], np.cumsum(np.bincount(i[keep] - lo, minlength=hi - lo))])
    return np.arange(lo, hi), ptr, u[keep][o]


def test_item_mask_lists_are_the_pairs_regrouped_by_item(data):
    rt, pairs = data
    items, ptr, users = rt.item_mask_lists(0)
    wi, wp, wu = _regroup(pairs, 0, N_ITEMS)
    assert items.dtype == np.uint32 and ptr.dtype == np.uint64 and users.dtype == np.uint32
    assert items.tolist() == wi.tolist() and ptr.tolist() == wp.tolist() and users.tolist() == wu.tolist()
    assert users.size == len(pairs) and len(pairs) > 100
    for it in (3, 11, N_ITEMS - 1):                                   # an item without validation users
        assert ptr[it] == ptr[it + 1]
    for b in range(N_ITEMS):                                          # users stay ascending inside an item
        seg = users[int(ptr[b]):int(ptr[b + 1])]
        assert np.all(np.diff(seg.astype(np.int64)) > 0)
    assert max(np.diff(ptr.astype(np.int64))) > 3
    # nothing held out at all (the test pairs were never read)
    items, ptr, users = rt.item_mask_lists(1, 2, 6)
    assert items.tolist() == [2, 3, 4, 5] and ptr.tolist() == [0] * 5 and users.size == 0


@pytest.mark.parametrize("chunk", [1, 3, 4, 12, 64])
def test_item_mask_lists_across_chunk_boundaries(data, chunk):
    rt, pairs = data
    one_i, one_p, one_u = rt.item_mask_lists(0)
    cat_i, cat_p, cat_u = [], [0], []
    for i0, i1 in hostlib.chunk_walk(N_ITEMS, chunk):                 # chunk = 4: a boundary between items 3 and 4, 11 and 12
        items, ptr, users = rt.item_mask_lists(0, i0, i1)
        wi, wp, wu = _regroup(pairs, i0, i1)
        assert items.tolist() == wi.tolist() and ptr.tolist() == wp.tolist() and users.tolist() == wu.tolist()
        cat_p += [len(cat_u) + int(p) for p in ptr[1:]]
        cat_i += items.tolist()
        cat_u += users.tolist()
    assert cat_i == one_i.tolist() and cat_p == one_p.tolist() and cat_u == one_u.tolist()
    items, ptr, users = rt.item_mask_lists(0, 7, 7)                   # an empty range
    assert items.size == 0 and ptr.tolist() == [0] and users.size == 0
