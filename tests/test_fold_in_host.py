"""No GPU: the reader of `-fold-in FILE` through hostlib (Ratings::read_fold_in), the CLI's parser for -fold-in /
-fold-iters / -fold-tol, and the hpf_fold_in symbol.

The reader's rules: FILE is read by the token rules of train.tsv against the items of the data set in -dir; users get
sequence numbers in order of first appearance; every copy of a duplicated pair carries the last rating; ratings the train
reader drops are dropped; lines whose item the data set does not know are skipped and counted.  A user ALL of whose lines
were skipped or dropped does not exist (the train reader registers a user at its first accepted record): it gets no
sequence number and no row.  An empty file is zero users and no error."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from hgaprec_amd import capi, hostlib

ROOT = Path(__file__).resolve().parent.parent
EXE = str(ROOT / "hgaprec_amd" / "hgaprec")
BASE = ["-dir", "x", "-n", "5", "-m", "5", "-k", "2"]


def model(tmp_path, binary=False, threshold=1):
    (tmp_path / "train.tsv").write_text("1\t70\t5\n1\t30\t4\n2\t90\t3\n2\t30\t1\n")
    r = hostlib.Ratings(10, 10, binary, threshold)
    assert r.read_train(tmp_path / "train.tsv") == 0 and r.m == 3
    assert list(r.seq2item()) == [70, 30, 90]
    return r


def fold(tmp_path, r, text):
    (tmp_path / "new.tsv").write_text(text)
    return r.read_fold_in(tmp_path / "new.tsv")


def test_first_appearance_duplicates_drops_and_unknown_items(tmp_path):
    r = model(tmp_path)
    f, skipped = fold(tmp_path, r, "50\t30\t2\n40\t70\t1\n50\t555\t5\n50\t30\t4\n60\t556\t1\n40\t90\t0\n50\t90\t300\n1\t90\t2\n")
    assert skipped == 2                                    # items 555 and 556
    assert f.n == 3 and f.m == 3 and list(f.seq2item()) == [70, 30, 90]
    assert list(f.seq2user()) == [50, 40, 1]               # first appearance; 60 had nothing but an unknown item: no such user
    rowptr, col, val = f.csr()
    assert list(rowptr) == [0, 3, 4, 5]
    assert list(col) == [1, 1, 2, 0, 2]                    # file order inside a row, both copies of the duplicated pair
    assert list(val) == [4, 4, 44, 1, 2]                   # the last rating on both; 300 wraps to 44; 40's rating 0 dropped
    assert col.dtype == np.uint32 and val.dtype == np.uint8 and rowptr.dtype == np.int64


def test_a_user_whose_lines_were_all_dropped_does_not_exist(tmp_path):
    r = model(tmp_path)
    f, skipped = fold(tmp_path, r, "9\t70\t0\n9\t999\t3\n8\t30\t1\n")
    assert skipped == 1 and f.n == 1 and list(f.seq2user()) == [8]
    assert list(f.csr()[0]) == [0, 1]


def test_binary_data_drops_below_the_threshold_and_stores_ones(tmp_path):
    r = model(tmp_path, binary=True, threshold=3)
    f, skipped = fold(tmp_path, r, "7\t70\t2\n7\t30\t3\n6\t90\t5\n6\t70\t1\n")
    assert skipped == 0 and list(f.seq2user()) == [7, 6]
    rowptr, col, val = f.csr()
    assert list(rowptr) == [0, 1, 2] and list(col) == [1, 2] and list(val) == [1, 1]


def test_empty_missing_and_malformed_files(tmp_path):
    r = model(tmp_path)
    f, skipped = fold(tmp_path, r, "")
    assert f is not None and skipped == 0 and f.n == 0 and f.nnz == 0 and list(f.csr()[0]) == [0]
    f, skipped = fold(tmp_path, r, "\n\n  \n")
    assert f is not None and f.n == 0
    assert r.read_fold_in(tmp_path / "does-not-exist.tsv") == (None, -1)
    assert fold(tmp_path, r, "5\t70\t1\nabc\t30\t1\n") == (None, -2)
    f, skipped = fold(tmp_path, r, "5  70 \t 1\n\n6\t30\t2")      # any white space separates fields; no trailing newline
    assert f.n == 2 and list(f.csr()[1]) == [0, 1]


def test_the_model_object_is_left_as_it_was(tmp_path):
    r = model(tmp_path)
    before = [a.copy() for a in r.csr()] + [r.seq2user(), r.seq2item()]
    fold(tmp_path, r, "50\t30\t2\n1\t70\t1\n")
    after = list(r.csr()) + [r.seq2user(), r.seq2item()]
    assert r.n == 2 and all(np.array_equal(a, b) for a, b in zip(before, after))


# ---- the CLI without a device ---------------------------------------------------------------------------------------
def test_parser_takes_fold_in_and_its_options():
    assert hostlib.prefix(BASE + ["-fold-in", "new.tsv"]) == hostlib.prefix(BASE)      # a score mode: the same directory name
    hostlib.prefix(BASE + ["-fold-in", "new.tsv", "-fold-iters", "5", "-fold-tol", "1e-4", "-recommend", "10"])


@pytest.mark.parametrize("tail,what", [(["-fold-in"], "-fold-in needs the file"), (["-fold-in", "-hier"], "-fold-in needs the file"),
                                       (["-fold-in", "f", "-fold-iters", "0"], "-fold-iters needs"),
                                       (["-fold-in", "f", "-fold-iters"], "-fold-iters needs"),
                                       (["-fold-in", "f", "-fold-tol", "-1"], "-fold-tol needs"),
                                       (["-fold-in", "f", "-fold-tol", "nan"], "-fold-tol needs")])
def test_usage_errors(tmp_path, tail, what):
    with pytest.raises(ValueError, match="-fold-"):
        hostlib.prefix(BASE + tail)
    r = subprocess.run([EXE] + BASE + tail, cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 2 and what in r.stderr and "unknown option" not in r.stdout
    assert not list(tmp_path.iterdir())                              # refused before the output directory exists


def test_cli_takes_fold_in_and_refuses_it_with_ngpus(tmp_path):
    base = [EXE, "-dir", str(tmp_path / "missing"), "-n", "5", "-m", "5", "-k", "2", "-fold-in", "new.tsv", "-fold-iters", "5"]
    r = subprocess.run(base, cwd=tmp_path, capture_output=True, text=True)
    assert "unknown option" not in r.stdout and "outside the MI355X hot-path build" not in r.stderr
    assert "ONE GPU" not in r.stderr and "-fold-iters needs" not in r.stderr           # accepted (fails later: no data)
    r = subprocess.run(base + ["-ngpus", "2", "-label", "two"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 1 and "-fold-in" in r.stderr and "ONE GPU" in r.stderr and "without -ngpus" in r.stderr
    assert not list(tmp_path.glob("*two*"))


def test_library_exports_hpf_fold_in():
    assert "hpf_fold_in" in capi.EXPORTS
    lib = capi.load_library()
    assert lib.hpf_fold_in.argtypes[1] is C.c_uint32 and lib.hpf_fold_in.argtypes[2] is C.c_double and len(lib.hpf_fold_in.argtypes) == 4
    out = subprocess.run(["nm", "-D", "--defined-only", str(ROOT / "hgaprec_amd" / "libhpf_hip.so")], capture_output=True, text=True)
    assert out.returncode == 0 and " T hpf_fold_in" in out.stdout
    assert lib.hpf_fold_in(None, 10, 0.0, None) == -1                # a null handle is refused before anything else
