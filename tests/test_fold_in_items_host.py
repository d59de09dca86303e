"""No GPU: the reader of `-fold-in-items FILE` through hostlib (Ratings::read_fold_in_items), the CLI's parser for the flag
and its conflicts, and the hpf_fold_in_items symbol.

The reader's rules: FILE is read by the token rules of train.tsv against the USERS of the data set in -dir; items get
sequence numbers in order of first appearance, their ids taken as given whether or not train.tsv knows them; every copy of a
duplicated pair carries the last rating; ratings the train reader drops are dropped; lines whose user the data set does not
know are skipped and counted.  An item ALL of whose lines were skipped or dropped does not exist.  The result holds m,
seq2item and a CSR over the data set's n users."""
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
    (tmp_path / "train.tsv").write_text("70\t1\t5\n30\t1\t4\n90\t2\t3\n30\t2\t1\n")
    r = hostlib.Ratings(10, 10, binary, threshold)
    assert r.read_train(tmp_path / "train.tsv") == 0 and r.n == 3
    assert list(r.seq2user()) == [70, 30, 90]
    return r


def fold(tmp_path, r, text):
    (tmp_path / "new.tsv").write_text(text)
    return r.read_fold_in_items(tmp_path / "new.tsv")


def test_first_appearance_duplicates_drops_and_unknown_users(tmp_path):
    r = model(tmp_path)
    f, skipped = fold(tmp_path, r, "30\t50\t2\n70\t40\t1\n555\t50\t5\n30\t50\t4\n556\t60\t1\n90\t40\t0\n90\t50\t300\n90\t1\t2\n")
    assert skipped == 2                                    # users 555 and 556
    assert f.n == 3 and list(f.seq2user()) == [70, 30, 90]
    assert f.m == 3 and list(f.seq2item()) == [50, 40, 1]  # first appearance; 60 had nothing but an unknown user; 1 is train.tsv's and new here
    rowptr, col, val = f.csr()
    assert list(rowptr) == [0, 1, 3, 5]                    # rows are the data set's users 70, 30, 90
    assert list(col) == [1, 0, 0, 0, 2]                    # file order inside a row, both copies of the duplicated pair
    assert list(val) == [1, 4, 4, 44, 2]                   # the last rating on both; 300 wraps to 44; 90's rating 0 dropped
    assert col.dtype == np.uint32 and val.dtype == np.uint8 and rowptr.dtype == np.int64


def test_an_item_whose_lines_were_all_dropped_does_not_exist(tmp_path):
    r = model(tmp_path)
    f, skipped = fold(tmp_path, r, "70\t9\t0\n999\t9\t3\n30\t8\t1\n")
    assert skipped == 1 and f.m == 1 and list(f.seq2item()) == [8]
    assert list(f.csr()[0]) == [0, 0, 1, 1] and list(f.csr()[1]) == [0]


def test_binary_data_drops_below_the_threshold_and_stores_ones(tmp_path):
    r = model(tmp_path, binary=True, threshold=3)
    f, skipped = fold(tmp_path, r, "70\t7\t2\n30\t7\t3\n90\t6\t5\n70\t6\t1\n")
    assert skipped == 0 and list(f.seq2item()) == [7, 6]
    rowptr, col, val = f.csr()
    assert list(rowptr) == [0, 0, 1, 2] and list(col) == [0, 1] and list(val) == [1, 1]


def test_empty_missing_and_malformed_files(tmp_path):
    r = model(tmp_path)
    f, skipped = fold(tmp_path, r, "")
    assert f is not None and skipped == 0 and f.m == 0 and f.n == 3 and f.nnz == 0 and list(f.csr()[0]) == [0, 0, 0, 0]
    f, skipped = fold(tmp_path, r, "\n\n  \n")
    assert f is not None and f.m == 0
    assert r.read_fold_in_items(tmp_path / "does-not-exist.tsv") == (None, -1)
    assert fold(tmp_path, r, "70\t5\t1\n30\tabc\t1\n") == (None, -2)
    f, skipped = fold(tmp_path, r, "70  5 \t 1\n\n30\t6\t2")       # any white space separates fields; no trailing newline
    assert f.m == 2 and list(f.csr()[1]) == [0, 1]


def test_the_model_object_is_left_as_it_was(tmp_path):
    r = model(tmp_path)
    before = [a.copy() for a in r.csr()] + [r.seq2user(), r.seq2item()]
    fold(tmp_path, r, "30\t50\t2\n70\t1\t1\n")
    after = list(r.csr()) + [r.seq2user(), r.seq2item()]
    assert r.m == 2 and all(np.array_equal(a, b) for a, b in zip(before, after))


# ---- the CLI without a device ---------------------------------------------------------------------------------------
def test_parser_takes_the_flag_and_its_options():
    assert hostlib.prefix(BASE + ["-fold-in-items", "new.tsv"]) == hostlib.prefix(BASE)   # a score mode: the same directory name
    hostlib.prefix(BASE + ["-fold-in-items", "new.tsv", "-fold-iters", "5", "-fold-tol", "1e-4"])


CONFLICTS = [["-fold-in", "users.tsv"], ["-recommend", "10"], ["-rmse"], ["-msr"], ["-eval-all"], ["-gen-ranking"],
             ["-similar-items", "5"], ["-similar-users", "5"], ["-topic-items", "5"], ["-topic-users", "5"]]


@pytest.mark.parametrize("tail,what", [(["-fold-in-items"], "-fold-in-items needs the file"),
                                       (["-fold-in-items", "-hier"], "-fold-in-items needs the file"),
                                       (["-fold-in-items", "f", "-fold-iters", "0"], "-fold-iters needs"),
                                       (["-fold-in-items", "f", "-fold-tol", "-1"], "-fold-tol needs")] +
                         [(["-fold-in-items", "f"] + c, "-fold-in-items runs alone") for c in CONFLICTS] +
                         [(CONFLICTS[0] + ["-fold-in-items", "f"], "-fold-in-items runs alone")])
def test_usage_errors_and_conflicts(tmp_path, tail, what):
    with pytest.raises(ValueError, match="-fold-"):
        hostlib.prefix(BASE + tail)
    r = subprocess.run([EXE] + BASE + tail, cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 2 and what in r.stderr and "unknown option" not in r.stdout
    assert not list(tmp_path.iterdir())                              # refused before the output directory exists


def test_cli_takes_the_flag_and_refuses_it_with_ngpus(tmp_path):
    base = [EXE, "-dir", str(tmp_path / "missing"), "-n", "5", "-m", "5", "-k", "2", "-fold-in-items", "new.tsv", "-fold-iters", "5"]
    r = subprocess.run(base, cwd=tmp_path, capture_output=True, text=True)
    assert "unknown option" not in r.stdout and "outside the MI355X hot-path build" not in r.stderr
    assert "ONE GPU" not in r.stderr and "-fold-iters needs" not in r.stderr           # accepted (fails later: no data)
    r = subprocess.run(base + ["-ngpus", "2", "-label", "two"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 1 and "-fold-in-items" in r.stderr and "ONE GPU" in r.stderr and "without -ngpus" in r.stderr
    assert not list(tmp_path.glob("*two*"))


def test_usage_text_names_the_flag(tmp_path):
    r = subprocess.run([EXE] + BASE + ["-nmf"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 2 and "-fold-in-items" in r.stderr and "outside the MI355X hot-path build" in r.stderr


def test_library_exports_hpf_fold_in_items():
    assert "hpf_fold_in_items" in capi.EXPORTS
    lib = capi.load_library()
    a = lib.hpf_fold_in_items.argtypes
    assert a[1] is C.c_uint32 and a[2] is C.c_double and len(a) == 4
    out = subprocess.run(["nm", "-D", "--defined-only", str(ROOT / "hgaprec_amd" / "libhpf_hip.so")], capture_output=True, text=True)
    assert out.returncode == 0 and " T hpf_fold_in_items" in out.stdout
    assert lib.hpf_fold_in_items(None, 10, 0.0, None) == -1          # a null handle is refused before anything else
    assert lib.hpf_abi_version() == 8                                # a new function only
