"""The model reader (hostlib.load_matrix / load_vector): the inverse of the factor TSV writers with the
reference's reading rules (strtod per field, seq and id skipped as values, rows in line order, lines beyond
the expected count ignored) and its deliberate strictness: a missing file, a short file, a short row and an
id column that is not the ratings' are errors that name the file and the line."""
import numpy as np
import pytest

from hgaprec_amd import hostlib


def _values(rows, cols, seed):
    rng = np.random.default_rng(seed)
    a = rng.gamma(0.3, 1.0, size=(rows, cols)) + 1e-3
    flat = a.reshape(-1)
    special = [0.0, 1.0, 3.3e-8, 1.2345678e-8, 4.9e-9, 123456.78901234, 99999.999999995]
    for j, v in enumerate(special[: flat.size]):
        flat[(7 * j) % flat.size] = v
    return a


def _fields(path):
    """float(field) of every printed value field, per line"""
    return [[float(x) for x in l.split("\t")[2:]] for l in path.read_text().splitlines()]


@pytest.mark.parametrize("rows,cols", [(1, 1), (7, 5), (300, 100)])
def test_load_matrix_returns_the_printed_fields(tmp_path, rows, cols):
    a = _values(rows, cols, seed=rows)
    ids = (np.random.default_rng(1).permutation(10 * rows)[:rows] + 1).astype(np.uint32)
    p = tmp_path / "htheta.tsv"
    assert hostlib.save_matrix(p, a, ids) == 0
    want = np.array(_fields(p))
    got = hostlib.load_matrix(p, rows, cols, ids)
    assert got.shape == (rows, cols) and got.dtype == np.float64
    assert np.array_equal(got, want)
    assert np.array_equal(hostlib.load_matrix(p, rows, cols), want)          # ids=None: the column is not compared
    assert np.max(np.abs(got - a)) <= 5e-9 + 1e-16                           # and that is the matrix, to %.8f


def test_load_vector_and_one_column_matrix(tmp_path):
    n = 211
    v = _values(n, 1, seed=5)
    ids = (np.arange(n) * 3 + 11).astype(np.uint32)
    pv, pm = tmp_path / "thetarate.tsv", tmp_path / "thetabias.tsv"
    assert hostlib.save_vector(pv, v[:, 0], ids) == 0
    assert hostlib.save_matrix(pm, v, ids) == 0                              # an n x 1 bias object
    want = np.array(_fields(pv))[:, 0]
    assert np.array_equal(hostlib.load_vector(pv, n, ids), want)
    assert np.array_equal(hostlib.load_vector(pm, n, ids), want)
    assert np.array_equal(hostlib.load_matrix(pm, n, 1, ids)[:, 0], want)


def test_trailing_lines_and_missing_final_newline(tmp_path):
    a = _values(9, 4, seed=2)
    p = tmp_path / "hbeta.tsv"
    hostlib.save_matrix(p, a)
    want = np.array(_fields(p))
    with open(p, "a") as f:
        f.write("9\t9\tnot a number at all\n\n10\t10\t1.0\n")                # beyond the 9 rows: never looked at
    assert np.array_equal(hostlib.load_matrix(p, 9, 4, np.arange(9)), want)
    assert np.array_equal(hostlib.load_matrix(p, 4, 4), want[:4])            # fewer rows asked for than written
    p.write_text(p.read_text().split("\n9\t9\t")[0])                         # the last row now ends without '\n'
    assert np.array_equal(hostlib.load_matrix(p, 9, 4), want)


def test_pieces_on_threads_give_the_same_matrix(tmp_path, monkeypatch):
    a = _values(300, 100, seed=8)
    ids = np.arange(300, dtype=np.uint32) + 1000
    p = tmp_path / "htheta.tsv"
    hostlib.save_matrix(p, a, ids)
    one = hostlib.load_matrix(p, 300, 100, ids)
    monkeypatch.setenv("HGAPREC_READ_PARALLEL_MIN", "1")
    monkeypatch.setenv("HGAPREC_READ_THREADS", "7")
    assert np.array_equal(hostlib.load_matrix(p, 300, 100, ids), one)
    lines = p.read_text().splitlines()
    lines[211] = "\t".join(lines[211].split("\t")[:50])                      # a short row in a later piece ...
    lines[97] = "97\t5\t" + "\t".join(lines[97].split("\t")[2:])             # ... and a wrong id in an earlier one
    p.write_text("\n".join(lines) + "\n")
    with pytest.raises(ValueError) as e:
        hostlib.load_matrix(p, 300, 100, ids)
    assert "htheta.tsv: line 98:" in str(e.value) and "id 5" in str(e.value) and "1097" in str(e.value)   # the first in file order
    with pytest.raises(ValueError) as e:
        hostlib.load_matrix(p, 300, 100)
    assert "htheta.tsv: line 212:" in str(e.value) and "48 values where 100" in str(e.value)


def test_errors_name_file_and_line(tmp_path):
    a = _values(7, 5, seed=3)
    ids = np.array([5, 9, 2, 77, 1, 30, 4], np.uint32)
    p = tmp_path / "hbeta.tsv"
    hostlib.save_matrix(p, a, ids)
    with pytest.raises(ValueError) as e:
        hostlib.load_matrix(tmp_path / "absent.tsv", 7, 5, ids)
    assert "absent.tsv" in str(e.value) and "cannot open" in str(e.value)
    with pytest.raises(ValueError) as e:                                     # a file with fewer rows than the model
        hostlib.load_matrix(p, 8, 5)
    assert "hbeta.tsv" in str(e.value) and "7 rows where the model has 8" in str(e.value)
    with pytest.raises(ValueError) as e:                                     # a row with fewer than K values
        hostlib.load_matrix(p, 7, 6)
    assert "hbeta.tsv: line 1:" in str(e.value) and "5 values where 6" in str(e.value)
    wrong = ids.copy()
    wrong[3] = 78
    with pytest.raises(ValueError) as e:                                     # the model of another data set
        hostlib.load_matrix(p, 7, 5, wrong)
    assert "hbeta.tsv: line 4:" in str(e.value) and "id 77" in str(e.value) and "78" in str(e.value)
    with pytest.raises(ValueError) as e:
        hostlib.load_vector(p, 7, wrong)
    assert "hbeta.tsv: line 4:" in str(e.value)
    (tmp_path / "empty.tsv").write_text("")
    with pytest.raises(ValueError) as e:
        hostlib.load_vector(tmp_path / "empty.tsv", 1)
    assert "empty.tsv" in str(e.value) and "0 rows" in str(e.value)
    lines = p.read_text().splitlines()
    lines[2] = ""                                                            # the reference would keep a row of zeros
    p.write_text("\n".join(lines) + "\n")
    with pytest.raises(ValueError) as e:
        hostlib.load_matrix(p, 7, 5)
    assert "hbeta.tsv: line 3:" in str(e.value) and "0 values where 5" in str(e.value)
    for blank in ("\f", "\v \f", "2\t2\t\v"):                                # white space strtod would skip across the '\n':
        lines[2] = blank                                                     # the row must not borrow the next line's fields
        p.write_text("\n".join(lines) + "\n")
        with pytest.raises(ValueError) as e:
            hostlib.load_matrix(p, 7, 5)
        assert "hbeta.tsv: line 3:" in str(e.value) and "0 values where 5" in str(e.value)


def test_non_hier_expectation_is_shape_over_rate(tmp_path):
    """without -hier the model is theta_shape.tsv (n x K) and theta_rate.tsv (a K-vector whose id column is
    seq2id[k]): E = shape / rate[k], as GPMatrixGR::load -> compute_expectations"""
    n, K = 23, 6
    shape = _values(n, K, seed=4) + 0.3
    rate = np.random.default_rng(6).gamma(2.0, 1.0, K) + 0.3
    ids = (np.arange(n) + 500).astype(np.uint32)
    hostlib.save_matrix(tmp_path / "theta_shape.tsv", shape, ids)
    hostlib.save_vector(tmp_path / "theta_rate.tsv", rate, ids)
    s = hostlib.load_matrix(tmp_path / "theta_shape.tsv", n, K, ids)
    r = hostlib.load_vector(tmp_path / "theta_rate.tsv", K)
    assert np.array_equal(r, np.array(_fields(tmp_path / "theta_rate.tsv"))[:, 0])
    E = s / r[None, :]
    assert np.max(np.abs(E - shape / rate[None, :]) / (shape / rate[None, :])) < 1e-6


# ---- the domain: every model file holds parameters or expectations of a Gamma (finite, >= 0) ----
BAD_VALUES = ["-1", "nan", "inf", "-inf"]
ROWS, COLS = 40, 3                                                            # ~1.2 kB: several pieces when threaded


def _domain_file(p, bad, at):
    """ROWS x COLS proper values with `bad` in the middle column of 0-based line `at` AND of the last line, which
    ends without a newline; the first bad line in file order is the one to be reported"""
    lines = []
    for r in range(ROWS):
        mid = bad if r in (at, ROWS - 1) else "0.25000000"
        lines.append(f"{r}\t{r + 100}\t0.50000000\t{mid}\t1.00000000")
    p.write_text("\n".join(lines))


@pytest.mark.parametrize("threaded", [False, True])
@pytest.mark.parametrize("at", [0, ROWS // 2, ROWS - 1], ids=["first", "middle", "last-no-newline"])
@pytest.mark.parametrize("bad", BAD_VALUES)
def test_values_outside_the_gamma_domain_are_errors(tmp_path, monkeypatch, bad, at, threaded):
    if threaded:
        monkeypatch.setenv("HGAPREC_READ_PARALLEL_MIN", "0")
        monkeypatch.setenv("HGAPREC_READ_THREADS", "5")
    p = tmp_path / "hbeta.tsv"
    _domain_file(p, bad, at)
    ids = np.arange(ROWS, dtype=np.uint32) + 100
    with pytest.raises(ValueError) as e:
        hostlib.load_matrix(p, ROWS, COLS, ids)
    msg = str(e.value)
    assert f"hbeta.tsv: line {at + 1}:" in msg and "where a Gamma expectation (finite, >= 0) is expected" in msg
    assert f"value {bad}" in msg
    got = hostlib.load_matrix(p, ROWS, 1, ids)                                # the bad column is beyond `cols`: never a value
    assert np.array_equal(got, np.full((ROWS, 1), 0.5))
    if at < ROWS - 1:
        got = hostlib.load_matrix(p, at, COLS, ids)                           # ... and so are the lines beyond `rows`
        assert got.shape == (at, COLS)


@pytest.mark.parametrize("threaded", [False, True])
@pytest.mark.parametrize("at", [0, 3, 6], ids=["first", "middle", "last-no-newline"])
@pytest.mark.parametrize("bad", BAD_VALUES)
def test_bad_values_in_a_vector_file(tmp_path, monkeypatch, bad, at, threaded):
    if threaded:
        monkeypatch.setenv("HGAPREC_READ_PARALLEL_MIN", "0")
        monkeypatch.setenv("HGAPREC_READ_THREADS", "5")
    p = tmp_path / "betabias.tsv"
    p.write_text("\n".join(f"{r}\t{r}\t{bad if r == at else '0.12500000'}" for r in range(7)))
    with pytest.raises(ValueError) as e:
        hostlib.load_vector(p, 7)
    assert f"betabias.tsv: line {at + 1}:" in str(e.value) and "(finite, >= 0)" in str(e.value)


@pytest.mark.parametrize("threaded", [False, True])
def test_zero_negative_zero_and_subnormal_load(tmp_path, monkeypatch, threaded):
    if threaded:
        monkeypatch.setenv("HGAPREC_READ_PARALLEL_MIN", "0")
        monkeypatch.setenv("HGAPREC_READ_THREADS", "5")
    p = tmp_path / "hbeta.tsv"
    p.write_text("0\t7\t0\t-0.0\t1e-320\n1\t8\t1e-320\t0\t-0.0\n2\t9\t-0.0\t1e-320\t0")
    got = hostlib.load_matrix(p, 3, 3, np.array([7, 8, 9], np.uint32))
    want = np.array([[0.0, -0.0, 1e-320], [1e-320, 0.0, -0.0], [-0.0, 1e-320, 0.0]])
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))          # bit for bit: the sign of -0.0 is kept


@pytest.mark.parametrize("bad", ["0", "nan", "-0.0", "-1", "inf"])
@pytest.mark.parametrize("at", [0, 2, 5], ids=["first", "middle", "last-no-newline"])
def test_non_hier_rate_must_be_positive_and_finite(tmp_path, bad, at):
    """without -hier E = shape / rate[k]: a zero rate would make every such E infinite (or NaN) and rank the item
    first for every user.  nan, inf and -1 never get past the reader; 0 and -0.0 do, and are refused before the
    division.  Either way the message names the rate file and the line."""
    n, K = 9, 6
    shape = _values(n, K, seed=11) + 0.3
    hostlib.save_matrix(tmp_path / "beta_shape.tsv", shape)
    rp = tmp_path / "beta_rate.tsv"
    rp.write_text("\n".join(f"{k}\t{k}\t{bad if k == at else '1.50000000'}" for k in range(K)))
    s = hostlib.load_matrix(tmp_path / "beta_shape.tsv", n, K)
    with pytest.raises(ValueError) as e:
        hostlib.shape_over_rate(s, hostlib.load_vector(rp, K), rp)
    assert f"beta_rate.tsv: line {at + 1}:" in str(e.value)
    if bad in ("0", "-0.0"):
        assert "where a Gamma rate (finite, > 0) is expected" in str(e.value)
    else:
        assert "where a Gamma expectation (finite, >= 0) is expected" in str(e.value)
    rp.write_text("\n".join(f"{k}\t{k}\t1.50000000" for k in range(K)))
    E = hostlib.shape_over_rate(s, hostlib.load_vector(rp, K), rp)
    assert np.array_equal(E, s / 1.5)
    with pytest.raises(ValueError) as e:                                      # a quotient beyond the largest double
        hostlib.shape_over_rate(s, np.full(K, 1e-320), rp)
    assert "beta_rate.tsv: line 1:" in str(e.value) and "not finite" in str(e.value)
