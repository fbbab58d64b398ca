"""hylight_amd.min_ev against tables the reference's own min_ev_table.py wrote (tests/golden/min_ev_*.tsv, recorded by
tests/golden/make_goldens_min_ev.py with scipy's normal CDF): byte for byte, and build_threshold_table's reuse rule."""
import os

import pytest

from hylight_amd import min_ev

# name -> (readlen, insert_size, stddev, hcov), as in make_goldens_min_ev.py; intseg = insert_size - 2 * readlen
CASES = {
    "hylight": (150.0, 450.0, 27.0, 10.0),
    "len250": (250.0, 450.0, 27.0, 10.0),
    "len148_7": (148.7, 450.0, 27.0, 10.0),
    "negseg": (150.0, 250.0, 27.0, 10.0),
    "hcov3": (150.0, 450.0, 27.0, 3.0),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_table_matches_the_reference(name, golden, tmp_path):
    readlen, insert, stddev, hcov = CASES[name]
    out = tmp_path / min_ev.FILENAME
    assert min_ev.write(out, readlen, insert - 2 * readlen, stddev, hcov) is True
    want = golden.text(f"min_ev_{name}.tsv")
    assert out.read_text() == want
    rows = [tuple(int(x) for x in l.split("\t")) for l in want.splitlines() if l[0] != "#"]
    assert min_ev.table(readlen, insert - 2 * readlen, stddev, hcov) == rows
    assert [r[0] for r in rows] == list(range(1, len(rows) + 1))


def test_the_cases_cover_both_ends_of_the_loop(golden):
    """hcov3 and the others stop at the first exp_ev == 0 row, which is written; their distances and thresholds differ."""
    last = {n: golden.lines(f"min_ev_{n}.tsv")[-1].split("\t") for n in CASES}
    assert all(v[1] == "0" for v in last.values())
    assert int(last["hcov3"][0]) < int(last["hylight"][0]) < int(last["len250"][0])
    assert golden.lines("min_ev_len250.tsv")[2] == "# intseg -50.0"
    assert golden.lines("min_ev_len148_7.tsv")[1] == "# readlen 148.7"


def test_find_min_ev_leaves_out_m_equal_c():
    """range(m1, c): for c = 1 the sum is empty, so the threshold stays 1 whatever the error rate."""
    assert min_ev.find_min_ev(1, 1) == 1
    assert min_ev.find_min_ev(0, 1) == 1
    assert min_ev.find_min_ev(10, 1) == 3          # P(3 .. 9 errors of 10 at 1 %) = 1.1e-4 <= 1e-3 < P(2 .. 9) = 4.3e-3
    assert min_ev.choose(10, 3) == 120 and min_ev.choose(60, 30) == 118264581564861424


def test_reuse_rule(tmp_path):
    p = tmp_path / min_ev.FILENAME
    assert min_ev.write(p, 150.0, 150.0, 27.0, 3.0) is True
    p.write_text(p.read_text() + "# kept as it is\n")
    marked = p.read_text()
    assert min_ev.write(p, 150, 150, 27, 3) is False           # the same four values (ints compare equal): not rebuilt
    assert p.read_text() == marked
    assert min_ev.write(p, 150.0, 150.0, 27.0, 4.0) is True    # another hcov: rebuilt
    assert "# hcov 4.0\n" in p.read_text() and "kept as it is" not in p.read_text()
    assert min_ev.header_params(p) == {"readlen": 150.0, "intseg": 150.0, "stddev": 27.0, "hcov": 4.0}


def test_no_scipy_in_the_module():
    src = open(os.path.join(os.path.dirname(min_ev.__file__), "min_ev.py")).read().splitlines()
    imports = [l.strip() for l in src if l.strip().startswith(("import ", "from "))]
    assert imports and not any("scipy" in l for l in imports)
