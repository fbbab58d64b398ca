"""CPU: the surface of hlmi_polish_q / hlmi_polish_reads_q.  The header's prototypes and rules with an unchanged
HLMI_ABI_VERSION; the binding's SYMBOLS entries and struct sizes against the header's field lists; the driver's and the polish
module's options; and hylight_amd/csrc/seq_scan.h - the reader that keeps qualities, the validation, the mean and the floor -
compiled with the plain host compiler into tests/capi/polish_qual_host_check.cpp's program, which holds it to literal answers;
the model (tests/polish_qual_model.py) then runs on the same texts."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import pytest

from hylight_amd import api, driver, polish

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "hylight_mi.h")
sys.path.insert(0, HERE)
import polish_qual_model as QM  # noqa: E402

CTYPE = {"int": C.c_int, "double": C.c_double, "uint64_t": C.c_uint64, "hlmi_polish_stats": api.PolishStats}


def struct_fields(text, name):
    """the field list of `typedef struct { ... } name;` -> [(field, C type name)]"""
    body = re.search(r"typedef struct \{((?:(?!typedef struct).)*?)\} " + name + ";", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        if decl.strip():
            typ, names = decl.split(None, 1)
            out += [(n.strip(), typ) for n in names.split(",")]
    return out


def test_header_prototypes_and_abi():
    text = open(HEADER).read()
    flat = re.sub(r"\s+", " ", text)
    assert ("int hlmi_polish_q(const char *contigs, const char *reads, const char *paf, const hlmi_polish_qopts *o, "
            "const char *out_fa, hlmi_polish_qstats *st);") in flat
    assert ("int hlmi_polish_reads_q(const char *contigs, const char *reads, const hlmi_ava_opts *ao, const hlmi_polish_qopts *po, "
            "const char *out_fa, hlmi_polish_qstats *st);") in flat
    assert "void hlmi_polish_qopts_default(hlmi_polish_qopts *o); /* 0, 0.0, 3, 1, 1, 10.0 */" in flat
    assert re.findall(r"#define HLMI_ABI_VERSION (\d+)", text) == ["7"] and api.ABI_VERSION == 7
    # the older calls keep their prototypes
    assert ("int hlmi_polish(const char *contigs, const char *reads, const char *paf, const hlmi_polish_opts *o, const char *out_fa, "
            "hlmi_polish_stats *st);") in flat
    for word in ("w = max(1, byte - 33)", "PARITY with racon UNPINNED", "rows_selected x 93 >= 2^32", "read[qe - 1 - i]"):
        assert word in flat


def test_symbols_and_struct_sizes():
    text = open(HEADER).read()
    opts, stats = struct_fields(text, "hlmi_polish_qopts"), struct_fields(text, "hlmi_polish_qstats")
    assert [(n, CTYPE[t]) for n, t in opts] == list(api.PolishQOpts._fields_)
    assert [(n, CTYPE[t]) for n, t in stats] == list(api.PolishQStats._fields_)
    assert [n for n, _ in opts] == ["min_len", "min_iden", "min_cov", "include_unpolished", "qual_weight", "min_avg_qual"]
    assert C.sizeof(api.PolishQOpts) == 40 and C.sizeof(api.PolishQStats) == C.sizeof(api.PolishStats) + 16
    assert api.SYMBOLS["hlmi_polish_qopts_default"] == (None, [C.POINTER(api.PolishQOpts)])
    assert api.SYMBOLS["hlmi_polish_q"] == (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(api.PolishQOpts), C.c_char_p,
                                                      C.POINTER(api.PolishQStats)])
    assert api.SYMBOLS["hlmi_polish_reads_q"] == (C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(api.AvaOpts), C.POINTER(api.PolishQOpts),
                                                            C.c_char_p, C.POINTER(api.PolishQStats)])
    # the older entries are what they were
    assert api.SYMBOLS["hlmi_polish"][1][3] == C.POINTER(api.PolishOpts) and api.SYMBOLS["hlmi_polish_reads"][1][3] == C.POINTER(api.PolishOpts)
    with pytest.raises(TypeError):
        api.polish("c.fa", "r.fa", "p.paf", "o.fa", qual_weight=1, window=500)


def test_driver_and_module_options(tmp_path):
    a = driver.build_parser().parse_args(["-l", "x.fq", "--polish_direct", "--polish_qual"])
    assert a.polish_qual and a.polish_min_avg_qual == 10.0
    a = driver.build_parser().parse_args(["-l", "x.fq", "--polish_native", "--polish_qual", "--polish_min_avg_qual", "7.5"])
    assert a.polish_min_avg_qual == 7.5
    assert not driver.build_parser().parse_args(["-l", "x.fq", "--polish_native"]).polish_qual
    with pytest.raises(SystemExit) as e:                     # given alone: refused before anything is read or written
        driver.main(["-l", str(tmp_path / "x.fq"), "-o", str(tmp_path / "out"), "--polish_qual"])
    assert "--polish_qual" in str(e.value) and "--polish_native" in str(e.value)
    assert not (tmp_path / "out").exists()
    p = polish.build_parser().parse_args(["--contigs", "c.fa", "--reads", "r.fq", "--out", "o.fa", "--qual_weight", "--min_avg_qual", "10"])
    assert p.qual_weight and p.min_avg_qual == 10.0
    p = polish.build_parser().parse_args(["--contigs", "c.fa", "--reads", "r.fq", "--out", "o.fa"])
    assert not p.qual_weight and p.min_avg_qual is None


def _model_facts(text, floor):
    """what polish_qual_host_check prints behind a case's text, from the model's functions"""
    recs = QM.parse_seqs_qual(text)
    has = "".join("0" if q is None else "1" for _, _, q in recs)
    names = ",".join(n.decode() for n, _, _ in recs)
    try:
        with_qual = QM.check_quals(recs)
    except QM.RefusedRecord as e:
        bad = [n for n, _, _ in recs].index(e.record)
        kind = 1 if "quality bytes" in str(e) else 2
        return f"bad={bad};kind={kind};with=0;low=-;has={has};names={names};quals=-"
    low = "-" if floor == 0.0 else "".join("1" if QM.is_low(s, q, floor) else "0" for _, s, q in recs)
    quals = b"".join(b"!" * len(s) if q is None else q for _, s, q in recs)
    return f"bad=-1;kind=0;with={with_qual};low={low};has={has};names={names};quals={quals.hex()}"


@pytest.mark.parametrize("sanitize", [False, True])
def test_reader_and_floor_host_program(sanitize, tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler on PATH")
    exe = tmp_path / "polish_qual_host_check"
    flags = ["-std=c++17", "-O1"] + (["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else [])
    subprocess.run([cxx, *flags, os.path.join(ROOT, "tests", "capi", "polish_qual_host_check.cpp"), "-o", str(exe)], check=True, cwd=ROOT)
    r = subprocess.run([str(exe), "--facts"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "polish_qual_host_check: ok" in r.stdout
    lines = [l.split("\t") for l in r.stdout.splitlines() if "\t" in l]
    assert len(lines) >= 12
    seen = set()
    for name, text_hex, floor, facts in lines:
        assert facts == _model_facts(bytes.fromhex(text_hex), float.fromhex(floor)), name
        seen.add(name)
    assert {"multi_line", "crlf", "plus_name_line", "quality_begins_with_at_or_gt", "truncated_at_end_of_file", "byte_32", "byte_127",
            "fasta_between_fastq", "mean_exactly_the_floor", "mean_one_step_below_the_floor"} <= seen
