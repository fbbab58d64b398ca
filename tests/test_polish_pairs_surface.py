"""CPU: the surface of hlmi_polish_pairs / hlmi_polish_reads_pairs.  The header's prototypes and rules with an unchanged
HLMI_ABI_VERSION; the binding's SYMBOLS entries and struct sizes against the header's field lists; the driver's and the polish
module's options; and hylight_amd/csrc/pair_list.h - the list scan and the pair set - compiled with the plain host compiler into
tests/capi/polish_pairs_host_check.cpp's program, plain and under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from hylight_amd import api, driver, polish

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "hylight_mi.h")


def test_header_prototypes_and_abi():
    text = open(HEADER).read()
    flat = re.sub(r"\s+", " ", text)
    assert ("int hlmi_polish_pairs(const char *contigs, const char *reads, const char *paf, const hlmi_polish_qopts *o, "
            "const char *pairs_paf, const char *out_fa, hlmi_polish_pstats *st);") in flat
    assert ("int hlmi_polish_reads_pairs(const char *contigs, const char *reads, const hlmi_ava_opts *ao, const hlmi_polish_qopts *po, "
            "const char *pairs_paf, const char *out_fa, hlmi_polish_pstats *st);") in flat
    assert re.findall(r"#define HLMI_ABI_VERSION (\d+)", text) == ["7"] and api.ABI_VERSION == 7
    # the older calls keep their prototypes
    assert ("int hlmi_polish_q(const char *contigs, const char *reads, const char *paf, const hlmi_polish_qopts *o, "
            "const char *out_fa, hlmi_polish_qstats *st);") in flat
    rules = re.sub(r"\s+", " ", re.sub(r"\n \* ?", " ", text))            # the comment's lines joined
    for word in ("pairs_paf == NULL", "only fields 1 and 6 are read", "fewer than 6 fields", "or to (t, q)", "claims nothing",
                 "tests/polish_pairs_model.py"):
        assert word in rules, word


def test_symbols_and_struct_sizes():
    text = open(HEADER).read()
    body = re.search(r"typedef struct \{([^{}]*?)\} hlmi_polish_pstats;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [tuple(reversed(d.split())) for d in body.split(";") if d.strip()]
    ctype = {"hlmi_polish_qstats": api.PolishQStats, "uint64_t": C.c_uint64}
    assert [(n, ctype[t]) for n, t in fields] == list(api.PolishPStats._fields_)
    assert [n for n, _ in fields] == ["q", "pairs_listed", "pairs_unknown", "rows_not_listed"]
    assert C.sizeof(api.PolishPStats) == C.sizeof(api.PolishQStats) + 24
    assert api.SYMBOLS["hlmi_polish_pairs"] == (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(api.PolishQOpts), C.c_char_p,
                                                          C.c_char_p, C.POINTER(api.PolishPStats)])
    assert api.SYMBOLS["hlmi_polish_reads_pairs"] == (C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(api.AvaOpts), C.POINTER(api.PolishQOpts),
                                                                C.c_char_p, C.c_char_p, C.POINTER(api.PolishPStats)])
    lib = api.load()
    assert lib.hlmi_polish_pairs is not None and lib.hlmi_polish_reads_pairs is not None
    # the older entries are what they were
    assert api.SYMBOLS["hlmi_polish_q"][1][5] == C.POINTER(api.PolishQStats) and len(api.SYMBOLS["hlmi_polish_reads_q"][1]) == 6
    with pytest.raises(TypeError):
        api.polish("c.fa", "r.fa", "p.paf", "o.fa", pairs="l.paf", window=500)
    with pytest.raises(TypeError):
        api.polish_reads("c.fa", "r.fa", "o.fa", None, pairs="l.paf", window=500)


def test_driver_and_module_options(tmp_path):
    a = driver.build_parser().parse_args(["-l", "x.fq", "--polish_direct", "--polish_strain"])
    assert a.polish_strain and a.polish_direct
    assert driver.build_parser().parse_args(["-l", "x.fq", "--polish_native", "--polish_strain", "--polish_qual"]).polish_strain
    assert not driver.build_parser().parse_args(["-l", "x.fq", "--polish_native"]).polish_strain
    with pytest.raises(SystemExit) as e:                     # given alone: refused before anything is read or written
        driver.main(["-l", str(tmp_path / "x.fq"), "-o", str(tmp_path / "out"), "--polish_strain"])
    assert "--polish_strain" in str(e.value) and "--polish_native" in str(e.value) and "--polish_direct" in str(e.value)
    assert not (tmp_path / "out").exists()
    p = polish.build_parser().parse_args(["--contigs", "c.fa", "--reads", "r.fq", "--out", "o.fa", "--pairs", "ov_long_ref.paf"])
    assert p.pairs == "ov_long_ref.paf"
    assert polish.build_parser().parse_args(["--contigs", "c.fa", "--reads", "r.fq", "--out", "o.fa"]).pairs is None


def test_polish_native_hands_the_list_on(tmp_path, monkeypatch):
    """driver.polish_native: `pairs` reaches api.polish / api.polish_reads as the keyword, and is absent without it"""
    seen = []
    monkeypatch.setattr(api, "ava", lambda *a, **k: None)
    monkeypatch.setattr(api, "polish", lambda *a, **k: seen.append(("polish", k)) or {})
    monkeypatch.setattr(api, "polish_reads", lambda *a, **k: seen.append(("polish_reads", k)) or {})
    driver.polish_native(1, "r.fa", "c.fa", str(tmp_path / "o.fa"), str(tmp_path), 3000, 0.95, pairs="ov.paf")
    driver.polish_native(1, "r.fa", "c.fa", str(tmp_path / "o.fa"), str(tmp_path), 3000, 0.95, direct=True, pairs="ov.paf")
    driver.polish_native(1, "r.fa", "c.fa", str(tmp_path / "o.fa"), str(tmp_path), 3000, 0.95, direct=True)
    assert [(w, k.get("pairs")) for w, k in seen] == [("polish", "ov.paf"), ("polish_reads", "ov.paf"), ("polish_reads", None)]
    assert "pairs" not in seen[2][1]


@pytest.mark.parametrize("sanitize", [False, True])
def test_list_scan_host_program(sanitize, tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler on PATH")
    exe = tmp_path / "polish_pairs_host_check"
    flags = ["-std=c++17", "-O1"] + (["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else [])
    subprocess.run([cxx, *flags, os.path.join(ROOT, "tests", "capi", "polish_pairs_host_check.cpp"), "-o", str(exe)], check=True, cwd=ROOT)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "polish_pairs_host_check: ok" in r.stdout
