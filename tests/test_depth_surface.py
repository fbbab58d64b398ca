"""CPU: the surface of hlmi_depth / hlmi_depth_reads.  The header's prototypes and rules with an unchanged HLMI_ABI_VERSION; the
binding's SYMBOLS entries and structs against the header's field lists; the depth module's and the driver's options; and
hylight_amd/csrc/depth_text.h - the records, the abundance, the TSV and bedGraph text - compiled with the plain host compiler into
tests/capi/depth_host_check.cpp's program under the address and undefined-behaviour sanitizers and run directly."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from hylight_amd import api, depth, driver

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "hylight_mi.h")


def _fields(text, name):
    body = re.search(r"typedef struct \{([^{}]*?)\} %s;" % name, text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [tuple(reversed(d.split())) for d in body.split(";") if d.strip()]


def test_header_prototypes_and_abi():
    text = open(HEADER).read()
    flat = re.sub(r"\s+", " ", text)
    assert ("int hlmi_depth(const char *contigs, const char *reads, const char *paf, const hlmi_depth_opts *o, const char *pairs_paf, "
            "const char *out_tsv, const char *out_bedgraph, hlmi_depth_stats *st);") in flat
    assert ("int hlmi_depth_reads(const char *contigs, const char *reads, const hlmi_ava_opts *ao, const hlmi_depth_opts *o, "
            "const char *pairs_paf, const char *out_tsv, const char *out_bedgraph, hlmi_depth_stats *st);") in flat
    assert "void hlmi_depth_opts_default(hlmi_depth_opts *o);" in flat
    assert re.findall(r"#define HLMI_ABI_VERSION (\d+)", text) == ["7"] and api.ABI_VERSION == 7
    # the polisher's calls keep their prototypes
    assert ("int hlmi_polish_pairs(const char *contigs, const char *reads, const char *paf, const hlmi_polish_qopts *o, "
            "const char *pairs_paf, const char *out_fa, hlmi_polish_pstats *st);") in flat
    rules = re.sub(r"\s+", " ", re.sub(r"\n \* ?", " ", text))            # the comment's lines joined
    for word in ("element (length - 1) / 2", "one double addition per contig", "A contig of 0 bases gets a row of zeros",
                 "a run never continues into the next contig", "the columns of its D ops included", "tests/depth_model.py",
                 "#contig\\tlength\\treads\\tbases\\tcovered\\tmean_depth\\tmedian_depth\\tabundance", "keyed by name"):
        assert word in rules, word


def test_symbols_and_structs():
    text = open(HEADER).read()
    ctype = {"uint64_t": C.c_uint64, "double": C.c_double, "int": C.c_int}
    assert [(n, ctype[t]) for n, t in _fields(text, "hlmi_depth_opts")] == list(api.DepthOpts._fields_)
    stats = _fields(text, "hlmi_depth_stats")
    assert [(n, ctype[t]) for n, t in stats] == list(api.DepthStats._fields_)
    assert tuple(n for n, t in stats if t == "uint64_t") == api.DEPTH_STATS
    assert api.DEPTH_STATS == ("rows", "rows_selected", "contigs", "contigs_covered", "positions", "covered", "bases", "runs",
                               "pairs_listed", "pairs_unknown", "rows_not_listed")
    assert C.sizeof(api.DepthStats) == 11 * 8 + 2 * 8 and C.sizeof(api.DepthOpts) == 16
    assert api.SYMBOLS["hlmi_depth_opts_default"] == (None, [C.POINTER(api.DepthOpts)])
    assert api.SYMBOLS["hlmi_depth"] == (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(api.DepthOpts), C.c_char_p, C.c_char_p,
                                                   C.c_char_p, C.POINTER(api.DepthStats)])
    assert api.SYMBOLS["hlmi_depth_reads"] == (C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(api.AvaOpts), C.POINTER(api.DepthOpts),
                                                         C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(api.DepthStats)])
    lib = api.load()
    assert lib.hlmi_depth is not None and lib.hlmi_depth_reads is not None
    o = api.DepthOpts(7, 0.5)
    lib.hlmi_depth_opts_default(C.byref(o))
    assert (o.min_len, o.min_iden) == (0, 0.0)
    with pytest.raises(TypeError):
        api.depth("c.fa", "r.fa", "p.paf", "o.tsv", min_cov=3)
    with pytest.raises(TypeError):
        api.depth_reads("c.fa", "r.fa", "o.tsv", window=500)


def test_module_and_driver_options():
    p = depth.build_parser().parse_args(["--contigs", "c.fa", "--reads", "r.fq", "--out", "d.tsv"])
    assert (p.paf, p.pairs, p.bedgraph, p.short, p.min_len, p.min_iden) == (None, None, None, False, 0, 0.0)
    p = depth.build_parser().parse_args(["--contigs", "c.fa", "--reads", "r.fq", "--paf", "p.paf", "--pairs", "l.paf", "--out", "d.tsv",
                                         "--bedgraph", "d.bg", "--min_len", "300", "--min_iden", "0.9"])
    assert (p.paf, p.pairs, p.bedgraph, p.min_len, p.min_iden) == ("p.paf", "l.paf", "d.bg", 300, 0.9)
    with pytest.raises(SystemExit):                          # --short is about the call that aligns
        depth.main(["--contigs", "c.fa", "--reads", "r.fq", "--paf", "p.paf", "--out", "d.tsv", "--short"])
    assert not driver.build_parser().parse_args(["-l", "x.fq"]).depth
    assert driver.build_parser().parse_args(["-l", "x.fq", "--depth"]).depth


def test_module_and_driver_hand_their_arguments_on(tmp_path, monkeypatch):
    seen = []
    monkeypatch.setattr(api, "depth", lambda *a, **k: seen.append(("depth", a, k)) or {})
    monkeypatch.setattr(api, "depth_reads", lambda *a, **k: seen.append(("depth_reads", a, k)) or {})
    assert depth.main(["--contigs", "c.fa", "--reads", "r.fq", "--paf", "p.paf", "--out", "d.tsv", "--pairs", "l.paf"]) == 0
    assert seen[-1] == ("depth", ("c.fa", "r.fq", "p.paf", "d.tsv", None), dict(pairs="l.paf", min_len=0, min_iden=0.0))
    assert depth.main(["--contigs", "c.fa", "--reads", "r.fq", "--out", "d.tsv", "--bedgraph", "d.bg", "--short", "--min_len", "70"]) == 0
    who, a, k = seen[-1]
    assert who == "depth_reads" and a[:4] == ("c.fa", "r.fq", "d.tsv", "d.bg") and k == dict(pairs=None, min_len=70, min_iden=0.0)
    short, long_ = api.ava_opts_short(), api.ava_opts_long()
    assert a[4].pair_once == 0 and a[4].k == short.k and a[4].w == short.w
    del seen[:]
    got = driver.depth_tables("final.fa", "long.fa", "short.fq", str(tmp_path))
    assert [(w, a[:2], os.path.basename(a[2]), os.path.basename(a[3])) for w, a, _ in seen] == [
        ("depth_reads", ("final.fa", "long.fa"), "final_contigs.long.depth.tsv", "final_contigs.long.depth.bedgraph"),
        ("depth_reads", ("final.fa", "short.fq"), "final_contigs.short.depth.tsv", "final_contigs.short.depth.bedgraph")]
    assert sorted(got) == ["long", "short"]
    assert [(a[4].pair_once, a[4].k == long_.k) for _, a, _ in seen] == [(0, True), (0, long_.k == short.k)]
    del seen[:]
    assert sorted(driver.depth_tables("final.fa", "long.fa", None, str(tmp_path))) == ["long"] and len(seen) == 1


def test_depth_text_host_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler on PATH")
    exe = tmp_path / "depth_host_check"
    flags = ["-std=c++17", "-O1", "-ffp-contract=off", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.run([cxx, *flags, os.path.join(ROOT, "tests", "capi", "depth_host_check.cpp"), "-o", str(exe)], check=True, cwd=ROOT)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "depth_host_check: ok" in r.stdout
