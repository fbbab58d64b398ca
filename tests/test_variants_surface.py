"""CPU: the surface of hlmi_variants / hlmi_variants_reads.  The header's prototypes and rules with an unchanged HLMI_ABI_VERSION;
the binding's SYMBOLS entries and structs against the header's field lists; the variants module's and the driver's options and
what they hand on; and hylight_amd/csrc/variants_text.h - the records, the alternative symbol, site_rate and both files' text -
compiled with the plain host compiler into tests/capi/variants_host_check.cpp's program under the address and undefined-behaviour
sanitizers and run directly."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from hylight_amd import api, driver, variants

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "hylight_mi.h")
DEFAULTS = dict(min_len=0, min_iden=0.0, min_cov=3, min_alt=2, min_frac=0.2)


def _fields(text, name):
    body = re.search(r"typedef struct \{([^{}]*?)\} %s;" % name, text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [tuple(reversed(d.split())) for d in body.split(";") if d.strip()]


def test_header_prototypes_and_abi():
    text = open(HEADER).read()
    flat = re.sub(r"\s+", " ", text)
    assert ("int hlmi_variants(const char *contigs, const char *reads, const char *paf, const hlmi_variant_opts *o, "
            "const char *pairs_paf, const char *out_sites, const char *out_summary, hlmi_variant_stats *st);") in flat
    assert ("int hlmi_variants_reads(const char *contigs, const char *reads, const hlmi_ava_opts *ao, const hlmi_variant_opts *o, "
            "const char *pairs_paf, const char *out_sites, const char *out_summary, hlmi_variant_stats *st);") in flat
    assert "void hlmi_variant_opts_default(hlmi_variant_opts *o);" in flat
    assert re.findall(r"#define HLMI_ABI_VERSION (\d+)", text) == ["7"] and api.ABI_VERSION == 7
    # the depth call keeps its prototype
    assert ("int hlmi_depth(const char *contigs, const char *reads, const char *paf, const hlmi_depth_opts *o, const char *pairs_paf, "
            "const char *out_tsv, const char *out_bedgraph, hlmi_depth_stats *st);") in flat
    rules = re.sub(r"\s+", " ", re.sub(r"\n \* ?", " ", text))            # the comment's lines joined
    for word in ("on a tie the first in the order A, C, G, T, del", "(double)v[alt] / (double)c >= min_frac", "own may be the minority symbol",
                 "Slots (the columns of I ops) and base qualities take no part", "counts in ref_other and is never a site",
                 "#contig\\tpos\\tref\\tdepth\\tA\\tC\\tG\\tT\\tdel\\talt\\talt_count\\talt_frac",
                 "#contig\\tlength\\treads\\tcallable\\tsites\\tsite_rate", "With no site the file is the header line alone",
                 "0.000000 when callable is 0", "tests/variants_model.py", "min_frac outside [0, 1] or not a number"):
        assert word in rules, word


def test_symbols_and_structs():
    text = open(HEADER).read()
    ctype = {"uint64_t": C.c_uint64, "double": C.c_double, "int": C.c_int}
    assert [(n, ctype[t]) for n, t in _fields(text, "hlmi_variant_opts")] == list(api.VariantOpts._fields_)
    stats = _fields(text, "hlmi_variant_stats")
    assert [(n, ctype[t]) for n, t in stats] == list(api.VariantStats._fields_)
    assert tuple(n for n, t in stats if t == "uint64_t") == api.VARIANT_STATS
    assert api.VARIANT_STATS == ("rows", "rows_selected", "contigs", "contigs_covered", "positions", "callable", "ref_other", "sites",
                                 "sites_base", "sites_del", "pairs_listed", "pairs_unknown", "rows_not_listed")
    assert C.sizeof(api.VariantStats) == 13 * 8 + 2 * 8 and C.sizeof(api.VariantOpts) == 32
    assert api.SYMBOLS["hlmi_variant_opts_default"] == (None, [C.POINTER(api.VariantOpts)])
    assert api.SYMBOLS["hlmi_variants"] == (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(api.VariantOpts), C.c_char_p,
                                                      C.c_char_p, C.c_char_p, C.POINTER(api.VariantStats)])
    assert api.SYMBOLS["hlmi_variants_reads"] == (C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(api.AvaOpts), C.POINTER(api.VariantOpts),
                                                            C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(api.VariantStats)])
    lib = api.load()
    assert lib.hlmi_variants is not None and lib.hlmi_variants_reads is not None
    o = api.VariantOpts(7, 0.5, 9, 9, 0.9)
    lib.hlmi_variant_opts_default(C.byref(o))
    assert {k: getattr(o, k) for k in DEFAULTS} == DEFAULTS
    with pytest.raises(TypeError):
        api.variants("c.fa", "r.fa", "p.paf", "o.tsv", qual_weight=1)
    with pytest.raises(TypeError):
        api.variants_reads("c.fa", "r.fa", "o.tsv", window=500)


def test_module_and_driver_options():
    p = variants.build_parser().parse_args(["--contigs", "c.fa", "--reads", "r.fq", "--out", "s.tsv"])
    assert (p.paf, p.pairs, p.summary, p.short) == (None, None, None, False)
    assert {k: getattr(p, k) for k in DEFAULTS} == DEFAULTS
    p = variants.build_parser().parse_args(["--contigs", "c.fa", "--reads", "r.fq", "--paf", "p.paf", "--pairs", "l.paf", "--out", "s.tsv",
                                            "--summary", "t.tsv", "--min_len", "300", "--min_iden", "0.9", "--min_cov", "5", "--min_alt",
                                            "3", "--min_frac", "0.25"])
    assert (p.paf, p.pairs, p.summary, p.min_len, p.min_iden, p.min_cov, p.min_alt, p.min_frac) == ("p.paf", "l.paf", "t.tsv", 300, 0.9, 5,
                                                                                                 3, 0.25)
    with pytest.raises(SystemExit):                          # --short is about the call that aligns
        variants.main(["--contigs", "c.fa", "--reads", "r.fq", "--paf", "p.paf", "--out", "s.tsv", "--short"])
    assert not driver.build_parser().parse_args(["-l", "x.fq"]).variants
    a = driver.build_parser().parse_args(["-l", "x.fq", "--variants"])
    assert a.variants and not a.depth


def test_module_and_driver_hand_their_arguments_on(tmp_path, monkeypatch):
    seen = []
    monkeypatch.setattr(api, "variants", lambda *a, **k: seen.append(("variants", a, k)) or {})
    monkeypatch.setattr(api, "variants_reads", lambda *a, **k: seen.append(("variants_reads", a, k)) or {})
    assert variants.main(["--contigs", "c.fa", "--reads", "r.fq", "--paf", "p.paf", "--out", "s.tsv", "--pairs", "l.paf"]) == 0
    assert seen[-1] == ("variants", ("c.fa", "r.fq", "p.paf", "s.tsv", None), dict(pairs="l.paf", **DEFAULTS))
    assert variants.main(["--contigs", "c.fa", "--reads", "r.fq", "--out", "s.tsv", "--summary", "t.tsv", "--short", "--min_alt", "4"]) == 0
    who, a, k = seen[-1]
    assert who == "variants_reads" and a[:4] == ("c.fa", "r.fq", "s.tsv", "t.tsv") and k == dict(pairs=None, **{**DEFAULTS, "min_alt": 4})
    short, long_ = api.ava_opts_short(), api.ava_opts_long()
    assert a[4].pair_once == 0 and a[4].k == short.k and a[4].w == short.w
    del seen[:]
    got = driver.variant_tables("final.fa", "long.fa", "short.fq", str(tmp_path))
    assert [(w, a[:2], os.path.basename(a[2]), os.path.basename(a[3]), k) for w, a, k in seen] == [
        ("variants_reads", ("final.fa", "long.fa"), "final_contigs.long.variants.tsv", "final_contigs.long.variants.summary.tsv",
         dict(pairs=None)),
        ("variants_reads", ("final.fa", "short.fq"), "final_contigs.short.variants.tsv", "final_contigs.short.variants.summary.tsv",
         dict(pairs=None))]
    assert sorted(got) == ["long", "short"]
    assert [(a[4].pair_once, a[4].k == long_.k) for _, a, _ in seen] == [(0, True), (0, long_.k == short.k)]
    del seen[:]
    # --polish_strain: the run's two lists
    driver.variant_tables("final.fa", "long.fa", "short.fq", str(tmp_path), long_pairs="ov_long_ref.paf", short_pairs="shortr1.paf")
    assert [k for _, _, k in seen] == [dict(pairs="ov_long_ref.paf"), dict(pairs="shortr1.paf")]
    del seen[:]
    assert sorted(driver.variant_tables("final.fa", "long.fa", None, str(tmp_path))) == ["long"] and len(seen) == 1


def test_variants_text_host_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler on PATH")
    exe = tmp_path / "variants_host_check"
    flags = ["-std=c++17", "-O1", "-ffp-contract=off", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.run([cxx, *flags, os.path.join(ROOT, "tests", "capi", "variants_host_check.cpp"), "-o", str(exe)], check=True, cwd=ROOT)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "variants_host_check: ok" in r.stdout
