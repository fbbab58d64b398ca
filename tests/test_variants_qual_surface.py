"""CPU: the surface of hlmi_variants_q and its _reads and _ins forms.  The header's prototypes and rules with an unchanged
HLMI_ABI_VERSION and unchanged older prototypes; the binding's SYMBOLS entries and structs against the header's field lists; the
variants module's --min_base_qual / --min_avg_qual and the driver's --variants_qual with their refusals, and what they hand on
(the api functions replaced by recorders); and hylight_amd/csrc/variants_qual.h - the text the kernel compiles - built with the
plain host compiler into tests/capi/variants_qual_host_check.cpp's program under the address and undefined-behaviour sanitizers
and run directly."""
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
QDEFAULTS = dict(DEFAULTS, min_base_qual=10, min_avg_qual=10.0)


def _fields(text, name):
    body = re.search(r"typedef struct \{([^{}]*?)\} %s;" % name, text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [tuple(reversed(d.split())) for d in body.split(";") if d.strip()]


def test_header_prototypes_and_abi():
    text = open(HEADER).read()
    flat = re.sub(r"\s+", " ", text)
    for proto in (
            "int hlmi_variants_q(const char *contigs, const char *reads, const char *paf, const hlmi_variant_qopts *o, "
            "const char *pairs_paf, const char *out_sites, const char *out_summary, hlmi_variant_stats *st, hlmi_variant_qcounts *qc);",
            "int hlmi_variants_reads_q(const char *contigs, const char *reads, const hlmi_ava_opts *ao, const hlmi_variant_qopts *o, "
            "const char *pairs_paf, const char *out_sites, const char *out_summary, hlmi_variant_stats *st, hlmi_variant_qcounts *qc);",
            "int hlmi_variants_ins_q(const char *contigs, const char *reads, const char *paf, const hlmi_variant_qopts *o, "
            "const char *pairs_paf, const char *out_sites, const char *out_summary, const char *out_ins, hlmi_variant_ins_stats *st, "
            "hlmi_variant_qcounts *qc);",
            "int hlmi_variants_reads_ins_q(const char *contigs, const char *reads, const hlmi_ava_opts *ao, const hlmi_variant_qopts *o, "
            "const char *pairs_paf, const char *out_sites, const char *out_summary, const char *out_ins, hlmi_variant_ins_stats *st, "
            "hlmi_variant_qcounts *qc);",
            "void hlmi_variant_qopts_default(hlmi_variant_qopts *o);",
            # the older calls keep their prototypes
            "int hlmi_variants(const char *contigs, const char *reads, const char *paf, const hlmi_variant_opts *o, "
            "const char *pairs_paf, const char *out_sites, const char *out_summary, hlmi_variant_stats *st);",
            "int hlmi_variants_reads_ins(const char *contigs, const char *reads, const hlmi_ava_opts *ao, const hlmi_variant_opts *o, "
            "const char *pairs_paf, const char *out_sites, const char *out_summary, const char *out_ins, hlmi_variant_ins_stats *st);"):
        assert proto in flat, proto
    assert re.findall(r"#define HLMI_ABI_VERSION (\d+)", text) == ["7"] and api.ABI_VERSION == 7
    rules = re.sub(r"\s+", " ", re.sub(r"\n \* ?", " ", text))
    for word in ("passes iff q >= min_base_qual", "the lower q of query columns qc - 1 and qc", "with neither present the op passes",
                 "column i has the quality of read[qe - 1 - i]", "counts once in columns_low_qual", "never again when a tile is revisited",
                 "FASTA records have no qualities", "a failing column still spans", "out_sites of an _ins_q call is byte for byte the _q call's",
                 "min_base_qual outside 0..93", "There is no rows_selected x 93 refusal", "no real data in this repository supports either figure",
                 "tests/variants_qual_model.py", "min_alt, depth, alt_count and alt_frac are counts of reads"):
        assert word in rules, word


def test_symbols_and_structs():
    text = open(HEADER).read()
    ctype = {"uint64_t": C.c_uint64, "double": C.c_double, "int": C.c_int}
    qopts = _fields(text, "hlmi_variant_qopts")
    assert [(n, ctype[t]) for n, t in qopts] == list(api.VariantQOpts._fields_)
    assert qopts[:5] == _fields(text, "hlmi_variant_opts") and [n for n, _ in qopts[5:]] == ["min_base_qual", "min_avg_qual"]
    counts = _fields(text, "hlmi_variant_qcounts")
    assert [(n, ctype[t]) for n, t in counts] == list(api.VariantQCounts._fields_)
    assert tuple(n for n, _ in counts) == api.VARIANT_QCOUNTS == ("reads_with_qual", "rows_low_qual", "columns_low_qual")
    assert C.sizeof(api.VariantQOpts) == 48 and C.sizeof(api.VariantQCounts) == 24
    assert C.sizeof(api.VariantOpts) == 32 and C.sizeof(api.VariantStats) == 15 * 8           # the older structs as they were
    P = C.POINTER
    s8 = [C.c_char_p] * 3
    assert api.SYMBOLS["hlmi_variant_qopts_default"] == (None, [P(api.VariantQOpts)])
    assert api.SYMBOLS["hlmi_variants_q"] == (C.c_int, [*s8, P(api.VariantQOpts), *s8, P(api.VariantStats), P(api.VariantQCounts)])
    assert api.SYMBOLS["hlmi_variants_reads_q"] == (C.c_int, [C.c_char_p, C.c_char_p, P(api.AvaOpts), P(api.VariantQOpts), *s8,
                                                              P(api.VariantStats), P(api.VariantQCounts)])
    assert api.SYMBOLS["hlmi_variants_ins_q"] == (C.c_int, [*s8, P(api.VariantQOpts), *s8, C.c_char_p, P(api.VariantInsStats),
                                                            P(api.VariantQCounts)])
    assert api.SYMBOLS["hlmi_variants_reads_ins_q"] == (C.c_int, [C.c_char_p, C.c_char_p, P(api.AvaOpts), P(api.VariantQOpts), *s8,
                                                                  C.c_char_p, P(api.VariantInsStats), P(api.VariantQCounts)])
    lib = api.load()
    for name in ("hlmi_variants_q", "hlmi_variants_reads_q", "hlmi_variants_ins_q", "hlmi_variants_reads_ins_q"):
        assert getattr(lib, name) is not None
    o = api.VariantQOpts(7, 0.5, 9, 9, 0.9, 50, 50.0)
    lib.hlmi_variant_qopts_default(C.byref(o))
    assert {k: getattr(o, k) for k in QDEFAULTS} == QDEFAULTS
    for call, args in ((api.variants_q, ("c.fa", "r.fa", "p.paf", "o.tsv")), (api.variants_reads_q, ("c.fa", "r.fa", "o.tsv")),
                       (api.variants_ins_q, ("c.fa", "r.fa", "p.paf", "o.tsv", "i.tsv")),
                       (api.variants_ins_reads_q, ("c.fa", "r.fa", "o.tsv", "i.tsv"))):
        with pytest.raises(TypeError):
            call(*args, qual_weight=1)
    with pytest.raises(TypeError):                           # the older call has no floors
        api.variants("c.fa", "r.fa", "p.paf", "o.tsv", min_base_qual=10)


def test_refusals_need_no_device():
    """the floors are refused before anything is read, the device included; then out_ins == NULL"""
    lib = api.load()
    st, ist, qc = api.VariantStats(), api.VariantInsStats(), api.VariantQCounts()
    err = lambda: lib.hlmi_last_error().decode()                                                   # noqa: E731
    for field, v, word in (("min_base_qual", -1, "min_base_qual"), ("min_base_qual", 94, "min_base_qual"),
                           ("min_avg_qual", -0.5, "min_avg_qual"), ("min_avg_qual", float("nan"), "min_avg_qual")):
        o = api.VariantQOpts()
        lib.hlmi_variant_qopts_default(C.byref(o))
        setattr(o, field, v)
        assert lib.hlmi_variants_q(b"/none/c.fa", b"/none/r.fa", b"/none/p.paf", C.byref(o), None, b"/none/o.tsv", None, C.byref(st),
                                   C.byref(qc)) == -1
        assert word in err() and "hlmi_variants_q" in err()
        assert lib.hlmi_variants_reads_ins_q(b"/none/c.fa", b"/none/r.fa", None, C.byref(o), None, b"/none/o.tsv", None, None, C.byref(ist),
                                             C.byref(qc)) == -1
        assert word in err() and "hlmi_variants_reads_ins_q" in err()      # in front of out_ins == NULL
    o = api.VariantQOpts()
    lib.hlmi_variant_qopts_default(C.byref(o))
    o.min_cov = 0
    assert lib.hlmi_variants_ins_q(b"/none/c.fa", b"/none/r.fa", b"/none/p.paf", C.byref(o), None, b"/none/o.tsv", None, None, C.byref(ist),
                                   C.byref(qc)) == -1
    assert "out_ins is NULL" in err()                                                # in front of min_cov


def test_module_options(monkeypatch):
    p = variants.build_parser().parse_args(["--contigs", "c.fa", "--reads", "r.fq", "--out", "s.tsv"])
    assert (p.min_base_qual, p.min_avg_qual) == (None, None)
    seen = []
    for name in ("variants", "variants_reads", "variants_ins", "variants_ins_reads", "variants_q", "variants_reads_q", "variants_ins_q",
                 "variants_ins_reads_q"):
        monkeypatch.setattr(api, name, lambda *a, _n=name, **k: seen.append((_n, a, k)) or {})
    base = ["--contigs", "c.fa", "--reads", "r.fq", "--out", "s.tsv"]
    # without both: the calls made today
    assert variants.main(base + ["--paf", "p.paf"]) == 0
    assert seen[-1] == ("variants", ("c.fa", "r.fq", "p.paf", "s.tsv", None), dict(pairs=None, **DEFAULTS))
    assert variants.main(base + ["--ins", "i.tsv"]) == 0 and seen[-1][0] == "variants_ins_reads" and "min_base_qual" not in seen[-1][2]
    # either selects the _q call, with or without --ins; the one not given is off
    assert variants.main(base + ["--paf", "p.paf", "--min_base_qual", "12", "--pairs", "l.paf"]) == 0
    assert seen[-1] == ("variants_q", ("c.fa", "r.fq", "p.paf", "s.tsv", None), dict(pairs="l.paf", **DEFAULTS, min_base_qual=12, min_avg_qual=0.0))
    assert variants.main(base + ["--min_avg_qual", "9.5", "--summary", "t.tsv", "--short"]) == 0
    who, a, k = seen[-1]
    assert who == "variants_reads_q" and a[:4] == ("c.fa", "r.fq", "s.tsv", "t.tsv") and a[4].k == api.ava_opts_short().k
    assert k == dict(pairs=None, **DEFAULTS, min_base_qual=0, min_avg_qual=9.5)
    assert variants.main(base + ["--paf", "p.paf", "--ins", "i.tsv", "--min_base_qual", "0"]) == 0
    assert seen[-1] == ("variants_ins_q", ("c.fa", "r.fq", "p.paf", "s.tsv", "i.tsv", None), dict(pairs=None, **DEFAULTS, min_base_qual=0,
                                                                                                  min_avg_qual=0.0))
    assert variants.main(base + ["--ins", "i.tsv", "--min_base_qual", "10", "--min_avg_qual", "10"]) == 0
    who, a, k = seen[-1]
    assert who == "variants_ins_reads_q" and a[:4] == ("c.fa", "r.fq", "s.tsv", "i.tsv") and k["min_base_qual"] == 10 and k["min_avg_qual"] == 10.0
    with pytest.raises(SystemExit):
        variants.main(base + ["--min_base_qual", "ten"])


def test_driver_options_and_what_they_hand_on(tmp_path, monkeypatch):
    a = driver.build_parser().parse_args(["-l", "x.fq", "--variants"])
    assert not a.variants_qual and (a.variants_min_base_qual, a.variants_min_avg_qual) == (10, 10.0)
    assert driver.variants_qual_args(a) == {}
    a = driver.build_parser().parse_args(["-l", "x.fq", "--variants", "--variants_qual", "--variants_min_base_qual", "20",
                                          "--variants_min_avg_qual", "7.5"])
    assert driver.variants_qual_args(a) == {"qual": dict(min_base_qual=20, min_avg_qual=7.5)}
    for flags in (["--variants_qual"], ["--variants_qual", "--phase"]):          # refused without --variants or --variants_ins
        with pytest.raises(SystemExit) as e:
            driver.main(["-l", "x.fq", "-o", str(tmp_path / "out"), *flags])
        assert "--variants_qual" in str(e.value)
    assert not (tmp_path / "out").exists()
    seen = []
    for name in ("variants_reads", "variants_ins_reads", "variants_reads_q", "variants_ins_reads_q"):
        monkeypatch.setattr(api, name, lambda *a, _n=name, **k: seen.append((_n, a, k)) or {})
    q = dict(min_base_qual=10, min_avg_qual=10.0)
    driver.variant_tables("final.fa", "long.fa", "short.fq", str(tmp_path), qual=q, long_pairs="ov.paf")
    assert [(w, a[:2], [os.path.basename(x) for x in a[2:4]], k) for w, a, k in seen] == [
        ("variants_reads_q", ("final.fa", "long.fa"), ["final_contigs.long.variants.tsv", "final_contigs.long.variants.summary.tsv"],
         dict(pairs="ov.paf", **q)),
        ("variants_reads_q", ("final.fa", "short.fq"), ["final_contigs.short.variants.tsv", "final_contigs.short.variants.summary.tsv"],
         dict(pairs=None, **q))]
    assert [a[4].pair_once for _, a, _ in seen] == [0, 0]
    del seen[:]
    driver.variant_tables("final.fa", "long.fa", None, str(tmp_path), ins=True, qual=q)
    who, a, k = seen[0]
    assert who == "variants_ins_reads_q" and [os.path.basename(x) for x in a[2:5]] == [
        "final_contigs.long.variants.tsv", "final_contigs.long.variants.ins.tsv", "final_contigs.long.variants.summary.tsv"] and k == dict(pairs=None, **q)
    del seen[:]
    driver.variant_tables("final.fa", "long.fa", None, str(tmp_path))            # without: the call made today
    assert [w for w, _, _ in seen] == ["variants_reads"] and seen[0][2] == dict(pairs=None)


def test_variants_qual_host_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler on PATH")
    exe = tmp_path / "variants_qual_host_check"
    flags = ["-std=c++17", "-O1", "-ffp-contract=off", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.run([cxx, *flags, os.path.join(ROOT, "tests", "capi", "variants_qual_host_check.cpp"), "-o", str(exe)], check=True, cwd=ROOT)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "variants_qual_host_check: ok" in r.stdout
