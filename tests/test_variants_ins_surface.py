"""CPU: the surface of hlmi_variants_ins / hlmi_variants_reads_ins.  The header's prototypes and rule sentences with an unchanged
HLMI_ABI_VERSION and the older calls' prototypes where they were; the binding's SYMBOLS entries and struct against the header's
field list; the variants module's --ins and the driver's --variants_ins and what they hand on, with the api functions
monkey-patched; and hylight_amd/csrc/variants_ins_text.h - the insertion records per contig, ins_rate, both files' text and the
records it refuses - compiled with the plain host compiler into tests/capi/variants_ins_host_check.cpp's program under the address
and undefined-behaviour sanitizers and run directly."""
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


def test_header_prototypes_rules_and_abi():
    text = open(HEADER).read()
    flat = re.sub(r"\s+", " ", text)
    assert ("int hlmi_variants_ins(const char *contigs, const char *reads, const char *paf, const hlmi_variant_opts *o, "
            "const char *pairs_paf, const char *out_sites, const char *out_summary, const char *out_ins, "
            "hlmi_variant_ins_stats *st);") in flat
    assert ("int hlmi_variants_reads_ins(const char *contigs, const char *reads, const hlmi_ava_opts *ao, const hlmi_variant_opts *o, "
            "const char *pairs_paf, const char *out_sites, const char *out_summary, const char *out_ins, "
            "hlmi_variant_ins_stats *st);") in flat
    # the older calls keep their prototypes, the ABI its number
    assert ("int hlmi_variants(const char *contigs, const char *reads, const char *paf, const hlmi_variant_opts *o, "
            "const char *pairs_paf, const char *out_sites, const char *out_summary, hlmi_variant_stats *st);") in flat
    assert ("int hlmi_variants_reads(const char *contigs, const char *reads, const hlmi_ava_opts *ao, const hlmi_variant_opts *o, "
            "const char *pairs_paf, const char *out_sites, const char *out_summary, hlmi_variant_stats *st);") in flat
    assert re.findall(r"#define HLMI_ABI_VERSION (\d+)", text) == ["7"] and api.ABI_VERSION == 7
    rules = re.sub(r"\s+", " ", re.sub(r"\n \* ?", " ", text))            # the comment's lines joined
    for word in ("Slot p, 0 < p < length, is the gap in front of 0-based position p", "with ts < p < te spans it",
                 "A row with 1..16 bases there inserts", "more than 16 bases there is a long row",
                 "I ops at p == ts or p == te belong to no slot and count in ins_edge",
                 "votes nothing (an N) still spans; a row that starts at p does not span",
                 "a slot is callable iff s >= min_cov", "i + l >= min_alt and (double)(i + l) / (double)s >= min_frac",
                 "a slot next to an N can be a site", "on a tie the smallest, 0 when i == 0",
                 "on a tie the first of A, C, G, T, with none N", "Strand '-' rows insert the reverse complement",
                 "#contig\\tpos\\tref\\tspan\\tins\\tins_long\\tins_frac\\tlen\\tlen_count\\tseq",
                 "#contig\\tlength\\treads\\tcallable\\tsites\\tsite_rate\\tslots\\tins_sites\\tins_rate",
                 "'*' when len is 0", "With no insertion site the file is the header line alone", "0.000000 when slots is 0",
                 "out_sites is byte for byte the file hlmi_variants writes for the same arguments",
                 "out_ins == NULL first, then hlmi_variants's refusals in its order", "tests/variants_ins_model.py",
                 "an unlisted row neither votes nor spans nor inserts"):
        assert word in rules, word


def test_symbols_and_structs():
    text = open(HEADER).read()
    ctype = {"uint64_t": C.c_uint64, "double": C.c_double, "int": C.c_int}
    stats = _fields(text, "hlmi_variant_ins_stats")
    assert [(n, ctype[t]) for n, t in stats] == list(api.VariantInsStats._fields_)
    assert tuple(n for n, t in stats if t == "uint64_t") == api.VARIANT_INS_STATS
    assert api.VARIANT_INS_STATS == api.VARIANT_STATS + ("slots_callable", "ins_sites", "ins_long", "ins_edge")
    # the thirteen shared fields lie where hlmi_variant_stats has them
    assert stats[:13] == _fields(text, "hlmi_variant_stats")[:13]
    assert C.sizeof(api.VariantInsStats) == 17 * 8 + 2 * 8
    assert api.SYMBOLS["hlmi_variants_ins"] == (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(api.VariantOpts), C.c_char_p,
                                                          C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(api.VariantInsStats)])
    assert api.SYMBOLS["hlmi_variants_reads_ins"] == (C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(api.AvaOpts), C.POINTER(api.VariantOpts),
                                                                C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p,
                                                                C.POINTER(api.VariantInsStats)])
    lib = api.load()
    assert lib.hlmi_variants_ins is not None and lib.hlmi_variants_reads_ins is not None
    with pytest.raises(TypeError):
        api.variants_ins("c.fa", "r.fa", "p.paf", "o.tsv", "i.tsv", qual_weight=1)
    with pytest.raises(TypeError):
        api.variants_ins_reads("c.fa", "r.fa", "o.tsv", "i.tsv", window=500)


def test_module_and_driver_options():
    p = variants.build_parser().parse_args(["--contigs", "c.fa", "--reads", "r.fq", "--out", "s.tsv"])
    assert p.ins is None
    p = variants.build_parser().parse_args(["--contigs", "c.fa", "--reads", "r.fq", "--out", "s.tsv", "--ins", "i.tsv"])
    assert p.ins == "i.tsv" and {k: getattr(p, k) for k in DEFAULTS} == DEFAULTS
    with pytest.raises(SystemExit):                          # --short is about the call that aligns
        variants.main(["--contigs", "c.fa", "--reads", "r.fq", "--paf", "p.paf", "--out", "s.tsv", "--ins", "i.tsv", "--short"])
    a = driver.build_parser().parse_args(["-l", "x.fq"])
    assert not a.variants_ins and not a.variants
    a = driver.build_parser().parse_args(["-l", "x.fq", "--variants_ins"])
    assert a.variants_ins and not a.variants
    a = driver.build_parser().parse_args(["-l", "x.fq", "--variants", "--variants_ins"])
    assert a.variants_ins and a.variants


def test_module_and_driver_hand_their_arguments_on(tmp_path, monkeypatch):
    seen = []
    for who in ("variants", "variants_reads", "variants_ins", "variants_ins_reads"):
        monkeypatch.setattr(api, who, lambda *a, _who=who, **k: seen.append((_who, a, k)) or {})
    base = ["--contigs", "c.fa", "--reads", "r.fq", "--out", "s.tsv"]
    assert variants.main(base + ["--paf", "p.paf", "--ins", "i.tsv", "--pairs", "l.paf"]) == 0
    assert seen[-1] == ("variants_ins", ("c.fa", "r.fq", "p.paf", "s.tsv", "i.tsv", None), dict(pairs="l.paf", **DEFAULTS))
    assert variants.main(base + ["--ins", "i.tsv", "--summary", "t.tsv", "--short", "--min_frac", "0.1"]) == 0
    who, a, k = seen[-1]
    assert who == "variants_ins_reads" and a[:5] == ("c.fa", "r.fq", "s.tsv", "i.tsv", "t.tsv")
    assert k == dict(pairs=None, **{**DEFAULTS, "min_frac": 0.1})
    short, long_ = api.ava_opts_short(), api.ava_opts_long()
    assert a[5].pair_once == 0 and a[5].k == short.k and a[5].w == short.w
    # without --ins the calls and their arguments are the older ones
    assert variants.main(base + ["--paf", "p.paf"]) == 0
    assert seen[-1] == ("variants", ("c.fa", "r.fq", "p.paf", "s.tsv", None), dict(pairs=None, **DEFAULTS))
    assert variants.main(base) == 0
    assert seen[-1][0] == "variants_reads" and seen[-1][1][:4] == ("c.fa", "r.fq", "s.tsv", None)
    del seen[:]
    # the driver: one call per read set, the third file beside the two
    got = driver.variant_tables("final.fa", "long.fa", "short.fq", str(tmp_path), ins=True, long_pairs="ov_long_ref.paf")
    assert [(w, a[:2], [os.path.basename(x) for x in a[2:5]], k) for w, a, k in seen] == [
        ("variants_ins_reads", ("final.fa", "long.fa"),
         ["final_contigs.long.variants.tsv", "final_contigs.long.variants.ins.tsv", "final_contigs.long.variants.summary.tsv"],
         dict(pairs="ov_long_ref.paf")),
        ("variants_ins_reads", ("final.fa", "short.fq"),
         ["final_contigs.short.variants.tsv", "final_contigs.short.variants.ins.tsv", "final_contigs.short.variants.summary.tsv"],
         dict(pairs=None))]
    assert sorted(got) == ["long", "short"]
    assert [(a[5].pair_once, a[5].k == long_.k) for _, a, _ in seen] == [(0, True), (0, long_.k == short.k)]
    del seen[:]
    # without the flag: today's calls, argument for argument
    driver.variant_tables("final.fa", "long.fa", None, str(tmp_path))
    assert [(w, len(a), k) for w, a, k in seen] == [("variants_reads", 5, dict(pairs=None))]


def test_variants_ins_text_host_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler on PATH")
    exe = tmp_path / "variants_ins_host_check"
    flags = ["-std=c++17", "-O1", "-ffp-contract=off", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.run([cxx, *flags, os.path.join(ROOT, "tests", "capi", "variants_ins_host_check.cpp"), "-o", str(exe)], check=True, cwd=ROOT)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "variants_ins_host_check: ok" in r.stdout
