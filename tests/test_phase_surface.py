"""CPU: the surface of hlmi_phase / hlmi_phase_reads.  The header's prototypes and rules with an unchanged HLMI_ABI_VERSION; the
binding's SYMBOLS entries and structs against the header's field lists; the phase module's and the driver's options and what they
hand on; PHASE_TILE where the tests read it; and hylight_amd/csrc/phase_text.h - the link rule, the blocks and bits, the hap rule
and the three files' text - compiled with the plain host compiler into tests/capi/phase_host_check.cpp's program under the address
and undefined-behaviour sanitizers and run directly."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import pytest

from hylight_amd import api, driver, phase

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import phase_inputs as HI  # noqa: E402
import phase_model as HM  # noqa: E402

HEADER = os.path.join(ROOT, "include", "hylight_mi.h")
DEFAULTS = dict(min_len=0, min_iden=0.0, min_cov=3, min_alt=2, min_frac=0.2, min_link=3, min_agree=0.8)


def _fields(text, name):
    body = re.search(r"typedef struct \{([^{}]*?)\} %s;" % name, text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [tuple(reversed(d.split())) for d in body.split(";") if d.strip()]


def test_header_prototypes_and_abi():
    text = open(HEADER).read()
    flat = re.sub(r"\s+", " ", text)
    assert ("int hlmi_phase(const char *contigs, const char *reads, const char *paf, const hlmi_phase_opts *o, const char *pairs_paf, "
            "const char *out_sites, const char *out_links, const char *out_reads, hlmi_phase_stats *st);") in flat
    assert ("int hlmi_phase_reads(const char *contigs, const char *reads, const hlmi_ava_opts *ao, const hlmi_phase_opts *o, "
            "const char *pairs_paf, const char *out_sites, const char *out_links, const char *out_reads, hlmi_phase_stats *st);") in flat
    assert "void hlmi_phase_opts_default(hlmi_phase_opts *o);" in flat
    assert re.findall(r"#define HLMI_ABI_VERSION (\d+)", text) == ["7"] and api.ABI_VERSION == 7
    # the variants call keeps its prototype
    assert ("int hlmi_variants(const char *contigs, const char *reads, const char *paf, const hlmi_variant_opts *o, "
            "const char *pairs_paf, const char *out_sites, const char *out_summary, hlmi_variant_stats *st);") in flat
    rules = re.sub(r"\s+", " ", re.sub(r"\n \* ?", " ", text))            # the comment's lines joined
    for word in ("0 if it is own, 1 if it is alt, 2 if it is another of the five symbols", "A D column votes del",
                 "a link never joins two contigs", "(double)top / (double)inf >= min_agree", "its direction is cis if cis > trans, otherwise trans",
                 "A block's id is the 1-based position of its first site", "previous bit XOR (the link is trans)",
                 "gets a record iff hap_a + hap_b + other >= 1", "#contig\\tpos\\tref\\talt\\tdepth\\tref_count\\talt_count\\tblock\\tphase",
                 "#contig\\tpos1\\tpos2\\tn00\\tn01\\tn10\\tn11\\tinformative\\tagree\\tphased",
                 "#read\\tcontig\\tblock\\tspanned\\thap_a\\thap_b\\tother\\thap", "0.000000 when inf is 0", "min_link < 1",
                 "min_agree not a number, <= 0.5 or > 1", "is 2^32 or more, or does not fit the device's free memory", "tests/phase_model.py"):
        assert word in rules, word
    assert (HM.SITES_HEAD, HM.LINKS_HEAD, HM.READS_HEAD) == tuple(
        h.encode().replace(b"\\t", b"\t") + b"\n" for h in re.findall(r'"(#(?:contig\\tpos\\tref\\talt|contig\\tpos1|read)[^"]*)"', rules))


def test_symbols_and_structs():
    text = open(HEADER).read()
    ctype = {"uint64_t": C.c_uint64, "double": C.c_double, "int": C.c_int}
    assert [(n, ctype[t]) for n, t in _fields(text, "hlmi_phase_opts")] == list(api.PhaseOpts._fields_)
    assert list(api.PhaseOpts._fields_)[:5] == list(api.VariantOpts._fields_)
    stats = _fields(text, "hlmi_phase_stats")
    assert [(n, ctype[t]) for n, t in stats] == list(api.PhaseStats._fields_)
    assert tuple(n for n, t in stats if t == "uint64_t") == api.PHASE_STATS == HM.STAT_KEYS
    assert api.PHASE_STATS[:13] == api.VARIANT_STATS
    assert api.PHASE_STATS[13:] == ("links", "links_phased", "blocks", "blocks_multi", "sites_phased", "alleles", "read_records", "reads_a",
                                    "reads_b", "reads_tie")
    assert C.sizeof(api.PhaseStats) == 23 * 8 + 2 * 8 and C.sizeof(api.PhaseOpts) == 48
    assert api.SYMBOLS["hlmi_phase_opts_default"] == (None, [C.POINTER(api.PhaseOpts)])
    assert api.SYMBOLS["hlmi_phase"] == (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(api.PhaseOpts), C.c_char_p, C.c_char_p,
                                                   C.c_char_p, C.c_char_p, C.POINTER(api.PhaseStats)])
    assert api.SYMBOLS["hlmi_phase_reads"] == (C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(api.AvaOpts), C.POINTER(api.PhaseOpts), C.c_char_p,
                                                         C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(api.PhaseStats)])
    lib = api.load()
    assert lib.hlmi_phase is not None and lib.hlmi_phase_reads is not None
    o = api.PhaseOpts(7, 0.5, 9, 9, 0.9, 9, 0.9)
    lib.hlmi_phase_opts_default(C.byref(o))
    assert {k: getattr(o, k) for k in DEFAULTS} == DEFAULTS
    with pytest.raises(TypeError):
        api.phase("c.fa", "r.fa", "p.paf", "o.tsv", qual_weight=1)
    with pytest.raises(TypeError):
        api.phase_reads("c.fa", "r.fa", "o.tsv", window=500)


def test_the_tests_read_the_kernels_constants():
    assert HI.PHASE_TILE >= 64 and HI.SHORT_RUN >= 1 and HI.T >= 64
    text = open(os.path.join(ROOT, "hylight_amd", "csrc", "phase.hip")).read()
    assert "s_n[4][PHASE_TILE]" in text and "vote_columns<false>" in text and "walk_row(" in text


def test_module_and_driver_options():
    p = phase.build_parser().parse_args(["--contigs", "c.fa", "--reads", "r.fq", "--out", "s.tsv"])
    assert (p.paf, p.pairs, p.links, p.read_haps, p.short) == (None, None, None, None, False)
    assert {k: getattr(p, k) for k in DEFAULTS} == DEFAULTS
    p = phase.build_parser().parse_args(["--contigs", "c.fa", "--reads", "r.fq", "--paf", "p.paf", "--pairs", "l.paf", "--out", "s.tsv",
                                         "--links", "l.tsv", "--read-haps", "h.tsv", "--min_len", "300", "--min_iden", "0.9", "--min_cov", "5",
                                         "--min_alt", "3", "--min_frac", "0.25", "--min_link", "4", "--min_agree", "0.75"])
    assert (p.paf, p.pairs, p.links, p.read_haps, p.min_len, p.min_iden, p.min_cov, p.min_alt, p.min_frac, p.min_link, p.min_agree) == (
        "p.paf", "l.paf", "l.tsv", "h.tsv", 300, 0.9, 5, 3, 0.25, 4, 0.75)
    with pytest.raises(SystemExit):                          # --short is about the call that aligns
        phase.main(["--contigs", "c.fa", "--reads", "r.fq", "--paf", "p.paf", "--out", "s.tsv", "--short"])
    assert not driver.build_parser().parse_args(["-l", "x.fq"]).phase
    a = driver.build_parser().parse_args(["-l", "x.fq", "--phase"])
    assert a.phase and not a.variants and not a.depth


def test_module_and_driver_hand_their_arguments_on(tmp_path, monkeypatch):
    seen = []
    monkeypatch.setattr(api, "phase", lambda *a, **k: seen.append(("phase", a, k)) or {})
    monkeypatch.setattr(api, "phase_reads", lambda *a, **k: seen.append(("phase_reads", a, k)) or {})
    assert phase.main(["--contigs", "c.fa", "--reads", "r.fq", "--paf", "p.paf", "--out", "s.tsv", "--pairs", "l.paf", "--links", "k.tsv"]) == 0
    assert seen[-1] == ("phase", ("c.fa", "r.fq", "p.paf", "s.tsv", "k.tsv", None), dict(pairs="l.paf", **DEFAULTS))
    assert phase.main(["--contigs", "c.fa", "--reads", "r.fq", "--out", "s.tsv", "--read-haps", "h.tsv", "--short", "--min_link", "4"]) == 0
    who, a, k = seen[-1]
    assert who == "phase_reads" and a[:5] == ("c.fa", "r.fq", "s.tsv", None, "h.tsv") and k == dict(pairs=None, **{**DEFAULTS, "min_link": 4})
    short, long_ = api.ava_opts_short(), api.ava_opts_long()
    assert a[5].pair_once == 0 and a[5].k == short.k and a[5].w == short.w
    del seen[:]
    got = driver.phase_tables("final.fa", "long.fa", "short.fq", str(tmp_path))
    assert [(w, a[:2], [os.path.basename(x) for x in a[2:5]], k) for w, a, k in seen] == [
        ("phase_reads", ("final.fa", "long.fa"), [f"final_contigs.long.phase.{e}.tsv" for e in ("sites", "links", "reads")], dict(pairs=None)),
        ("phase_reads", ("final.fa", "short.fq"), [f"final_contigs.short.phase.{e}.tsv" for e in ("sites", "links", "reads")], dict(pairs=None))]
    assert sorted(got) == ["long", "short"]
    assert [(a[5].pair_once, a[5].k == long_.k) for _, a, _ in seen] == [(0, True), (0, long_.k == short.k)]
    del seen[:]
    # --polish_strain: the run's two lists
    driver.phase_tables("final.fa", "long.fa", "short.fq", str(tmp_path), long_pairs="ov_long_ref.paf", short_pairs="shortr1.paf")
    assert [k for _, _, k in seen] == [dict(pairs="ov_long_ref.paf"), dict(pairs="shortr1.paf")]
    del seen[:]
    assert sorted(driver.phase_tables("final.fa", "long.fa", None, str(tmp_path))) == ["long"] and len(seen) == 1


def test_phase_text_host_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler on PATH")
    exe = tmp_path / "phase_host_check"
    flags = ["-std=c++17", "-O1", "-ffp-contract=off", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.run([cxx, *flags, os.path.join(ROOT, "tests", "capi", "phase_host_check.cpp"), "-o", str(exe)], check=True, cwd=ROOT)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "phase_host_check: ok" in r.stdout
