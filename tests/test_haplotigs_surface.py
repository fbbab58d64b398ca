"""CPU: the surface of hlmi_haplotigs / hlmi_haplotigs_reads.  The header's prototypes and rules with an unchanged HLMI_ABI_VERSION;
the binding's SYMBOLS entries and structs against the header's field lists; the haplotigs module's and the driver's options and
what they hand on; HAP_TILE where the tests read it; and hylight_amd/csrc/haplotigs_text.h - the split rule, the extents and the
blocks file's lines - compiled with the plain host compiler into tests/capi/haplotigs_host_check.cpp's program under the address
and undefined-behaviour sanitizers and run directly."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import pytest

from hylight_amd import api, driver, haplotigs

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import haplotigs_inputs as GI  # noqa: E402
import haplotigs_model as GM  # noqa: E402

HEADER = os.path.join(ROOT, "include", "hylight_mi.h")
DEFAULTS = dict(min_len=0, min_iden=0.0, min_cov=3, min_alt=2, min_frac=0.2, min_link=3, min_agree=0.8, min_side=3, include_unpolished=1)


def _fields(text, name):
    body = re.search(r"typedef struct \{([^{}]*?)\} %s;" % name, text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [tuple(reversed(d.split())) for d in body.split(";") if d.strip()]


def test_header_prototypes_and_abi():
    text = open(HEADER).read()
    flat = re.sub(r"\s+", " ", text)
    assert ("int hlmi_haplotigs(const char *contigs, const char *reads, const char *paf, const hlmi_haplotig_opts *o, "
            "const char *pairs_paf, const char *out_fa, const char *out_blocks, hlmi_haplotig_stats *st);") in flat
    assert ("int hlmi_haplotigs_reads(const char *contigs, const char *reads, const hlmi_ava_opts *ao, const hlmi_haplotig_opts *o, "
            "const char *pairs_paf, const char *out_fa, const char *out_blocks, hlmi_haplotig_stats *st);") in flat
    assert "void hlmi_haplotig_opts_default(hlmi_haplotig_opts *o);" in flat
    assert re.findall(r"#define HLMI_ABI_VERSION (\d+)", text) == ["7"] and api.ABI_VERSION == 7
    # the phase and polish calls keep their prototypes
    assert ("int hlmi_phase(const char *contigs, const char *reads, const char *paf, const hlmi_phase_opts *o, const char *pairs_paf, "
            "const char *out_sites, const char *out_links, const char *out_reads, hlmi_phase_stats *st);") in flat
    assert ("int hlmi_polish(const char *contigs, const char *reads, const char *paf, const hlmi_polish_opts *o, const char *out_fa, "
            "hlmi_polish_stats *st);") in flat
    rules = re.sub(r"\s+", " ", re.sub(r"\n \* ?", " ", text))
    for word in ("at least min_side of its (row, block) records have side A and at least min_side have side B",
                 "lies inside the extent iff first < p <= last", "Extents of different blocks never overlap",
                 "a row with no side in a block votes on both sides inside that block's extent", "a tie prefers the contig's own base",
                 "byte for byte what hlmi_polish writes for it", "HB:i:<split blocks> HP:i:<positions inside their extents>",
                 "A record whose consensus is empty is not written", "pseudo-haplotigs",
                 "#contig\\tblock\\tstart\\tend\\tsites\\trows_a\\trows_b\\tsplit\\tdiff_positions", "0 when the block is not split",
                 "no kernel of csrc/haplotigs.hip is launched", "insertion sites as phasing evidence", "min_side < 1",
                 "the rows' interval table does not fit the device's free memory", "tests/haplotigs_model.py"):
        assert word in rules, word
    assert GM.BLOCKS_HEAD == re.findall(r'"(#contig\\tblock[^"]*)"', rules)[0].encode().replace(b"\\t", b"\t") + b"\n"


def test_symbols_and_structs():
    text = open(HEADER).read()
    ctype = {"uint64_t": C.c_uint64, "double": C.c_double, "int": C.c_int, "hlmi_phase_stats": api.PhaseStats}
    assert [(n, ctype[t]) for n, t in _fields(text, "hlmi_haplotig_opts")] == list(api.HaplotigOpts._fields_)
    assert list(api.HaplotigOpts._fields_)[:7] == list(api.PhaseOpts._fields_)
    stats = _fields(text, "hlmi_haplotig_stats")
    assert [(n, ctype[t]) for n, t in stats] == list(api.HaplotigStats._fields_)
    assert tuple(n for n, t in stats if t == "uint64_t") == api.HAPLOTIG_STATS == GM.OWN_KEYS
    assert api.PHASE_STATS + api.HAPLOTIG_STATS == GM.STAT_KEYS
    assert C.sizeof(api.HaplotigStats) == C.sizeof(api.PhaseStats) + 11 * 8 + 2 * 8 and C.sizeof(api.HaplotigOpts) == 56
    assert api.SYMBOLS["hlmi_haplotig_opts_default"] == (None, [C.POINTER(api.HaplotigOpts)])
    assert api.SYMBOLS["hlmi_haplotigs"] == (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(api.HaplotigOpts), C.c_char_p, C.c_char_p,
                                                       C.c_char_p, C.POINTER(api.HaplotigStats)])
    assert api.SYMBOLS["hlmi_haplotigs_reads"] == (C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(api.AvaOpts), C.POINTER(api.HaplotigOpts),
                                                             C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(api.HaplotigStats)])
    lib = api.load()
    assert lib.hlmi_haplotigs is not None and lib.hlmi_haplotigs_reads is not None
    o = api.HaplotigOpts(7, 0.5, 9, 9, 0.9, 9, 0.9, 9, 0)
    lib.hlmi_haplotig_opts_default(C.byref(o))
    assert {k: getattr(o, k) for k in DEFAULTS} == DEFAULTS
    with pytest.raises(TypeError):
        api.haplotigs("c.fa", "r.fa", "p.paf", "o.fa", qual_weight=1)
    with pytest.raises(TypeError):
        api.haplotigs_reads("c.fa", "r.fa", "o.fa", window=500)


def test_the_tests_read_the_kernels_constants():
    assert GI.HAP_TILE >= 64 and GI.SHORT_RUN >= 1
    text = open(os.path.join(ROOT, "hylight_amd", "csrc", "haplotigs.hip")).read()
    assert "s_cnt[2][HAP_CNT][HAP_TILE]" in text and "vote_columns<false>" in text and "walk_row(" in text and "polish_tail(" in text
    assert "haplotigs.hip" in "\n".join(__import__("hylight_amd.build", fromlist=["sources"]).sources())


def test_module_and_driver_options():
    p = haplotigs.build_parser().parse_args(["--contigs", "c.fa", "--reads", "r.fq", "--out", "h.fa"])
    assert (p.paf, p.pairs, p.blocks, p.short) == (None, None, None, False)
    assert {k: getattr(p, k) for k in DEFAULTS} == DEFAULTS
    p = haplotigs.build_parser().parse_args(["--contigs", "c.fa", "--reads", "r.fq", "--paf", "p.paf", "--pairs", "l.paf", "--out", "h.fa",
                                             "--blocks", "b.tsv", "--min_len", "300", "--min_iden", "0.9", "--min_cov", "5", "--min_alt", "3",
                                             "--min_frac", "0.25", "--min_link", "4", "--min_agree", "0.75", "--min_side", "5",
                                             "--include_unpolished", "0"])
    assert (p.paf, p.pairs, p.blocks, p.min_len, p.min_iden, p.min_cov, p.min_alt, p.min_frac, p.min_link, p.min_agree, p.min_side,
            p.include_unpolished) == ("p.paf", "l.paf", "b.tsv", 300, 0.9, 5, 3, 0.25, 4, 0.75, 5, 0)
    with pytest.raises(SystemExit):                          # --short is about the call that aligns
        haplotigs.main(["--contigs", "c.fa", "--reads", "r.fq", "--paf", "p.paf", "--out", "h.fa", "--short"])
    assert not driver.build_parser().parse_args(["-l", "x.fq"]).haplotigs
    a = driver.build_parser().parse_args(["-l", "x.fq", "--haplotigs"])
    assert a.haplotigs and not a.phase and not a.variants


def test_module_and_driver_hand_their_arguments_on(tmp_path, monkeypatch):
    seen = []
    monkeypatch.setattr(api, "haplotigs", lambda *a, **k: seen.append(("haplotigs", a, k)) or {})
    monkeypatch.setattr(api, "haplotigs_reads", lambda *a, **k: seen.append(("haplotigs_reads", a, k)) or {})
    assert haplotigs.main(["--contigs", "c.fa", "--reads", "r.fq", "--paf", "p.paf", "--out", "h.fa", "--pairs", "l.paf", "--blocks", "b.tsv"]) == 0
    assert seen[-1] == ("haplotigs", ("c.fa", "r.fq", "p.paf", "h.fa", "b.tsv"), dict(pairs="l.paf", **DEFAULTS))
    assert haplotigs.main(["--contigs", "c.fa", "--reads", "r.fq", "--out", "h.fa", "--short", "--min_side", "4"]) == 0
    who, a, k = seen[-1]
    assert who == "haplotigs_reads" and a[:4] == ("c.fa", "r.fq", "h.fa", None) and k == dict(pairs=None, **{**DEFAULTS, "min_side": 4})
    short, long_ = api.ava_opts_short(), api.ava_opts_long()
    assert a[4].pair_once == 0 and a[4].k == short.k and a[4].w == short.w
    del seen[:]
    got = driver.haplotig_files("final.fa", "long.fa", "short.fq", str(tmp_path))
    assert [(w, a[:2], [os.path.basename(x) for x in a[2:4]], k) for w, a, k in seen] == [
        ("haplotigs_reads", ("final.fa", "long.fa"), ["final_contigs.long.haplotigs.fa", "final_contigs.long.haplotigs.blocks.tsv"], dict(pairs=None)),
        ("haplotigs_reads", ("final.fa", "short.fq"), ["final_contigs.short.haplotigs.fa", "final_contigs.short.haplotigs.blocks.tsv"],
         dict(pairs=None))]
    assert sorted(got) == ["long", "short"]
    assert [(a[4].pair_once, a[4].k == long_.k) for _, a, _ in seen] == [(0, True), (0, long_.k == short.k)]
    del seen[:]
    # --polish_strain: the run's two lists
    driver.haplotig_files("final.fa", "long.fa", "short.fq", str(tmp_path), long_pairs="ov_long_ref.paf", short_pairs="shortr1.paf")
    assert [k for _, _, k in seen] == [dict(pairs="ov_long_ref.paf"), dict(pairs="shortr1.paf")]
    del seen[:]
    assert sorted(driver.haplotig_files("final.fa", "long.fa", None, str(tmp_path))) == ["long"] and len(seen) == 1


def test_haplotigs_text_host_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler on PATH")
    exe = tmp_path / "haplotigs_host_check"
    flags = ["-std=c++17", "-O1", "-ffp-contract=off", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.run([cxx, *flags, os.path.join(ROOT, "tests", "capi", "haplotigs_host_check.cpp"), "-o", str(exe)], check=True, cwd=ROOT)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "haplotigs_host_check: ok" in r.stdout
