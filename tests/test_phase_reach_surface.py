"""CPU: the surface of hlmi_phase_reach / hlmi_phase_reads_reach / hlmi_haplotigs_reach / hlmi_haplotigs_reads_reach.  The header's
prototypes and rules with an unchanged HLMI_ABI_VERSION and the older prototypes where they were; the binding's SYMBOLS entries
and struct against the header's field list; the modules' and the driver's options and what they hand on for --reach 1 (exactly
today's calls) and --reach 3; PHASE_REACH_TILE and HLMI_PHASE_REACH_MAX where the tests read them; and
hylight_amd/csrc/phase_reach_text.h - the block rule, the conflict count, the two files' text - compiled with the plain host
compiler into tests/capi/phase_reach_host_check.cpp's program under the address and undefined-behaviour sanitizers and run
directly."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import pytest

from hylight_amd import api, driver, haplotigs, phase
from hylight_amd import build as B

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import phase_reach_inputs as RI  # noqa: E402
import phase_reach_model as RM  # noqa: E402

HEADER = os.path.join(ROOT, "include", "hylight_mi.h")
PHASE_DEFAULTS = dict(min_len=0, min_iden=0.0, min_cov=3, min_alt=2, min_frac=0.2, min_link=3, min_agree=0.8)
HAP_DEFAULTS = dict(PHASE_DEFAULTS, min_side=3, include_unpolished=1)


def test_header_prototypes_and_abi():
    text = open(HEADER).read()
    flat = re.sub(r"\s+", " ", text)
    for proto in (
            "int hlmi_phase_reach(const char *contigs, const char *reads, const char *paf, const hlmi_phase_opts *o, int reach, "
            "const char *pairs_paf, const char *out_sites, const char *out_links, const char *out_reads, hlmi_phase_reach_stats *st);",
            "int hlmi_phase_reads_reach(const char *contigs, const char *reads, const hlmi_ava_opts *ao, const hlmi_phase_opts *o, int reach, "
            "const char *pairs_paf, const char *out_sites, const char *out_links, const char *out_reads, hlmi_phase_reach_stats *st);",
            "int hlmi_haplotigs_reach(const char *contigs, const char *reads, const char *paf, const hlmi_haplotig_opts *o, int reach, "
            "const char *pairs_paf, const char *out_fa, const char *out_blocks, hlmi_haplotig_stats *st);",
            "int hlmi_haplotigs_reads_reach(const char *contigs, const char *reads, const hlmi_ava_opts *ao, const hlmi_haplotig_opts *o, "
            "int reach, const char *pairs_paf, const char *out_fa, const char *out_blocks, hlmi_haplotig_stats *st);",
            # the older calls keep theirs
            "int hlmi_phase(const char *contigs, const char *reads, const char *paf, const hlmi_phase_opts *o, const char *pairs_paf, "
            "const char *out_sites, const char *out_links, const char *out_reads, hlmi_phase_stats *st);",
            "int hlmi_haplotigs(const char *contigs, const char *reads, const char *paf, const hlmi_haplotig_opts *o, const char *pairs_paf, "
            "const char *out_fa, const char *out_blocks, hlmi_haplotig_stats *st);"):
        assert proto in flat, proto
    assert re.findall(r"#define HLMI_ABI_VERSION (\d+)", text) == ["7"] and api.ABI_VERSION == 7
    rules = re.sub(r"\s+", " ", re.sub(r"\n \* ?", " ", text))
    for word in ("1 <= K <= HLMI_PHASE_REACH_MAX", "what the rows read at the sites in between plays no part",
                 "the nearest such member decides: bit[i] = bit[j] XOR (the link is trans)", "more than K sites behind the last member",
                 "a bridged site has no phase bit", "With K = 1 this is hlmi_phase's rule", "counted in links_conflict and changes nothing",
                 "counts in spanned and in none of hap_a, hap_b, other", "\".\" in the phase column",
                 "ordered by (left site, right site)", "reach < 1 or > HLMI_PHASE_REACH_MAX", "tests/phase_reach_model.py",
                 "bridged ones included"):
        assert word in rules, word


def test_symbols_and_structs():
    text = open(HEADER).read()
    body = re.search(r"typedef struct \{([^{}]*?)\} hlmi_phase_reach_stats;", text, re.S).group(1)
    fields = [tuple(reversed(d.split())) for d in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";") if d.strip()]
    ctype = {"uint64_t": C.c_uint64, "hlmi_phase_stats": api.PhaseStats}
    assert [(n, ctype[t]) for n, t in fields] == list(api.PhaseReachStats._fields_)
    assert tuple(n for n, t in fields if t == "uint64_t") == api.PHASE_REACH_STATS == RM.FAR_KEYS
    assert api.PHASE_STATS + api.PHASE_REACH_STATS == RM.STAT_KEYS
    assert C.sizeof(api.PhaseReachStats) == C.sizeof(api.PhaseStats) + 5 * 8
    s, p, i = C.c_char_p, C.POINTER, C.c_int
    assert api.SYMBOLS["hlmi_phase_reach"] == (i, [s, s, s, p(api.PhaseOpts), i, s, s, s, s, p(api.PhaseReachStats)])
    assert api.SYMBOLS["hlmi_phase_reads_reach"] == (i, [s, s, p(api.AvaOpts), p(api.PhaseOpts), i, s, s, s, s, p(api.PhaseReachStats)])
    assert api.SYMBOLS["hlmi_haplotigs_reach"] == (i, [s, s, s, p(api.HaplotigOpts), i, s, s, s, p(api.HaplotigStats)])
    assert api.SYMBOLS["hlmi_haplotigs_reads_reach"] == (i, [s, s, p(api.AvaOpts), p(api.HaplotigOpts), i, s, s, s, p(api.HaplotigStats)])
    lib = api.load()
    assert all(getattr(lib, n) is not None for n in ("hlmi_phase_reach", "hlmi_phase_reads_reach", "hlmi_haplotigs_reach",
                                                     "hlmi_haplotigs_reads_reach"))
    with pytest.raises(TypeError):
        api.phase_reach("c.fa", "r.fa", "p.paf", "o.tsv", reach=2, qual_weight=1)
    with pytest.raises(TypeError):
        api.haplotigs_reads_reach("c.fa", "r.fa", "o.fa", reach=2, window=500)


def test_the_tests_read_the_kernels_constants():
    text = open(HEADER).read()
    assert re.findall(r"#define HLMI_PHASE_REACH_MAX (\d+)", text) == ["8"] and RI.REACH_MAX == api.PHASE_REACH_MAX == RM.REACH_MAX == 8
    assert RI.TILE >= 64 and 16 * RI.REACH_MAX * RI.TILE <= 65536
    kernel = open(os.path.join(ROOT, "hylight_amd", "csrc", "phase_reach.hip")).read()
    assert "extern __shared__ uint32_t s_n[]" in kernel and "16 * K * (size_t)PHASE_REACH_TILE" in kernel and "wave_shl1(" in kernel
    assert 'KTimer kt("phase_link_reach")' in open(os.path.join(ROOT, "hylight_amd", "csrc", "phase.hip")).read()
    assert "phase_reach.hip" in B.sources()
    host = open(os.path.join(ROOT, "hylight_amd", "csrc", "phase_reach_text.h")).read()
    assert "hip" not in re.sub(r"//.*", "", host).lower()


def test_module_and_driver_options():
    for mod in (phase, haplotigs):
        assert mod.build_parser().parse_args(["--contigs", "c.fa", "--reads", "r.fq", "--out", "o"]).reach == 1
        assert mod.build_parser().parse_args(["--contigs", "c.fa", "--reads", "r.fq", "--out", "o", "--reach", "3"]).reach == 3
    assert driver.build_parser().parse_args(["-l", "x.fq"]).phase_reach == 1
    a = driver.build_parser().parse_args(["-l", "x.fq", "--phase", "--phase_reach", "4"])
    assert a.phase and not a.haplotigs and a.phase_reach == 4


def test_modules_and_driver_hand_their_arguments_on(tmp_path, monkeypatch):
    seen = []
    for name in ("phase", "phase_reads", "phase_reach", "phase_reads_reach", "haplotigs", "haplotigs_reads", "haplotigs_reach",
                 "haplotigs_reads_reach"):
        monkeypatch.setattr(api, name, lambda *a, _n=name, **k: seen.append((_n, a, k)) or {})
    files = ["--contigs", "c.fa", "--reads", "r.fq"]
    # --reach 1 is the call without it, with its arguments
    assert phase.main(files + ["--paf", "p.paf", "--out", "s.tsv", "--links", "k.tsv", "--reach", "1"]) == 0
    assert seen[-1] == ("phase", ("c.fa", "r.fq", "p.paf", "s.tsv", "k.tsv", None), dict(pairs=None, **PHASE_DEFAULTS))
    assert phase.main(files + ["--out", "s.tsv", "--reach", "1"]) == 0
    assert seen[-1][0] == "phase_reads" and seen[-1][2] == dict(pairs=None, **PHASE_DEFAULTS)
    assert haplotigs.main(files + ["--paf", "p.paf", "--out", "h.fa", "--reach", "1"]) == 0
    assert seen[-1] == ("haplotigs", ("c.fa", "r.fq", "p.paf", "h.fa", None), dict(pairs=None, **HAP_DEFAULTS))
    assert haplotigs.main(files + ["--out", "h.fa", "--reach", "1"]) == 0
    assert seen[-1][0] == "haplotigs_reads" and seen[-1][2] == dict(pairs=None, **HAP_DEFAULTS)
    # --reach 3
    assert phase.main(files + ["--paf", "p.paf", "--out", "s.tsv", "--read-haps", "h.tsv", "--pairs", "l.paf", "--reach", "3"]) == 0
    assert seen[-1] == ("phase_reach", ("c.fa", "r.fq", "p.paf", "s.tsv", None, "h.tsv"), dict(pairs="l.paf", reach=3, **PHASE_DEFAULTS))
    assert phase.main(files + ["--out", "s.tsv", "--short", "--reach", "3", "--min_link", "4"]) == 0
    who, a, k = seen[-1]
    assert who == "phase_reads_reach" and a[:5] == ("c.fa", "r.fq", "s.tsv", None, None)
    assert k == dict(pairs=None, reach=3, **{**PHASE_DEFAULTS, "min_link": 4}) and a[5].k == api.ava_opts_short().k and a[5].pair_once == 0
    assert haplotigs.main(files + ["--paf", "p.paf", "--out", "h.fa", "--blocks", "b.tsv", "--reach", "3"]) == 0
    assert seen[-1] == ("haplotigs_reach", ("c.fa", "r.fq", "p.paf", "h.fa", "b.tsv"), dict(pairs=None, reach=3, **HAP_DEFAULTS))
    assert haplotigs.main(files + ["--out", "h.fa", "--reach", "3"]) == 0
    assert seen[-1][0] == "haplotigs_reads_reach" and seen[-1][2] == dict(pairs=None, reach=3, **HAP_DEFAULTS)
    # the driver's two functions: reach 1 is today's call, above it the _reach call with the same files
    del seen[:]
    driver.phase_tables("final.fa", "long.fa", None, str(tmp_path), reach=1)
    driver.phase_tables("final.fa", "long.fa", "short.fq", str(tmp_path), long_pairs="ov.paf", reach=3)
    assert [(w, k) for w, _, k in seen] == [("phase_reads", dict(pairs=None)), ("phase_reads_reach", dict(pairs="ov.paf", reach=3)),
                                            ("phase_reads_reach", dict(pairs=None, reach=3))]
    assert [os.path.basename(x) for x in seen[1][1][2:5]] == [f"final_contigs.long.phase.{e}.tsv" for e in ("sites", "links", "reads")]
    assert seen[0][1][:5] == seen[1][1][:5] and seen[2][1][5].k == api.ava_opts_short().k
    del seen[:]
    driver.haplotig_files("final.fa", "long.fa", None, str(tmp_path))
    driver.haplotig_files("final.fa", "long.fa", None, str(tmp_path), reach=2)
    assert [(w, k) for w, _, k in seen] == [("haplotigs_reads", dict(pairs=None)), ("haplotigs_reads_reach", dict(pairs=None, reach=2))]
    assert seen[0][1][:4] == seen[1][1][:4]


def test_phase_reach_text_host_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler on PATH")
    exe = tmp_path / "phase_reach_host_check"
    flags = ["-std=c++17", "-O1", "-ffp-contract=off", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.run([cxx, *flags, os.path.join(ROOT, "tests", "capi", "phase_reach_host_check.cpp"), "-o", str(exe)], check=True, cwd=ROOT)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "phase_reach_host_check: ok" in r.stdout
