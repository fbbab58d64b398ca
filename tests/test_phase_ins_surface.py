"""CPU: hlmi_phase_ins / hlmi_phase_reads_ins without a GPU.  The model (tests/phase_ins_model.py) on the hand cases of
tests/phase_ins_inputs.py, whose three files are written out by hand, and on its shapes (each sits where it claims to); the model's
property that on every older phasing input in which no insertion site takes part its files are phase_reach_model's; the two-strain
input of insertions alone; the header's prototypes and rules with an unchanged HLMI_ABI_VERSION; the binding's SYMBOLS entries
and struct against the header's field list; the options and refusals of `python -m hylight_amd.phase --ins` and `driver
--phase_ins`; and hylight_amd/csrc/phase_ins_text.h compiled with the plain host compiler into
tests/capi/phase_ins_host_check.cpp's program under the address and undefined-behaviour sanitizers and run directly."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import pytest

from hylight_amd import api, driver, phase
from hylight_amd import build as B

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import phase_inputs as HI  # noqa: E402
import phase_ins_inputs as II  # noqa: E402
import phase_ins_model as IM  # noqa: E402
import phase_model as HM  # noqa: E402
import phase_reach_inputs as RI  # noqa: E402
import phase_reach_model as RM  # noqa: E402

HEADER = os.path.join(ROOT, "include", "hylight_mi.h")
PHASE_DEFAULTS = dict(min_len=0, min_iden=0.0, min_cov=3, min_alt=2, min_frac=0.2, min_link=3, min_agree=0.8)
HAND, SHAPES = II.hand_cases(), II.shapes()
OLD = {**{n: (h.case, h.opts, (1, 2)) for n, h in HI.hand_cases().items()},
       **{n: (s.case, s.opts, (1,)) for n, s in HI.shapes().items() if not n.startswith("deep")},
       **{n: (h.case, h.opts, (h.reach,)) for n, h in RI.hand_cases().items()}}


def model(c, reach, **opts):
    return IM.phase(c.contigs_bytes(), c.reads_bytes(), c.paf_bytes(), None, reach, **opts)


@pytest.mark.parametrize("name", sorted(HAND))
def test_model_on_the_hand_cases(name):
    h = HAND[name]
    sites, links, reads, st = model(h.case, h.reach, **h.opts)
    assert sites == HM.SITES_HEAD + b"".join(line + b"\n" for line in h.sites)
    assert links == HM.LINKS_HEAD + b"".join(line + b"\n" for line in h.links)
    assert reads == HM.READS_HEAD + b"".join(line + b"\n" for line in h.reads)
    assert {k: v for k, v in st.items() if v} == h.stats


def test_model_left_out_sites_leave_hlmi_phase_reach():
    h = HAND["insertion_sites_left_out"]
    got = model(h.case, 1)
    want = RM.phase(h.case.contigs_bytes(), h.case.reads_bytes(), h.case.paf_bytes(), None, 1)
    assert got[:3] == want[:3] and {k: got[3][k] for k in RM.STAT_KEYS} == want[3]
    assert got[3]["ins_sites"] == got[3]["ins_sites_left_out"] == 2


@pytest.mark.parametrize("name", sorted(n for n in SHAPES if not n.startswith("deep")))       # (4 097 rows: the GPU test's)
def test_model_on_the_shapes(name):
    s = SHAPES[name]
    for reach in s.reaches:
        s.where(reach, *model(s.case, reach, **s.opts))


@pytest.mark.parametrize("name", sorted(OLD))
def test_model_is_phase_reach_model_where_no_insertion_site_takes_part(name):
    c, opts, reaches = OLD[name]
    for reach in reaches:
        got = model(c, reach, **opts)
        if got[3]["ins_sites_phasing"]:
            assert "cigar_of" in name, name                        # the only older inputs whose I ops have support
            continue
        want = RM.phase(c.contigs_bytes(), c.reads_bytes(), c.paf_bytes(), None, reach, **opts)
        assert got[:3] == want[:3] and {k: got[3][k] for k in RM.STAT_KEYS} == want[3], (name, reach)


def test_model_phases_strains_that_differ_by_insertions_alone():
    s = II.insertion_strains()
    plain = RM.phase(s.case.contigs_bytes(), s.case.reads_bytes(), s.case.paf_bytes(), None, 1)
    assert plain[3]["sites"] == plain[3]["blocks_multi"] == 0
    sites, links, reads, st = model(s.case, 1)
    assert [(p, a, b) for _, p, a, b, _ in II.site_rows(sites)] == [(300, b"+G", b"300+"), (600, b"+TGA", b"300+"), (900, b"+" + II.S16, b"300+")]
    assert (st["blocks"], st["blocks_multi"], st["ins_sites_phased"], st["sites"]) == (1, 1, 3, 0)
    rr = II.read_rows(reads)
    assert len(rr) == 16 and all(hap == (b"B" if read.startswith(s.minor) else b"A") for read, _, _, _, _, _, _, hap in rr)


def test_header_prototypes_and_abi():
    text = open(HEADER).read()
    flat = re.sub(r"\s+", " ", text)
    for proto in (
            "int hlmi_phase_ins(const char *contigs, const char *reads, const char *paf, const hlmi_phase_opts *o, int reach, "
            "const char *pairs_paf, const char *out_sites, const char *out_links, const char *out_reads, hlmi_phase_ins_stats *st);",
            "int hlmi_phase_reads_ins(const char *contigs, const char *reads, const hlmi_ava_opts *ao, const hlmi_phase_opts *o, int reach, "
            "const char *pairs_paf, const char *out_sites, const char *out_links, const char *out_reads, hlmi_phase_ins_stats *st);",
            # the older calls keep theirs
            "int hlmi_phase_reach(const char *contigs, const char *reads, const char *paf, const hlmi_phase_opts *o, int reach, "
            "const char *pairs_paf, const char *out_sites, const char *out_links, const char *out_reads, hlmi_phase_reach_stats *st);"):
        assert proto in flat, proto
    assert re.findall(r"#define HLMI_ABI_VERSION (\d+)", text) == ["7"] and api.ABI_VERSION == 7
    rules = re.sub(r"\s+", " ", re.sub(r"\n \* ?", " ", text))
    for word in ("takes part iff len >= 1 and len_count >= min_alt", "slot p sorts directly in front of position p",
                 "key 2 p for the slot, 2 p + 1 for the position", "come position site first", "iff ts < p < te",
                 "The alt is matched by length alone", "more than 16 bases included", "\"None\" does not occur inside the span",
                 "[2 ts + 1, 2 te)", "a slot endpoint carries a trailing '+'", "with a trailing '+' when that site is an insertion site",
                 "byte for byte hlmi_phase_reach's at the same reach", "keeps 2 p + 1 below 2^32", "tests/phase_ins_model.py"):
        assert word in rules, word


def test_symbols_and_structs():
    text = open(HEADER).read()
    body = re.search(r"typedef struct \{([^{}]*?)\} hlmi_phase_ins_stats;", text, re.S).group(1)
    fields = [tuple(reversed(d.split())) for d in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";") if d.strip()]
    ctype = {"uint64_t": C.c_uint64, "hlmi_phase_reach_stats": api.PhaseReachStats}
    assert [(n, ctype[t]) for n, t in fields] == list(api.PhaseInsStats._fields_)
    assert tuple(n for n, t in fields if t == "uint64_t") == api.PHASE_INS_STATS == IM.INS_KEYS
    assert api.PHASE_STATS + api.PHASE_REACH_STATS + api.PHASE_INS_STATS == IM.STAT_KEYS
    assert C.sizeof(api.PhaseInsStats) == C.sizeof(api.PhaseReachStats) + 7 * 8
    s, p, i = C.c_char_p, C.POINTER, C.c_int
    assert api.SYMBOLS["hlmi_phase_ins"] == (i, [s, s, s, p(api.PhaseOpts), i, s, s, s, s, p(api.PhaseInsStats)])
    assert api.SYMBOLS["hlmi_phase_reads_ins"] == (i, [s, s, p(api.AvaOpts), p(api.PhaseOpts), i, s, s, s, s, p(api.PhaseInsStats)])
    lib = api.load()
    assert all(getattr(lib, n) is not None for n in ("hlmi_phase_ins", "hlmi_phase_reads_ins"))
    with pytest.raises(TypeError):
        api.phase_ins("c.fa", "r.fa", "p.paf", "o.tsv", reach=2, qual_weight=1)
    with pytest.raises(TypeError):
        api.phase_reads_ins("c.fa", "r.fa", "o.tsv", window=500)


def test_the_new_files_are_built_and_host_only_where_they_say():
    assert "phase_ins.hip" in B.sources() and "phase_ins_host.cpp" in B.sources()
    kernel = open(os.path.join(ROOT, "hylight_amd", "csrc", "phase_ins.hip")).read()
    for word in ("phase_span_ins_kernel", "phase_fill_ins_kernel", "phase_allele_ins_kernel", 'KTimer kt("phase_allele_ins")', "vote_columns<false>(",
                 "walk_row("):
        assert word in kernel, word
    assert "asm" not in re.sub(r"//.*", "", kernel)
    host = open(os.path.join(ROOT, "hylight_amd", "csrc", "phase_ins_text.h")).read()
    assert "hip" not in re.sub(r"//.*", "", host).lower()


def test_module_and_driver_options(tmp_path, monkeypatch):
    files = ["--contigs", "c.fa", "--reads", "r.fq", "--out", "s.tsv"]
    assert phase.build_parser().parse_args(files).ins is False and phase.build_parser().parse_args(files + ["--ins"]).ins is True
    seen = []
    for name in ("phase", "phase_reads", "phase_reach", "phase_reads_reach", "phase_ins", "phase_reads_ins"):
        monkeypatch.setattr(api, name, lambda *a, _n=name, **k: seen.append((_n, a, k)) or {})
    # without --ins the module calls what it called
    assert phase.main(files + ["--paf", "p.paf"]) == 0 and seen[-1][0] == "phase"
    assert phase.main(files + ["--reach", "2"]) == 0 and seen[-1][0] == "phase_reads_reach"
    # with it: hlmi_phase_ins at reach 1 and above, with and without a PAF
    assert phase.main(files + ["--paf", "p.paf", "--links", "k.tsv", "--ins"]) == 0
    assert seen[-1] == ("phase_ins", ("c.fa", "r.fq", "p.paf", "s.tsv", "k.tsv", None), dict(pairs=None, reach=1, **PHASE_DEFAULTS))
    assert phase.main(files + ["--paf", "p.paf", "--read-haps", "h.tsv", "--pairs", "l.paf", "--ins", "--reach", "3", "--min_alt", "4"]) == 0
    assert seen[-1] == ("phase_ins", ("c.fa", "r.fq", "p.paf", "s.tsv", None, "h.tsv"),
                        dict(pairs="l.paf", reach=3, **{**PHASE_DEFAULTS, "min_alt": 4}))
    assert phase.main(files + ["--ins", "--short", "--reach", "2"]) == 0
    who, a, k = seen[-1]
    assert who == "phase_reads_ins" and a[:5] == ("c.fa", "r.fq", "s.tsv", None, None) and a[5].k == api.ava_opts_short().k
    assert k == dict(pairs=None, reach=2, **PHASE_DEFAULTS)
    with pytest.raises(SystemExit):
        phase.main(files + ["--paf", "p.paf", "--ins", "--short"])
    # the driver: --phase_ins is a flag of --phase
    a = driver.build_parser().parse_args(["-l", "x.fq", "--phase", "--phase_ins", "--phase_reach", "4"])
    assert a.phase and a.phase_ins and a.phase_reach == 4 and not driver.build_parser().parse_args(["-l", "x.fq", "--phase"]).phase_ins
    with pytest.raises(SystemExit) as e:
        driver.main(["-l", "x.fq", "-o", str(tmp_path / "out"), "--phase_ins"])
    assert "--phase_ins" in str(e.value) and "--phase" in str(e.value) and not os.path.exists(tmp_path / "out")
    del seen[:]
    driver.phase_tables("final.fa", "long.fa", None, str(tmp_path), reach=1)
    driver.phase_tables("final.fa", "long.fa", "short.fq", str(tmp_path), long_pairs="ov.paf", reach=3, ins=True)
    driver.phase_tables("final.fa", "long.fa", None, str(tmp_path), ins=True)
    assert [(w, k) for w, _, k in seen] == [("phase_reads", dict(pairs=None)), ("phase_reads_ins", dict(pairs="ov.paf", reach=3)),
                                            ("phase_reads_ins", dict(pairs=None, reach=3)), ("phase_reads_ins", dict(pairs=None, reach=1))]
    assert [os.path.basename(x) for x in seen[1][1][2:5]] == [f"final_contigs.long.phase.{e}.tsv" for e in ("sites", "links", "reads")]
    assert seen[0][1][:5] == seen[1][1][:5] and seen[2][1][5].k == api.ava_opts_short().k


def test_phase_ins_text_host_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler on PATH")
    exe = tmp_path / "phase_ins_host_check"
    flags = ["-std=c++17", "-O1", "-ffp-contract=off", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.run([cxx, *flags, os.path.join(ROOT, "tests", "capi", "phase_ins_host_check.cpp"), "-o", str(exe)], check=True, cwd=ROOT)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "phase_ins_host_check: ok" in r.stdout
