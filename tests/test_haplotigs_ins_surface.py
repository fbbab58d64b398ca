"""CPU: hlmi_haplotigs_ins / hlmi_haplotigs_reads_ins without a GPU.  The header's prototypes and rules, the binding's SYMBOLS
entries and structs against the header's field lists; `--ins` on the haplotigs module and the driver's `--haplotigs_ins`, refused
without `--haplotigs`; the model (tests/haplotigs_ins_model.py) on the cases of tests/haplotigs_ins_inputs.py, each of which
asserts against literals where its block lies, and on two strains that differ by insertions alone; and
hylight_amd/csrc/haplotigs_ins_text.h compiled with the plain host compiler into tests/capi/haplotigs_ins_host_check.cpp's
program under the address and undefined-behaviour sanitizers and run directly."""
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
import haplotigs_ins_inputs as KI  # noqa: E402
import haplotigs_ins_model as KM  # noqa: E402
import haplotigs_reach_model as GR  # noqa: E402
import phase_ins_model as IM  # noqa: E402

HEADER = os.path.join(ROOT, "include", "hylight_mi.h")
DEFAULTS = dict(min_len=0, min_iden=0.0, min_cov=3, min_alt=2, min_frac=0.2, min_link=3, min_agree=0.8, min_side=3, include_unpolished=1)
CASES = KI.cases()


def test_header_prototypes_and_rules():
    text = open(HEADER).read()
    flat = re.sub(r"\s+", " ", text)
    assert ("int hlmi_haplotigs_ins(const char *contigs, const char *reads, const char *paf, const hlmi_haplotig_opts *o, int reach, "
            "const char *pairs_paf, const char *out_fa, const char *out_blocks, hlmi_haplotig_ins_stats *st);") in flat
    assert ("int hlmi_haplotigs_reads_ins(const char *contigs, const char *reads, const hlmi_ava_opts *ao, const hlmi_haplotig_opts *o, int reach, "
            "const char *pairs_paf, const char *out_fa, const char *out_blocks, hlmi_haplotig_ins_stats *st);") in flat
    assert re.findall(r"#define HLMI_ABI_VERSION (\d+)", text) == ["7"] and api.ABI_VERSION == 7
    # the older haplotig calls keep their prototypes
    assert ("int hlmi_haplotigs_reach(const char *contigs, const char *reads, const char *paf, const hlmi_haplotig_opts *o, int reach, "
            "const char *pairs_paf, const char *out_fa, const char *out_blocks, hlmi_haplotig_stats *st);") in flat
    rules = re.sub(r"\s+", " ", re.sub(r"\n \* ?", " ", text))
    for word in ("Position p is inside iff kf <= 2 p + 1 <= kl, slot p iff kf <= 2 p <= kl", "shuts them out of slot p and not out of position p",
                 "Every extent holds a position; extents never overlap", "((kl - 1) >> 1) - (kf >> 1) + 1 per extent",
                 "a shut slot has length 0", "byte for byte hlmi_haplotigs_reach's at the same reach", "no kernel of csrc/haplotigs.hip is launched",
                 "insertions of more than 16 bases", "hlmi_haplotigs_reach's, in its order, under these names", "in 12 bytes",
                 "tests/haplotigs_ins_model.py", "insertion sites as phasing evidence: hlmi_haplotigs_ins below"):
        assert word in rules, word


def test_symbols_and_structs():
    text = open(HEADER).read()
    body = re.search(r"typedef struct \{([^{}]*?)\} hlmi_haplotig_ins_stats;", text, re.S).group(1)
    fields = [tuple(reversed(d.split())) for d in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";") if d.strip()]
    ctype = {"uint64_t": C.c_uint64, "hlmi_haplotig_stats": api.HaplotigStats}
    assert [(n, ctype[t]) for n, t in fields] == list(api.HaplotigInsStats._fields_)
    assert tuple(n for n, t in fields if t == "uint64_t") == api.HAPLOTIG_INS_STATS == IM.INS_KEYS + ("diff_slots",) == KM.INS_KEYS
    assert C.sizeof(api.HaplotigInsStats) == C.sizeof(api.HaplotigStats) + 8 * 8
    assert set(KM.STAT_KEYS) == set(GR.STAT_KEYS) | set(KM.INS_KEYS)
    i, s, p = C.c_int, C.c_char_p, C.POINTER
    assert api.SYMBOLS["hlmi_haplotigs_ins"] == (i, [s, s, s, p(api.HaplotigOpts), i, s, s, s, p(api.HaplotigInsStats)])
    assert api.SYMBOLS["hlmi_haplotigs_reads_ins"] == (i, [s, s, p(api.AvaOpts), p(api.HaplotigOpts), i, s, s, s, p(api.HaplotigInsStats)])
    lib = api.load()
    assert all(getattr(lib, n) is not None for n in ("hlmi_haplotigs_ins", "hlmi_haplotigs_reads_ins"))
    o = api.HaplotigOpts(7, 0.5, 9, 9, 0.9, 9, 0.9, 9, 0)
    lib.hlmi_haplotig_opts_default(C.byref(o))
    assert {k: getattr(o, k) for k in DEFAULTS} == DEFAULTS
    with pytest.raises(TypeError):
        api.haplotigs_ins("c.fa", "r.fa", "p.paf", "o.fa", reach=2, qual_weight=1)
    with pytest.raises(TypeError):
        api.haplotigs_reads_ins("c.fa", "r.fa", "o.fa", window=500)


def test_sources_and_kernel_forms():
    from hylight_amd import build as B
    assert "haplotigs_ins_host.cpp" in B.sources() and "haplotigs.hip" in B.sources()
    kernel = open(os.path.join(ROOT, "hylight_amd", "csrc", "haplotigs.hip")).read()
    assert "template <int ENC, bool KEYS = false>" in kernel and "template <int MODE, int ENC, bool KEYS = false>" in kernel
    assert "constexpr int IV_CAP_KEYS = HAP_TILE + 1;" in kernel and "static_assert(2 * (IV_CAP_KEYS - 2) + 2 >= 2 * HAP_TILE" in kernel
    host = open(os.path.join(ROOT, "hylight_amd", "csrc", "haplotigs_ins_text.h")).read()
    assert "#include <hip" not in host and "_internal.h" not in host and '#include "haplotigs_text.h"' in host and '#include "phase_ins_text.h"' in host


def test_module_and_driver_options(tmp_path, monkeypatch):
    seen = []
    for name in ("haplotigs", "haplotigs_reads", "haplotigs_reach", "haplotigs_reads_reach", "haplotigs_ins", "haplotigs_reads_ins"):
        monkeypatch.setattr(api, name, lambda *a, _n=name, **k: seen.append((_n, a, k)) or {})
    base = ["--contigs", "c.fa", "--reads", "r.fq", "--out", "h.fa"]
    assert not haplotigs.build_parser().parse_args(base).ins
    # without --ins the older calls, with it hlmi_haplotigs_ins at reach 1 and above, with and without a PAF
    assert haplotigs.main(base + ["--paf", "p.paf"]) == 0 and seen[-1][0] == "haplotigs"
    assert haplotigs.main(base + ["--paf", "p.paf", "--reach", "3"]) == 0 and seen[-1][0] == "haplotigs_reach"
    assert haplotigs.main(base + ["--paf", "p.paf", "--blocks", "b.tsv", "--ins"]) == 0
    assert seen[-1] == ("haplotigs_ins", ("c.fa", "r.fq", "p.paf", "h.fa", "b.tsv"), dict(pairs=None, reach=1, **DEFAULTS))
    assert haplotigs.main(base + ["--paf", "p.paf", "--ins", "--reach", "3", "--pairs", "l.paf"]) == 0
    assert seen[-1] == ("haplotigs_ins", ("c.fa", "r.fq", "p.paf", "h.fa", None), dict(pairs="l.paf", reach=3, **DEFAULTS))
    assert haplotigs.main(base + ["--ins", "--reach", "2", "--short"]) == 0
    who, a, k = seen[-1]
    assert who == "haplotigs_reads_ins" and a[:4] == ("c.fa", "r.fq", "h.fa", None) and k == dict(pairs=None, reach=2, **DEFAULTS)
    assert a[4].pair_once == 0 and a[4].k == api.ava_opts_short().k
    # the driver: --haplotigs_ins is a flag of --haplotigs
    a = driver.build_parser().parse_args(["-l", "x.fq", "--haplotigs", "--haplotigs_ins", "--phase_reach", "4"])
    assert a.haplotigs and a.haplotigs_ins and a.phase_reach == 4 and not driver.build_parser().parse_args(["-l", "x.fq", "--haplotigs"]).haplotigs_ins
    with pytest.raises(SystemExit) as e:
        driver.main(["-l", "x.fq", "-o", str(tmp_path / "out"), "--haplotigs_ins"])
    assert "--haplotigs_ins" in str(e.value) and "--haplotigs " in str(e.value) and not os.path.exists(tmp_path / "out")
    del seen[:]
    driver.haplotig_files("final.fa", "long.fa", "short.fq", str(tmp_path), long_pairs="ov_long_ref.paf", short_pairs="shortr1.paf", reach=2, ins=True)
    assert [(w, k) for w, _, k in seen] == [("haplotigs_reads_ins", dict(pairs="ov_long_ref.paf", reach=2)),
                                            ("haplotigs_reads_ins", dict(pairs="shortr1.paf", reach=2))]
    del seen[:]
    driver.haplotig_files("final.fa", "long.fa", None, str(tmp_path), reach=2)
    assert [(w, k) for w, _, k in seen] == [("haplotigs_reads_reach", dict(pairs=None, reach=2))]


@pytest.mark.parametrize("name,reach", [(n, r) for n in sorted(CASES) for r in CASES[n].reaches])
def test_the_model_on_the_cases(name, reach):
    k = CASES[name]
    c = k.case
    fa, blocks, st = KM.haplotigs(c.contigs_bytes(), c.reads_bytes(), c.paf_bytes(), None, reach, **k.opts)
    k.where(reach, fa, blocks, st)
    assert st["blocks_split"] >= 1 and blocks.startswith(KM.BLOCKS_HEAD) and st["records"] == 2


def test_the_model_on_an_extent_from_a_slot_to_a_slot():
    """by hand: REF with TT in front of 5, T on 10 and C in front of 14 on side B; rows that start and end on the edges"""
    k = CASES["extent_from_a_slot_to_a_slot"]
    c = k.case
    fa, blocks, st = KM.haplotigs(c.contigs_bytes(), c.reads_bytes(), c.paf_bytes(), None, 1)
    ref = KI.REF
    hap_b = ref[:5] + b"TT" + ref[5:10] + b"T" + ref[11:14] + b"C" + ref[14:]
    assert fa == (GI.head(b"c_hapA", 20, 11, b"1.000000", 1, 9) + ref + b"\n" + GI.head(b"c_hapB", 23, 11, b"1.000000", 1, 9) + hap_b + b"\n")
    assert blocks == KM.BLOCKS_HEAD + b"c\t5+\t5+\t14+\t3\t4\t6\t1\t1\t2\n"
    assert (st["positions_split"], st["diff_positions"], st["diff_slots"], st["slots_opened"], st["inserted_bases"]) == (9, 1, 2, 2, 3)


def test_the_model_on_insertion_strains_only():
    s = KI.insertion_strains_only()
    c = s.case
    a = (c.contigs_bytes(), c.reads_bytes(), c.paf_bytes())
    fa1, blocks1, st1 = GR.haplotigs(*a)
    assert len(GI.records(fa1)) == 1 and st1["blocks_split"] == 0 and blocks1 == GR.GM.BLOCKS_HEAD
    fa, blocks, st = KM.haplotigs(*a)
    assert [n for n, _, _ in GI.records(fa)] == [b"major_contig_hapA", b"major_contig_hapB"]
    assert KI.block_rows(blocks) == [(b"major_contig", b"300+", b"300+", b"900+", 3, 8, 8, 1, 0, 3)]
    assert st["diff_positions"] == 0 and st["diff_slots"] == 3 and st["positions_split"] == 600


def test_no_insertion_site_is_the_reach_model():
    for name, h in sorted(GI.hand_cases().items()):
        c = h.case
        a = (c.contigs_bytes(), c.reads_bytes(), c.paf_bytes())
        popts = {k: v for k, v in h.opts.items() if k not in ("min_side", "include_unpolished")}
        for reach in (1, 2):
            fa, blocks, st = KM.haplotigs(*a, None, reach, **h.opts)
            if KM.takes_part(IM.phase(*a, None, reach, **popts)[0]):
                continue
            fa0, blocks0, st0 = GR.haplotigs(*a, None, reach, **h.opts)
            assert fa == fa0 and {k: st[k] for k in GR.STAT_KEYS} == st0, name
            assert blocks0 == b"".join(line.rsplit(b"\t", 1)[0] + b"\n" for line in blocks.split(b"\n")[:-1]), name


def test_haplotigs_ins_text_host_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler on PATH")
    exe = tmp_path / "haplotigs_ins_host_check"
    flags = ["-std=c++17", "-O1", "-ffp-contract=off", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.run([cxx, *flags, os.path.join(ROOT, "tests", "capi", "haplotigs_ins_host_check.cpp"), "-o", str(exe)], check=True, cwd=ROOT)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "haplotigs_ins_host_check: ok" in r.stdout
