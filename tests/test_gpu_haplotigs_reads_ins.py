"""GPU: hlmi_haplotigs_reads_ins against the chain hlmi_ava -> PAF -> hlmi_haplotigs_ins: both files byte for byte and every
integer stat, and the chain's against the model (tests/haplotigs_ins_model.py) on the PAF hlmi_ava wrote.  The two-strain set of
tests/test_gpu_variants_ins_reads.py, whose reads carry indels against their contigs: the fused call reads the overlapper's
resident read codes (hap_count_kernel<READS_CODES, true>), the chain the reads' ASCII.  Without a list both strains' reads lie on
either contig: blocks are split, the count kernel runs, and the insertion site that takes part lies inside a split extent.  With
the same-strain list no block is split; driver.haplotig_files with ins=True writes the same two files."""
import os
import sys

import pytest

from hylight_amd import api, driver

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import haplotigs_ins_inputs as KI  # noqa: E402
import haplotigs_ins_model as KM  # noqa: E402
import phase_ins_inputs as II  # noqa: E402
import phase_ins_model as IM  # noqa: E402
import polish_reads_inputs as RI  # noqa: E402
import test_gpu_variants_ins_reads as VR  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = ("fa", "blocks.tsv")
LOOSE = dict(min_side=1, min_link=2)


def ints(st):
    return {k: st[k] for k in KM.STAT_KEYS}


@pytest.fixture(scope="module")
def chain(tmp_path_factory):
    return VR.Chain(False, tmp_path_factory.mktemp("haplotigs_ins_long"))


def check(c, lst, reach, **more):
    """model == chain == fused call -> the model's (fasta, blocks, stats)"""
    c.n += 1
    opts = {**c.opts, **more}
    path = None
    if lst is not None:
        path = os.path.join(c.d, f"list{c.n}.paf")
        with open(path, "wb") as f:
            f.write(lst)
    want = KM.haplotigs(RI.fasta(c.contigs), RI.fasta(c.reads), c.paf_bytes, lst, reach, **opts)
    for who in ("chain", "direct"):
        out = [os.path.join(c.d, f"{who}{c.n}.{e}") for e in NAMES]
        st = (api.haplotigs_ins(c.cfa, c.rfa, c.paf, *out, pairs=path, reach=reach, **opts) if who == "chain" else
              api.haplotigs_reads_ins(c.cfa, c.rfa, *out, VR.ava_opts(False), pairs=path, reach=reach, **opts))
        assert ints(st) == want[2], who
        for p, data in zip(out, want[:2]):
            assert VR.read(p) == data, (who, p)
        assert (api.last_stats().get("kernel_ms.hap_count", 0) > 0) == (want[2]["blocks_split"] > 0), who
    return want


def test_the_fused_call_is_the_chain(chain):
    _, _, st = check(chain, None, 1)
    assert st["rows_selected"] >= 40 and st["blocks_split"] >= 2 and st["diff_positions"] >= 20
    # at reach 2 the first contig's blocks are one, and the insertion site that takes part lies inside its split extent
    _, blocks, st = check(chain, None, 2)
    sites = IM.phase(RI.fasta(chain.contigs), RI.fasta(chain.reads), chain.paf_bytes, None, 2, **chain.opts)[0]
    slots = [(r[0], r[1]) for r in II.site_rows(sites) if r[2].startswith(b"+")]
    split = [(r[0], int(r[2].rstrip(b"+")), int(r[3].rstrip(b"+"))) for r in KI.block_rows(blocks) if r[7]]
    assert st["blocks_split"] >= 1 and st["ins_sites_phasing"] >= 1 and st["slots_opened"] >= 1
    assert any(n == m and first < p <= last for n, p in slots for m, first, last in split), (slots, split)
    check(chain, None, 3, min_cov=1, min_alt=1, min_frac=0.0, min_link=1, min_agree=0.6, min_side=1)      # every column and slot that differs


def test_with_the_same_strain_list(chain):
    _, _, st = check(chain, chain.same_strain, 2, **LOOSE)
    assert st["rows_not_listed"] >= 10 and st["ins_sites_phasing"] >= 1
    fa, blocks, st0 = check(chain, b"", 2)
    assert st0["rows_selected"] == st0["blocks_split"] == st0["diff_slots"] == 0 and blocks == KM.BLOCKS_HEAD


def test_driver_haplotig_files_with_insertions(chain, tmp_path):
    c = chain
    out = tmp_path / "out"
    out.mkdir()
    lst = str(tmp_path / "ov_long_ref.paf")
    with open(lst, "wb") as f:
        f.write(c.same_strain)
    st = driver.haplotig_files(c.cfa, c.rfa, None, str(out), 0, long_pairs=lst, reach=2, ins=True)
    assert sorted(os.listdir(out)) == ["final_contigs.long.haplotigs.blocks.tsv", "final_contigs.long.haplotigs.fa"]
    want = KM.haplotigs(RI.fasta(c.contigs), RI.fasta(c.reads), c.paf_bytes, c.same_strain, 2)
    for e, data in zip(NAMES, want[:2]):
        assert (out / f"final_contigs.long.haplotigs.{e}").read_bytes() == data, e
    assert ints(st["long"]) == want[2]
