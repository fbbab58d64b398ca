"""GPU: the driver's --variants_qual, through driver.variant_tables as --variants is tested: the file names are those of the run
without the flag; with FASTA long reads the long files equal that run's byte for byte (every column passes, no read is low: the
identity), the short-read FASTQ is where the floors bite, and its files are the model's (tests/variants_qual_model.py) on the PAF
hlmi_ava writes; with ins=True the third file appears beside them."""
import os
import sys

import pytest

from hylight_amd import api, driver

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import polish_qual_inputs as QI  # noqa: E402
import polish_reads_inputs as RI  # noqa: E402
import variants_qual_model as VQ  # noqa: E402

pytestmark = pytest.mark.gpu
QUAL = dict(min_base_qual=10, min_avg_qual=10.0)


def test_driver_variants_qual(tmp_path):
    long_in, _ = QI.overlap_input(0)
    short_in, quals = QI.overlap_input(1)
    contigs = list(long_in.contigs) + [("s0", short_in.contigs[0][1])]          # the long reads' two contigs, the short reads' one
    cfa, lfa, sfq = tmp_path / "final.fa", tmp_path / "long.fa", tmp_path / "short.fq"
    cfa.write_bytes(RI.fasta(contigs))
    lfa.write_bytes(RI.fasta(long_in.reads))
    sfq.write_bytes(QI.fastq(short_in.reads, quals))
    plain, qual, ins = tmp_path / "plain", tmp_path / "qual", tmp_path / "ins"
    for d in (plain, qual, ins):
        d.mkdir()
    st0 = driver.variant_tables(str(cfa), str(lfa), str(sfq), str(plain), 0)
    st = driver.variant_tables(str(cfa), str(lfa), str(sfq), str(qual), 0, qual=QUAL)
    names = [f"final_contigs.{k}.variants.{e}" for k in ("long", "short") for e in ("summary.tsv", "tsv")]
    assert sorted(os.listdir(plain)) == sorted(os.listdir(qual)) == names
    for n in names[:2]:                                                        # FASTA long reads: the identity
        assert (qual / n).read_bytes() == (plain / n).read_bytes(), n
    assert st["long"]["columns_low_qual"] == st["long"]["rows_low_qual"] == st["long"]["reads_with_qual"] == 0
    assert {k: st["long"][k] for k in api.VARIANT_STATS} == {k: st0["long"][k] for k in api.VARIANT_STATS}
    # the short-read FASTQ: the floors bite, and the files are the model's
    assert st["short"]["columns_low_qual"] > 0 and st["short"]["reads_with_qual"] == len(short_in.reads)
    assert (qual / names[3]).read_bytes() != (plain / names[3]).read_bytes()
    paf = tmp_path / "short.paf"
    o = api.ava_opts_short()
    o.pair_once = 0
    api.ava(str(cfa), str(sfq), str(paf), o)
    want = VQ.variants_q(cfa.read_bytes(), sfq.read_bytes(), paf.read_bytes(), **QUAL)
    assert (qual / names[3]).read_bytes() == want[0] and (qual / names[2]).read_bytes() == want[1]
    assert {k: st["short"][k] for k in VQ.STAT_KEYS} == want[2]
    # with the insertion sites: the third file per read set, the other two unchanged
    driver.variant_tables(str(cfa), str(lfa), str(sfq), str(ins), 0, ins=True, qual=QUAL)
    assert sorted(os.listdir(ins)) == sorted(names + [f"final_contigs.{k}.variants.ins.tsv" for k in ("long", "short")])
    assert (ins / names[3]).read_bytes() == want[0] and (ins / names[1]).read_bytes() == (plain / names[1]).read_bytes()
