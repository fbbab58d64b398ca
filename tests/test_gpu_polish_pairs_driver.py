"""GPU: the driver with --polish_strain.  On a simulated two-strain read set `--corrected --polish_direct --polish_strain
--stop_after polish` writes the contigs that direct api.polish_reads(..., pairs=<the stage's filtered PAF of the site>) calls
give, and two runs without the flag give one and the same file: the flag alone changes what the polisher is handed."""
import os

import pytest

from hylight_amd import api, driver, polish, simulate as S

pytestmark = pytest.mark.gpu


def run(lfq, out, *flags):
    argv = ["-l", str(lfq), "-o", str(out), "--corrected", "--nsplit", "3", "-t", "4", "--stop_after", "polish", "--polish_direct", *flags]
    assert driver.main(argv) == 0
    return out / "tmp"


def test_driver_polish_strain(tmp_path):
    reads, _ = S.simulate_reads(seed=83, n_strains=2, genome_len=30000, n_reads=90, mean_len=9000, min_len=7000, max_len=14000)
    lfq = tmp_path / "long.fq"
    S.write_fastq(reads, lfq)
    plain = [(run(lfq, tmp_path / f"plain{k}") / "long_con_polished.fa").read_bytes() for k in (0, 1)]
    assert plain[0] == plain[1] and plain[0].count(b">") >= 1
    tmp = run(lfq, tmp_path / "strain", "--polish_strain")
    got = (tmp / "long_con_polished.fa").read_bytes()
    assert got != plain[0]                                   # the lists change what the sites are handed
    # site 1 by hand: the same reads and contigs, and the stage's list - rows a later round appended to it name other contigs,
    # which this call does not know and ignores
    infile = tmp_path / "strain" / "1.split_fastx" / "s1.fa"
    out1, out2 = tmp_path / "by_hand1.fa", tmp_path / "by_hand2.fa"
    opts = dict(min_len=3000, min_iden=0.95)
    st = api.polish_reads(tmp / "contigs1.fa", infile, out1, polish.read_ava_opts(), pairs=tmp / "ov_long_ref.paf", **opts)
    assert st["pairs_listed"] > 0 and st["rows_selected"] > 0 and st["rows_not_listed"] > 0
    rounds = (tmp / "polish2.fa").exists()
    assert (st["pairs_unknown"] > 0) == rounds
    assert (tmp / "polish1.fa").read_bytes() == out1.read_bytes()
    p2 = (tmp / "polish2.fa").read_bytes() if rounds else b""
    if rounds:                                               # site 2: remain_con.fa and ov_long_ref2.paf are the last round's
        st2 = api.polish_reads(tmp / "remain_con.fa", infile, out2, polish.read_ava_opts(), pairs=tmp / "ov_long_ref2.paf", **opts)
        assert st2["pairs_listed"] > 0 and st2["pairs_unknown"] == 0
        assert out2.read_bytes() and p2.endswith(out2.read_bytes())
    want = b"".join(l if i % 2 else b">longr_con_%d\n" % (i // 2) for i, l in enumerate((out1.read_bytes() + p2).splitlines(keepends=True)))
    assert got == want
