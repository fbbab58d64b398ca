"""GPU: the driver's `--polyte_native` on the small hybrid set of test_gpu_cluster_driver.py - the library's own POLYTE in every
cluster directory, then the hand-over of HyLight.py:244-275 exactly as behind `--polyte_cmd`."""
import os
import stat

import pytest

from hylight_amd import driver, simulate as S

pytestmark = pytest.mark.gpu
SIZE, THREADS = 60, 4


def _hybrid(tmp_path, monkeypatch):
    reads, strains = S.simulate_reads(seed=83, n_strains=2, genome_len=30000, n_reads=90, mean_len=9000, min_len=7000,
                                      max_len=14000)
    lfq, sfq = tmp_path / "long.fq", tmp_path / "short.fq"
    S.write_fastq(reads, lfq)
    S.write_fastq(S.simulate_short_pairs(84, strains, 2500, read_len=150), sfq)
    bin_dir = tmp_path / "bin"
    bin_dir.mkdir()
    racon = bin_dir / "racon"
    racon.write_text('#!/bin/sh\ncat "$7"\n')                     # racon ... reads overlaps contigs: contigs unchanged
    racon.chmod(racon.stat().st_mode | stat.S_IEXEC)
    monkeypatch.setenv("PATH", f"{bin_dir}:{os.environ['PATH']}")
    return lfq, sfq


def test_driver_polyte_native_hands_over_the_cluster_contigs(tmp_path, monkeypatch, capsys):
    lfq, sfq = _hybrid(tmp_path, monkeypatch)
    out = tmp_path / "OUT"
    rc = driver.main(["-l", str(lfq), "-s", str(sfq), "-o", str(out), "--corrected", "--nsplit", "3", "-t", str(THREADS),
                      "--size", str(SIZE), "--average_read_len", "150", "--polyte_native"])
    assert rc == driver.EXIT_NO_FINAL                   # no --stageb_cmd: final_contigs.fa is not written, as behind --polyte_cmd
    tmp = out / "tmp"
    ids = sorted(os.listdir(tmp / f"fq_{SIZE}"))
    assert len(ids) >= 2
    assert not (tmp / "cmd_polyte.sh").exists()
    want, with_contigs = b"", 0
    for i in ids:
        d = tmp / f"fq_{SIZE}" / i
        assert (d / "log.txt").exists()
        if (d / "contigs.fasta").exists():
            assert (d / "assembly" / "s_p1_p2.fastq").exists() and not (d / "assembly" / "original_overlaps.txt").exists()
            want += (d / "contigs.fasta").read_bytes()
            with_contigs += 1
    assert with_contigs >= 1 and want.count(b">") >= 1
    printed = capsys.readouterr().out
    assert printed.count("You need to rerun polyte in") == len(ids) - with_contigs
    assert (tmp / f"all.contigs_{SIZE}.fasta").read_bytes() == want
    assert not (out / "short_stageb.fa").exists()
    assert (out / "all_contigs.fa").read_bytes() == want + (out / "long_con_polished.fa").read_bytes()


def test_both_polyte_flags_are_refused(tmp_path):
    with pytest.raises(SystemExit) as e:
        driver.main(["-l", str(tmp_path / "x.fq"), "-o", str(tmp_path / "OUT"), "--polyte_native", "--polyte_cmd", "polyte"])
    assert "--polyte_native" in str(e.value)
    assert not (tmp_path / "OUT").exists()
