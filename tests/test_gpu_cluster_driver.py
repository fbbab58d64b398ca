"""GPU: the driver's opt-in short-read branch - `--stop_after clusters` (the clustering of HyLight.py:215-226 into tmp/)
and `--polyte_cmd` (POLYTE per cluster and the contig hand-over of HyLight.py:228-275) - on a small simulated hybrid
set.  racon and POLYTE are external: stubs written into tmp_path stand in for them."""
import os
import stat
import sys

import pytest

from hylight_amd import driver, simulate as S

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cluster_model as CM  # noqa: E402

pytestmark = pytest.mark.gpu
SIZE, THREADS = 60, 4


def _exe(path, text):
    path.write_text(text)
    path.chmod(path.stat().st_mode | stat.S_IEXEC)
    return path


def _hybrid(tmp_path, monkeypatch):
    reads, strains = S.simulate_reads(seed=83, n_strains=2, genome_len=30000, n_reads=90, mean_len=9000, min_len=7000,
                                      max_len=14000)
    lfq, sfq = tmp_path / "long.fq", tmp_path / "short.fq"
    S.write_fastq(reads, lfq)
    S.write_fastq(S.simulate_short_pairs(84, strains, 2500, read_len=150), sfq)
    bin_dir = tmp_path / "bin"
    bin_dir.mkdir()
    _exe(bin_dir / "racon", '#!/bin/sh\ncat "$7"\n')               # racon ... reads overlaps contigs: contigs unchanged
    monkeypatch.setenv("PATH", f"{bin_dir}:{os.environ['PATH']}")
    return lfq, sfq


def _cluster_tree(tmp):
    keep = ("readnames.txt", f"HiStrain_max{SIZE}_final_clusters_grouped.json")
    return {k: v for k, v in CM.tree(tmp).items() if k in keep or k.startswith(f"fq_{SIZE}/")}


def test_driver_stop_after_clusters_matches_model(tmp_path, monkeypatch):
    lfq, sfq = _hybrid(tmp_path, monkeypatch)
    out = tmp_path / "OUT"
    rc = driver.main(["-l", str(lfq), "-s", str(sfq), "-o", str(out), "--corrected", "--nsplit", "3", "-t", str(THREADS),
                      "--size", str(SIZE), "--stop_after", "clusters"])
    assert rc == 0
    tmp = out / "tmp"
    paf = (tmp / "shortr2.paf").read_bytes() if (tmp / "shortr2.paf").exists() else b""
    want, st = CM.run(paf, sfq.read_bytes(), SIZE, THREADS)
    assert st["names"] == 2500
    assert _cluster_tree(tmp) == want
    assert not (out / "all_contigs.fa").exists()


def test_driver_polyte_cmd_hands_over_the_cluster_contigs(tmp_path, monkeypatch):
    lfq, sfq = _hybrid(tmp_path, monkeypatch)
    polyte = _exe(tmp_path / "bin" / "polyte_stub",
                  '#!/bin/sh\nd=$(basename "$PWD")\nprintf ">cl_%s\\n%s\\n" "$d" "$(printf \'ACGT%.0s\' $(seq 60))" '
                  '> contigs.fasta\n')
    out = tmp_path / "OUT"
    rc = driver.main(["-l", str(lfq), "-s", str(sfq), "-o", str(out), "--corrected", "--nsplit", "3", "-t", str(THREADS),
                      "--size", str(SIZE), "--polyte_cmd", str(polyte)])
    assert rc == driver.EXIT_NO_FINAL                   # no --stageb_cmd: final_contigs.fa is not written
    tmp = out / "tmp"
    ids = sorted(os.listdir(tmp / f"fq_{SIZE}"))
    lines = (tmp / "cmd_polyte.sh").read_text().splitlines()
    assert len(lines) == len(ids)
    assert all(f"{polyte} -p1 " in l and "--insert_size  450" in l and "--average_read_len 250" in l for l in lines)
    want = "".join(f">cl_{i}\n{'ACGT' * 60}\n" for i in ids)
    assert (tmp / f"all.contigs_{SIZE}.fasta").read_text() == want
    assert not (out / "short_stageb.fa").exists()
    assert (out / "all_contigs.fa").read_text() == want + (out / "long_con_polished.fa").read_text()
