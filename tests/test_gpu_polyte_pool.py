"""GPU: the native POLYTE step in several processes (driver.polyte_native(..., workers=W), hylight_amd/polyte_pool.py) writes
what the loop in one process writes, byte for byte, in every cluster directory.

Five cluster directories made by hand under tmp/fq_60/ - 3, 7, 10, 21 with 40, 80, 150 and 300 simulated pairs of 2 x 150 bases
from two haplotypes of 3 kb at 1 % divergence (the smallest that still give several iterations of every kind), 40 with a .2.fq
one record short, which POLYTE refuses ("Unequal number of /1 and /2 reads": logged, no contigs.fasta).  The tree is copied; one
copy is run as before this argument existed, the others with 3 workers (two children: three processes on the card) and with 8
(more bins than clusters: the empty ones start nothing).  Run with one pytest process."""
import os
import shutil

import numpy as np
import pytest

from hylight_amd import api, driver, simulate as S

pytestmark = pytest.mark.gpu
SIZE, READ_LEN = 60, 150
PAIRS = {"3": 40, "7": 80, "10": 150, "21": 300, "40": 60}
NAMED = ("contigs.fasta", "log.txt", "assembly/singles.fastq", "assembly/subreads.txt", "assembly/stats.txt")


def tree_bytes(root):
    """Every file below `root`: relative path -> content."""
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            p = os.path.join(d, f)
            with open(p, "rb") as fh:
                out[os.path.relpath(p, root)] = fh.read()
    return out


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    """(the input tree, the files of its copy after the step in one process)."""
    base = tmp_path_factory.mktemp("polyte_pool")
    strains = S.make_strains(np.random.default_rng(301), 2, 3000, 0.01)
    for k, (cid, n) in enumerate(PAIRS.items()):
        d = base / "in" / f"fq_{SIZE}" / cid
        d.mkdir(parents=True)
        reads = S.simulate_short_pairs(310 + k, strains, n, read_len=READ_LEN)
        S.write_fastq(reads[0::2], d / f"{cid}.1.fq")
        S.write_fastq(reads[1::2][:n - 1] if cid == "40" else reads[1::2], d / f"{cid}.2.fq")
    api.init(0, 4)
    serial = base / "serial"
    shutil.copytree(base / "in", serial)
    driver.polyte_native(str(serial), SIZE, 450, READ_LEN)                     # as the parent commit is called
    return base, tree_bytes(serial / f"fq_{SIZE}")


def test_one_process_baseline_is_what_the_step_writes(trees):
    _, want = trees
    assert sum(len(want.get(f"{cid}/contigs.fasta", b"")) > 0 for cid in PAIRS) >= 2
    assert "40/contigs.fasta" not in want
    assert want["40/log.txt"] == b"hylight_amd.polyte: Unequal number of /1 and /2 reads\n"
    assert not [p for p in os.listdir(trees[0] / "serial") if p.startswith("polyte_share")]     # no worker was started


@pytest.mark.parametrize("workers", [3, 8])
def test_workers_write_the_same_files(trees, workers):
    base, want = trees
    tmp = base / f"w{workers}"
    shutil.copytree(base / "in", tmp)
    driver.polyte_native(str(tmp), SIZE, 450, READ_LEN, workers=workers, device=0, host_threads=4)
    got = tree_bytes(tmp / f"fq_{SIZE}")
    assert sorted(got) == sorted(want)
    for cid in PAIRS:
        for name in NAMED:
            key = f"{cid}/{name}"
            assert got.get(key) == want.get(key), key
    diff = [k for k in want if got[k] != want[k]]
    assert not diff, diff
    assert sum(len(got.get(f"{cid}/contigs.fasta", b"")) > 0 for cid in PAIRS) >= 2
    # five clusters: 3 workers fill their bins, 8 leave three empty - bin 0 is this process, the others one child each
    shares = sorted(p for p in os.listdir(tmp) if p.startswith("polyte_share_") and p.endswith(".txt"))
    assert len(shares) == min(workers, len(PAIRS)) - 1
