"""GPU: python -m hylight_amd.polyte on one simulated cluster, and the same sequence of library calls replayed by hand.

The cluster: two haplotypes of 1200 bases that differ every 40 bases, 180 error-free read pairs of 2 x 100 bases (about 15x per
haplotype), insert N(450, 27).  Every overlap of 50 bases and more covers a difference, no consensus ever writes N (min_qual 0)
and the reads carry no errors, so every contig must be a piece of one haplotype.
"""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from hylight_amd import api, min_ev, polyte, simulate as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GLEN, STEP, N_PAIRS, READ_LEN = 1200, 40, 180, 100
OPTS = ["-m", "50", "-m_EC", "60", "-t", "1", "--hap_cov", "10", "--insert_size", "450", "--stddev", "27", "--mismatch_rate", "0",
        "--min_clique_size", "2", "--average_read_len", str(READ_LEN), "--edge1", "0.93", "--edge2", "1.0", "--no_EC"]
STATE = ("singles.fastq", "subreads.txt", "overlaps.txt")
# the calls the loop makes on this fixture (fixed seed): reads 360 -> 356 -> 205 -> 116 -> 67 -> 38 -> 22 -> 13 -> 8 -> 5 -> 3, then the
# ninth merge leaves 2 reads and no overlap, the branch iteration and the final one find nothing to do
KINDS = ["clique_first"] + ["merge"] * 9 + ["branch", "final"]


def haplotypes():
    rng = np.random.default_rng(201)
    h0 = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=GLEN)].copy()
    h1 = h0.copy()
    for p in range(STEP // 2, GLEN, STEP):
        h1[p] = b"ACGT"[(b"ACGT".index(h1[p]) + 1 + int(rng.integers(0, 3))) % 4]
    return [h0, h1]


@pytest.fixture(scope="module")
def cluster(tmp_path_factory):
    d = tmp_path_factory.mktemp("polyte_in")
    haps = haplotypes()
    reads = S.simulate_short_pairs(202, haps, N_PAIRS, read_len=READ_LEN, err_sub=0.0)
    S.write_fastq(reads[0::2], d / "c.1.fq")
    S.write_fastq(reads[1::2], d / "c.2.fq")
    return d, haps


def snapshot(d):
    return {n: open(os.path.join(d, n), "rb").read() if os.path.exists(os.path.join(d, n)) else None for n in STATE}


@pytest.fixture(scope="module")
def cli_run(cluster, tmp_path_factory):
    d, _ = cluster
    w = tmp_path_factory.mktemp("polyte_cli")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "hylight_amd.polyte", "-p1", str(d / "c.1.fq"), "-p2", str(d / "c.2.fq"), *OPTS],
                       cwd=w, env=env, capture_output=True, text=True, timeout=120)
    return w, r


def test_cli_run(cli_run):
    w, r = cli_run
    print(r.stdout)
    assert r.returncode == 0, r.stderr
    a = w / "assembly"
    fa = w / "check.fasta"
    polyte.fastq2fasta(a / "singles.fastq", fa)
    assert (w / "contigs.fasta").read_bytes() == fa.read_bytes() and fa.stat().st_size > 0
    assert not (a / "original_overlaps.txt").exists()
    tab = w / "table.tsv"
    min_ev.write(tab, float(READ_LEN), 450.0 - 2 * READ_LEN, 27.0, 10.0)
    assert (a / "evidence_threshold_table.tsv").read_bytes() == tab.read_bytes()
    n_it = int(r.stdout.split("Assembly done in ")[1].split()[0])            # the reference counts from 1: calls + 1
    assert n_it - 1 >= 4                                                      # clique, merge, branch, final at the least
    # stats.txt: one line per iteration that built a graph with edges.  A call that constructs no edge ends at
    # ViralQuasispecies.cpp:284-291 - graph.txt removed, no line - in the reference as in the library; here that is the final
    # iteration, whose overlaps.txt is empty (test_replay_by_hand_matches_every_step counts the lines against the edge counts).
    lines = len((a / "stats.txt").read_text().splitlines())
    assert lines == n_it - 1 - (0 if (a / "graph.txt").exists() else 1)
    assert (a / "s_p1_p2.fastq").read_text().splitlines()[0::4] == [f"@{k}" for k in range(2 * N_PAIRS)]


def test_contigs_are_pieces_of_one_haplotype(cli_run, cluster):
    w, r = cli_run
    _, haps = cluster
    assert r.returncode == 0, r.stderr
    text = [h.tobytes().decode() for h in haps]
    text += [S.revcomp(h).tobytes().decode() for h in haps]
    contigs = (w / "contigs.fasta").read_text().splitlines()[1::2]
    assert contigs
    bad = [c for c in contigs if not any(c in t for t in text)]
    assert not bad, (len(bad), len(contigs))
    assert max(len(c) for c in contigs) > 2 * READ_LEN                        # reads were merged


def _replay_call(kind, cwd_fastq):
    """The library call of one iteration, written out from polyte.tune_params.py:689-743 for this fixture's options."""
    common = dict(keep_singletons=0, remove_trans=1, remove_tips=False, ignore_inclusions=False, merge_contigs=0.0, min_read_len=0,
                  max_tip_len=READ_LEN, remove_backedges=True, min_qual=0.0)
    if kind == "clique_first":
        api.vq_clique_iteration("s_p1_p2.fastq", "original_overlaps.txt", ".", min_overlap_len=60, edge_threshold=0.93, first_it=True,
                                min_clique_size=2, remove_branches=True, error_correction=False, **common)
    elif kind == "branch":
        api.vq_branch_iteration("singles.fastq", "overlaps.txt", cwd_fastq, "evidence_threshold_table.tsv", ".",
                                subreads_in="subreads.txt", min_overlap_len=50, edge_threshold=1.0, first_it=False, min_clique_size=2,
                                remove_branches=False, error_correction=False, se_count=0, pe_count=N_PAIRS, careful=True, **common)
    else:
        api.vq_iteration("singles.fastq", "overlaps.txt", ".", subreads_in="subreads.txt", min_overlap_len=50, edge_threshold=1.0,
                         first_it=False, min_clique_size=2, remove_branches=True, store_tips_separately=kind == "final", **common)
    if os.path.getsize("singles.fastq"):
        api.sr_overlaps("singles.fastq", "overlaps.txt", 50, 0.98, 1, 0.8)


def test_replay_by_hand_matches_every_step(cluster, cli_run, tmp_path, monkeypatch):
    """polyte.run in one directory with a snapshot of the state files after every step, the same calls made by hand from a
    literal list in another: the files agree after every step, and the lists run() returns have the lengths the calls imply."""
    d, _ = cluster
    api.init(0, 0)
    loop_dir, hand_dir = tmp_path / "loop", tmp_path / "hand"
    loop_dir.mkdir()
    hand_dir.mkdir()
    states = []
    real = {n: getattr(api, n) for n in ("vq_clique_iteration", "vq_iteration", "vq_branch_iteration")}
    pending = []

    def wrap(name):
        def fn(*a, **k):
            if pending:
                states.append(snapshot("."))                   # the step before this call is complete
            pending.append(name)
            return real[name](*a, **k)
        return fn

    for n in real:
        monkeypatch.setattr(api, n, wrap(n))
    monkeypatch.chdir(loop_dir)
    r = polyte.run(d / "c.1.fq", d / "c.2.fq", 50, 60, 10, 450, 27, READ_LEN, 2, 0.93, 1.0)
    states.append(snapshot("assembly"))
    for n, f in real.items():
        monkeypatch.setattr(api, n, f)
    calls = len(r["kinds"])
    print("kinds:", r["kinds"])
    assert (r["iterations"], len(r["reads"]), len(r["overlaps"]), len(r["edges"]), len(r["max_read_lengths"])) == \
        (calls + 1, calls + 1, calls + 1, calls, calls)
    assert r["reads"][0] == 2 * N_PAIRS and len(states) == calls
    stats_txt = (loop_dir / "assembly" / "stats.txt").read_text()
    assert len(stats_txt.splitlines()) == sum(e != -2 for e in r["edges"])     # -2: no graph.txt, the call ended at :284-291
    assert stats_txt == (cli_run[0] / "assembly" / "stats.txt").read_text()
    assert r["kinds"] == KINDS
    # by hand
    monkeypatch.chdir(hand_dir)
    shutil.copyfile(loop_dir / "assembly" / "s_p1_p2.fastq", "s_p1_p2.fastq")
    shutil.copyfile(loop_dir / "assembly" / "evidence_threshold_table.tsv", "evidence_threshold_table.tsv")
    api.sr_overlaps("s_p1_p2.fastq", "original_overlaps.txt", 60, 0.98, 1, 0.8)
    open("removed_tip_sequences.fastq", "w").close()
    for k, kind in enumerate(KINDS):
        _replay_call(kind, str(hand_dir / "s_p1_p2.fastq"))
        assert snapshot(".") == states[k], (k, kind)
