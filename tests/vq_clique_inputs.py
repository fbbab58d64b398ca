"""Inputs of tests/test_gpu_vq_cliques.py.  TEST INFRASTRUCTURE ONLY."""
import random

import numpy as np

from hylight_amd import simulate as S


def haplotype_reads(seed=5, n_strains=3, genome_len=2000, n_reads=400, read_len=150, err=0.01, snp_rate=0.01):
    """Short single-end reads of `n_strains` haplotypes (hylight_amd.simulate.make_strains) with substitution errors and
    qualities that know about them: a correct base mostly phred 30 .. 40, a wrong one mostly 8 .. 20.  -> [(start, haplotype,
    sequence, qualities)] ordered by start."""
    strains = S.make_strains(np.random.default_rng(seed), n_strains, genome_len, snp_rate)
    rng = random.Random(seed)
    reads = []
    for _ in range(n_reads):
        h = rng.randrange(n_strains)
        g = strains[h].tobytes().decode()
        s = rng.randrange(len(g) - read_len + 1)
        seq, qual = [], []
        for c in g[s:s + read_len]:
            if rng.random() < err:
                c = rng.choice([b for b in "ACGT" if b != c])
                q = rng.randint(8, 20) if rng.random() < 0.8 else rng.randint(30, 40)
            else:
                q = rng.randint(30, 40) if rng.random() < 0.9 else rng.randint(12, 29)
            seq.append(c)
            qual.append(chr(33 + q))
        reads.append((s, h, "".join(seq), "".join(qual)))
    reads.sort(key=lambda r: r[0])
    return reads


def write_inputs(reads, fq, ov, min_ovl=60):
    """singles.fastq (ids 0 ..) and the overlaps the coordinates give, every pair of reads that share min_ovl columns and more,
    whichever haplotype they come from: the score decides which of them are edges."""
    with open(fq, "w") as f:
        f.write("".join(f"@{k}\n{s}\n+\n{q}\n" for k, (_, _, s, q) in enumerate(reads)))
    rows = []
    for i, (si, _, a, _) in enumerate(reads):
        for j in range(i + 1, len(reads)):
            sj, b = reads[j][0], reads[j][2]
            n = min(si + len(a), sj + len(b)) - sj
            if n < min_ovl:
                break
            rows.append(f"{i}\t{j}\t{sj - si}\t-\t-\t+\t+\t{100 * n // min(len(a), len(b))}\t-\t{n}\t-\ts\ts\n")
    with open(ov, "w") as f:
        f.write("".join(rows))
    return len(rows)
