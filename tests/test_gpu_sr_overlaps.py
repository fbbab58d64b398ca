"""GPU: hlmi_sr_overlaps against the chain it fuses.  Every case writes a small read set, runs the four existing calls one
after the other (ava with driver.contig_ava_opts -> filter_ovlp_inline -> minimap22sfo(0, 0) -> sfo2overlaps: the oracle,
each link pinned to the reference's scripts by goldens) and api.sr_overlaps on the same reads, and compares the two files
byte for byte - after asserting on the chain's own output that the case exercises what it is there for.

Sizes: id order 16 reads of 150 bases; rounding 5 reads of 60 .. 200 bases, twice; windows 64 reads of 150 bases (more than
1000 raw PAF rows); empty 2 reads and 1 read.  min_ovlp_len 40, identity 0.98, o 1, r 0.8 unless a case says otherwise.
"""
import numpy as np
import pytest

from hylight_amd import api, driver

pytestmark = pytest.mark.gpu
COMP = bytes.maketrans(b"ACGT", b"TGCA")


@pytest.fixture(scope="module", autouse=True)
def _init():
    api.init(0, 0)


def genome(seed, n):
    return bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(seed).integers(0, 4, size=n)])


def rc(s):
    return s.translate(COMP)[::-1]


def write_fastq(path, reads):
    with open(path, "wb") as f:
        for name, seq in reads:
            f.write(b"@%s\n%s\n+\n%s\n" % (str(name).encode(), seq, b"I" * len(seq)))


def chain(tmp, fq, n, min_len, iden=0.98, o=1, r=0.8):
    """The four calls -> (raw PAF lines, SAVAGE file bytes)."""
    fa, paf, flt, sfo, sav = (tmp / f"c.{e}" for e in ("fa", "paf", "flt", "sfo", "savage"))
    with open(fq) as f, open(fa, "w") as w:                    # fastq2fasta.py
        for k, line in enumerate(f):
            if k % 4 == 0:
                w.write(">" + line[1:])
            elif k % 4 == 1:
                w.write(line)
    api.ava(fa, fa, paf, driver.contig_ava_opts())
    api.filter_ovlp_inline(paf, flt, min_len, iden, o, r)
    api.minimap22sfo(flt, sfo, 0, 0.0)
    api.sfo2overlaps(sfo, sav, num_singles=n, num_pairs=0)
    return paf.read_text().splitlines(), sav.read_bytes()


def both(tmp_path, reads, min_len=40):
    fq = tmp_path / "reads.fastq"
    write_fastq(fq, reads)
    raw, want = chain(tmp_path, fq, len(reads), min_len)
    out = tmp_path / "fused.txt"
    n = api.sr_overlaps(fq, out, min_len, 0.98, 1, 0.8)
    got = out.read_bytes()
    assert n == got.count(b"\n")
    return raw, want, got


def rows(savage):
    return [l.split("\t") for l in savage.decode().splitlines()]


def test_id_order_string_against_number(tmp_path):
    """16 error-free reads of 150 bases, 30 apart on 600 bases, every third reverse-complemented; ids 8..15 and 98..105
    (they hold 8..11 and 98..101), dealt so that the file order is not the genome order: "10" < "8" and "100" < "98" as strings."""
    g = genome(11, 600)
    ids = [100, 9, 98, 11, 8, 101, 10, 99, 14, 103, 12, 105, 102, 15, 104, 13]
    tiles = []
    for k in range(16):
        s = g[30 * k:30 * k + 150]
        tiles.append((ids[k], rc(s) if k % 3 == 2 else s))
    order = [5, 12, 0, 9, 14, 3, 7, 10, 1, 15, 4, 8, 13, 2, 11, 6]
    reads = [tiles[k] for k in order]
    raw, want, got = both(tmp_path, reads)
    r = rows(want)
    assert len(r) >= 30
    assert any(x[5] == "-" or x[6] == "-" for x in r)
    assert any(int(x[0]) > int(x[1]) for x in r)
    assert any(str(x[0]) > str(x[1]) and int(x[0]) < int(x[1]) for x in r)      # the two orders disagree on a written pair
    assert got == want


def _rounding_reads(g, swap):
    # (offset, length): 80 @ 0 with 150 @ 30 -> 50 / 80 = 62.5; 80 @ 410 with 150 @ 420 -> 70 / 80 = 87.5; 60 inside 200
    spans = [(0, 80), (30, 150), (410, 80), (420, 150), (700, 200), (760, 60)]
    ids = [1, 2, 3, 4, 5, 6]
    if swap:
        ids = [2, 1, 4, 3, 6, 5]
    return [(i, g[o:o + n]) for i, (o, n) in zip(ids, spans)]


@pytest.mark.parametrize("swap", [False, True])
def test_rounding_and_overhang_branches(tmp_path, swap):
    """Reads cut from one sequence at chosen offsets: overlap 50 of 80 (62.5 -> 62, half to even), 70 of 80 (87.5 -> 88), a
    60-base read inside a 200-base one (ohb < 0, 100); then the same with the ids of each pair swapped."""
    g = genome(12, 1000)
    raw, want, got = both(tmp_path, _rounding_reads(g, swap))
    perc = sorted(int(x[7]) for x in rows(want))
    assert perc == [62, 88, 100], (perc, want)
    assert got == want


def test_more_than_1000_raw_rows(tmp_path):
    """64 reads of 150 bases from a 300-base region of two haplotypes 3 SNPs apart: about 2000 raw rows, so rows of one pair
    lie in different windows of the filter and the sort | uniq has rows to put together."""
    rng = np.random.default_rng(13)
    h0 = bytearray(genome(14, 300))
    h1 = bytearray(h0)
    for p in (75, 150, 225):
        h1[p] = ord("ACGT"[("ACGT".index(chr(h1[p])) + 1) % 4])
    reads = []
    for k in range(64):
        h = bytes(h1 if k % 2 else h0)
        s = int(rng.integers(0, 151))
        seq = h[s:s + 150]
        reads.append((int(k * 7 % 64), rc(seq) if k % 5 == 0 else seq))
    raw, want, got = both(tmp_path, reads)
    assert len(raw) > 1000, len(raw)
    assert want.count(b"\n") > 500
    assert got == want


def test_empty_results(tmp_path):
    for k, reads in enumerate(([(0, genome(15, 150)), (1, genome(16, 150))], [(0, genome(17, 150))])):
        d = tmp_path / str(k)
        d.mkdir()
        raw, want, got = both(d, reads)
        assert want == b"" and got == b""
        assert api.sr_overlaps(d / "reads.fastq", d / "again.txt", 40) == 0


@pytest.mark.parametrize("names", [("0", "r1"), ("3", "3"), ("7", "007"), ("-1", "2")])
def test_refusals_write_nothing(tmp_path, names):
    g = genome(18, 200)
    fq = tmp_path / "bad.fastq"
    write_fastq(fq, [(names[0], g[:150]), (names[1], g[40:190])])
    out = tmp_path / "out.txt"
    with pytest.raises(api.HlmiError) as e:
        api.sr_overlaps(fq, out, 40)
    assert e.value.code == -1                                   # HLMI_EINVAL
    assert not out.exists()
