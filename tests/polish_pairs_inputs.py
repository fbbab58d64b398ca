"""Inputs of the pair-list tests (hlmi_polish_pairs / hlmi_polish_reads_pairs, tests/polish_pairs_model.py): hand cases with
their answers written out, the two-strain case that states what the list is for, and lists of an exact number of distinct keys
around the borders of the device's key search.  Everything comes from seeds; nothing is read from a file."""
import collections

import numpy as np

import polish_inputs as PI
import polish_reads_inputs as RI
from hylight_amd import simulate as S

REF = b"ACGTACGTAC"
Hand = collections.namedtuple("Hand", "case pairs want stats refused_line")


def row(a, b, n_fields=6, end=b"\n"):
    """a list row with a in field 1 and b in field 6; 14 fields: the stage's scored row, with its trailing TAB"""
    f = [a, b"10", b"0", b"10", b"+", b, b"10", b"0", b"10", b"10", b"10", b"0.9876", b"3", b"1.0000", b""]
    return b"\t".join(f[:n_fields] if n_fields < 14 else f) + end


def _head(name, ln, rc):
    return b">%s LN:i:%d RC:i:%d XC:f:1.000000\n" % (name, ln, rc)


def vote_case():
    """contig c = REF (min_cov 1); r1 votes C, r10 votes G and r2 votes A on position 4: all three leave the contig's A (a
    three-way tie with the own base among the tied), r1 alone C, r10 alone G, r1 and r10 C (the first of A C G T)"""
    c = PI.Case([("c", REF)], dict(min_cov=1))
    c.add(0, "4=1X5=", REF[:4] + b"C" + REF[5:], name="r1")
    c.add(0, "4=1X5=", REF[:4] + b"G" + REF[5:], name="r10")
    c.add(0, "10=", REF, name="r2")
    return c


def _voted(base, rc):
    return _head(b"c", 10, rc) + REF[:4] + base + REF[5:] + b"\n"


def hand_cases():
    """name -> Hand(case, list bytes, expected file, expected non-zero stats, refused line), each worked by hand from the
    header's rules"""
    H = {}
    base = dict(rows=3, contigs=1)
    one = dict(base, rows_selected=1, contigs_polished=1, substituted=1, rows_not_listed=2, pairs_listed=1)
    H["reverse_order"] = Hand(vote_case(), row(b"c", b"r10", 14), _voted(b"G", 1), one, 0)
    H["duplicate_rows"] = Hand(vote_case(), row(b"r1", b"c") * 3, _voted(b"C", 1), one, 0)
    H["prefix_r1_not_r10"] = Hand(vote_case(), row(b"r1", b"c", 12), _voted(b"C", 1), one, 0)
    H["prefix_r10_not_r1"] = Hand(vote_case(), row(b"r10", b"c", 12), _voted(b"G", 1), one, 0)
    none = dict(base, rows_not_listed=3)
    H["crlf_matches_nothing"] = Hand(vote_case(), row(b"r1", b"c", end=b"\r\n"), b">c\n" + REF + b"\n", dict(none, pairs_unknown=1), 0)
    H["crlf_behind_field_14"] = Hand(vote_case(), row(b"r1", b"c", 14, end=b"\r\n"), _voted(b"C", 1), one, 0)
    H["no_trailing_newline"] = Hand(vote_case(), row(b"r1", b"c") + row(b"r10", b"c", end=b""), _voted(b"C", 2),
                                    dict(base, rows_selected=2, contigs_polished=1, substituted=1, rows_not_listed=1, pairs_listed=2), 0)
    H["five_fields_on_line_2"] = Hand(vote_case(), row(b"r1", b"c") + row(b"r10", b"c", 5) + row(b"r2", b"c", 3), None, None, 2)
    H["empty_line"] = Hand(vote_case(), row(b"r1", b"c") + row(b"r2", b"c") + b"\n" + row(b"r10", b"c"), None, None, 3)
    H["empty_list"] = Hand(vote_case(), b"", b">c\n" + REF + b"\n", none, 0)
    H["every_pair"] = Hand(vote_case(), row(b"r1", b"c") + row(b"c", b"r2", 14) + row(b"r10", b"c", 12), _head(b"c", 10, 3) + REF + b"\n",
                           dict(base, rows_selected=3, contigs_polished=1, pairs_listed=3), 0)
    H["foreign_contig"] = Hand(vote_case(), row(b"r1", b"c") + row(b"r1", b"remain_7") + row(b"utg9", b"c"), _voted(b"C", 1),
                               dict(one, pairs_unknown=2), 0)
    H["one_name_twice"] = Hand(vote_case(), row(b"r1", b"r1") + row(b"c", b"c"), b">c\n" + REF + b"\n", none, 0)

    # read r0 has a row of 20 columns on c2, not listed, and one of 10 columns on c1, listed: the long row claims nothing
    c2 = b"ACGTACGTACGGTTAACCGG"
    c = PI.Case([("c1", b"ACGTTCGTAC"), ("c2", c2)], dict(min_cov=1))
    c.add(0, "20=", c2, target="c2", name="r0")
    c.add(0, "4=1X5=", c2[:10], target="c1", read="r0")
    H["unlisted_long_row_does_not_shadow"] = Hand(c, row(b"r0", b"c1"), _head(b"c1", 10, 1) + c2[:10] + b"\n>c2\n" + c2 + b"\n",
                                                  dict(rows=2, contigs=2, rows_selected=1, contigs_polished=1, substituted=1,
                                                       rows_not_listed=1, pairs_listed=1), 0)
    return H


# ---- two strains: the point of the list --------------------------------------------------------------------------------------
Strains = collections.namedtuple("Strains", "case minor major snps same_strain_list starts per_start")


def two_strains(seed=4242, genome_len=3000, read_len=1000, step=500, minor_copies=3, ratio=5):
    """Two strains of 3 kb (simulate.make_strains), error-free reads of 1 kb on a grid of starts, `minor_copies` of the minor
    strain and ratio x as many of the major one at every start: 5 k : k votes on every position.  The contig is the minor
    strain's genome; every read has one row over its whole length (hand-built, as simulate.truth_paf would give for error-free
    reads: runs of = with an X on every SNP)."""
    rng = np.random.default_rng(seed)
    major, minor = (bytes(s.tobytes()) for s in S.make_strains(rng, 2, genome_len, 0.01))
    snps = [p for p in range(genome_len) if major[p] != minor[p]]
    case = PI.Case([("minor_contig", minor)], dict(min_cov=3, min_len=500))
    starts = list(range(0, genome_len - read_len + 1, step))
    same = b""
    for s in starts:
        for k in range(minor_copies * (1 + ratio)):
            is_minor = k % (1 + ratio) == 0                   # the strains interleaved in file order
            seg = (minor if is_minor else major)[s:s + read_len]
            runs, n = [], 0
            for j in range(read_len):
                if seg[j] == minor[s + j]:
                    n += 1
                else:
                    runs.append(f"{n}=1X" if n else "1X")
                    n = 0
            if n:
                runs.append(f"{n}=")
            name = f"{'min' if is_minor else 'maj'}_{s}_{k}"
            case.add(s, "".join(runs), seg, strand="-" if k % 2 else "+", name=name)
            if is_minor:
                same += row(name.encode(), b"minor_contig", 14)
    return Strains(case, minor, major, snps, same, starts, minor_copies)


# ---- the fused call: generated reads with names around the real ones -------------------------------------------------------
def fused_input(contig_name):
    """tests/polish_reads_inputs.py's long input, its middle contig alone under `contig_name`, and 200 reads of 40 random bases
    that align nowhere: a000 .. a099 sort in front of every real name, z000 .. z099 behind"""
    inp = RI.every_kind_long()
    rng = np.random.default_rng(77)
    fill = [(f"{p}{i:03d}", RI.genome(rng, 40)) for p in "az" for i in range(100)]
    return RI.Input([(contig_name, inp.contigs[1][1])], inp.reads + fill, False, inp.opts)


def list_of_keys(n_keys, real_pairs, side):
    """A list with exactly n_keys distinct known keys: the real (read, contig) pairs first, two keys each (an odd count: one
    row naming the side's first fill name twice, a single key), then pairs of fill names on `side` ("a": in front of the real keys, "z": behind, "az": in
    turn) -> (list bytes, the real pairs that got in)"""
    out, got, left = [], [], n_keys
    if left % 2:
        out.append(row(b"%s000" % side[:1].encode(), b"%s000" % side[:1].encode()))
        left -= 1
    for q, t in real_pairs:
        if left < 2:
            break
        out.append(row(q, t, 14) if len(got) % 2 else row(t, q))
        got.append((q, t))
        left -= 2
    k = 0
    for i in range(100):
        for j in range(i + 1, 100):
            if left < 2:
                break
            p = side[k % len(side)]
            out.append(row(b"%s%03d" % (p.encode(), i), b"%s%03d" % (p.encode(), j), 12))
            k += 1
            left -= 2
    assert left == 0, (n_keys, left)
    return b"".join(out), got


def sorted_keys(list_bytes, names):
    """the device's key array for a list, from the strcmp ranks of `names` (bytes): [(rank_a, rank_b)] ascending"""
    rank = {n: i for i, n in enumerate(sorted(set(names)))}
    keys = set()
    for line in list_bytes.split(b"\n")[:-1]:
        f = line.split(b"\t")
        if f[0] in rank and f[5] in rank:
            keys.add((rank[f[0]], rank[f[5]]))
            keys.add((rank[f[5]], rank[f[0]]))
    return sorted(keys), rank
