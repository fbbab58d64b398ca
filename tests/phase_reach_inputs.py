"""Inputs of the tests of hlmi_phase_reach (against tests/phase_reach_model.py), built with tests/phase_inputs.py's helpers.

hand_cases(): piles on phase_inputs.REF with the three files written out by hand from the header's rules - a noisy site between
two linked ones (far link cis, far link trans), two noisy sites in a row at reach 2 (still cut) and at reach 3 (joined), a far link
that contradicts the bits the near links gave.
shapes(): piles at the smallest sizes where phase_link_reach_kernel can go wrong - PHASE_REACH_TILE is read from the kernels'
header.  Each shape comes with the reaches to run it at and `where`, a function of (reach, the model's output) that asserts the
case sits where it claims to.
noisy_two_strains(): polish_pairs_inputs.two_strains() with added sites whose alt allele rides on every other read of both strains.

-> {name: Hand(case, opts, reach, sites lines, links lines, reads lines, non-zero stats)}, {name: Shape(case, opts, reaches, where)}"""
import collections

import numpy as np

import phase_inputs as HI
import polish_inputs as PI
from hylight_amd import simulate as S

Hand = collections.namedtuple("Hand", "case opts reach sites links reads stats")
Shape = collections.namedtuple("Shape", "case opts reaches where")
TILE = HI._constant("phase_internal.h", r"constexpr int PHASE_REACH_TILE = (\d+);")
REACH_MAX = HI._constant("phase_reach_text.h", r"constexpr int PHASE_REACH_MAX = (\d+);")
REF = HI.REF


def hand_cases():
    H = {}
    base = dict(contigs=1, contigs_covered=1, positions=20, callable=20)
    # REF has G on positions 2, 6, 10, 14; T is the other allele everywhere below

    def one(name, reads, reach, site_lines, link_lines, read_lines, opts=None, **stats):
        n = len(reads)
        H[name] = Hand(HI.pile(REF, reads), opts or {}, reach, site_lines, link_lines, read_lines, {**base, "rows": n, "rows_selected": n, **stats})

    # r0 - r2 carry T on 2 and 10, r3 - r5 the contig's G; r0 and r3 - one read of either side - carry T on 6.  Both links of
    # site 6 are ties (cis 3, trans 3); the link (2, 10) is cis 6 of 6: site 10 joins site 2's block, site 6 is bridged
    noisy = [{2: b"T", 6: b"T", 10: b"T"}, {2: b"T", 10: b"T"}, {2: b"T", 10: b"T"}, {6: b"T"}, {}, {}]
    one("noisy_site_between_two_cis", noisy, 2,
        [b"c\t3\tG\tT\t6\t3\t3\t3\t0|1", b"c\t7\tG\tT\t6\t4\t2\t3\t.", b"c\t11\tG\tT\t6\t3\t3\t3\t0|1"],
        [b"c\t3\t7\t2\t1\t2\t1\t6\t0.500000\t-", b"c\t3\t11\t3\t0\t0\t3\t6\t1.000000\tcis", b"c\t7\t11\t2\t2\t1\t1\t6\t0.500000\t-"],
        [b"r%d\tc\t3\t3\t0\t2\t0\tB" % i for i in range(3)] + [b"r%d\tc\t3\t3\t2\t0\t0\tA" % i for i in range(3, 6)],
        sites=3, sites_base=3, links=2, blocks=1, blocks_multi=1, sites_phased=2, alleles=18, read_records=6, reads_a=3, reads_b=3,
        links_far=1, links_far_phased=1, joins_far=1, sites_bridged=1)
    # the same with T on 2 against T on 10: the far link is trans, site 10 gets bit 1 through it
    noisy = [{2: b"T", 6: b"T"}, {2: b"T"}, {2: b"T"}, {6: b"T", 10: b"T"}, {10: b"T"}, {10: b"T"}]
    one("noisy_site_between_two_trans", noisy, 2,
        [b"c\t3\tG\tT\t6\t3\t3\t3\t0|1", b"c\t7\tG\tT\t6\t4\t2\t3\t.", b"c\t11\tG\tT\t6\t3\t3\t3\t1|0"],
        [b"c\t3\t7\t2\t1\t2\t1\t6\t0.500000\t-", b"c\t3\t11\t0\t3\t3\t0\t6\t1.000000\ttrans", b"c\t7\t11\t2\t2\t1\t1\t6\t0.500000\t-"],
        [b"r%d\tc\t3\t3\t0\t2\t0\tB" % i for i in range(3)] + [b"r%d\tc\t3\t3\t2\t0\t0\tA" % i for i in range(3, 6)],
        sites=3, sites_base=3, links=2, blocks=1, blocks_multi=1, sites_phased=2, alleles=18, read_records=6, reads_a=3, reads_b=3,
        links_far=1, links_far_phased=1, joins_far=1, sites_bridged=1)
    # sites 2, 6, 10, 14: r0 - r2 carry T on 2 and 14, r3 - r5 G; T on 6 in r0 and r3, T on 10 in r1 and r4.  Every link but
    # (2, 14) is unphased (ties, and (6, 10) with 4 of 6): at reach 2 the link (2, 14) does not exist and every site is a block
    # of one; at reach 3 site 14 joins site 2's block across two bridged sites
    two = [{2: b"T", 6: b"T", 14: b"T"}, {2: b"T", 10: b"T", 14: b"T"}, {2: b"T", 14: b"T"}, {6: b"T"}, {10: b"T"}, {}]
    near = [b"c\t3\t7\t2\t1\t2\t1\t6\t0.500000\t-", b"c\t3\t11\t2\t1\t2\t1\t6\t0.500000\t-", b"c\t7\t11\t2\t2\t2\t0\t6\t0.666667\t-",
            b"c\t7\t15\t2\t2\t1\t1\t6\t0.500000\t-", b"c\t11\t15\t2\t2\t1\t1\t6\t0.500000\t-"]
    alt = [{0: 1, 1: 1, 3: 1}, {0: 1, 2: 1, 3: 1}, {0: 1, 3: 1}, {1: 1}, {2: 1}, {}]         # site index -> allele 1, per read
    four = dict(sites=4, sites_base=4, links=3, alleles=24)
    one("two_noisy_sites_in_a_row_reach_2", two, 2,
        [b"c\t3\tG\tT\t6\t3\t3\t3\t0|1", b"c\t7\tG\tT\t6\t4\t2\t7\t0|1", b"c\t11\tG\tT\t6\t4\t2\t11\t0|1", b"c\t15\tG\tT\t6\t3\t3\t15\t0|1"], near,
        [b"r%d\tc\t%d\t1\t%d\t%d\t0\t%s" % (i, 4 * s + 3, 1 - alt[i].get(s, 0), alt[i].get(s, 0), b"B" if alt[i].get(s, 0) else b"A")
         for i in range(6) for s in range(4)],
        **dict(four, blocks=4, read_records=24, reads_a=14, reads_b=10, links_far=2))
    one("two_noisy_sites_in_a_row_reach_3", two, 3,
        [b"c\t3\tG\tT\t6\t3\t3\t3\t0|1", b"c\t7\tG\tT\t6\t4\t2\t3\t.", b"c\t11\tG\tT\t6\t4\t2\t3\t.", b"c\t15\tG\tT\t6\t3\t3\t3\t0|1"],
        near[:2] + [b"c\t3\t15\t3\t0\t0\t3\t6\t1.000000\tcis"] + near[2:],
        [b"r%d\tc\t3\t4\t0\t2\t0\tB" % i for i in range(3)] + [b"r%d\tc\t3\t4\t2\t0\t0\tA" % i for i in range(3, 6)],
        **dict(four, blocks=1, blocks_multi=1, sites_phased=2, read_records=6, reads_a=3, reads_b=3, links_far=3, links_far_phased=1,
               joins_far=1, sites_bridged=2))
    # r0 - r5 over [0, 8): sites 2 and 6 cis; r12 - r17 over [4, 12): sites 6 and 10 cis: bits 0 0 0 through the near links.
    # r6 - r11 span all three with an N on 6: T on 2 against T on 10, the far link (2, 10) is trans: one conflict, the bits stay
    n6 = {6: b"N"}
    conflict = [(0, 8, {2: b"T", 6: b"T"})] * 3 + [(0, 8, {})] * 3 + [{2: b"T", **n6}] * 3 + [{10: b"T", **n6}] * 3 + \
               [(4, 12, {6: b"T", 10: b"T"})] * 3 + [(4, 12, {})] * 3
    one("far_link_against_the_near_bits", conflict, 2, [b"c\t%d\tG\tT\t12\t6\t6\t3\t0|1" % p for p in (3, 7, 11)],
        [b"c\t3\t7\t3\t0\t0\t3\t6\t1.000000\tcis", b"c\t3\t11\t0\t3\t3\t0\t6\t1.000000\ttrans", b"c\t7\t11\t3\t0\t0\t3\t6\t1.000000\tcis"],
        [b"r%d\tc\t3\t2\t0\t2\t0\tB" % i for i in range(3)] + [b"r%d\tc\t3\t2\t2\t0\t0\tA" % i for i in range(3, 6)] +
        [b"r%d\tc\t3\t3\t1\t1\t0\t-" % i for i in range(6, 12)] +
        [b"r%d\tc\t3\t2\t0\t2\t0\tB" % i for i in range(12, 15)] + [b"r%d\tc\t3\t2\t2\t0\t0\tA" % i for i in range(15, 18)],
        sites=3, sites_base=3, links=2, links_phased=2, blocks=1, blocks_multi=1, sites_phased=3, alleles=42, read_records=18, reads_a=6,
        reads_b=6, reads_tie=6, links_far=1, links_far_phased=1, links_conflict=1)
    return H


def far_links(links):
    """phase_inputs.link_rows of a links file, as {(0-based pos1, pos2): [n00, n01, n10, n11]} (one contig)"""
    return {(p, q): n for _, p, q, n, _ in HI.link_rows(links)}


def shapes():
    Sh = {}

    # TILE + 10 sites on every second position: left sites TILE - 1 (tile 0, every partner in tile 1), TILE and TILE + 1 have
    # links of every distance up to 8.  r0, r1 carry the other base everywhere, r2, r3 the contig's; r4 carries it on every fifth
    # site, whose links agree 4 : 1 - unphased at min_agree 0.9, bridged at reach >= 2; r5 spans six sites around the border,
    # r6 starts on site TILE, r7 ends on site TILE + 4 (a row that ends inside tile 1), r8 lies inside tile 0
    n_sites = TILE + 10
    ln = 2 * n_sites + 9
    ref = HI._seq(ln, 3)
    at = [4 + 2 * i for i in range(n_sites)]
    alt = {p: HI.other_base(ref[p]) for p in at}
    reads = [alt, alt, {}, {}, {p: alt[p] for p in at[::5]}, (at[TILE - 3], at[TILE + 2] + 1, alt), (at[TILE], ln, alt),
             (at[TILE - 40], at[TILE + 4] + 1, {}), (at[7], at[70], alt)]
    c = HI.pile(ref, reads, strands="+-")

    def where(reach, sites, links, reads, st, at=tuple(at), n_sites=n_sites):
        assert [p for _, p, _, _, _ in HI.site_rows(sites)] == list(at)
        assert st["links"] == n_sites - 1 and st["links_far"] == sum(n_sites - d for d in range(2, reach + 1))
        fl = far_links(links)
        for left in (TILE - 1, TILE, TILE + 1):
            for d in range(1, reach + 1):
                n = fl[(at[left], at[left + d])]
                assert sum(n) >= 5 and n[0] >= 2 and n[3] >= 2, (left, d, n)       # the four whole rows, r4 and one of r5 - r7
        assert fl[(at[TILE - 1], at[TILE])][3] == 3 and fl[(at[TILE], at[TILE + 1])][3] == 4
        if reach >= 2:
            assert st["sites_bridged"] >= TILE // 5 - 1 and st["joins_far"] >= TILE // 5 - 1 and st["blocks"] <= 3
    Sh["sites_around_the_reach_tile"] = Shape(c, dict(min_agree=0.9), (2, 3, 8), where)

    # 140 sites; beside the four whole rows, rows over exactly 63, 64, 65 and 129 sites (the partner of the last d lanes of a
    # 64-site step comes from the next step's bytes), one starting on site 0 and one on site 3, and rows over 0, 1, 2 and 3
    # sites (fewer than d + 1)
    n_sites = 140
    ln = 2 * n_sites + 20
    ref = HI._seq(ln, 5)
    at = [6 + 2 * i for i in range(n_sites)]
    alt = {p: HI.other_base(ref[p]) for p in at}
    reads = [alt, alt, {}, {}]
    for k, n in enumerate((63, 64, 65, 129)):
        reads.append((at[0], at[n - 1] + 1, alt if k % 2 else {}))
        reads.append((at[3], at[3 + n - 1] + 1, {} if k % 2 else alt))
    reads += [(at[9] + 1, at[10], {}), (at[9], at[9] + 1, alt), (at[20], at[21] + 1, alt), (at[30], at[32] + 1, {})]
    c = HI.pile(ref, reads, strands="+-")

    def where(reach, sites, links, reads, st, at=tuple(at), n_sites=n_sites):
        assert [p for _, p, _, _, _ in HI.site_rows(sites)] == list(at) and st["blocks"] == 1 and st["sites_bridged"] == 0
        assert st["alleles"] == 4 * n_sites + 2 * (63 + 64 + 65 + 129) + 0 + 1 + 2 + 3
        fl = far_links(links)
        if reach >= 2:
            # left site 62: the rows from site 0 over 63 sites end on it, those over 64 hold its link of distance 1 alone
            assert sum(fl[(at[62], at[63])]) == sum(fl[(at[62], at[64])]) + 1
            assert sum(fl[(at[66], at[67])]) == sum(fl[(at[66], at[68])]) + 1         # the same from site 3
    Sh["rows_over_63_64_65_129_sites"] = Shape(c, {}, (1, 2, 3, 8), where)

    # 4 097 rows on one far link: sites 55, 57 and 60; every third row carries the other base on 55 and 60, every second on 57
    ref = HI._seq(400, 1)
    o = {p: HI.other_base(ref[p]) for p in (55, 57, 60)}
    c = HI.pile(ref, [(40, 80, {**({55: o[55], 60: o[60]} if i % 3 == 0 else {}), **({57: o[57]} if i % 2 == 0 else {})}) for i in range(4097)],
                strands="+-")

    def where(reach, sites, links, reads, st):
        assert far_links(links)[(55, 60)] == [2731, 0, 0, 1366] and st["links_far_phased"] == 1 and st["links_phased"] == 0
        assert st["blocks"] == 1 and st["sites_bridged"] == 1 and st["read_records"] == 4097 and st["reads_b"] == 1366
    Sh["deep_pile_on_one_far_link"] = Shape(c, {}, (2,), where)

    # phase_inputs's junction and empty-contig shapes at reaches above the number of sites on either side: no link crosses
    old = HI.shapes()
    for name, n_links in (("sites_on_both_sides_of_a_contig_junction", 2), ("middle_contig_without_rows", 4)):
        def where(reach, sites, links, reads, st, n_links=n_links, name=name):
            lr = HI.link_rows(links)
            assert st["links"] == n_links and len(lr) == st["links"] + st["links_far"]
            assert st["links_far"] == (0 if n_links == 2 else 2 if reach == 2 else 3)      # z's four sites: (0, 2), (1, 3), (0, 3)
            assert len({b for _, _, _, b, _ in HI.site_rows(sites)}) >= 2
        Sh[name] = Shape(old[name].case, old[name].opts, (3, 8) if n_links == 2 else (2, 8), where)
    return Sh


Noisy = collections.namedtuple("Noisy", "case snps noise")


def noisy_two_strains(n_noise, seed=4242, genome_len=3000, read_len=1000, step=500, minor_copies=3, ratio=5):
    """polish_pairs_inputs.two_strains() - same seed, same strains, same reads in the same order - with n_noise (1 or 2) added
    sites between the two middle SNPs: on the first the reads of either strain carry another base in turn (every other read of
    the strain), on the second two reads in turn of every four.  -> Noisy(case, the SNPs, the noisy positions)"""
    rng = np.random.default_rng(seed)
    major, minor = (bytes(s.tobytes()) for s in S.make_strains(rng, 2, genome_len, 0.01))
    snps = [p for p in range(genome_len) if major[p] != minor[p]]
    m = len(snps) // 2
    assert snps[m + 1] - snps[m] >= 4, "room for two positions between the middle SNPs"
    noise = [snps[m] + 1, snps[m] + 2][:n_noise]
    case = PI.Case([("minor_contig", minor)], dict(min_cov=3, min_len=500))
    seen = {True: 0, False: 0}
    for s in range(0, genome_len - read_len + 1, step):
        for k in range(minor_copies * (1 + ratio)):
            is_minor = k % (1 + ratio) == 0
            seg = bytearray((minor if is_minor else major)[s:s + read_len])
            turn = seen[is_minor]
            seen[is_minor] += 1
            for which, p in enumerate(noise):
                if s <= p < s + read_len and (turn % 2 == 0 if which == 0 else turn % 4 < 2):
                    seg[p - s] = HI.other_base(minor[p], 1 if major[p] == minor[p] else 2)[0]
            runs, n = [], 0
            for j in range(read_len):
                if seg[j] == minor[s + j]:
                    n += 1
                else:
                    runs.append(f"{n}=1X" if n else "1X")
                    n = 0
            if n:
                runs.append(f"{n}=")
            case.add(s, "".join(runs), bytes(seg), strand="-" if k % 2 else "+", name=f"{'min' if is_minor else 'maj'}_{s}_{k}")
    return Noisy(case, snps, noise)
