"""GPU: hlmi_polish_pairs and hlmi_polish_reads_pairs against their model (tests/polish_pairs_model.py) - the file byte for byte
and every integer stat.  The hand cases of tests/test_polish_pairs_model.py through hlmi_polish_pairs; their kinds again on
generated reads through both calls (for the fused call the model runs on the PAF hlmi_ava writes for the same inputs, as in
tests/test_gpu_polish_reads.py); no list and a list of every aligned pair against the _q calls; lists of exactly 0 .. 4097
distinct keys around the round borders of the device's key search (wave_search.h: 64, 4096) and the sort's 1024 border, with the
rows' keys first, last, below, above and between the listed ones; the malformed line; two strains through the real overlapper."""
import os
import sys

import pytest

from hylight_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import polish_pairs_inputs as XI  # noqa: E402
import polish_pairs_model as XM  # noqa: E402
import polish_reads_inputs as RI  # noqa: E402

pytestmark = pytest.mark.gpu
HAND = XI.hand_cases()
INT_STATS = XM.STAT_KEYS
WAVES = 4                                                    # polish_rows.hip: rows a workgroup of pr_facts_kernel takes at a time


def ints(st):
    return {k: st[k] for k in INT_STATS}


def refused(call, line, out):
    with pytest.raises(api.HlmiError) as e:
        call()
    assert e.value.code == -1 and f"pairs.paf:{line}:" in str(e.value), str(e.value)      # HLMI_EINVAL, the 1-based line
    assert not os.path.exists(out)
    return str(e.value)


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_case(name, tmp_path):
    h = HAND[name]
    cfa, rfa, paf = h.case.write(tmp_path)
    lst, out = tmp_path / "pairs.paf", tmp_path / "polished.fa"
    lst.write_bytes(h.pairs)
    if h.refused_line:
        refused(lambda: api.polish(cfa, rfa, paf, out, pairs=lst, **h.case.opts), h.refused_line, out)
    else:
        st = api.polish(cfa, rfa, paf, out, pairs=lst, **h.case.opts)
        assert ints(st) == {**dict.fromkeys(INT_STATS, 0), **h.stats}
        assert out.read_bytes() == h.want
    assert sorted(os.listdir(tmp_path)) == ["contigs.fa", "pairs.paf"] + ["polished.fa"] * (not h.refused_line) + ["reads.fa", "rows.paf"]


# ---- both calls on generated reads ------------------------------------------------------------------------------------------
def ava_opts():
    o = api.ava_opts_long()
    o.pair_once = 0
    return o


class Chain:
    """an input's files and the PAF hlmi_ava writes for them: what the model and hlmi_polish_pairs read"""

    def __init__(self, inp, d):
        self.inp, self.d = inp, str(d)
        self.cfa, self.rfa, self.paf = (os.path.join(self.d, n) for n in ("contigs.fa", "reads.fa", "chain.paf"))
        with open(self.cfa, "wb") as f:
            f.write(RI.fasta(inp.contigs))
        with open(self.rfa, "wb") as f:
            f.write(RI.fasta(inp.reads))
        api.ava(self.cfa, self.rfa, self.paf, ava_opts())
        with open(self.paf, "rb") as f:
            self.paf_bytes = f.read()
        self.rows = RI.paf_rows(self.paf_bytes)
        self.pairs = list(dict.fromkeys((r["q"], r["t"]) for r in self.rows))      # aligned (read, contig) pairs, in line order
        self.n = 0

    def model(self, lst, **over):
        return XM.polish_pairs(RI.fasta(self.inp.contigs), RI.fasta(self.inp.reads), self.paf_bytes, lst, **{**self.inp.opts, **over})

    def both(self, lst, **over):
        """the list through hlmi_polish_pairs over the PAF and through hlmi_polish_reads_pairs -> [(stats, file bytes)]"""
        self.n += 1
        path = None
        if lst is not None:
            path = os.path.join(self.d, f"list{self.n}", "pairs.paf")
            os.makedirs(os.path.dirname(path))
            with open(path, "wb") as f:
                f.write(lst)
        opts = {**self.inp.opts, **over}
        got = []
        for who in ("chain", "direct"):
            out = os.path.join(self.d, f"{who}{self.n}.fa")
            call = ((lambda out=out: api.polish(self.cfa, self.rfa, self.paf, out, pairs=path, **opts)) if who == "chain" else
                    (lambda out=out: api.polish_reads(self.cfa, self.rfa, out, ava_opts(), pairs=path, **opts)))
            got.append((call, out))
        return got

    def check(self, lst, **over):
        want, want_st = self.model(lst, **over)
        for call, out in self.both(lst, **over):
            st = call()
            if lst is None:                                  # api routes a call without a list to the older symbols
                st = {**dict.fromkeys(INT_STATS, 0), **st}
            assert ints(st) == want_st, out
            with open(out, "rb") as f:
                assert f.read() == want, out
        return want, want_st


@pytest.fixture(scope="module")
def long_chain(tmp_path_factory):
    return Chain(RI.every_kind_long(), tmp_path_factory.mktemp("pairs_long"))


@pytest.fixture(scope="module")
def named_chains(tmp_path_factory):
    return {c: Chain(XI.fused_input(c), tmp_path_factory.mktemp("pairs_" + c)) for c in ("k", "s")}


@pytest.mark.parametrize("grid", ["1", "3"])
def test_a_wave_takes_several_rows(grid, long_chain, monkeypatch):
    """pr_facts_kernel gives every row a wave of its own until there are more than 262 144 rows; HLMI_POLISH_ROWS_GRID caps the
    grid, so that 4 or 12 waves stride over these rows and a wave goes on behind a row that is not
    listed: listed and unlisted pairs alternate in line order"""
    c = long_chain
    assert len(c.rows) >= 4 * WAVES * int(grid) + 1
    lst = b"".join(XI.row(q, t, 14) for q, t in c.pairs[::2])
    want, st = c.check(lst)
    assert st["rows_not_listed"] >= 10 and st["rows_selected"] >= 10
    monkeypatch.setenv("HLMI_POLISH_ROWS_GRID", grid)
    assert c.check(lst) == (want, st)
    c.check(None)


def test_no_list_and_every_pair_equal_the_q_calls(long_chain):
    c = long_chain
    plain_out = os.path.join(c.d, "plain_q.fa")
    st_q = api.polish_reads(c.cfa, c.rfa, plain_out, ava_opts(), qual_weight=0, min_avg_qual=0.0, **c.inp.opts)
    with open(plain_out, "rb") as f:
        plain = f.read()
    assert st_q["substituted"] > 0 and st_q["inserted_bases"] > 0
    # pairs_paf == NULL through the new symbols themselves
    lib = api.load()
    for who in ("hlmi_polish_pairs", "hlmi_polish_reads_pairs"):
        o, st = api._polish_qopts(who, c.inp.opts), api.PolishPStats()
        out = os.path.join(c.d, who + "_null.fa").encode()
        args = ((c.cfa.encode(), c.rfa.encode(), c.paf.encode(), api.C.byref(o), None, out, api.C.byref(st)) if who == "hlmi_polish_pairs" else
                (c.cfa.encode(), c.rfa.encode(), api.C.byref(ava_opts()), api.C.byref(o), None, out, api.C.byref(st)))
        assert getattr(lib, who)(*args) == 0
        got = api._polish_pstats(st)
        assert {k: got[k] for k in st_q if not k.startswith("ms_")} == {k: v for k, v in st_q.items() if not k.startswith("ms_")}
        assert (got["pairs_listed"], got["pairs_unknown"], got["rows_not_listed"]) == (0, 0, 0)
        with open(out, "rb") as f:
            assert f.read() == plain
    every = b"".join(XI.row(q, t, 14) for q, t in c.pairs)
    want, st = c.check(every)
    assert want == plain and st["rows_not_listed"] == 0 and st["pairs_listed"] == len(c.pairs)


def test_the_hand_cases_kinds_on_generated_reads(long_chain):
    """half of the aligned pairs listed - in either order, some twice, r1 but not r10, a last line without \\n - between rows
    with \\r\\n ends and rows against contigs of another set, which count as unknown"""
    c = long_chain
    reads = sorted({q for q, _ in c.pairs})
    assert b"r1" in reads and b"r10" in reads
    keep = {q for i, q in enumerate(reads) if i % 2 == 0} | {b"r1"}
    keep.discard(b"r10")
    lines, n_unknown = [], 0
    for i, (q, t) in enumerate(c.pairs):
        if q in keep:
            lines += [XI.row(t, q, 12) if i % 3 == 0 else XI.row(q, t, 14)] * (2 if i % 5 == 0 else 1)
        else:
            lines.append(XI.row(q, t, 6, end=b"\r\n") if i % 2 else XI.row(q, b"remain_" + t, 14))
            n_unknown += 1
    lst = b"".join(lines) + XI.row(b"r1", b"c1", 14, end=b"")
    want, st = c.check(lst)
    assert st["pairs_unknown"] == n_unknown > 5 and st["rows_not_listed"] > 5 and st["rows_selected"] > 5
    assert st["pairs_listed"] == len({p for p in c.pairs if p[0] in keep} | {(b"r1", b"c1")})
    assert want != c.model(None)[0]
    # an empty list: every contig as it was
    want, st = c.check(b"")
    assert want == RI.fasta(c.inp.contigs) and st["rows_selected"] == 0 and st["rows_not_listed"] == len([r for r in c.rows if r["q"] != r["t"]])


def test_an_unlisted_row_does_not_shadow(tmp_path):
    """reads inside a segment two contigs share have two rows of equal span; the earlier line (cA or cB) wins unless it is not
    listed - then the other contig gets the read"""
    c = Chain(RI.tie_between_contigs(), tmp_path)
    _, st0 = c.check(None)
    both = sorted({q for q, t in c.pairs if t == b"cA"} & {q for q, t in c.pairs if t == b"cB"})
    assert len(both) >= 6
    want, st = c.check(b"".join(XI.row(q, b"cB") for q in both))
    assert st["rows_selected"] == len(both) and st["rows_not_listed"] >= len(both)
    assert b"RC:i:%d" % len(both) in want.split(b"\n")[2] and want.split(b"\n")[0] == b">cA"      # cA unpolished, cB has them all


KEY_COUNTS = [0, 1, 2, 63, 64, 65, 1024, 1025, 4095, 4096, 4097]


def key_classes(chain, lst):
    """where the keys of the alignment rows lie in the device's sorted key array"""
    names = [n.encode() for n, _ in chain.inp.contigs + chain.inp.reads]
    keys, rank = XI.sorted_keys(lst + b"\n" if lst and not lst.endswith(b"\n") else lst, names)
    seen = set()
    for q, t in chain.pairs:
        k = (rank[q], rank[t])
        if not keys:
            seen.add("empty")
        elif k in keys:
            seen.add("first" if k == keys[0] else "last" if k == keys[-1] else "inside")
        else:
            seen.add("below" if k < keys[0] else "above" if k > keys[-1] else "between")
    return seen, keys, rank


LAYOUTS = {  # contig name, fill side, are the smallest and the largest aligned read listed -> where row keys must be seen
    "k_a_ends": ("k", "a", True, {"last", "inside", "between"}),
    "k_a_inner": ("k", "a", False, {"above", "inside", "between"}),
    "s_z_ends": ("s", "z", True, {"first", "inside", "between"}),
    "s_z_inner": ("s", "z", False, {"below", "inside", "between"}),
    "k_az_inner": ("k", "az", False, {"inside", "between"}),
}


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("n_keys", KEY_COUNTS)
def test_list_sizes(n_keys, layout, named_chains):
    """contig k sorts in front of the reads r*, contig s behind them: a row's key rank(read) << 32 | rank(contig) is the larger
    or the smaller of its pair's two.  Fill keys in front (a), behind (z) or on both sides; every other aligned read listed,
    with or without the two at the ends of the name order."""
    contig, side, ends, need = LAYOUTS[layout]
    c = named_chains[contig]
    P = sorted(c.pairs)
    real = ([P[0], P[-1]] if ends else []) + P[1:-1][::2]
    lst, got = XI.list_of_keys(n_keys, real, side)
    seen, keys, rank = key_classes(c, lst)
    assert len(keys) == n_keys
    want, st = c.check(lst)
    assert st["pairs_listed"] == n_keys // 2 and st["pairs_unknown"] == 0 and st["rows_selected"] <= len(got)
    if n_keys >= 63:
        assert len(got) == min(len(real), n_keys // 2) >= 20 and st["rows_selected"] >= 10 and st["rows_not_listed"] >= 10
        assert need <= seen, seen                            # the wanted keys at the array's ends, the absent ones outside and between


def test_rank_zero_and_the_largest_rank(named_chains):
    """keys with rank 0 and with the largest rank in either word, next to the rows' keys: (a000, contig), (contig, a000),
    (z099, contig), (contig, z099) - and each read with its fill neighbour, so that the two orders of a pair differ in the
    high word only from a listed key"""
    for c in named_chains.values():
        t = c.pairs[0][1]
        lst = XI.row(b"a000", t) + XI.row(t, b"z099") + XI.row(b"a000", b"z099")
        lst += b"".join(XI.row(q, b"a000") + XI.row(b"z099", q) for q, _ in c.pairs[::2]) + b"".join(XI.row(q, t) for q, t in c.pairs[1::2])
        _, keys, rank = key_classes(c, lst)
        assert rank[b"a000"] == 0 and rank[b"z099"] == len(rank) - 1 and keys[0][0] == 0 and keys[-1][0] == len(rank) - 1
        _, st = c.check(lst)
        assert st["rows_selected"] > 0 and st["rows_not_listed"] > 0


def test_the_malformed_line_has_one_number(long_chain):
    c = long_chain
    rows = [XI.row(q, t, 14) for q, t in c.pairs[:40]]
    rows[28] = XI.row(b"r3", b"c0", 5)
    rows[33] = b"\n"
    msgs = []
    for call, out in c.both(b"".join(rows)):
        msgs.append(refused(call, 29, out))
    assert "hlmi_polish_pairs" in msgs[0] and "hlmi_polish_reads_pairs" in msgs[1]
    # a refusal of the call itself comes first
    for call, out in c.both(b"".join(rows), min_cov=0):
        with pytest.raises(api.HlmiError) as e:
            call()
        assert "min_cov" in str(e.value) and "pairs.paf" not in str(e.value)


def test_two_strains_through_the_overlapper(tmp_path):
    """the minor strain's contig, five reads of the major strain to one of its own: with the same-strain list the contig comes
    back as it was; without it the major strain's alleles are written into it"""
    s = XI.two_strains()
    c = Chain(RI.Input([(n.decode(), b) for n, b in s.case.contigs], [(n.decode(), b) for n, b in s.case.reads], False, s.case.opts), tmp_path)
    assert {q for q, _ in c.pairs} == {n for n, _ in s.case.reads}          # the overlapper aligns both strains to the contig
    want, st = c.check(s.same_strain_list)
    assert want.split(b"\n")[1] == s.minor and st["rows_selected"] == 15 and st["rows_not_listed"] >= 75 and st["substituted"] == 0
    without, st0 = c.check(None)
    got = without.split(b"\n")[1]
    assert got != s.minor and st0["substituted"] >= 20
    assert sum(1 for p in s.snps if len(got) == 3000 and got[p] == s.major[p]) >= 20
