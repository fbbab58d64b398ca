"""GPU parity of the overlapper on low-complexity and repeat-rich sequence: raw hlmi_ava rows against the CPU oracle,
whole file, byte for byte, CIGAR included.  Every other input of the suite is uniform random sequence, where the optimal
alignment is essentially unique; the inputs of tests/structured_inputs.py are the ones where two alignments tie - a gap
that can sit anywhere inside a homopolymer or a short tandem repeat, a block that matches itself shifted by a base or
two (the fourth and seventh certificate of classify_kernel), equal-score predecessors and several chains per (target,
strand, query) group in the chaining.  tests/test_structured_inputs.py checks on the CPU that the oracle's rows on these
inputs are true alignments and that the inputs hold what they are for.

A failing comparison names the first differing row; the micro cases spell their case in the read names
(structured_inputs.micro_cases)."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import structured_inputs as SI  # noqa: E402
from hylight_amd import api  # noqa: E402
from hylight_amd import simulate as S  # noqa: E402
from oracle import ava as OA  # noqa: E402
from oracle import filters as F  # noqa: E402

pytestmark = pytest.mark.gpu

# the constants of tests/test_gpu_ava.py::test_ava_other_constants that decide between tied paths
VARIANTS = {
    "one_piece": dict(gap_open2=0),
    "all_ones": dict(match=1, mismatch=1, gap_open=1, gap_ext=1, gap_open2=0),        # many ties: whole repeat units tie here
    "wide_scores": dict(mismatch=16, gap_open=20, gap_ext=2, gap_open2=0),            # the 32-bit narrow form by itself
}

# every fallback form (names: the table of runtime.cpp) -> the set it runs on next to the micro cases
HOOKS = {
    "HLMI_NO_SHIFT_CERT": "long", "HLMI_NO_GAP1_CERT": "long", "HLMI_NO_GAP2_CERT": "long", "HLMI_NO_SUFFIX_TRIM": "long",
    "HLMI_NO_ONE_PIECE_CERT": "long", "HLMI_NO_EXT_CERT": "long", "HLMI_NARROW_UNPACKED": "long",
    "HLMI_NARROW_LONG_UNPACKED": "long", "HLMI_CHAIN_NO_DP16": "long", "HLMI_CHAIN_NO_SMALL": "short",
    "HLMI_CHAIN_UNPACKED": "long", "HLMI_SEED_GROUP": "long", "HLMI_ASM_WAVE": "short", "HLMI_NO_RANK_WORD": "long",
    "HLMI_ANCHOR_PAIRS": "long", "HLMI_LANES": "long", "HLMI_LONG_SIDE_STREAM": "long",
}


def _first_difference(got, want):
    if got == want:
        return None
    g, w = got.split("\n"), want.split("\n")
    for k in range(max(len(g), len(w))):
        a, b = (g[k] if k < len(g) else "<end of file>"), (w[k] if k < len(w) else "<end of file>")
        if a != b:
            return f"row {k} of {len(w) - 1}:\n  got  {a[:400]}\n  want {b[:400]}"


class Inputs:
    """the FASTA files of the fixed sets, the oracle's rows per (set, constants) - each computed once per module"""

    def __init__(self, d):
        self.d = d
        self.fa, self.reads, self._want = {}, {}, {}
        for name, rd in (("long0", SI.long_set(SI.LONG_SEEDS[0])[0]), ("long1", SI.long_set(SI.LONG_SEEDS[1])[0]),
                         ("short", SI.short_set()[0]), ("contigs", SI.contig_set()[0]), ("micro", SI.micro_set())):
            self.fa[name] = d / f"{name}.fa"
            self.reads[name] = rd
            S.write_fasta(rd, self.fa[name])
        self.n = 0

    @staticmethod
    def opts(mod, mode, changes):
        o = (mod.ava_opts_short if mod is api else mod.opts_short)() if mode == "short" else \
            (mod.ava_opts_long if mod is api else mod.opts_long)()
        for k, v in changes.items():
            setattr(o, k, v)
        return o

    def want(self, name, mode="long", **changes):
        key = (name, mode, tuple(sorted(changes.items())))
        if key not in self._want:
            p = self.d / f"oracle{len(self._want)}.paf"
            OA.ava(self.fa[name], self.fa[name], p, self.opts(OA, mode, changes))
            self._want[key] = open(p).read()
        return self._want[key]

    def got(self, name, mode="long", **changes):
        self.n += 1
        p = self.d / f"gpu{self.n}.paf"
        api.ava(self.fa[name], self.fa[name], p, self.opts(api, mode, changes))
        text = open(p).read()
        os.remove(p)
        return text, dict(api.last_stats())

    def compare(self, name, mode="long", **changes):
        got, st = self.got(name, mode, **changes)
        want = self.want(name, mode, **changes)
        assert want.count("\n") > 1000
        diff = _first_difference(got, want)
        assert diff is None, diff
        return st


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    return Inputs(tmp_path_factory.mktemp("structured"))


@pytest.mark.parametrize("name", ["long0", "long1"])
def test_long_set_matches_oracle(inputs, name):
    st = inputs.compare(name)
    print(f"{name}: " + ", ".join(f"{k} {st[k]}" for k in ("align_tasks", "align_tasks_fast", "align_tasks_dp", "align_tasks_narrow",
                                                          "align_tasks_wide", "align_tasks_long", "chain_groups", "pieces")))
    # every class of alignment task takes part.  Measured on long0 / long1: 438 617 / 340 173 tasks, 375 671 / 289 121 of them
    # finished by the classifier; narrow 31 342 / 26 676, wide 6 830 / 6 006, long 23 220 / 17 422 (floors: a tenth)
    assert st["align_tasks_narrow"] > 2_600 and st["align_tasks_wide"] > 600 and st["align_tasks_long"] > 1_700, st


def test_short_set_matches_oracle(inputs):
    """The short constants: chain_small_kernel and the lane forms of the row assembly."""
    st = inputs.compare("short", "short")
    print("short: " + ", ".join(f"{k} {st[k]}" for k in ("align_tasks", "align_tasks_fast", "align_tasks_dp", "chain_groups", "pieces")))
    assert st["chain_groups"] > 6_000          # measured: 62 890 groups, 60 287 pieces, 276 281 tasks (79 309 through a DP)


def test_contigs_at_bandwidth_zero_match_oracle(inputs):
    """The contig-vs-contig call of extend_con (tests/test_gpu_ungapped.py): chains without a diagonal shift, every block
    and extension along the diagonal - on contigs whose strains differ by a repeat unit here and there."""
    st = inputs.compare("contigs", "short", pair_once=1, bandwidth=0)
    assert st.get("kernel_launches.align_ungapped", 0) >= 1
    assert "I" not in "".join(l.split("\t")[-1][5:] for l in inputs.want("contigs", "short", pair_once=1, bandwidth=0).split("\n")[:-1])


@pytest.mark.parametrize("mode", ["long", "short"])
def test_micro_cases_match_oracle(inputs, mode):
    inputs.compare("micro", mode)


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_long_set_with_other_constants_matches_oracle(inputs, variant):
    inputs.compare("long0", "long", **VARIANTS[variant])


# the sets of the sweep: name -> (input, constants)
SWEEP_SETS = {"long0": ("long0", "long"), "micro": ("micro", "long"), "short": ("short", "short"), "micro_short": ("micro", "short")}


@pytest.fixture(scope="module")
def sweep(inputs):
    """One hlmi_ava call per fallback form and set -> {(hook, set): (first difference with the oracle or None, statistics)};
    hook None: the default forms."""
    out = {}

    def run(hook, name):
        got, st = inputs.got(*SWEEP_SETS[name])
        out[(hook, name)] = (_first_difference(got, inputs.want(*SWEEP_SETS[name])), st)

    saved = {h: os.environ.pop(h, None) for h in HOOKS}
    try:
        for name in SWEEP_SETS:
            run(None, name)
        for hook in HOOKS:
            os.environ[hook] = "1"
            try:
                for name in _sets_of(hook):
                    run(hook, name)
            finally:
                del os.environ[hook]
    finally:
        for h, v in saved.items():
            if v is not None:
                os.environ[h] = v
    return out


def _sets_of(hook):
    return ("short", "micro_short") if HOOKS[hook] == "short" else ("long0", "micro")


@pytest.mark.parametrize("hook", sorted(HOOKS))
def test_fallback_forms_match_oracle(sweep, hook):
    for name in _sets_of(hook):
        assert sweep[(None, name)][0] is None, (name, sweep[(None, name)][0])
        assert sweep[(hook, name)][0] is None, (hook, name, sweep[(hook, name)][0])


def test_fallback_forms_are_taken(sweep):
    """The hooks that show in the statistics do what their names say on these inputs."""
    for name in ("long0", "micro"):
        assert sweep[("HLMI_LANES", name)][1].get("ava_lanes", 1) == 1
        st = sweep[("HLMI_ANCHOR_PAIRS", name)][1]
        assert st["anchor_bytes"] == 16 * st["anchors"]
    st = sweep[("HLMI_SEED_GROUP", "long0")][1]
    assert st["anchors_grouped_in_lds"] + st.get("seed_group_gave_up", 0) > 0
    assert sweep[(None, "long0")][1].get("anchors_grouped_in_lds", 0) == 0
    # long0 runs about 23 000 LONG tasks: with the hook their launches go to the second stream
    assert sweep[("HLMI_LONG_SIDE_STREAM", "long0")][1]["align_long_side_launches"] >= 1
    assert "align_long_side_launches" not in sweep[(None, "long0")][1]


# the statistic that a certificate's hook must lower; measured (default forms -> hook set) on long0 (438 617 tasks) and on
# the micro cases (38 708 tasks)
CERTS = {
    "HLMI_NO_SHIFT_CERT": "align_tasks_fast",                    # long0 375 671 -> 372 765, micro 37 291 -> 37 215
    "HLMI_NO_GAP1_CERT": "align_tasks_fast",                     # long0 375 671 -> 348 921, micro 37 291 -> 36 924
    "HLMI_NO_GAP2_CERT": "align_tasks_fast",                     # long0 375 671 -> 369 096, micro 37 291 -> 37 091
    "HLMI_NO_EXT_CERT": "align_ext_certified",                   # long0 1 375 -> 0, micro 58 -> 0 (the end<..> cases)
    "HLMI_NO_ONE_PIECE_CERT": "align_tasks_wide_one_piece",      # long0 2 679 -> 0, micro 166 -> 0 (the end<..> cases)
}


@pytest.mark.parametrize("name", ["long0", "micro"])
@pytest.mark.parametrize("hook", sorted(CERTS))
def test_each_certificate_is_met_and_refused(sweep, hook, name):
    """With a certificate's hook set fewer tasks finish in the classifier (fewer extensions are certified, fewer wide tasks
    run with one gap piece): the certificate is granted on these inputs.  It is refused on them as well: tasks remain for the
    DP kernels in either run."""
    key = CERTS[hook]
    with_cert, without = sweep[(None, name)][1], sweep[(hook, name)][1]
    print(f"{hook} on {name}: {key} {with_cert[key]} -> {without[key]}; align_tasks {with_cert['align_tasks']}, "
          f"align_tasks_dp {with_cert['align_tasks_dp']} -> {without['align_tasks_dp']}")
    assert without[key] < with_cert[key], (hook, name, key, with_cert[key], without[key])
    assert with_cert["align_tasks_dp"] > 0                       # measured: long0 61 392, micro 776
    assert with_cert["align_tasks"] == without["align_tasks"]


def test_stage_on_the_long_set_matches_oracle_pipeline(inputs, tmp_path, monkeypatch):
    """The whole stage as tests/test_gpu_ava.py::test_split_reads2_matches_oracle_pipeline runs it: the pile-up of the SNP rule
    sees X events next to gaps that were placed inside repeats.  HLMI_SNP_SORT (the sorting form of the event table) equal
    to it."""
    fa = inputs.fa["long0"]
    out = tmp_path / "s1_s1.paf"
    api.split_reads2(fa, fa, 4, tmp_path, out, threads=4, len_over=1000, mc=2, iden=0.95, long=True)
    rows_out = api.last_stats()["rows_out"]
    lines = open(fa).read().split("\n")[:-1]
    chunks = []
    for i, (lo, hi) in enumerate(F.chunk_ranges(len(lines), 4)):
        cf = tmp_path / f"chunk{i}.fa"
        cf.write_text("\n".join(lines[lo:hi]) + "\n")
        OA.ava(cf, fa, tmp_path / f"chunk{i}.paf")
        chunks.append(open(tmp_path / f"chunk{i}.paf").read().split("\n")[:-1])
    want = F.stage(chunks, True, 1000, 2, 0.95)
    got = open(out).read().split("\n")[:-1]
    assert len(want) > 100
    assert got == want
    assert rows_out == len(want)
    monkeypatch.setenv("HLMI_SNP_SORT", "1")
    alt = tmp_path / "snp_sort.paf"
    api.split_reads2(fa, fa, 4, tmp_path, alt, threads=4, len_over=1000, mc=2, iden=0.95, long=True)
    assert open(alt).read().split("\n")[:-1] == want
