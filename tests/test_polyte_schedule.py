"""hylight_amd.polyte without a GPU: the control flow of run_savage_assembly (polyte.tune_params.py:583-682) against traces
worked out by hand, the keyword arguments of every kind of library call against a table written out from :689-743, the
file_len quirk, the preprocessing, the refusals, and the new entry point's place in the header and the binding."""
import os
import re

import pytest

from hylight_amd import api, polyte

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def scripted(counts):
    """step() that hands out `counts` in turn and records what it was asked for."""
    calls = []
    it = iter(counts)

    def step(kind, iteration):
        calls.append((kind, iteration))
        return next(it)
    return step, calls


def test_immediate_stop():
    """0 reads after the first iteration: neither loop is entered (:630) and the final iteration is skipped (:674)."""
    step, calls = scripted([(0, 0, 0)])
    s = polyte.schedule(step)
    assert calls == [("clique_first", 1)]
    assert s == dict(kinds=["clique_first"], reads=[0], overlaps=[0], edges=[0])


def test_no_overlaps_left_still_runs_the_final_iteration():
    step, calls = scripted([(7, 0, 3), (7, 0, 0)])
    assert polyte.schedule(step)["kinds"] == ["clique_first", "final"]
    step, calls = scripted([(7, 5, -2), (7, 0, 0)])                  # no graph.txt: -2 edges
    assert polyte.schedule(step)["kinds"] == ["clique_first", "final"]


def test_constant_twice_in_the_inner_loop():
    """reads 9 -> 6 (counter 0) -> 6 (1) -> 6 (2): the inner loop ends, the branch iteration runs once all the same (:641-645),
    finds 6 again (3), the outer loop ends, the final iteration runs."""
    step, calls = scripted([(9, 5, 4), (6, 5, 4), (6, 5, 4), (6, 5, 4), (6, 5, 4), (6, 2, 1)])
    s = polyte.schedule(step)
    assert s["kinds"] == ["clique_first", "merge", "merge", "merge", "branch", "final"]
    assert [i for _, i in calls] == [1, 2, 3, 4, 5, 6]
    assert s["reads"] == [9, 6, 6, 6, 6, 6]


def test_first_merge_compares_with_the_first_iteration():
    """The first merge iteration's count is compared with the clique iteration's (:637): equal twice ends the inner loop after
    two merges."""
    step, calls = scripted([(6, 5, 4), (6, 5, 4), (6, 5, 4), (6, 5, 4), (6, 5, 4)])
    assert polyte.schedule(step)["kinds"] == ["clique_first", "merge", "merge", "branch", "final"]


def test_branch_iteration_resets_the_counter():
    """Inner loop ends on the counter (8, 8, 8); the branch iteration merges (5): counter 0, so the outer loop turns again:
    merge 5 (1), merge 5 (2), branch 5 (3), final."""
    step, calls = scripted([(8, 5, 4), (8, 5, 4), (8, 5, 4), (5, 5, 4), (5, 5, 4), (5, 5, 4), (5, 5, 4), (5, 5, 4)])
    s = polyte.schedule(step)
    assert s["kinds"] == ["clique_first", "merge", "merge", "branch", "merge", "merge", "branch", "final"]


def test_inner_loop_ends_on_edges_and_the_outer_with_it():
    """A merge iteration that leaves no edge ends the inner loop; the branch iteration runs; its counts end the outer loop."""
    step, calls = scripted([(9, 5, 4), (4, 3, 0), (4, 3, 0), (4, 3, 0)])
    assert polyte.schedule(step)["kinds"] == ["clique_first", "merge", "branch", "final"]


def test_final_iteration_skipped_without_reads():
    step, calls = scripted([(9, 5, 4), (3, 2, 1), (0, 0, -2), (0, 0, -2)])
    s = polyte.schedule(step)
    assert s["kinds"] == ["clique_first", "merge", "merge", "branch"]
    assert s["reads"][-1] == 0


# ---- the arguments of every kind of call, from polyte.tune_params.py:689-743 with EC "false", diploid "false" ---------------
COMMON = dict(keep_singletons=0, remove_trans=1, remove_tips=False, ignore_inclusions=False, merge_contigs=0.0, min_read_len=0,
              max_tip_len=100, remove_backedges=True, min_qual=0.0, min_overlap_perc=0, ov_threshold=0.9, mismatch=0.0,
              max_overlaps=100000000, no_inclusion_overlaps=False)
WANT = {
    "clique_first": ("vq_clique_iteration", ("s_p1_p2.fastq", "original_overlaps.txt", "."),
                     dict(COMMON, min_overlap_len=60, edge_threshold=0.93, first_it=True, min_clique_size=3, remove_branches=True,
                          error_correction=False)),
    "merge": ("vq_iteration", ("singles.fastq", "overlaps.txt", "."),
              dict(COMMON, min_overlap_len=50, edge_threshold=1.0, first_it=False, min_clique_size=2, remove_branches=True,
                   store_tips_separately=False, subreads_in="subreads.txt")),
    "branch": ("vq_branch_iteration", ("singles.fastq", "overlaps.txt", "<cwd>/assembly/s_p1_p2.fastq", "evidence_threshold_table.tsv", "."),
               dict(COMMON, min_overlap_len=50, edge_threshold=1.0, first_it=False, min_clique_size=2, remove_branches=False,
                    error_correction=False, subreads_in="subreads.txt", se_count=0, pe_count=4, careful=True)),
    "final": ("vq_iteration", ("singles.fastq", "overlaps.txt", "."),
              dict(COMMON, min_overlap_len=50, edge_threshold=1.0, first_it=False, min_clique_size=2, remove_branches=True,
                   store_tips_separately=True, subreads_in="subreads.txt")),
}


def fastq(names_seqs):
    return "".join(f"@{n} extra\n{s}\n+{n}\n{'I' * len(s)}\n" for n, s in names_seqs)


@pytest.fixture
def pair(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    p1 = [("a/1", "ACGT" * 25), ("b/1", "CCGT" * 25), ("c/1", "ACGA" * 25), ("d/1", "TTGA" * 25)]
    p2 = [("a/2", "GGGT" * 25), ("b/2", "CAGT" * 25), ("c/2", "ACTA" * 25), ("d/2", "TTAA" * 25)]
    (tmp_path / "x.1.fq").write_text(fastq(p1))
    (tmp_path / "x.2.fq").write_text(fastq(p2))
    return tmp_path, p1, p2


def test_run_passes_the_reference_arguments(pair, monkeypatch):
    """api patched with recorders that write the files the loop reads back; the counts they leave behind walk the schedule
    through all four kinds of call."""
    tmp, p1, p2 = pair
    calls, sr = [], []
    # reads / overlap lines / graph lines left by the calls, in turn: clique_first, merge, merge, merge, branch, final
    script = iter([(5, 4, 5), (4, 4, 5), (4, 4, 5), (4, 4, 5), (4, 4, 5), (4, 1, 2)])

    def recorder(name):
        def fn(*pos, **kw):
            calls.append((name, tuple(str(x) for x in pos), kw))
            reads, ov, graph = next(script)
            with open("singles.fastq", "w") as f:
                f.write("".join(f"@{k}\nACGT\n+\nIIII\n" for k in range(reads)))
            with open("overlaps.txt", "w") as f:
                f.write("from findNextOverlaps\n")
            with open("graph.txt", "w") as f:
                f.write("x\n" * graph)
            recorder.ov = ov
        return fn

    def sr_overlaps(reads, out, min_len, iden, o, r):
        sr.append((str(reads), str(out), min_len, iden, o, r))
        n = recorder.ov if str(reads) == "singles.fastq" else 6
        with open(out, "w") as f:
            f.write("row\n" * n)
        return n

    for name in ("vq_clique_iteration", "vq_iteration", "vq_branch_iteration"):
        monkeypatch.setattr(api, name, recorder(name))
    monkeypatch.setattr(api, "sr_overlaps", sr_overlaps)
    r = polyte.run("x.1.fq", "x.2.fq", min_overlap_len=50, min_overlap_len_EC=60, hap_cov=10, insert_size=450, stddev=27,
                   average_read_len=100, min_clique_size=3, edge1=0.93, edge2=1.0)
    kinds = ["clique_first", "merge", "merge", "merge", "branch", "final"]
    assert r["kinds"] == kinds
    assert len(calls) == len(kinds)
    for kind, (name, pos, kw) in zip(kinds, calls):
        w_name, w_pos, w_kw = WANT[kind]
        assert name == w_name
        assert pos == tuple(x.replace("<cwd>", os.getcwd()) for x in w_pos)
        assert kw == w_kw, kind
    # the overlaps: the input's with min_overlap_len_EC, then every singles.fastq with min_overlap_len (next_min_overlap)
    assert sr[0] == ("s_p1_p2.fastq", "original_overlaps.txt", 60, 0.98, 1, 0.8)
    assert sr[1:] == [("singles.fastq", "overlaps.txt", 50, 0.98, 1, 0.8)] * 6
    # what run() returns: the lists the reference prints; one line of overlaps.txt counts as none (file_len)
    assert r["iterations"] == 7
    assert r["reads"] == [8, 5, 4, 4, 4, 4, 4]
    assert r["overlaps"] == [6, 4, 4, 4, 4, 4, 0]
    assert r["edges"] == [3, 3, 3, 3, 3, 0]
    assert r["max_read_lengths"] == [4] * 6
    # what it leaves behind
    assert (tmp / "contigs.fasta").read_text() == "".join(f">{k}\nACGT\n" for k in range(4))
    assert not (tmp / "assembly" / "original_overlaps.txt").exists()
    for name in ("pipeline.log", "stats.txt", "removed_tip_sequences.fastq", "evidence_threshold_table.tsv"):
        assert (tmp / "assembly" / name).exists()
    head = (tmp / "assembly" / "evidence_threshold_table.tsv").read_text().splitlines()[:5]
    assert head == ["# INPUT:", "# readlen 100.0", "# intseg 250.0", "# stddev 27.0", "# hcov 10.0"]


def test_preprocessing(pair):
    tmp, p1, p2 = pair
    out = tmp / "s_p1_p2.fastq"
    assert polyte.preprocess(tmp / "x.1.fq", tmp / "x.2.fq", out) == 8
    want = "".join(f"@{k}\n{s}\n+\n{'I' * len(s)}\n" for k, (_, s) in enumerate(p1 + p2))     # p1 before p2, ids 0 .. 7, bare +
    assert out.read_text() == want


def test_file_len_quirk(tmp_path):
    p = tmp_path / "f"
    assert polyte.file_len(p) == 0                              # missing
    for text, want in (("", 0), ("one line\n", 0), ("a\nb\n", 2), ("a\nb\nc", 3)):
        p.write_text(text)
        assert polyte.file_len(p) == want, text
    assert polyte.get_edge_count(tmp_path / "none") == -2
    p.write_text("h1\nh2\ne\n")
    assert polyte.get_edge_count(p) == 1
    assert int(round(2.5)) == 2 and int(round(250.5)) == 250    # max_tip_len = int(round(average_read_len)): half to even


@pytest.mark.parametrize("argv", [["-s", "s.fq"], ["--diploid"], ["--ref_guided_mode"], ["--count_strains"], ["NO_EC_MISSING"]])
def test_refusals_do_no_work(argv, tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(polyte, "run", lambda *a, **k: pytest.fail("run() was called"))
    base = ["-p1", "a.1.fq", "-p2", "a.2.fq"]
    args = base + (["--no_EC"] + argv if argv != ["NO_EC_MISSING"] else [])
    assert polyte.main(args) == polyte.EXIT_REFUSED
    assert "not built" in capsys.readouterr().err
    assert os.listdir(tmp_path) == []


def test_cli_defaults_are_hylights():
    a = polyte.build_parser().parse_args(["-p1", "a", "-p2", "b", "--no_EC"])
    assert (a.min_overlap_len, a.min_overlap_len_EC, a.hap_cov, a.insert_size, a.stddev, a.average_read_len, a.min_clique_size,
            a.edge1, a.edge2, a.max_tip_len, a.error_correction) == (50, 60, 10.0, 450.0, 27.0, 250.0, 2, 0.93, 1.0, None, False)


def test_symbol_in_header_and_binding():
    header = open(os.path.join(ROOT, "include", "hylight_mi.h")).read()
    assert re.search(r"\bint hlmi_sr_overlaps\(const char \*reads, int min_ovlp_len, double min_identity, int o, double r,", header)
    assert "#define HLMI_ABI_VERSION 7" in header and api.ABI_VERSION == 7
    assert "hlmi_sr_overlaps" in api.SYMBOLS and len(api.SYMBOLS["hlmi_sr_overlaps"][1]) == 7


def test_driver_refuses_both_polyte_flags():
    from hylight_amd import driver
    with pytest.raises(SystemExit) as e:
        driver.main(["-l", "x.fq", "--polyte_native", "--polyte_cmd", "polyte"])
    assert "--polyte_native" in str(e.value)
