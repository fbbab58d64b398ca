"""GPU: the filter chain on the inputs of tests/pileup_inputs.py (tile borders, segment classes, CIGAR caches, deep
positions, the row cap, row selection, short mode, mixes) against the oracle, byte for byte, in both forms of the
pile-up: the LDS form (tiny / light / heavy kernels) and the sorted event table (HLMI_SNP_SORT).  Every row of an input
states the same match count M, so the chain at thre = (c + 0.5) / M for every c up to the oracle's largest count pins each
pair's supported-key count exactly, not only zero against non-zero.  tests/test_pileup_inputs.py (CPU) proves that the
inputs sit on the edges."""
import pytest

import pileup_inputs as P
from hylight_amd import api
from oracle import filters as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def written(tmp_path_factory):
    """One input file per case, shared by its thresholds and both forms."""
    d = tmp_path_factory.mktemp("pileup_edges")
    paths = {}

    def path(name):
        if name not in paths:
            paths[name] = d / f"{name}.paf"
            paths[name].write_text(P.get(name).text())
        return paths[name]
    return path


def _runs(name):
    """(mc, thre, oracle rows) of every chain run of a case."""
    c = P.get(name)
    if c.long_mode:
        th = P.thresholds(name)
        assert len(th) <= P.MAX_THRESHOLDS
        sweep = F.worker_sweep(c.lines, True, P.M, c.mc, 0.0, th)
        return [(c.mc, t, sweep[t]) for t in th]
    return [(mc, 0.0025, F.worker(c.lines, False, P.M, mc, 0.0)) for mc in c.mcs]


@pytest.mark.parametrize("form", ["lds", "sort"])
@pytest.mark.parametrize("name", P.NAMES)
def test_chain_and_event_statistic_match_the_oracle(written, tmp_path, monkeypatch, name, form):
    """Chain output at every threshold (short mode: every mc), and `snp_events`.

    The statistic counts one event per X op of every row selected for the pile-up, once per side that is piled (long mode:
    target and query, short mode: target only) - P.event_statistic restates it from F.snp_pileup.  The LDS form adds it up
    from three kernels, one per segment class, so the comparison also checks that the classes partition the segments; the
    sorting form takes it from a scan over the rows.  Each form is held to the oracle's number, not to the other's."""
    if form == "sort":
        monkeypatch.setenv("HLMI_SNP_SORT", "1")
    c = P.get(name)
    src, out = written(name), tmp_path / "out.paf"
    events = P.event_statistic(name)
    for mc, thre, want in _runs(name):
        api.filter_chunk(src, out, len_over=P.M, mc=mc, iden=0.0, thre=thre, long_mode=c.long_mode)
        got = open(out).read().split("\n")[:-1]
        assert len(got) == len(want), (name, form, mc, thre, len(got), len(want))
        assert got == want, (name, form, mc, thre)
        assert api.last_stats()["snp_events"] == events, (name, form, mc, thre)
