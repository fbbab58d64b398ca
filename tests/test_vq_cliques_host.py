"""CPU: hlmi_vq_cliques_of_graph against the reference's own clique enumerator.  tests/golden/fxK_<name>.cliques.txt hold what
quick-cliques' binary printed (stdout of `qc --algorithm=degeneracy --input-file=graph.txt`) for fxK_<name>.graph.txt;
tests/golden/make_goldens_cliques.py wrote both.  The order of the lines decides every new read id, so the comparison is
byte for byte."""
import glob
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
NAMES = sorted(os.path.basename(p)[4:-len(".graph.txt")] for p in glob.glob(os.path.join(GOLD, "fxK_*.graph.txt")))
EXPECTED = {"path6": 5, "triangle_pendant": 2, "k5": 1, "two_k4": 2, "star8": 7, "k333": 27, "empty5": 5}


def test_every_shape_is_there():
    assert set(EXPECTED) <= set(NAMES) and {"gnp60_s1", "gnp60_s2", "gnp60_s3", "gnp300", "stageb"} <= set(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_cliques_byte_for_byte(tmp_path, name):
    from hylight_amd import api
    out = str(tmp_path / "cliques.txt")
    n = api.vq_cliques_of_graph(os.path.join(GOLD, f"fxK_{name}.graph.txt"), out)
    want = open(os.path.join(GOLD, f"fxK_{name}.cliques.txt"), "rb").read()
    assert open(out, "rb").read() == want
    assert n == want.count(b"\n") - 2                     # two text lines, then one clique per line
    assert want.startswith(b"NOTE: Quick Cliques v2.0beta.\nReading .edges file format. \n")
    if name in EXPECTED:
        assert n == EXPECTED[name]
    assert len(want) < 100_000


@pytest.mark.parametrize("text", ["", "3\n", "3\n2\n0,1\n", "2\n2\n0,5\n5,0\n", "2\n2\n0,0\n0,0\n", "2\n4\n0,1\n0,1\n1,0\n1,0\n"])
def test_bad_graph_is_refused(tmp_path, text):
    from hylight_amd import api
    g = tmp_path / "graph.txt"
    g.write_text(text)
    with pytest.raises(api.HlmiError) as e:
        api.vq_cliques_of_graph(str(g), str(tmp_path / "cliques.txt"))
    assert e.value.code == -1                              # HLMI_EINVAL
