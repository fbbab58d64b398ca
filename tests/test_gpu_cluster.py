"""GPU: hlmi_cluster_short (HyLight.py:215-226 in one library call) against the reference's own outputs
(tests/golden/fxH_cluster_*.json, written by make_goldens_cluster.py from the four reference scripts) and against
tests/cluster_model.py on larger random inputs; its refusals and its CLI.

HLMI_CLUSTER_LARGE=1 runs the larger comparison at 2e5 pairs / 1e6 rows (about two minutes of model time)."""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import cluster_inputs as CI  # noqa: E402
import cluster_model as CM  # noqa: E402
import make_goldens_cluster as MG  # noqa: E402
from hylight_amd import api  # noqa: E402

pytestmark = pytest.mark.gpu

COUNTS = ("names", "rows", "chunks", "sessions", "survivors", "strict_rejects", "unions", "clusters_ge20", "reads_sliced",
          "files")
LARGE = os.environ.get("HLMI_CLUSTER_LARGE") == "1"


def _manifest(name):
    with open(os.path.join(HERE, "golden", f"fxH_cluster_{name}.json")) as f:
        return json.load(f)


def _inputs(tmp_path, params):
    fq, paf = CI.make_case(**params)
    fp, pp = tmp_path / "reads.fq", tmp_path / "shortr2.paf"
    fp.write_bytes(fq)
    pp.write_bytes(paf)
    return fq, paf, str(fp), str(pp)


@pytest.mark.parametrize("name", sorted(MG.CASES))
def test_library_matches_reference_manifest(tmp_path, name):
    m = _manifest(name)
    _, _, fp, pp = _inputs(tmp_path, m["params"])
    out = tmp_path / "tmp"
    st = api.cluster_short(pp, fp, out, size=m["size"], threads=m["threads"])
    assert CM.manifest_of(CM.tree(out)) == m["outputs"]
    assert {k: st[k] for k in COUNTS} == m["model_stats"]
    assert st["survivors"] <= st["rows"] and st["unions"] < max(st["names"], 1)


def test_one_session_per_window_changes_nothing(tmp_path):
    m = _manifest("multi")
    _, _, fp, pp = _inputs(tmp_path, m["params"])
    st = api.cluster_short(pp, fp, tmp_path / "a", size=m["size"], threads=m["threads"], window_bytes=1)
    assert st["windows"] == st["sessions"] == 3
    assert CM.manifest_of(CM.tree(tmp_path / "a")) == m["outputs"]


@pytest.mark.parametrize("size,threads", [(200, 20), (40, 3)])
def test_library_matches_model_on_larger_input(tmp_path, size, threads):
    n_pairs, n_rows = (200000, 1000000) if LARGE else (100000, 500000)
    fq, paf, fp, pp = _inputs(tmp_path, dict(seed=11, n_pairs=n_pairs, n_rows=n_rows, name_fmt=CI.LONG_NAMES))
    want, wst = CM.run(paf, fq, size, threads)
    out = tmp_path / "tmp"
    st = api.cluster_short(pp, fp, out, size=size, threads=threads)
    assert {k: st[k] for k in COUNTS} == wst
    assert CM.tree(out) == want
    if threads == 3:                  # again with one session per window
        out1 = tmp_path / "w1"
        st1 = api.cluster_short(pp, fp, out1, size=size, threads=threads, window_bytes=1)
        assert st1["windows"] == st1["sessions"] > 1
        assert CM.tree(out1) == want


FQ = b"@r/1\nA\n+\nI\n@r/2\nC\n+\nI\n"


@pytest.mark.parametrize("fq,paf,size,threads", [
    (FQ, b"", 10, 0),
    (FQ, b"", 10, 101),
    (FQ, b"", 0, 1),
    (b">r/1\nA\n", b"", 10, 1),                                               # FASTA
    (b"@r/1\r\nA\n+\nI\n", b"", 10, 1),                                       # CR in the FASTQ
    (b"@r\xc3\xa9/1\nA\n+\nI\n", b"", 10, 1),                                 # byte >= 0x80
    (FQ + FQ, b"", 10, 1),                                                    # duplicate name
    (b'@r"/1\nA\n+\nI\n', b"", 10, 1),                                        # '"' in a name
    (FQ, b"x/1\t1\t2\t3\t+\tr/1\t1\t2\t3\t4\t5\t6\n", 10, 1),                # unknown endpoint
    (FQ, b"r/1\t1\t2\n", 10, 1),                                              # short row
    (FQ, b"r/1\t1\t2\t3\t+\tr/2\t1\t2\t3\t4\t5\t6\r\n", 10, 1),              # CR in the PAF
    (FQ, b">r/1\nACGT\n", 10, 1),                                             # FASTA in place of the PAF
    (b"", b"", 10, 1),                                                        # empty FASTQ
])
def test_refusals_leave_no_tree(tmp_path, fq, paf, size, threads):
    (tmp_path / "r.fq").write_bytes(fq)
    (tmp_path / "r.paf").write_bytes(paf)
    out = tmp_path / "tmp"
    with pytest.raises(api.HlmiError) as e:
        api.cluster_short(tmp_path / "r.paf", tmp_path / "r.fq", out, size=size, threads=threads)
    assert e.value.code == -1
    assert os.listdir(out) == []


def test_cli_gives_the_same_tree(tmp_path):
    m = _manifest("mid")
    _, _, fp, pp = _inputs(tmp_path, m["params"])
    out = tmp_path / "cli"
    r = subprocess.run([sys.executable, "-m", "hylight_amd.cluster_short", pp, fp, "-o", str(out), "--size", str(m["size"]),
                        "-t", str(m["threads"])], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    st = json.loads(r.stdout.strip().splitlines()[-1])
    assert st["files"] == m["model_stats"]["files"]
    assert CM.manifest_of(CM.tree(out)) == m["outputs"]
    (tmp_path / "bad.fq").write_bytes(b">x\nA\n")
    r = subprocess.run([sys.executable, "-m", "hylight_amd.cluster_short", pp, str(tmp_path / "bad.fq"), "-o",
                        str(tmp_path / "bad")], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 4
