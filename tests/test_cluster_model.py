"""CPU: tests/cluster_model.py (the plain-Python restatement of HyLight's short-read clustering) against the manifests
that tests/golden/make_goldens_cluster.py wrote from the reference scripts themselves, and its refusals."""
import hashlib
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import cluster_inputs as CI  # noqa: E402
import cluster_model as CM  # noqa: E402
import make_goldens_cluster as MG  # noqa: E402

CASES = sorted(MG.CASES)


def manifest(name):
    with open(os.path.join(HERE, "golden", f"fxH_cluster_{name}.json")) as f:
        return json.load(f)


def test_every_case_has_a_manifest_with_its_parameters():
    for name in CASES:
        m = manifest(name)
        params, size, threads = MG.CASES[name]
        assert (m["params"], m["size"], m["threads"]) == (params, size, threads)


@pytest.mark.parametrize("name", CASES)
def test_model_matches_reference_manifest(name):
    m = manifest(name)
    fq, paf = CI.make_case(**m["params"])
    assert [len(fq), hashlib.sha256(fq).hexdigest()] == m["inputs"]["fastq"]
    assert [len(paf), hashlib.sha256(paf).hexdigest()] == m["inputs"]["paf"]
    files, st = CM.run(paf, fq, m["size"], m["threads"])
    assert CM.manifest_of(files) == m["outputs"]
    assert st == m["model_stats"]


def test_cases_cover_the_quirks():
    hand, multi, t64, few = manifest("hand_s30"), manifest("multi"), manifest("t64"), manifest("few")
    assert hand["model_stats"]["files"] > 0
    st = multi["model_stats"]
    assert st["chunks"] >= 5 and st["chunks"] % multi["threads"] != 0          # a short last session
    assert st["strict_rejects"] >= 1                                         # rows dropped only by '<'
    assert t64["model_stats"]["reads_sliced"] > 0
    assert few["outputs"][f"HiStrain_max{few['size']}_final_clusters_grouped.json"][0] == 2       # "{}"
    assert [k for k in few["outputs"] if k.startswith("fq_")] == [f"fq_{few['size']}/"]


def test_hand_case_header_oddities():
    fq, paf = CI.make_case(**MG.CASES["hand_s30"][0])
    names = CM.readnames(fq)
    assert b"x/1y" in names and b"a/b" in names and b"" in names and b"noslash" not in names
    files, _ = CM.run(paf, fq, 30, 1)
    grouped = json.loads(files["HiStrain_max30_final_clusters_grouped.json"])
    (cid, members), = grouped.items()
    assert "x/1y" in members
    # "@x/1y/2" is a mate-2 record that demuxes under the name "1y" (no such read): it is written nowhere
    assert not any(b"@x/1y/2" in v for v in files.values() if v)


def test_forest_pathlen_rule():
    """bin_pointer:83-91: the root of the endpoint with the shorter path hangs under the other; ties hang root 1 under 2"""
    F = CM.Forest(4)
    F.parent[2] = 1                  # 2 -> 1 (depth 1)
    assert F.find(2) == (1, 2) and F.find(3) == (3, 1)


@pytest.mark.parametrize("fq,paf,size,threads,what", [
    (b"@r/1\nA\n+\nI\n", b"", 10, 0, "threads"),
    (b"@r/1\nA\n+\nI\n", b"", 10, 101, "threads"),
    (b"@r/1\nA\n+\nI\n", b"", 0, 1, "size"),
    (b">r/1\nA\n", b"", 10, 1, "'@'"),
    (b"@r/1\r\nA\n+\nI\n", b"", 10, 1, "CR"),
    (b"@r/1\nA\n+\nI\n@r/1\nA\n+\nI\n", b"", 10, 1, "duplicate"),
    (b'@r"/1\nA\n+\nI\n', b"", 10, 1, '"'),
    (b"@r/1\nA\n+\nI\n", b"x/1\t1\t2\t3\t+\tr/1\t1\t2\t3\t4\t5\t6\n", 10, 1, "readnames"),
    (b"@r/1\nA\n+\nI\n", b"r/1\t1\t2\n", 10, 1, "12 columns"),
    (b"@r/1\nA\n+\nI\n", b"r/1\t1\t2\t3\t+\tr/1\t1\t2\t3\t4\t5\t6\r\n", 10, 1, "CR"),
    (b"", b"", 10, 1, "empty"),
])
def test_model_refusals(fq, paf, size, threads, what):
    with pytest.raises(CM.Refused, match=what if what != '"' else '"'):
        CM.run(paf, fq, size, threads)
