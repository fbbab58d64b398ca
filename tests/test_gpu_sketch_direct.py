"""The read store and the sketch, checked directly (tests/capi/sketch_gpu_check.cpp): a stand-alone HIP program that links
against libhylight_mi.so, calls upload_reads (both overloads), subset_reads_device, DevReads::pack (through the uploads),
sketch_device and sketch_device_into of csrc/sketch.hip themselves and compares every byte of the store, every packed base,
every ambiguity flag, every minimizer and every per-read count exactly with plain sequential host C++ written from the
definitions: a 256-entry table, a loop over the bases, and for the sketch a triple loop (slot, window, key) per read - no
queue, no rolling word, no tile.

CPU: the program compiles and links; `--host` holds the references to literal hand cases; `--dump` of the plain reference
equals oracle.ava.sketch entry for entry at six (k, w, hpc), so the new reference and the specification oracle hold each other
before anything runs on a card.
GPU: ONE run of the program for all groups; a test per group reads its line.

What the groups put on an edge: k in {3 .. 27} x w in {1 .. 64} x hpc on one mixed set (the LDS tiles of kmer_kernel and
pick_kernel have room for w + k - 1 <= 91 symbols and 2 (w - 1) keys of halo); reads of 0, 1, k - 1, k, k + w - 2, k + w - 1,
k + w, k + 2w slots; a read boundary, an ambiguous base, the first valid window and the end of the slot array at slots
255 / 256 / 257 of a 256-slot tile; equal keys inside one window; k-mers of 254 .. 257 bases (the span byte); 5000 reads of
0 .. 3 bases; parts of a set sketched with a rid_base; stores whose granule count passes 32, 64 and 256 (one flag word per
half wave of pack_kernel)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "capi", "sketch_gpu_check.cpp")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
GROUPS = ["encode", "pack", "subset", "sketch_grid", "sketch_lengths", "sketch_tiles", "sketch_ties", "sketch_spans",
          "sketch_many_reads", "sketch_parts", "refusal"]
HOST_GROUPS = ["ref_encode", "ref_hash", "ref_pack", "ref_sketch"]
DUMP_SETTINGS = [(19, 5, 1), (21, 11, 0), (15, 8, 1), (27, 64, 1), (3, 1, 0), (5, 2, 1)]


def _compile(out):
    from hylight_amd import api
    api.load()                                     # (the library exists)
    lib_dir = os.path.join(ROOT, "hylight_amd")
    cmd = [HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O2", "-x", "hip", "-I" + os.path.join(ROOT, "hylight_amd", "csrc"),
           "-I" + os.path.join(ROOT, "include"), SRC, "-o", str(out), "-L" + lib_dir, "-lhylight_mi", "-Wl,-rpath," + lib_dir]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(out)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("sketch_check") / "sketch_gpu_check")


def test_check_program_compiles_and_host_references_hold(exe):
    r = subprocess.run([exe, "--host"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    for g in HOST_GROUPS:
        assert any(ln.startswith(f"host {g} cases=") and ln.endswith(" ok") for ln in lines), r.stdout


def _dump_sequences():
    """Random reads, one with Ns, one lower-case, one with a 300-base run, a period-3 repeat, 15 bases, an empty read."""
    rng = np.random.default_rng(20)

    def rand(n):
        return "".join("ACGT"[i] for i in rng.integers(0, 4, n))
    with_n = list(rand(400))
    for at in (0, 57, 58, 200, 399):
        with_n[at] = "N"
    return [rand(500), rand(333), "".join(with_n), rand(300).lower(), rand(150) + "G" * 300 + rand(150), "ACG" * 100,
            rand(15), "", rand(700)]


@pytest.fixture(scope="module")
def dump_file(tmp_path_factory):
    seqs = _dump_sequences()
    path = tmp_path_factory.mktemp("sketch_dump") / "seqs.txt"
    path.write_text("".join(s + "\n" for s in seqs))
    return str(path), seqs


@pytest.mark.parametrize("k,w,hpc", DUMP_SETTINGS)
def test_plain_reference_equals_oracle(exe, dump_file, k, w, hpc):
    from oracle import ava as OA
    path, seqs = dump_file
    r = subprocess.run([exe, "--dump", path, str(k), str(w), str(hpc)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    got, total = [], 0
    for ln in r.stdout.splitlines():
        if ln.startswith("read "):
            got.append([])
            assert int(ln.split()[1]) == len(got) - 1
            declared = int(ln.split("n=")[1])
            total += declared
        else:
            x, y = ln.split()
            got[-1].append((int(x), int(y)))
    assert len(got) == len(seqs) and sum(len(g) for g in got) == total
    n_mz = 0
    for rid, seq in enumerate(seqs):
        want = [(int(x), int(y)) for x, y in OA.sketch(seq.encode(), rid, k, w, hpc)]
        assert got[rid] == want, (rid, len(want), len(got[rid]))
        n_mz += len(want)
    assert n_mz > 40                                  # (the comparison is not of empty lists; w = 64 keeps about one slot in 32)


@pytest.fixture(scope="module")
def device_run(exe):
    return subprocess.run([exe], capture_output=True, text=True, timeout=180)


@pytest.mark.gpu
@pytest.mark.parametrize("group", GROUPS)
def test_device_group(device_run, group):
    r = device_run
    out = r.stdout + r.stderr
    assert r.returncode == 0, out
    line = [ln for ln in r.stdout.splitlines() if ln.startswith(f"group {group} cases=")]
    assert len(line) == 1 and line[0].endswith(" ok") and int(line[0].split("cases=")[1].split()[0]) > 0, out
