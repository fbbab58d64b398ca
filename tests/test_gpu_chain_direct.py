"""The index, the seeds and the chains, checked directly (tests/capi/chain_gpu_check.cpp): a stand-alone HIP program that links
against libhylight_mi.so, calls build_index, plan_seeds and seed_and_chain of csrc/ava_chain.hip themselves on FABRICATED
minimizers and read lengths (nothing in this layer reads a base) and compares every index array, every per-minimizer count and
run, every anchor (through the isolating options max_gap = 0, min_cnt = 1, min_chain_score = 1: an anchor is then a chain of one
piece) and every piece with its fixed points exactly with plain sequential host C++ written from DESIGN.md section 5 items 2-5.

CPU: the program compiles and links; `--host` holds the references to hand-worked literal cases; `--dump` of the plain chain
reference equals the oracle's own chain_group (oracle.ava.chain_pieces) on the anchor groups of the device cases (`--cases`) and
on a few thousand random groups, so the new reference and the specification oracle hold each other before anything runs on a
card.
GPU: ONE run of the program for all groups; a test per group reads its line.

What the groups put on an edge: index_cutoff - 1 / 2 / 257 chunks (HIST_LDS_CHUNKS 256), run lengths 7 / 8 / 9 (HIST_LDS_LEN),
a quantile run length of 1022 / 1023 / 1024 in chunk 0 and in a later chunk (the 1024-bin histogram and the exact-quantile path
behind it), f <= 0, a count at and above the cut-off, the clamp; index_order - equal names, several positions of a hash, too
frequent entries, n = 0 .. 33, bucket bits capped by 2k, rank_bits = 0 by widths and by hook; seed_count - buckets of 15 / 16 / 17
words and the 16-word guess window; seed_fill - SHORT_RUN 32, four short runs at a time, spans 1 and 255, the three anchor word
forms by widths and by hook; chain_sizes - SMALL_N 32, rows of 16, 64-anchor windows, more than 65 535 anchors; chain_window -
predecessors 1 .. 64 back and one 65 back; chain_limits - max_gap, bandwidth, the gap cost, PEN_TAB 2048, the byte / 16-bit
table, either side of the packed form; chain_ties; emit_windows - 64-anchor windows and their last 8 lanes; emit_splits -
SHIFT_MAX 39 and PIECE_BUF 32; refusal - the limits of seed_and_chain; seed_group - the chain_* and emit_* sets once more
under HLMI_SEED_GROUP after seed_group_prepare, with the statistics showing that every batch that may take seed_group.hip does."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "capi", "chain_gpu_check.cpp")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
GROUPS = ["index_cutoff", "index_order", "seed_count", "seed_fill", "chain_sizes", "chain_window", "chain_limits", "chain_ties",
          "emit_windows", "emit_splits", "refusal", "seed_group"]
HOST_GROUPS = ["ref_gap_cost", "ref_chain", "ref_index"]


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
    return _compile(tmp_path_factory.mktemp("chain_check") / "chain_gpu_check")


def test_check_program_compiles_and_host_references_hold(exe):
    r = subprocess.run([exe, "--host"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    for g in HOST_GROUPS:
        assert any(ln.startswith(f"host {g} cases=") and ln.endswith(" ok") for ln in lines), r.stdout


def _read_groups(path):
    """[(opts tuple (k, max_gap, bandwidth, min_chain_score, min_cnt), [(tpos, qpos, span)])] of a --cases / --dump input file."""
    groups = []
    with open(path) as f:
        tok = f.read().split()
    x = 0
    while x < len(tok):
        assert tok[x] == "group"
        k, gap, bw, ms, mc, n = (int(v) for v in tok[x + 1:x + 7])
        a = [(int(tok[x + 7 + 3 * i]), int(tok[x + 8 + 3 * i]), int(tok[x + 9 + 3 * i])) for i in range(n)]
        groups.append(((k, gap, bw, ms, mc), a))
        x += 7 + 3 * n
    return groups


def _write_groups(path, groups):
    with open(path, "w") as f:
        for (k, gap, bw, ms, mc), a in groups:
            f.write(f"group {k} {gap} {bw} {ms} {mc} {len(a)}\n")
            f.write("".join(f"{t} {q} {s}\n" for t, q, s in a))


def _reference_pieces(exe, path, n_groups):
    r = subprocess.run([exe, "--dump", path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = []
    for ln in r.stdout.splitlines():
        if ln.startswith("group "):
            assert int(ln.split()[1]) == len(got)
            got.append([])
        else:
            v = [int(t) for t in ln.split()]
            assert len(v) == 3 + 2 * v[2]
            got[-1].append((v[0], v[1], [(v[3 + 2 * i], v[4 + 2 * i]) for i in range(v[2])]))
    assert len(got) == n_groups
    return got


def _oracle_pieces(groups):
    from oracle import ava as OA
    out = []
    for (k, gap, bw, ms, mc), a in groups:
        o = OA.opts_long()
        o.k, o.max_gap, o.bandwidth, o.min_chain_score, o.min_cnt = k, gap, bw, ms, mc
        out.append(OA.chain_pieces(a, o))
    return out


def _assert_equal(groups, ref, ora):
    n_pieces = 0
    for i, (r, o) in enumerate(zip(ref, ora)):
        assert r == o, (i, groups[i][0], len(groups[i][1]), r[:2], o[:2])
        n_pieces += len(r)
    return n_pieces


def test_plain_reference_equals_oracle_on_the_device_cases(exe, tmp_path):
    path = str(tmp_path / "cases.txt")
    r = subprocess.run([exe, "--cases", path], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    groups = _read_groups(path)
    assert len(groups) > 150
    n_pieces = _assert_equal(groups, _reference_pieces(exe, path, len(groups)), _oracle_pieces(groups))
    assert n_pieces > len(groups) // 2                # (the comparison is not of empty lists)


def _random_groups(n_groups, seed):
    """Sizes 1-300; mostly collinear with jitter, strays far off the diagonal, duplicated query positions, shifts around 39,
    both presets' chaining constants and a few others; query positions ascend (the chaining order of a group)."""
    rng = np.random.default_rng(seed)
    presets = [(19, 10000, 2000, 100, 3), (21, 200, 50, 30, 2), (19, 500, 300, 40, 3), (19, 10000, 0, 40, 2), (15, 100, 2047, 1, 1),
               (19, 0, 2000, 1, 1)]
    groups = []
    for g in range(n_groups):
        opt = presets[int(rng.integers(0, len(presets)))]
        n = int(rng.integers(1, 301)) if g % 4 else int(rng.integers(1, 12))
        step_hi = int(rng.choice([3, 20, 45, 120]))
        jitter = int(rng.choice([0, 1, 3, 45]))
        q, t = int(rng.integers(0, 40)), int(rng.integers(0, 40))
        a = []
        for _ in range(n):
            u = rng.random()
            if u < 0.08 and a:                        # the query position of the anchor before
                a.append((int(rng.integers(0, 60000)), a[-1][1], int(rng.integers(1, 256))))
                continue
            d = int(rng.integers(1, step_hi + 1))
            q += d
            t += d + (int(rng.integers(-jitter, jitter + 1)) if rng.random() < 0.3 else 0)
            if u < 0.16:                              # a stray
                a.append((int(rng.integers(0, 60000)), q, 19))
            elif u < 0.2:                             # a shift at the edge of one block
                t += int(rng.choice([38, 39, 40, 41]))
                a.append((max(t, 0), q, 19))
            else:
                a.append((max(t, 0), q, int(rng.choice([15, 19, 21, 1, 255])) if rng.random() < 0.2 else opt[0]))
        groups.append((opt, a))
    return groups


def test_plain_reference_equals_oracle_on_random_groups(exe, tmp_path):
    groups = _random_groups(3000, 5)
    path = str(tmp_path / "random.txt")
    _write_groups(path, groups)
    n_pieces = _assert_equal(groups, _reference_pieces(exe, path, len(groups)), _oracle_pieces(groups))
    assert n_pieces > 2000


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
