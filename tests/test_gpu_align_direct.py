"""The alignment pass, checked directly (tests/capi/align_gpu_check.cpp): a stand-alone HIP program that links against
libhylight_mi.so, calls align_pieces of csrc/ava_align.hip itself on FABRICATED pieces - real bases through upload_reads, Piece
records and fixed points written by the case - and compares every field of every row, the order keys, every CIGAR op, the
set-aside parts and the driver's counts exactly with plain sequential host C++ written from DESIGN.md section 5 items 5 and 7.

CPU: the program compiles and links; `--host` holds the reference to hand-worked literals and to the enumeration of all
alignments of tasks up to 6 x 6; `--dump` of the reference equals the oracle's own align_block / extend_left / extend_right /
close_piece (oracle.ava.align_pieces) on every device case (`--cases`) and on 2 000 random pieces.
GPU: ONE run of the program for all groups; a test per group reads its line."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "capi", "align_gpu_check.cpp")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
GROUPS = ["task_geometry", "band_rule", "certificates", "gap_cost", "run_buffers", "long_tasks", "ungapped", "assembly", "driver"]
DROP_GROUPS = ["assembly", "driver"]                    # groups whose subject includes dropping a piece: both outcomes must occur
HOST_GROUPS = ["ref_task", "ref_enumeration", "ref_piece"]
OPT_FIELDS = ["k", "w", "hpc", "min_chain_score", "max_gap", "bandwidth", "min_cnt", "min_mid_occ", "match", "mismatch", "gap_open",
              "gap_ext", "ambi", "min_dp_score", "end_bonus", "pair_once", "gap_open2", "gap_ext2", "stub_oh", "zdrop"]
VARIANTS = {                                            # tests/test_gpu_ava_structured.py
    "one_piece": dict(gap_open2=0),
    "all_ones": dict(match=1, mismatch=1, gap_open=1, gap_ext=1, gap_open2=0),
    "wide_scores": dict(mismatch=16, gap_open=20, gap_ext=2, gap_open2=0),
}


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
    return _compile(tmp_path_factory.mktemp("align_check") / "align_gpu_check")


def test_check_program_compiles_and_host_references_hold(exe):
    r = subprocess.run([exe, "--host"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    for g in HOST_GROUPS:
        assert any(ln.startswith(f"host {g} cases=") and ln.endswith(" ok") for ln in lines), r.stdout


def _read_cases(path):
    """[(name, opts dict, queries, targets, [(q, t, strand, [(q, t) fixed points])])] of a --cases / --dump input file."""
    cases = []
    with open(path) as f:
        tok = f.read().split()
    x = 0
    while x < len(tok):
        assert tok[x] == "case" and tok[x + 2] == "opts"
        name = tok[x + 1]
        o = {k: int(v) for k, v in zip(OPT_FIELDS, tok[x + 3:x + 23])}
        x += 23
        assert tok[x] == "reads"
        nq, nt = int(tok[x + 1]), int(tok[x + 2])
        Q, T = tok[x + 3:x + 3 + nq], tok[x + 3 + nq:x + 3 + nq + nt]
        x += 3 + nq + nt
        assert tok[x] == "pieces"
        pieces = []
        n = int(tok[x + 1])
        x += 2
        for _ in range(n):
            q, t, strand, _chain, _piece, nf = (int(v) for v in tok[x:x + 6])
            pieces.append((q, t, strand, [(int(tok[x + 6 + 2 * i]), int(tok[x + 7 + 2 * i])) for i in range(nf)]))
            x += 6 + 2 * nf
        cases.append((name, o, Q, T, pieces))
    return cases


def _write_cases(path, cases):
    with open(path, "w") as f:
        for name, o, Q, T, pieces in cases:
            f.write(f"case {name}\nopts " + " ".join(str(o[k]) for k in OPT_FIELDS) + f"\nreads {len(Q)} {len(T)}\n")
            f.write("".join(s + "\n" for s in Q + T))
            f.write(f"pieces {len(pieces)}\n")
            for q, t, strand, fp in pieces:
                f.write(f"{q} {t} {strand} 0 0 {len(fp)} " + " ".join(f"{a} {b}" for a, b in fp) + "\n")


def _reference_rows(exe, path, cases):
    r = subprocess.run([exe, "--dump", path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    got = []
    for ln in r.stdout.splitlines():
        if ln.startswith("case "):
            assert int(ln.split()[1]) == len(got)
            got.append([])
        else:
            got[-1].append(None if ln == "-" else tuple(ln.split()))
    assert [len(g) for g in got] == [len(c[4]) for c in cases]
    return got


def _oracle_rows(cases):
    from oracle import ava as OA
    out = []
    for _name, o, Q, T, pieces in cases:
        opts = OA.opts_long()
        for k, v in o.items():
            setattr(opts, k, v)
        rows = []
        for q, t, strand, fp in pieces:
            c = OA.align_pieces(Q[q], T[t], strand, fp, opts)
            if c is None:
                rows.append(None)
                continue
            assert c[4] == "-+"[1 - strand] and c[12] == f"NM:i:{int(c[10]) - int(c[9])}", c[:13]
            rows.append((c[2], c[3], c[7], c[8], c[9], c[10], c[14][len("cg:Z:"):]))
        out.append(rows)
    return out


def _assert_equal(cases, ref, ora):
    """every piece of every case, no exclusion; returns (rows, dropped)"""
    rows = dropped = 0
    for i, (r, o) in enumerate(zip(ref, ora)):
        for k, (a, b) in enumerate(zip(r, o)):
            assert a == b, (i, cases[i][0], k, cases[i][4][k][2], a, b)
            rows += a is not None
            dropped += a is None
    return rows, dropped


def test_plain_reference_equals_oracle_on_the_device_cases(exe, tmp_path):
    path = str(tmp_path / "cases.txt")
    r = subprocess.run([exe, "--cases", path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    cases = _read_cases(path)
    assert {c[0].split(":")[0] for c in cases} == set(GROUPS)
    rows, dropped = _assert_equal(cases, _reference_rows(exe, path, cases), _oracle_rows(cases))
    assert rows > 2000 and dropped > 10                # (the comparison is not of empty lists, and both outcomes occur)


def _random_cases(n_pieces, seed):
    """Pieces of 1-700 bases per block chain, 2-70 fixed points, block shifts drawn around 0, 5 / 6, 7 / 8 and 39, both presets and
    the three other constant sets, bandwidth 0, both strands, a few ambiguous bases, planted substitutions and indels.  The
    fixed points follow the planted indels, so most pieces clear min_dp_score."""
    from oracle import ava as OA
    rng = np.random.default_rng(seed)
    comp = str.maketrans("ACGTN", "TGCAN")
    sets = []
    for base in (OA.opts_long(), OA.opts_short()):
        sets.append({k: getattr(base, k) for k in OPT_FIELDS})
    for v in VARIANTS.values():
        d = dict(sets[0])
        d.update(v)
        sets.append(d)
    d = dict(sets[0])
    d["bandwidth"] = 0
    sets.append(d)
    d = dict(sets[1])
    d["stub_oh"] = 3
    sets.append(d)
    cases = []
    for g in range(n_pieces):
        o = dict(sets[int(rng.integers(0, len(sets)))])
        if rng.random() < 0.3:
            o["max_gap"] = int(rng.choice([200, 300, 1000]))
        ungapped = o["bandwidth"] == 0
        n_fp = int(rng.integers(2, 71)) if g % 3 else int(rng.integers(2, 6))
        total = int(rng.integers(1, 701))
        bases = "ACGT"
        rs = lambda n: "".join(bases[i] for i in rng.integers(0, 4, n))
        q, t, fp = [rs(int(rng.integers(0, 400)))], None, None
        t = [q[0][len(q[0]) - min(len(q[0]), int(rng.integers(0, 400))):] if rng.random() < 0.8 else rs(int(rng.integers(0, 400)))]
        t[0] = rs(int(rng.integers(0, 60))) + t[0] if rng.random() < 0.5 else t[0]
        ql, tl = len(q[0]), len(t[0])
        fp = [(ql, tl)]
        err = float(rng.choice([0.0, 0.01, 0.03, 0.08, 0.5], p=[0.25, 0.25, 0.2, 0.2, 0.1]))   # (0.5: a piece that is dropped)
        for b in range(n_fp - 1):
            first, last = b == 0, b == n_fp - 2
            m = int(rng.integers(1, 256)) if first else max(1 if last else 32, total // n_fp + int(rng.integers(0, 40)))
            if rng.random() < 0.03:
                m = int(rng.integers(250, 330))
            shift = 0
            if not ungapped and not first:
                c = int(rng.choice([0, 0, 0, 5, 7, 39]))
                shift = int(rng.integers(-1, 2)) + c if c else int(rng.integers(-2, 3))
                shift = int(np.clip(shift * int(rng.choice([-1, 1])), -39, 39))
            n = m + shift
            if n < (1 if last else 32):
                shift = 0
                n = m
            bq = rs(m)
            bt = bq
            at = int(rng.integers(0, min(m, n)))
            if shift > 0:
                bt = bq[:at] + rs(shift) + bq[at:]
            elif shift < 0:
                bt = bq[:at] + bq[at - shift:] if at - shift <= m else bq[:m + shift]
            bt = list(bt[:n].ljust(n, "A"))
            for pos in np.nonzero(rng.random(n) < err)[0]:
                bt[pos] = bases[int(rng.integers(0, 4))]
            if rng.random() < 0.05:
                bt[int(rng.integers(0, n))] = "N"
            q.append(bq)
            t.append("".join(bt))
            ql += m
            tl += n
            fp.append((ql, tl))
        tail = rs(int(rng.integers(0, 500)))
        q.append(tail[:int(rng.integers(0, len(tail) + 1))])
        t.append(tail[:int(rng.integers(0, len(tail) + 1))] if rng.random() < 0.8 else rs(int(rng.integers(0, 300))))
        qs, ts = "".join(q), "".join(t)
        if not qs or not ts:
            continue
        strand = int(rng.integers(0, 2))
        if strand:
            qs = qs.translate(comp)[::-1]
        cases.append((f"random_{g}", o, [qs], [ts], [(0, 0, strand, fp)]))
    return cases


def test_plain_reference_equals_oracle_on_random_pieces(exe, tmp_path):
    cases = _random_cases(2000, 11)
    assert len(cases) >= 1990
    ora = _oracle_rows(cases)
    kept = sum(r[0] is not None for r in ora)
    assert 2 * kept >= len(cases), (kept, len(cases))   # (the generator: the oracle alone yields a row for at least half the pieces)
    path = str(tmp_path / "random.txt")
    _write_cases(path, cases)
    rows, dropped = _assert_equal(cases, _reference_rows(exe, path, cases), ora)
    assert rows == kept and dropped > 20


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
    kept, dropped = (int(line[0].split(k + "=")[1].split()[0]) for k in ("kept", "dropped"))
    assert kept > 0, out
    if group in DROP_GROUPS:
        assert dropped > 0, out
