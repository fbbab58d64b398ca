"""bench.py --dump-outputs without a GPU: the PAF rows of a stage call as float64 arrays (tests/golden/fxA_stage_nsplit4.paf, a
stage output), the seeded sample when they do not fit, and the files one dump writes."""
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

PAF = os.path.join(ROOT, "tests", "golden", "fxA_stage_nsplit4.paf")


def test_every_row_and_column_of_a_stage_output():
    lines = open(PAF).read().split("\n")[:-1]
    a = bench.paf_arrays(PAF, 1 << 30)
    assert a.dtype == np.float64 and a.shape == (len(lines), 14 + 2)
    for i in (0, len(lines) // 2, len(lines) - 1):
        f = lines[i].rstrip("\t").split("\t")
        assert a[i, 0] == i and a[i, -1] == zlib.crc32(lines[i].encode())
        assert a[i, 1] == zlib.crc32(f[0].encode()) and a[i, 6] == zlib.crc32(f[5].encode())
        assert a[i, 5] == (1.0 if f[4] == "+" else -1.0)
        assert list(a[i, 2:5]) == [float(x) for x in f[1:4]] and list(a[i, 7:15]) == [float(x) for x in f[6:14]]


def test_a_larger_output_is_a_fixed_sample_within_the_budget():
    a = bench.paf_arrays(PAF, 1 << 30)
    b = bench.paf_arrays(PAF, 100 * 8 * 16)
    assert b.shape == (100, 16) and b.nbytes <= 100 * 8 * 16
    assert (np.diff(b[:, 0]) > 0).all() and np.array_equal(a[b[:, 0].astype(int)], b)
    assert np.array_equal(b, bench.paf_arrays(PAF, 100 * 8 * 16))


def test_one_dump(tmp_path):
    bench.dump_outputs(str(tmp_path / "d"), [PAF, PAF], [7, 9])
    assert sorted(os.listdir(tmp_path / "d")) == ["overlaps.npy", "stage_rows.npy", "stage_rows_call1.npy"]
    assert np.load(tmp_path / "d" / "overlaps.npy").tolist() == [7.0, 9.0]
    assert np.array_equal(np.load(tmp_path / "d" / "stage_rows.npy"), np.load(tmp_path / "d" / "stage_rows_call1.npy"))
    assert sum(os.path.getsize(tmp_path / "d" / f) for f in os.listdir(tmp_path / "d")) <= bench.DUMP_LIMIT_BYTES
