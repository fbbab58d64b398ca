"""The device primitives and the wave operations, checked directly (tests/capi/dev_prims_gpu_check.cpp): a stand-alone HIP
program that links against libhylight_mi.so, calls the hlmi:: functions of csrc/dev_prims.hip, csrc/wave_ops.h and
csrc/dev_search.h themselves and compares every result exactly with plain host C++ - sequential loops for the selections and
the run heads, std::stable_sort on the masked key for the sorts, a 64-bit sequential sum for the scans, std::lower_bound, a
per-lane loop over 64 values for each wave operation.  No C-ABI entry point is involved: the library is built without a
visibility flag, so the C++ symbols are dynamic (nm -DC libhylight_mi.so lists hlmi::sort_*, hlmi::select_*,
hlmi::exclusive_scan_*, hlmi::stream, hlmi::dev_alloc).

CPU: the program compiles and links, and `--host` (bits_for, every host reference against literal hand cases) passes.
GPU: ONE run of the program for all groups; a test per group reads its line.

Sizes: 0 1 2 3 4 5 63 64 65 127 128 129 255 256 257 1023 1024 1025 4095 4096 4097 100003 for every primitive (a block of the
four-per-thread kernels covers 1024 elements, a wave 256, a mask word 64).  The sorts add 16383 16384 16385 and 1049605.
Where the last one comes from: rocprim/device/device_radix_sort.hpp (radix_sort_impl) takes merge sort while
`size <= merge_sort_limit && (sizeof(key_type) > 2 || size < 100000)` and onesweep above; merge_sort_limit is the fourth
parameter of radix_sort_config in rocprim/device/device_radix_sort_config.hpp, 1024 * 1024 unless a configuration sets it,
and the project's two configurations (dev_prims.hip: PairsOnesweep, KeysOnesweep) do not.  So 1049605 = 2^20 + 1029 puts the
64- and 32-bit keys on the onesweep path, and the 16-bit keys are there from 100000 on (100003).  For 16-bit keys the range
[8, 24) of the wider keys is [4, 12): bits above 15 do not exist.

Full waves only, and no in-place scan.  Every call site of a wave operation in csrc (ava_align.hip, ava_chain.hip,
dev_prims.hip, filter_stage.hip, polish.hip, polish_rows.hip, seed_group.hip) was read: each is reached in wave-uniform control
flow with all 64 lanes active, lanes without work contribute a neutral operand.  No caller passes in == out to
exclusive_scan_u32 or exclusive_scan_u64."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "capi", "dev_prims_gpu_check.cpp")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
GROUPS = ["select", "classes4", "heads", "sort", "scan", "search", "wave", "refusal"]
HOST_GROUPS = ["bits_for", "ref_select", "ref_classes4", "ref_heads", "ref_sort", "ref_scan", "ref_lower_bound", "ref_wave"]


def _compile(out):
    from hylight_amd import api
    api.load()                                     # (the library exists)
    lib_dir = os.path.join(ROOT, "hylight_amd")
    cmd = [HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O2", "-x", "hip", "-I" + os.path.join(ROOT, "hylight_amd", "csrc"),
           "-I" + os.path.join(ROOT, "include"), SRC, "-o", str(out), "-L" + lib_dir, "-lhylight_mi", "-Wl,-rpath," + lib_dir]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(out)


def test_check_program_compiles_and_host_references_hold(tmp_path):
    exe = _compile(tmp_path / "dev_prims_gpu_check")
    r = subprocess.run([exe, "--host"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    for g in HOST_GROUPS:
        assert any(ln.startswith(f"host {g} cases=") and ln.endswith(" ok") for ln in lines), r.stdout


@pytest.fixture(scope="module")
def device_run(tmp_path_factory):
    exe = _compile(tmp_path_factory.mktemp("dev_prims") / "dev_prims_gpu_check")
    return subprocess.run([exe], capture_output=True, text=True, timeout=180)


@pytest.mark.gpu
@pytest.mark.parametrize("group", GROUPS)
def test_device_group(device_run, group):
    r = device_run
    out = r.stdout + r.stderr
    assert r.returncode == 0, out
    line = [ln for ln in r.stdout.splitlines() if ln.startswith(f"group {group} cases=")]
    assert len(line) == 1 and line[0].endswith(" ok") and int(line[0].split("cases=")[1].split()[0]) > 0, out
