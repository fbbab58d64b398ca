"""CPU: the surface of hlmi_polish_reads.  The per-op rule of hylight_amd/csrc/polish_rows.h, compiled with the plain host
compiler into tests/capi/polish_rows_host_check.cpp's program and run; the header's prototype, the binding's SYMBOLS entry
with six arguments and an unchanged HLMI_ABI_VERSION; the driver's and the polish module's new options."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from hylight_amd import api, driver, polish

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hylight_mi.h")


def test_per_op_rule_host_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler on PATH")
    exe = tmp_path / "polish_rows_host_check"
    subprocess.run([cxx, "-std=c++17", "-O1", os.path.join(ROOT, "tests", "capi", "polish_rows_host_check.cpp"), "-o", str(exe)],
                   check=True, cwd=ROOT)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "polish_rows_host_check: ok" in r.stdout


def test_header_prototype_and_abi():
    text = open(HEADER).read()
    flat = re.sub(r"\s+", " ", text)
    assert ("int hlmi_polish_reads(const char *contigs, const char *reads, const hlmi_ava_opts *ao, const hlmi_polish_opts *po, "
            "const char *out_fa, hlmi_polish_stats *st);") in flat
    assert re.findall(r"#define HLMI_ABI_VERSION (\d+)", text) == ["7"] and api.ABI_VERSION == 7
    for word in ("two records of one name", "stub_oh >= 0", "2^32 overlapper rows"):       # the three stated differences
        assert word in flat


def test_symbols_entry():
    res, args = api.SYMBOLS["hlmi_polish_reads"]
    assert res is C.c_int and len(args) == 6
    assert args == [C.c_char_p, C.c_char_p, C.POINTER(api.AvaOpts), C.POINTER(api.PolishOpts), C.c_char_p, C.POINTER(api.PolishStats)]
    assert callable(api.polish_reads)


def test_driver_and_module_options():
    a = driver.build_parser().parse_args(["-l", "x.fq", "--polish_direct"])
    assert a.polish_direct and not a.polish_native
    assert not driver.build_parser().parse_args(["-l", "x.fq"]).polish_direct
    with pytest.raises(SystemExit) as e:
        driver.main(["-l", "x.fq", "--polish_native", "--polish_direct"])
    assert "--polish_direct" in str(e.value)
    p = polish.build_parser().parse_args(["--contigs", "c.fa", "--reads", "r.fa", "--out", "o.fa", "--short"])
    assert p.paf is None and p.short
