"""CPU: hylight_amd/csrc/align_score_setup.h - the kernel forms and certificates the alignment pass derives from the scoring
options - compiled with the plain host compiler into tests/capi/align_setup_host_check.cpp's program, once plain and once under
the address and undefined-behaviour sanitizers, and run directly."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.mark.parametrize("extra", [[], SANITIZE], ids=["plain", "sanitized"])
def test_align_setup_host_program(tmp_path, extra):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler on PATH")
    exe = tmp_path / "align_setup_host_check"
    flags = ["-std=c++17", "-O1", "-Wall", "-Werror", *extra]
    subprocess.run([cxx, *flags, os.path.join(ROOT, "tests", "capi", "align_setup_host_check.cpp"), "-o", str(exe)], check=True, cwd=ROOT)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "align_setup_host_check: ok" in r.stdout

