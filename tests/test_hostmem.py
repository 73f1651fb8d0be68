"""csrc/hostmem.hpp on the CPU: the owning grow-only buffer, the doubling rule and the polled wait.

tests/host/hostmem_check.cpp is a stand-alone program (its own main, no HIP, not loaded into Python) over a fake memory kind; it is
built here with the address and undefined-behaviour sanitizers and run once.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hostmem_check(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build tests/host/hostmem_check.cpp")
    exe = str(tmp_path / "hostmem_check")
    src = os.path.join(ROOT, "tests", "host", "hostmem_check.cpp")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-pthread", "-o", exe, src], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "hostmem ok" in r.stdout
