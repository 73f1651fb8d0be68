"""The trajectory generator's kernel text (csrc/trajgen.hpp) on the CPU, against the numpy model.

tests/host/trajgen_check.cpp is a stand-alone program (its own main, no HIP, not loaded into Python): it includes the kernel over
tests/host/hip_stub (threads for lanes, a barrier for __syncthreads, a global array for LDS), is built here with the address and
undefined-behaviour sanitizers and run once over a small ragged batch: an out-of-bounds LDS index, row or record is the sanitizer's
to report, and the numbers are compared with the model.
"""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import trajgen_model as M  # noqa: E402


def test_kernel_text_on_the_cpu_matches_the_model(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build tests/host/trajgen_check.cpp")
    exe = str(tmp_path / "trajgen_check")
    subprocess.run([gxx, "-std=c++20", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-pthread", "-I" + os.path.join(ROOT, "tests", "host", "hip_stub"), "-I" + os.path.join(ROOT, "include"),
                    "-o", exe, os.path.join(ROOT, "tests", "host", "trajgen_check.cpp")], check=True)
    cases = M.cases()
    prm = M.params(max_vel=6.0, max_acc=12.0, max_iter=150)
    sixteen = M.generator_corridor(4, 16, order=12)
    cands = [cases["quintic"], cases["bend"], cases["gen5"],
             dict(cases["big2"], seg_time=np.array([1.0, -1.0])),                                                    # INVALID: a time that is not > 0
             dict(centres=sixteen[0], radius=sixteen[1], seg_time=sixteen[2], orders=sixteen[3], start=M.rest(sixteen[0][0]), end=M.rest(sixteen[0][-1])),
             dict(cases["big3"], orders=np.array([5, 12, 7], np.int32))]
    stride = 39
    M.write_batch_text(str(tmp_path / "in.txt"), cands, prm, stride)
    r = subprocess.run([exe, str(tmp_path / "in.txt"), str(tmp_path / "out.txt")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    rows, res = M.read_result_text(str(tmp_path / "out.txt"), len(cands), stride)
    mrows, mres = M.solve_batch(cands, prm, stride)
    assert np.array_equal(res["status"], mres["status"]) and np.array_equal(res["iterations"], mres["iterations"]), (res, mres)
    assert list(res["status"]) == [M.OK, M.OK, M.NOT_CONVERGED, M.INVALID, M.NOT_CONVERGED, M.OK]
    bad = res["status"] == M.INVALID
    offs = M.pack(cands)["seg_offsets"]
    for b in range(len(cands)):
        a, e = offs[b], offs[b + 1]
        if bad[b]:
            assert np.all(np.isnan(rows[a:e])) and np.isnan(res["cost"][b])
            continue
        assert np.abs(rows[a:e] - mrows[a:e]).max() < 1e-8
        for name in ("cost", "duration", "r_prim", "r_dual", "sphere_slack", "max_vel_ctrl", "max_acc_ctrl"):
            assert abs(res[name][b] - mres[name][b]) <= 1e-7 * max(1.0, abs(mres[name][b])), (b, name, res[name][b], mres[name][b])
