"""The polyhedral trajectory generator's kernel text (csrc/trajgen.hpp over csrc/trajgen_poly.hpp) on the CPU, against the numpy model.

tests/host/trajgen_poly_check.cpp is a stand-alone program (its own main, no HIP, not loaded into Python): it includes the kernel over
tests/host/hip_stub (threads for lanes, a barrier for __syncthreads, a global array of sizeof(PolyLds) for LDS), is built here with
the address and undefined-behaviour sanitizers exactly as tests/test_trajgen_host.py builds its program, and run once over one ragged
batch: an out-of-bounds LDS index, plane, row or record is the sanitizer's to report, and the numbers are compared with the model.

Status and iteration counts are compared exactly.  Measured here over this table: the largest difference of a row entry from the
model 1.8e-9 (the sixteen-segment candidate, stopped at 150 iterations far from convergence; every other candidate is below 3e-12)
and of a record field 7.1e-9 relative to max(1, |model|) (its cost); the tolerances are 100 x those, the rule tests/test_gpu_trajgen.py
states for itself: both sides reassociate fp64 sums differently (LAPACK inverses there, block Cholesky factors here)."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import trajgen_poly_model as PM  # noqa: E402

ROW_TOL = 1.8e-7          # 100 x the measured 1.8e-9
REC_TOL = 7.1e-7          # 100 x the measured 7.1e-9, relative to max(1, |model|)


def host_table():
    """the ragged batch of the issue: (names, candidates, expected status)"""
    cs, inv = PM.cases(), PM.invalid_cases()
    names = ["quintic_plane", "face", "bend", "vertex", "free2", "sixteen", "planes25", "zero_norm", "empty", "quintic_touch"]
    cands = [cs[n] for n in names[:5]] + [PM.sixteen_route(), inv["planes25"], inv["zero_norm"], PM.empty_case(), PM.quintic_touch_case()]
    want = [PM.OK, PM.OK, PM.OK, PM.OK, PM.OK, PM.NOT_CONVERGED, PM.INVALID, PM.INVALID, PM.NOT_CONVERGED, PM.NOT_CONVERGED]
    return names, cands, want


def test_kernel_text_on_the_cpu_matches_the_model(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build tests/host/trajgen_poly_check.cpp")
    exe = str(tmp_path / "trajgen_poly_check")
    subprocess.run([gxx, "-std=c++20", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-pthread", "-I" + os.path.join(ROOT, "tests", "host", "hip_stub"), "-I" + os.path.join(ROOT, "include"),
                    "-o", exe, os.path.join(ROOT, "tests", "host", "trajgen_poly_check.cpp")], check=True)
    names, cands, want = host_table()
    assert [len(p) for p in cands[5]["planes"]] == [PM.MAX_PLANES] * 16 and list(cands[5]["orders"]) == [12] * 16
    assert max(len(p) for p in cands[6]["planes"]) == PM.MAX_PLANES + 1
    prm = PM.params(max_vel=6.0, max_acc=12.0, max_iter=150)
    stride = 39
    PM.write_batch_text(str(tmp_path / "in.txt"), cands, prm, stride)
    r = subprocess.run([exe, str(tmp_path / "in.txt"), str(tmp_path / "out.txt")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    rows, res = PM.read_result_text(str(tmp_path / "out.txt"), len(cands), stride)
    stages = []
    mrows, mres = PM.solve_batch(cands, prm, stride, stages=stages)
    assert {0, 1, 2, 3, -1} <= set(stages), "the table is meant to reach every stage of the projection"
    assert np.array_equal(res["status"], mres["status"]) and np.array_equal(res["iterations"], mres["iterations"]), (res, mres)
    assert list(res["status"]) == want
    offs = PM.pack(cands)["seg_offsets"]
    worst_row = worst_rec = 0.0
    for b, name in enumerate(names):
        a, e = offs[b], offs[b + 1]
        if want[b] == PM.INVALID:
            assert np.all(np.isnan(rows[a:e])) and np.isnan(res["cost"][b])
            continue
        gap = float(np.abs(rows[a:e] - mrows[a:e]).max())
        worst_row = max(worst_row, gap)
        for f in ("cost", "duration", "r_prim", "r_dual", "sphere_slack", "max_vel_ctrl", "max_acc_ctrl"):
            worst_rec = max(worst_rec, abs(res[f][b] - mres[f][b]) / max(1.0, abs(mres[f][b])))
        print(f"{name}: status {res['status'][b]} iterations {res['iterations'][b]} row gap {gap:.3e}")
    print(f"largest row gap {worst_row:.3e}, largest record gap {worst_rec:.3e}")
    assert worst_row <= ROW_TOL and worst_rec <= REC_TOL
    assert res["sphere_slack"][4] > 40.0 and res["sphere_slack"][8] < 0.0 and res["r_prim"][8] > prm["eps"]
    # the single quintic with its plane active: inside the plane, outside the shrunk one, honest residuals
    assert 4e-6 < res["sphere_slack"][9] < 6e-6 and 1.4e-5 < res["r_prim"][9] < 1.6e-5
