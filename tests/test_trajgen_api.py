"""The trajectory generator as the interface states it (no GPU needed): the prototypes, the record's size and layout in C, ctypes and
the model, the header's contract paragraph, the exported symbols, that the header is C99 and C++17, the Python binding, the C++ mirror
members and the example the build compiles."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import trajgen_model as M  # noqa: E402

SYMBOLS = {
    "pct_bezier_generate_batch": ["const pct_trajgen_batch *batch", "const pct_trajgen_params *params", "double *polycoef", "int64_t row_stride",
                                  "pct_trajgen_result *result"],
    "pct_bezier_generate_batch_dev": ["const pct_trajgen_batch *d_fields", "const pct_trajgen_params *params", "double *d_polycoef", "int64_t row_stride",
                                      "pct_trajgen_result *d_res", "void *stream"],
    "pct_time_allocation": ["const double *centres", "const double *radius", "int64_t n", "const double start[3]", "const double end[3]",
                            "const double init_vel[3]", "double vel_mean", "double acc_mean", "double *seg_time"],
}
RESULT_FIELDS = ("status", "iterations", "cost", "duration", "r_prim", "r_dual", "sphere_slack", "max_vel_ctrl", "max_acc_ctrl")


def header():
    return open(os.path.join(ROOT, "include", "pct_trajgen.h")).read()


def test_header_declares_the_prototypes():
    code = re.sub(r"/\*.*?\*/", " ", header(), flags=re.S)
    for name, want in SYMBOLS.items():
        m = re.search(r"int\s+" + name + r"\s*\((.*?)\)\s*;", code, flags=re.S)
        assert m, f"{name} is not declared"
        assert [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")] == want, name
    for k, name in enumerate(("PCT_GEN_OK", "PCT_GEN_NOT_CONVERGED", "PCT_GEN_INVALID")):
        assert re.search(name + r"\s*=\s*%d\b" % k, code), name
    assert (M.OK, M.NOT_CONVERGED, M.INVALID) == (0, 1, 2)
    for field in ("centres", "radius", "seg_time", "orders", "seg_offsets", "start_state", "end_state", "minimize_order", "max_iter", "check_every",
                  "max_vel", "max_acc", "margin", "eps", "rho"):
        assert re.search(r"\b" + field + r"\b", code), field


def test_record_is_64_bytes_in_c_python_and_the_model(tmp_path):
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "pct_trajgen.h"\nint main(void) { printf("%zu %zu %zu", sizeof(pct_trajgen_result), '
                   "sizeof(pct_trajgen_batch), sizeof(pct_trajgen_params)); "
                   + " ".join(f'printf(" %zu", offsetof(pct_trajgen_result, {f}));' for f in RESULT_FIELDS) + ' printf("\\n"); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [64, 64, 56, 0, 4, 8, 16, 24, 32, 40, 48, 56]
    from pointcloudtraj_amd import engine
    for dt in (engine.GEN_RESULT_DTYPE, M.GEN_RESULT_DTYPE):
        assert dt.itemsize == 64 and dt.names == RESULT_FIELDS and [dt.fields[n][1] for n in dt.names] == got[3:]
    assert C.sizeof(engine.TrajGenBatch) == 64 and C.sizeof(engine.TrajGenParams) == 56
    assert (engine.GEN_OK, engine.GEN_NOT_CONVERGED, engine.GEN_INVALID) == (0, 1, 2)


def test_header_compiles_as_c99_and_cxx17(tmp_path):
    for compiler, std, name in (("gcc", "-std=c99", "t.c"), ("g++", "-std=c++17", "t.cpp")):
        src = tmp_path / name
        src.write_text('#include "pct_trajgen.h"\nint main(void) { pct_trajgen_params p; p.rho = 0.0; return (int)p.rho + (int)PCT_GEN_OK; }\n')
        subprocess.run([compiler, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)], check=True)


def test_contract_paragraph_states_the_rules():
    text = re.sub(r"\s*\n \* ?", " ", header())
    m = re.search(r"Trajectory generation \(pct_bezier_generate_batch\*\): the contract\.(.*?)\*/", text, flags=re.S)
    assert m, "the contract paragraph is missing"
    para = m.group(1)
    for phrase in ("P = blockdiag_i(2 * T_i^(1-2k) * M_k(n_i))", "M_k(n) = f^2 * D_k^T * G * D_k", "G[a][b] = C(q,a) * C(q,b) / C(2q,a+b) / (2q+1)",
                   "9 start, 9 end and 9 per joint", "traj_optimizer.cpp:263-445", "g1 = (n'/T') * (T/n)", "|d1| <= max_vel * T_i/n_i",
                   "A limit <= 0 or +inf drops its rows", "Q = P / max|P|", "alpha = 1.6", "x = w - H^-1 E^T nu", "z = projection of v onto C",
                   "radius r - margin - 2 eps", "Every check_every iterations, and at max_iter", "r_prim = max |A x - z|",
                   "r_dual = rho * max |A^T (z - z_before)|", "r_prim <= eps and r_dual <= eps", "rho starts at 1e-5", "clamped to [1e-9, 1e3]",
                   "more than a factor 5", "u is scaled by rho/rho'", "from x itself, not from the split variable", "sphere_slack >= 0",
                   "(r - margin) - |P - c|", "sqrt(3) eps < 2 eps", "reported, not guaranteed", "polycoef[row][d*(n+1)+j] = P_j[d] / seg_time[row]",
                   "unused slots of a row written as 0", "is a pct_bezier_batch", "a non-finite input", "seg_time <= 0", "radius - margin - 2 eps <= 0",
                   "an order outside 5..12", "more than 16 segments", "for that candidate only", "written as NaN", "the other candidates are untouched",
                   "PCT_ERR_INVALID with nothing written", "PCT_GEN_NOT_CONVERGED with the last iterate and honest residuals", "it is never OK",
                   "B == 0: PCT_OK", "asynchronous on `stream`", "no host synchronisation inside", "can be captured", "the same bytes"):
        assert phrase in para, phrase
    # the model restates the same constants
    assert (M.ALPHA, M.RHO_AUTO, M.RHO_MIN, M.RHO_MAX, M.RHO_STEP) == (1.6, 1e-5, 1e-9, 1e3, 5.0)
    assert (M.MIN_ORDER, M.MAX_ORDER, M.MAX_SEG) == (5, 12, 16)


def test_library_exports_the_symbols():
    from pointcloudtraj_amd import build
    path = os.path.join(build.LIB, "libpct_engine.so")
    assert os.path.exists(path), f"{path} is missing: build first"
    exported = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    names = {line.split()[-1] for line in exported.splitlines() if line.strip()}
    assert set(SYMBOLS) <= names, sorted(set(SYMBOLS) - names)


def test_python_binding():
    from pointcloudtraj_amd import engine
    assert callable(engine.bezier_generate) and callable(engine.bezier_generate_device) and callable(engine.time_allocation)
    L = engine.lib()
    assert len(L.pct_bezier_generate_batch.argtypes) == 5 and len(L.pct_bezier_generate_batch_dev.argtypes) == 6 and len(L.pct_time_allocation.argtypes) == 9
    assert L.pct_bezier_generate_batch.argtypes[0] == C.POINTER(engine.TrajGenBatch) and L.pct_bezier_generate_batch.argtypes[1] == C.POINTER(engine.TrajGenParams)
    # the packing the model and the binding share, and the fan helper
    case = M.cases()["gen5"]
    fan = engine.corridor_fan(case["centres"], case["radius"], case["seg_time"], case["orders"], (0.5, 1.0, 2.0), case["start"], case["end"])
    batch, arr = engine.pack_corridors(fan)
    want = M.pack(fan)
    assert batch.B == 3 and sorted(arr) == sorted(want)
    for k in want:
        assert arr[k].dtype == want[k].dtype and np.array_equal(arr[k], want[k]), k
    assert np.array_equal(arr["seg_time"].reshape(3, -1), np.outer((0.5, 1.0, 2.0), case["seg_time"])) and list(arr["seg_offsets"]) == [0, 5, 10, 15]
    p = engine.gen_params(**M.params(max_vel=2.0, margin=0.1))
    assert (p.minimize_order, p.max_iter, p.check_every, p.max_vel, p.max_acc, p.margin, p.eps, p.rho) == (3, 4000, 25, 2.0, 0.0, 0.1, 1e-5, 0.0)
    # bad params are refused before anything touches a device
    bad = engine.gen_params(minimize_order=0)
    try:
        engine.bezier_generate(fan, bad)
    except engine.EngineError as e:
        assert e.code == 2
    else:
        raise AssertionError("minimize_order = 0 was accepted")


def test_cxx_mirror_and_example():
    hpp = open(os.path.join(ROOT, "include", "pct_obstacle_map.hpp")).read()
    assert '#include "pct_trajgen.h"' in hpp and "struct GeneratedTrajectories" in hpp
    assert re.search(r"inline int64_t generateTrajectories\(const double \*path, const double \*radius, const double \*times, const int32_t \*orders, int32_t m,", hpp)
    assert re.search(r"int64_t generateSafeTrajectory\(const double \*path, const double \*radius, const double \*times, const int32_t \*orders, int32_t m,", hpp)
    assert "pct_bezier_generate_batch(&b, &params" in hpp and "certifyTrajectories(out.batch(), certificates, max_depth)" in hpp
    assert os.path.exists(os.path.join(ROOT, "examples", "trajectory_generate.cpp"))
    build_py = open(os.path.join(ROOT, "pointcloudtraj_amd", "build.py")).read()
    assert '"trajectory_generate.cpp"' in build_py and '"trajgen.hip"' in build_py and '"trajgen.hpp"' in build_py and '"pct_trajgen.h"' in build_py
    from pointcloudtraj_amd import build
    assert os.path.exists(os.path.join(build.LIB, "trajectory_generate")), "the example is not built: build first"
