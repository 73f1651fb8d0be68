"""The polyhedral trajectory generator as the interface states it (no GPU needed): the prototypes, the batch struct in C and ctypes,
the header's contract paragraph and its constants against the model's, the exported symbols, that the headers are C99 and C++17,
the Python binding, the C++ mirror members and the example the build compiles, and that without a device the call fails loudly."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import trajgen_poly_model as PM  # noqa: E402

SYMBOLS = {
    "pct_bezier_generate_poly_batch": ["const pct_trajgen_poly_batch *batch", "const pct_trajgen_params *params", "double *polycoef", "int64_t row_stride",
                                       "pct_trajgen_result *result"],
    "pct_bezier_generate_poly_batch_dev": ["const pct_trajgen_poly_batch *d_fields", "const pct_trajgen_params *params", "double *d_polycoef",
                                           "int64_t row_stride", "pct_trajgen_result *d_res", "void *stream"],
    "pct_trajgen_max_planes": ["void"],
}
BATCH_FIELDS = ("anchors", "planes", "plane_offsets", "seg_time", "orders", "seg_offsets", "start_state", "end_state", "B")


def header():
    return open(os.path.join(ROOT, "include", "pct_trajgen.h")).read()


def test_header_declares_the_prototypes():
    code = re.sub(r"/\*.*?\*/", " ", header(), flags=re.S)
    for name, want in SYMBOLS.items():
        m = re.search(r"int\s+" + name + r"\s*\((.*?)\)\s*;", code, flags=re.S)
        assert m, f"{name} is not declared"
        assert [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")] == want, name
    m = re.search(r"typedef struct pct_trajgen_poly_batch \{(.*?)\} pct_trajgen_poly_batch;", code, flags=re.S)
    assert m and tuple(re.findall(r"\*?(\w+);", m.group(1))) == BATCH_FIELDS


def test_batch_struct_in_c_and_python(tmp_path):
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "pct_trajgen.h"\nint main(void) { printf("%zu", sizeof(pct_trajgen_poly_batch)); '
                   + " ".join(f'printf(" %zu", offsetof(pct_trajgen_poly_batch, {f}));' for f in BATCH_FIELDS) + ' printf("\\n"); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [72] + [8 * i for i in range(9)]
    from pointcloudtraj_amd import engine
    assert C.sizeof(engine.TrajGenPolyBatch) == 72
    assert tuple(n for n, _ in engine.TrajGenPolyBatch._fields_) == BATCH_FIELDS
    assert [getattr(engine.TrajGenPolyBatch, n).offset for n in BATCH_FIELDS] == got[1:]


def test_headers_compile_as_c99_and_cxx17(tmp_path):
    body = ('int main(void) { pct_trajgen_poly_batch b; b.B = 0; int (*f)(void) = pct_trajgen_max_planes; return (int)b.B + (f ? 0 : 1); }\n')
    for compiler, std, name, inc in (("gcc", "-std=c99", "t.c", "pct_trajgen.h"), ("g++", "-std=c++17", "t.cpp", "pct_trajgen.h"),
                                     ("g++", "-std=c++17", "m.cpp", "pct_obstacle_map.hpp")):
        src = tmp_path / name
        src.write_text(f'#include "{inc}"\n' + body)
        flags = ["-Wall", "-Wextra", "-Werror", "-pedantic"] if inc.endswith(".h") else ["-Wall", "-Werror"]
        subprocess.run([compiler, std, *flags, "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)], check=True)


def test_contract_paragraph_states_the_rules():
    text = re.sub(r"\s*\n \* ?", " ", header())
    m = re.search(r"Trajectory generation in polyhedra \(pct_bezier_generate_poly_batch\*\): the contract\.(.*?)\*/", text, flags=re.S)
    assert m, "the contract paragraph is missing"
    para = re.sub(r"\s+", " ", m.group(1))
    for phrase in ("pct_trajgen_max_planes() = 24", "C_g = { y : nh_k . y <= o_k }", "word for word", "there are no balls in this form",
                   "len = |n| = sqrt((n0 n0 + n1 n1) + n2 n2)", "nh = n / len, o = off / len - margin", "its projection is the identity",
                   "x = the segment's anchor", "g_k(y) = nh_k . y - (o_k - 2 eps)", "nh . y = (nh0 y0 + nh1 y1) + nh2 y2", "less than 2 eps",
                   "v itself, if g_k(v) <= 0 for every k", "one plane (i ascending), then two (i < j, i outer), then three (i < j < k)",
                   "det = 1 - a a", "l_i = (g_i - a g_j) / det", "det = ((1 + 2 ((a b) c)) - (a a + b b)) - c c", "det < 1e-8 is skipped",
                   "every multiplier is >= 0", "w <= 1e-9", "the counting candidate with the smallest w", "better by more than 1e-9",
                   "ulp <= 1.2e-13", "The previous iteration's active set is not tried first", "the corridor slack", "o_k - nh_k . P",
                   "no 2 eps", "slack >= 0", "whatever the projection did", "the whole curve is in the polytope", "a non-finite anchor",
                   "|n| as computed above is 0 or not finite", "more than 24 planes on one segment", "plane_offsets descending inside the candidate",
                   "an empty polytope", "a start point outside its polytope", "without a common point", "never OK", "plane_offsets[0] != 0",
                   "PCT_ERR_INVALID with nothing written"):
        assert phrase in para, phrase
    assert (PM.MAX_PLANES, PM.ACCEPT, PM.DET_MIN) == (24, 1e-9, 1e-8)
    hpp = open(os.path.join(ROOT, "pointcloudtraj_amd", "csrc", "trajgen_poly.hpp")).read()
    assert "kMaxPlanes = 24" in hpp and "kPolyAccept = 1e-9" in hpp and "kPolyDet = 1e-8" in hpp


def test_library_exports_the_symbols_and_the_plane_limit():
    from pointcloudtraj_amd import build, engine
    path = os.path.join(build.LIB, "libpct_engine.so")
    assert os.path.exists(path), f"{path} is missing: build first"
    exported = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    names = {line.split()[-1] for line in exported.splitlines() if line.strip()}
    assert set(SYMBOLS) <= names, sorted(set(SYMBOLS) - names)
    assert engine.lib().pct_trajgen_max_planes() == 24 == engine.trajgen_max_planes()


def test_python_binding_and_the_loud_failure_without_a_device():
    from pointcloudtraj_amd import engine
    assert callable(engine.bezier_generate_poly) and callable(engine.bezier_generate_poly_device) and callable(engine.pack_poly_corridors)
    L = engine.lib()
    assert len(L.pct_bezier_generate_poly_batch.argtypes) == 5 and len(L.pct_bezier_generate_poly_batch_dev.argtypes) == 6
    assert L.pct_bezier_generate_poly_batch.argtypes[0] == C.POINTER(engine.TrajGenPolyBatch)
    case = PM.cases()["bend"]
    fan = engine.corridor_fan(case, (0.5, 1.0, 2.0))
    assert [sorted(c) for c in fan] == [sorted(case)] * 3 and fan[0]["planes"] is case["planes"]
    batch, arr = engine.pack_poly_corridors(fan)
    want = PM.pack(fan)
    assert batch.B == 3 and sorted(arr) == sorted(want)
    for k in want:
        assert arr[k].dtype == want[k].dtype and np.array_equal(arr[k], want[k]), k
    assert np.array_equal(arr["seg_time"].reshape(3, -1), np.outer((0.5, 1.0, 2.0), case["seg_time"]))
    assert list(arr["seg_offsets"]) == [0, 2, 4, 6] and list(arr["plane_offsets"]) == [0, 6, 12, 18, 24, 30, 36]
    # the sphere fan is what it was
    sph = engine.corridor_fan(np.zeros((2, 3)), np.ones(2), np.array([1.0, 2.0]), np.array([7, 7]), (0.5, 2.0), np.zeros(9), np.zeros(9))
    assert len(sph) == 2 and np.array_equal(sph[1]["seg_time"], [2.0, 4.0]) and "radius" in sph[0]
    # a corridor without a single plane still hands the library a pointer
    _, none = engine.pack_poly_corridors([dict(case, planes=[np.zeros((0, 4)), np.zeros((0, 4))])])
    assert none["planes"].shape == (1, 4) and list(none["plane_offsets"]) == [0, 0, 0]
    # bad params are refused before anything touches a device
    with pytest.raises(engine.EngineError) as e:
        engine.bezier_generate_poly(fan, engine.gen_params(minimize_order=0))
    assert e.value.code == 2
    # and so are bad offsets
    b2, a2 = engine.pack_poly_corridors(fan)
    a2["plane_offsets"][0] = 1
    with pytest.raises(engine.EngineError) as e:
        engine.bezier_generate_poly((b2, a2), engine.gen_params())
    assert e.value.code == 2
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    if not has_gpu:
        # no device: an error that says so, never a host fallback
        with pytest.raises(engine.EngineError) as e:
            engine.bezier_generate_poly(fan, engine.gen_params())
        assert e.value.code != 0 and "device" in str(e.value).lower()


def test_cxx_mirror_and_example():
    hpp = open(os.path.join(ROOT, "include", "pct_obstacle_map.hpp")).read()
    assert re.search(r"inline int64_t generateTrajectoriesInPolyhedra\(const double \*waypoints, const double \*planes, const int64_t \*plane_offsets,", hpp)
    assert re.search(r"int64_t generateSafeTrajectoryInPolyhedra\(const double \*waypoints, int32_t m, double reach,", hpp)
    assert "pct_bezier_generate_poly_batch(&b, &params" in hpp and "prm.margin = 0.0;" in hpp
    assert os.path.exists(os.path.join(ROOT, "examples", "trajectory_polyhedra.cpp"))
    build_py = open(os.path.join(ROOT, "pointcloudtraj_amd", "build.py")).read()
    assert '"trajectory_polyhedra.cpp"' in build_py and '"trajgen_poly.hpp"' in build_py
    from pointcloudtraj_amd import build
    assert os.path.exists(os.path.join(build.LIB, "trajectory_polyhedra")), "the example is not built: build first"
