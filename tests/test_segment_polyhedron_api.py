"""The free-space polyhedra as the interface states them (no GPU needed): the four prototypes, the contract paragraph of the header,
the exported symbols, the LDS constant, the Python methods and the C++ mirror's member."""
import ctypes as C
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOTYPES = {
    "pct_segment_polyhedron_batch": ["pct_cloud *c", "int algo", "const double *seg", "const double *reach", "int64_t Q", "int64_t *offsets",
                                     "int64_t *total"],
    "pct_segment_polyhedron_read": ["pct_cloud *c", "int64_t first", "int64_t n", "uint32_t *idx", "double *d2", "double *s", "double *plane"],
    "pct_segment_supports_dev": ["pct_cloud *c", "const double *d_seg", "int64_t Q", "const int64_t *d_row_offsets", "int64_t row_cap",
                                 "const uint32_t *d_row_idx", "int64_t *d_offsets", "int64_t cap", "uint32_t *d_idx", "double *d_d2", "double *d_s",
                                 "double *d_plane", "void *stream"],
    "pct_polyhedron_lds_rows": ["void"],
}


def test_header_declares_the_prototypes():
    code = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "pct_engine.h")).read(), flags=re.S)
    for name, want in PROTOTYPES.items():
        m = re.search(r"int\s+" + name + r"\s*\((.*?)\)\s*;", code, flags=re.S)
        assert m, f"{name} is not declared in pct_engine.h"
        assert [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")] == want, name


def test_contract_paragraph():
    text = open(os.path.join(ROOT, "include", "pct_engine.h")).read()
    head = text[:text.index("#ifndef PCT_ENGINE_H")]
    m = re.search(r"\n \* Free-space polyhedra \(.*?\n \*\n", head, flags=re.S)
    assert m, "the paragraph \"Free-space polyhedra\" is missing from the header comment"
    assert head.index("\n * Capsule search (") < m.start(), "\"Free-space polyhedra\" comes after \"Capsule search\""
    para = re.sub(r"\s*\n \*\s*", " ", m.group(0))
    for phrase in ("SUPPORT", "support", "\"Capsule search\"", "\"Segment queries\"", "PCT_ORDER_DISTANCE", "h >= 0", "inclusive", "(0, 0, 0, -1)",
                   "h = (n0*u0 + n1*u1) + n2*u2", "n_k = w_k - s*e_k", "off = (nh0*p0 + nh1*p1) + nh2*p2", "d2 == 0", "PCT_ERR_EMPTY", "PCT_ERR_INVALID",
                   "every entry of d_offsets is then -1", "d_offsets[Q] <= cap", "never dereferenced", "does not re-sort", "graph capture",
                   "pct_segment_search_read still reads", "pct_polyhedron_lds_rows", "off - m"):
        assert phrase in para, phrase
    # the pinned paragraphs are where they were
    for name in ("Segment queries", "Segment sweeps", "Capsule search"):
        assert len(re.findall(r"\n \* " + name + r" \(", head)) == 1


def test_library_exports_the_symbols_and_answers_the_lds_constant():
    from pointcloudtraj_amd import build
    path = os.path.join(build.LIB, "libpct_engine.so")
    assert os.path.exists(path), f"{path} is missing: build first"
    exported = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    names = {line.split()[-1] for line in exported.splitlines() if line.strip()}
    assert set(PROTOTYPES) <= names, sorted(set(PROTOTYPES) - names)
    from pointcloudtraj_amd import engine
    L = engine.polyhedron_lds_rows()                         # no GPU is touched
    assert L >= 256 and L % 256 == 0
    src = open(os.path.join(ROOT, "pointcloudtraj_amd", "csrc", "segment_polyhedron.hpp")).read()
    assert re.search(r"constexpr int kPolyLds = %d;" % L, src)
    assert 12 * L + L // 8 <= 65536, "the row and its mask stay within 64 KiB of LDS"


def test_python_signatures_and_argtypes():
    from pointcloudtraj_amd import engine
    sig = inspect.signature(engine.Cloud.segment_polyhedron)
    assert list(sig.parameters) == ["self", "segments", "reach", "algo"] and sig.parameters["algo"].default == engine.ALGO_AUTO
    sig = inspect.signature(engine.Cloud.segment_polyhedron_read)
    assert list(sig.parameters)[:3] == ["self", "first", "n"]
    sig = inspect.signature(engine.Cloud.segment_supports_device)
    assert list(sig.parameters) == ["self", "seg_ptr", "Q", "row_offsets_ptr", "row_cap", "row_idx_ptr", "offsets_ptr", "cap", "idx_ptr", "d2_ptr", "s_ptr",
                                    "plane_ptr", "stream"]
    assert sig.parameters["stream"].default == 0
    L = engine.lib()
    vp, i32, i64 = C.c_void_p, C.c_int, C.c_int64
    assert L.pct_segment_polyhedron_batch.argtypes == [vp, i32, vp, vp, i64, vp, C.POINTER(i64)]
    assert L.pct_segment_polyhedron_read.argtypes == [vp, i64, i64, vp, vp, vp, vp]
    assert L.pct_segment_supports_dev.argtypes == [vp, vp, i64, vp, i64, vp, vp, i64, vp, vp, vp, vp, vp]


def test_kernels_live_in_their_own_header():
    src = open(os.path.join(ROOT, "pointcloudtraj_amd", "csrc", "segment_polyhedron.hpp")).read()
    assert "#pragma clang fp contract(off)" in src and '#include "segment_search.hpp"' in src
    for kernel in ("poly_filter_kernel", "poly_emit_kernel"):
        assert re.search(r"__global__[^;{]*\b" + kernel + r"\b", src), kernel
    assert "atomic" not in src.replace("no atomics", ""), "the filter needs no atomics"
    eng = open(os.path.join(ROOT, "pointcloudtraj_amd", "csrc", "engine.hip")).read()
    assert eng.index('#include "segment_search.hpp"') < eng.index('#include "segment_polyhedron.hpp"')


def test_cxx_mirror_has_the_member_and_compiles(tmp_path):
    omap = open(os.path.join(ROOT, "include", "pct_obstacle_map.hpp")).read()
    for pat in (r"void\s+segmentPolyhedra\s*\(", r"pct_segment_polyhedron_batch\(cloud_", r"pct_segment_polyhedron_read\(cloud_"):
        assert re.search(pat, omap), pat
    src = tmp_path / "use_polyhedra.cpp"
    src.write_text('#include "pct_obstacle_map.hpp"\n'
                   "int64_t around(pct::ObstacleMap &m, const std::vector<double> &segs, std::vector<int64_t> &off, std::vector<double> &planes,\n"
                   "               std::vector<uint32_t> &idx)\n"
                   "{\n    m.segmentPolyhedra(segs, 1.5, 0.2, off, planes);\n    m.segmentPolyhedra(segs, 1.5, 0.2, off, planes, &idx);\n"
                   "    return off.back();\n}\n")
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src)], check=True)
