"""The capsule search as the interface states it (no GPU needed): the five prototypes, the contract paragraph of the header, the
exported symbols, the Python methods with their defaults and argtypes, and the C++ mirror's members."""
import ctypes as C
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOTYPES = {
    "pct_segment_count_batch": ["pct_cloud *c", "int algo", "const double *seg", "const double *reach", "int64_t Q", "uint32_t *count"],
    "pct_segment_count_batch_dev": ["pct_cloud *c", "int algo", "const double *d_seg", "const double *d_reach", "int64_t Q", "uint32_t *d_count", "void *stream"],
    "pct_segment_search_batch": ["pct_cloud *c", "int algo", "const double *seg", "const double *reach", "int64_t Q", "int order", "int64_t *offsets",
                                 "int64_t *total"],
    "pct_segment_search_read": ["pct_cloud *c", "int64_t first", "int64_t n", "uint32_t *idx", "double *d2", "double *s"],
    "pct_segment_search_batch_dev": ["pct_cloud *c", "int algo", "const double *d_seg", "const double *d_reach", "int64_t Q", "int order", "int64_t *d_offsets",
                                     "int64_t cap", "uint32_t *d_idx", "double *d_d2", "double *d_s", "void *stream"],
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
    m = re.search(r"\n \* Capsule search \(.*?\n \*\n", head, flags=re.S)
    assert m, "the paragraph \"Capsule search\" is missing from the header comment"
    assert head.index("\n * Segment queries (") < head.index("\n * Segment sweeps (") < m.start(), "\"Capsule search\" comes after the two segment paragraphs"
    para = re.sub(r"\s*\n \*\s*", " ", m.group(0))
    for phrase in ("\"Segment queries\"", "d2 <= min(reach*reach, DBL_MAX)", "inclusive", "empty row", "a == b", "pct_radius_search_batch", "bit for bit",
                   "offsets[i + 1] - offsets[i]", "PCT_ORDER_INDEX", "PCT_ORDER_DISTANCE", "never NaN", "removed rows", "PCT_ALGO_STREAM", "PCT_ALGO_GRID",
                   "PCT_ALGO_RING", "PCT_ALGO_AUTO", "PCT_ALGO_STREAM_EXACT", "without a grid", "PCT_ERR_EMPTY", "PCT_ERR_INVALID", "PCT_ERR_CAPACITY",
                   "d_offsets[Q] <= cap", "pct_cloud_reserve_queries", "pct_segment_search_read", "pct_last_work"):
        assert phrase in para, phrase
    # the pinned paragraphs are where they were
    for name in ("Segment queries", "Segment sweeps"):
        assert len(re.findall(r"\n \* " + name + r" \(", head)) == 1


def test_library_exports_the_symbols():
    from pointcloudtraj_amd import build
    path = os.path.join(build.LIB, "libpct_engine.so")
    assert os.path.exists(path), f"{path} is missing: build first"
    exported = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    names = {line.split()[-1] for line in exported.splitlines() if line.strip()}
    assert set(PROTOTYPES) <= names, sorted(set(PROTOTYPES) - names)


def test_python_signatures_and_argtypes():
    from pointcloudtraj_amd import engine
    sig = inspect.signature(engine.Cloud.segment_count)
    assert list(sig.parameters) == ["self", "segments", "reach", "algo"] and sig.parameters["algo"].default == engine.ALGO_AUTO
    sig = inspect.signature(engine.Cloud.segment_search)
    assert list(sig.parameters) == ["self", "segments", "reach", "order", "algo"]
    assert sig.parameters["order"].default == engine.ORDER_DISTANCE and sig.parameters["algo"].default == engine.ALGO_AUTO
    sig = inspect.signature(engine.Cloud.segment_count_device)
    assert list(sig.parameters) == ["self", "seg_ptr", "reach_ptr", "Q", "cnt_ptr", "stream", "algo"]
    assert sig.parameters["algo"].default == engine.ALGO_AUTO and sig.parameters["stream"].default == 0
    sig = inspect.signature(engine.Cloud.segment_search_device)
    assert list(sig.parameters) == ["self", "seg_ptr", "reach_ptr", "Q", "order", "offsets_ptr", "cap", "idx_ptr", "d2_ptr", "s_ptr", "stream", "algo"]
    assert sig.parameters["algo"].default == engine.ALGO_AUTO and sig.parameters["stream"].default == 0
    L = engine.lib()
    vp, i32, i64 = C.c_void_p, C.c_int, C.c_int64
    f64p = u32p = vp                                     # the binding passes every array as a void pointer (engine._ptr)
    assert L.pct_segment_count_batch.argtypes == [vp, i32, f64p, f64p, i64, u32p]
    assert L.pct_segment_count_batch_dev.argtypes == [vp, i32, vp, vp, i64, vp, vp]
    assert L.pct_segment_search_batch.argtypes == [vp, i32, f64p, f64p, i64, i32, vp, C.POINTER(i64)]
    assert L.pct_segment_search_read.argtypes == [vp, i64, i64, u32p, f64p, f64p]
    assert L.pct_segment_search_batch_dev.argtypes == [vp, i32, vp, vp, i64, i32, vp, i64, vp, vp, vp, vp]


def test_kernels_live_in_their_own_header():
    src = open(os.path.join(ROOT, "pointcloudtraj_amd", "csrc", "segment_search.hpp")).read()
    assert "#pragma clang fp contract(off)" in src and '#include "segment.hpp"' in src
    for kernel in ("ss_stream_count_kernel", "ss_stream_fill_kernel", "ss_ring_count_kernel", "ss_ring_fill_kernel", "ss_grid_count_kernel",
                   "ss_grid_fill_kernel", "ss_param_kernel"):
        assert re.search(r"__global__[^;{]*\b" + kernel + r"\b", src), kernel
    eng = open(os.path.join(ROOT, "pointcloudtraj_amd", "csrc", "engine.hip")).read()
    assert eng.index('#include "segment.hpp"') < eng.index('#include "segment_search.hpp"')


def test_cxx_mirror_has_the_members_and_compiles(tmp_path):
    path = os.path.join(ROOT, "include", "pct_obstacle_map.hpp")
    omap = open(path).read()
    for pat in (r"void\s+segmentNeighbours\s*\(", r"void\s+segmentCounts\s*\(", r"pct_segment_search_batch\(cloud_", r"pct_segment_search_read\(cloud_",
                r"pct_segment_count_batch\(cloud_"):
        assert re.search(pat, omap), pat
    src = tmp_path / "use_neighbours.cpp"
    src.write_text('#include "pct_obstacle_map.hpp"\n'
                   "int64_t around(pct::ObstacleMap &m, const std::vector<double> &segs, std::vector<int64_t> &off, std::vector<uint32_t> &idx,\n"
                   "               std::vector<double> &d2, std::vector<double> &s, std::vector<uint32_t> &cnt)\n"
                   "{\n    m.segmentNeighbours(segs, 0.5, off, idx, d2);\n    m.segmentNeighbours(segs, 0.5, off, idx, d2, &s);\n"
                   "    m.segmentCounts(segs, 0.5, cnt);\n    return off.back();\n}\n")
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src)], check=True)
