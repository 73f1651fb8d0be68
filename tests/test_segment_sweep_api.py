"""Segment sweeps as the interface states them (no GPU needed): the two prototypes, the contract paragraph of the header, the exported
symbols, the Python methods with their argtypes, and the C++ mirror's members."""
import ctypes as C
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOTYPES = {
    "pct_segment_sweep_batch": ["pct_cloud *c", "int algo", "const double *seg", "const double *radius", "int64_t Q", "uint32_t *idx", "double *t"],
    "pct_segment_sweep_batch_dev": ["pct_cloud *c", "int algo", "const double *d_seg", "const double *d_radius", "int64_t Q", "uint32_t *d_idx", "double *d_t",
                                    "void *stream"],
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
    m = re.search(r"\n \* Segment sweeps \(.*?\n \*\n", head, flags=re.S)
    assert m, "the paragraph \"Segment sweeps\" is missing from the header comment"
    assert head.index("\n * Segment queries (") < m.start(), "\"Segment sweeps\" comes after \"Segment queries\""
    para = re.sub(r"\s*\n \*\s*", " ", m.group(0))
    for phrase in ("lowest index", "inclusive", "PCT_NO_INDEX", "NaN", "PCT_ERR_EMPTY", "PCT_ERR_INVALID", "PCT_ALGO_GRID", "PCT_ALGO_STREAM_EXACT"):
        assert phrase in para, phrase
    # the arithmetic, in its order
    order = ["r2 = min(r*r, DBL_MAX)", "d2 <= r2", "ww = (w0*w0 + w1*w1) + w2*w2", "if (ww <= r2) t = 0", "g = ww - r2", "disc = dot*dot - L2*g",
             "if (!(disc > 0)) disc = 0", "t = (dot - sqrt(disc)) / L2", "if (!(t > 0)) t = 0", "t > s"]
    at = [para.find(p) for p in order]
    assert all(a >= 0 for a in at), [p for p, a in zip(order, at) if a < 0]
    assert at == sorted(at)
    assert "t = 1" in para and "t = NaN" in para and "never \"free\"" in para and "t may be NULL" in para
    assert "bit for bit" in para


def test_library_exports_the_symbols():
    from pointcloudtraj_amd import build
    path = os.path.join(build.LIB, "libpct_engine.so")
    assert os.path.exists(path), f"{path} is missing: build first"
    exported = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    names = {line.split()[-1] for line in exported.splitlines() if line.strip()}
    assert set(PROTOTYPES) <= names, sorted(set(PROTOTYPES) - names)


def test_python_signatures_and_argtypes():
    from pointcloudtraj_amd import engine
    sig = inspect.signature(engine.Cloud.segment_sweep)
    assert list(sig.parameters) == ["self", "segments", "radius", "algo"] and sig.parameters["algo"].default == engine.ALGO_AUTO
    sig = inspect.signature(engine.Cloud.segment_sweep_device)
    assert list(sig.parameters) == ["self", "seg_ptr", "radius_ptr", "Q", "idx_ptr", "t_ptr", "stream", "algo"]
    assert sig.parameters["algo"].default == engine.ALGO_AUTO and sig.parameters["stream"].default == 0
    L = engine.lib()
    vp, i32, i64 = C.c_void_p, C.c_int, C.c_int64
    f64p = u32p = vp                                     # the binding passes every array as a void pointer (engine._ptr)
    assert L.pct_segment_sweep_batch.argtypes == [vp, i32, f64p, f64p, i64, u32p, f64p]
    assert L.pct_segment_sweep_batch_dev.argtypes == [vp, i32, vp, vp, i64, vp, vp, vp]


def test_cxx_mirror_has_the_members_and_compiles(tmp_path):
    path = os.path.join(ROOT, "include", "pct_obstacle_map.hpp")
    omap = open(path).read()
    for pat in (r"void\s+sweepSegments\s*\(\s*const double \*segments\s*,\s*int64_t n\s*,\s*double radius\s*,\s*uint32_t \*index\s*,\s*double \*t\s*\)",
                r"double\s+freeFraction\s*\(\s*const double a\[3\]\s*,\s*const double b\[3\]\s*\)",
                r"pct_segment_sweep_batch\(cloud_", r"prm_\.search_margin", r"(?i)inclusive", r"checkTrajPtCol collides on a strict `<`"):
        assert re.search(pat, omap), pat
    # a translation unit that uses the two members, C++17, no GPU header on the include path
    src = tmp_path / "use_sweeps.cpp"
    src.write_text('#include "pct_obstacle_map.hpp"\n'
                   "double how_far(pct::ObstacleMap &m, const double *segs, int64_t n, uint32_t *idx, double *t)\n"
                   "{\n    m.sweepSegments(segs, n, 0.5, idx, t);\n    m.sweepSegments(segs, n, 0.5, idx, nullptr);\n"
                   "    return m.freeFraction(segs, segs + 3);\n}\n")
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src)], check=True)
