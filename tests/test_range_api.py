"""Range images on the rolling map as the interface states them (no GPU needed): the declared and exported symbols, the struct, the
Python names and the C++ mirror members, the header's contract paragraph, and pct_range_pseudo_angle -- a host function -- called
through ctypes against the numpy model (tests/helpers/range_model.py)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import range_model as G  # noqa: E402

ENGINE_SYMBOLS = {
    "pct_cloud_ring_carve_range": ("int", ["pct_cloud *c", "const pct_range_view *v", "const float *image", "double margin", "int64_t *removed"]),
    "pct_cloud_append_range": ("int", ["pct_cloud *c", "const pct_range_view *v", "const float *image", "double max_range", "int64_t *offered", "int64_t *kept"]),
    "pct_range_classify": ("int", ["const pct_range_view *views", "const float *const *images", "int32_t n_views", "const double *pts", "int64_t n",
                                   "double margin", "int32_t *seen_by", "int32_t *pixel"]),
    "pct_range_pseudo_angle": ("double", ["double x", "double y"]),
}
CORRIDOR_SYMBOLS = {
    "pct_corridor_clear_seen_through_range": ("int", ["pct_corridor *c", "const pct_range_view *view", "const float *image", "double margin", "int64_t *removed"]),
    "pct_corridor_append_range": ("int", ["pct_corridor *c", "const pct_range_view *view", "const float *image", "double max_range", "int64_t *kept"]),
}
FIELDS = ["double t[3]", "double R[9]", "double near_range", "int32_t width, height", "int32_t reserved[2]", "const double *col_edge",
          "const double *row_edge", "const double *col_dir", "const double *row_dir"]


def code_of(header):
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)


@pytest.mark.parametrize("header,symbols", [("pct_engine.h", ENGINE_SYMBOLS), ("pct_corridor.h", CORRIDOR_SYMBOLS)])
def test_headers_declare_the_symbols(header, symbols):
    code = code_of(header)
    for name, (ret, want) in symbols.items():
        m = re.search(ret + r"\s+" + name + r"\s*\((.*?)\)\s*;", code, flags=re.S)
        assert m, f"{name} is not declared in {header}"
        assert [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")] == want, name


def test_header_declares_the_view_and_python_mirrors_it():
    code = re.sub(r"\s+", " ", code_of("pct_engine.h"))
    m = re.search(r"typedef struct pct_range_view \{(.*?)\} pct_range_view;", code)
    assert m, "struct pct_range_view is not declared"
    assert [f.strip() for f in m.group(1).split(";") if f.strip()] == FIELDS
    assert '#include "pct_engine.h"' in open(os.path.join(ROOT, "include", "pct_corridor.h")).read()
    from pointcloudtraj_amd import engine
    V = engine.RangeView
    assert ctypes.sizeof(V) == 24 + 72 + 8 + 8 + 8 + 4 * ctypes.sizeof(ctypes.c_void_p) == 152
    assert [f[0] for f in V._fields_] == ["t", "R", "near_range", "width", "height", "reserved", "col_edge", "row_edge", "col_dir", "row_dir"]
    assert (V.near_range.offset, V.width.offset, V.reserved.offset, V.col_edge.offset, V.row_dir.offset) == (96, 104, 112, 120, 144)


@pytest.mark.parametrize("lib,symbols", [("libpct_engine.so", ENGINE_SYMBOLS), ("libpct_corridor.so", CORRIDOR_SYMBOLS)])
def test_libraries_export_the_symbols(lib, symbols):
    from pointcloudtraj_amd import build
    path = os.path.join(build.LIB, lib)
    assert os.path.exists(path), f"{path} is missing: build first"
    exported = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    names = {line.split()[-1] for line in exported.splitlines() if line.strip()}
    assert set(symbols) <= names, sorted(set(symbols) - names)


def test_python_names_exist():
    from pointcloudtraj_amd import corridor, engine, scenarios
    for name in ("ring_carve_range", "append_range"):
        assert callable(getattr(engine.Cloud, name)), name
    for name in ("range_view", "range_view_uniform", "range_classify", "pseudo_angle"):
        assert callable(getattr(engine, name)), name
    for name in ("clearSeenThroughRange", "appendRangeImage"):
        assert callable(getattr(corridor.SafeRegionRrtStar, name)), name
    assert callable(scenarios.run_lidar_range_window_scenario) and callable(scenarios.lidar_range_view)
    ce, re_ = np.float64([0.0, 1.0, 2.0]), np.float64([-1.0, 1.0])
    v = engine.range_view((1, 2, 3), np.eye(3), ce, re_)
    assert (v.width, v.height, v.near_range, tuple(v.reserved)) == (2, 1, 0.05, (0, 0)) and not v.col_dir and not v.row_dir
    del ce, re_                                                                    # the view keeps its tables alive
    assert [v.col_edge[k] for k in range(3)] == [0.0, 1.0, 2.0] and [v.row_edge[k] for k in range(2)] == [-1.0, 1.0]
    with pytest.raises(ValueError):
        engine.range_view((0, 0, 0), np.eye(3), [0.0, 1.0], [-1.0, 1.0], col_dir=[[1, 0], [0, 1]])


def test_cxx_mirrors_have_the_members():
    pats = (r"int64_t\s+clearSeenThroughRange\s*\(\s*const pct_range_view &view\s*,\s*const float \*image\s*,\s*double margin\s*\)",
            r"int64_t\s+appendRangeImage\s*\(\s*const pct_range_view &view\s*,\s*const float \*image\s*,\s*double max_range\s*\)")
    omap = open(os.path.join(ROOT, "include", "pct_obstacle_map.hpp")).read()
    finder = open(os.path.join(ROOT, "include", "pct_corridor_finder.hpp")).read()
    for pat in pats:
        assert re.search(pat, omap), pat
        assert re.search(pat, finder), pat
    assert "pct_cloud_ring_carve_range(cloud_" in omap and "pct_cloud_append_range(cloud_" in omap
    assert "clearSeenThroughRange -> appendRangeImage -> SafeRegionEvaluate -> SafeRegionRefine" in finder


def test_contract_paragraph_pins_the_projection():
    text = open(os.path.join(ROOT, "include", "pct_engine.h")).read()
    m = re.search(r"Range images \(pct_cloud_ring_carve_range.*?\n \*\n", text, flags=re.S)
    assert m, "the contract paragraph is missing from the header comment"
    para = re.sub(r"\s*\n \*\s*", " ", m.group(0))
    for phrase in ("den = |x| + |y|", "p = y / den", "pa = 2.0 - p", "pa = 4.0 + p", "r2 = (d0*d0 + d1*d1) + d2*d2",
                   "s_k = (d0*R[0][k] + d1*R[1][k]) + d2*R[2][k]", "h = sqrt(s0*s0 + s1*s1)", "q = s2 / h", "r2 >= near_range*near_range",
                   "col_edge[0] <= a < col_edge[width]", "row_edge[0] <= q < row_edge[height]", "a NaN fails every one of them",
                   "belongs to the cell above it", "defined by these counts, not by the search", "w > 0 && r2 < w*w", "strict",
                   "+inf pixel proves nothing", "e0 = row_dir[r][0]*col_dir[c][0]", "e1 = row_dir[r][0]*col_dir[c][1]", "e2 = row_dir[r][1]",
                   "p_k = t[k] + rho*((e0*R[k][0] + e1*R[k][1]) + e2*R[k][2])", "row-major order", "no sin, cos or atan2",
                   "col_edge[0] = 0 and col_edge[width] = 4", "azimuth 0 (the +x axis) is not inside its span", "staggered beams",
                   "NaN-row equivalence", "empty-window rule", "carve first, then append", "|range - val| <=", "pixel[2i] = c, pixel[2i + 1] = r"):
        assert phrase in para, phrase
    # the depth paragraph stands as it stood
    assert re.search(r"Depth images \(pct_cloud_ring_carve_depth.*?\n \*\n", text, flags=re.S)


# ---- pct_range_pseudo_angle: a host function, called without a device ---------------------------------------------------------------

@pytest.fixture(scope="module")
def pa():
    from pointcloudtraj_amd import engine
    f = engine.lib().pct_range_pseudo_angle
    return lambda x, y: f(float(x), float(y))


def same_bits(a, b):
    return np.array_equal(np.float64(a).view(np.uint64), np.float64(b).view(np.uint64)) or (np.isnan(a) and np.isnan(b))


def test_pseudo_angle_on_the_axes_and_diagonals(pa):
    want = {(1, 0): 0.0, (1, 1): 0.5, (0, 1): 1.0, (-1, 1): 1.5, (-1, 0): 2.0, (-1, -1): 2.5, (0, -1): 3.0, (1, -1): 3.5}
    for (x, y), a in want.items():
        for scale in (1.0, 3.0, 2.0 ** -40, 2.0 ** 600):
            assert pa(x * scale, y * scale) == a == float(G.pseudo_angle(x * scale, y * scale)), (x, y, scale)


def test_pseudo_angle_signed_zeros_and_what_has_no_angle(pa):
    for x in (0.5, 7.0):
        assert pa(-0.0, x) == 1.0 and pa(-0.0, -x) == 3.0 and pa(0.0, x) == 1.0, "x = -0.0 is not 'x < 0'"
        assert pa(x, -0.0) == 0.0 and pa(-x, -0.0) == 2.0 and pa(-x, 0.0) == 2.0
    for x, y in ((0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0)):
        assert np.isnan(pa(x, y)) and np.isnan(G.pseudo_angle(x, y))
    for x, y in ((np.inf, 1.0), (1.0, np.inf), (-np.inf, 0.0), (0.0, -np.inf), (np.inf, np.inf), (np.nan, 1.0), (1.0, np.nan), (1e308, 1e308)):
        assert np.isnan(pa(x, y)) and np.isnan(G.pseudo_angle(x, y)), (x, y)


def test_pseudo_angle_equals_the_model_bit_for_bit(pa):
    rng = np.random.default_rng(7)
    xy = rng.standard_normal((10000, 2)) * 10.0 ** rng.uniform(-6, 6, (10000, 1))
    xy[::50, 0] = 0.0
    xy[25::50, 1] = 0.0
    got = np.float64([pa(x, y) for x, y in xy])
    want = G.pseudo_angle(xy[:, 0], xy[:, 1])
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert np.all((got >= 0.0) & (got <= 4.0))


def test_pseudo_angle_is_monotone_around_the_circle(pa):
    th = np.arange(4096) * (2.0 * np.pi / 4096)
    a = np.float64([pa(np.cos(t), np.sin(t)) for t in th])
    assert a[0] == 0.0 and np.all(np.diff(a) > 0.0) and a[-1] < 4.0
    assert np.array_equal(a.view(np.uint64), G.pseudo_angle(np.cos(th), np.sin(th)).view(np.uint64))
    from pointcloudtraj_amd import engine
    assert engine.pseudo_angle(-1.0, 1.0) == 1.5
