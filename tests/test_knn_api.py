"""CPU tests of the k-nearest-neighbour interface: the header declares it, the built library exports it, the Python binding and the
C++ mirror carry it.  No compute call is made (the kernels are tested in tests/test_gpu_knn.py on the GPU)."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
KNN_FUNCTIONS = ["pct_knn_batch", "pct_knn_batch_algo", "pct_knn_batch_dev"]


def header_code():
    text = open(os.path.join(INCLUDE, "pct_engine.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


@pytest.fixture(scope="module")
def built():
    from pointcloudtraj_amd import build
    build.build_all()
    return build


def test_header_declares_the_three_entry_points_and_the_limit():
    code = header_code()
    assert re.search(r"#define\s+PCT_KNN_MAX_K\s+64\b", code)
    want = {
        "pct_knn_batch": r"int\s+pct_knn_batch\s*\(\s*pct_cloud\s*\*\s*c\s*,\s*const\s+float\s*\*\s*q\s*,\s*int64_t\s+Q\s*,\s*int32_t\s+k\s*,"
                         r"\s*uint32_t\s*\*\s*idx\s*,\s*double\s*\*\s*d2\s*\)\s*;",
        "pct_knn_batch_algo": r"int\s+pct_knn_batch_algo\s*\(\s*pct_cloud\s*\*\s*c\s*,\s*int\s+algo\s*,\s*const\s+float\s*\*\s*q\s*,\s*int64_t\s+Q\s*,"
                              r"\s*int32_t\s+k\s*,\s*uint32_t\s*\*\s*idx\s*,\s*double\s*\*\s*d2\s*\)\s*;",
        "pct_knn_batch_dev": r"int\s+pct_knn_batch_dev\s*\(\s*pct_cloud\s*\*\s*c\s*,\s*int\s+algo\s*,\s*const\s+float\s*\*\s*d_q\s*,\s*int64_t\s+Q\s*,"
                             r"\s*int32_t\s+k\s*,\s*uint32_t\s*\*\s*d_idx\s*,\s*double\s*\*\s*d_d2\s*,\s*void\s*\*\s*stream\s*\)\s*;",
    }
    for name, pattern in want.items():
        assert re.search(pattern, code), f"{name} is not declared as specified"


def test_header_states_the_contract_with_the_non_finite_cases():
    text = open(os.path.join(INCLUDE, "pct_engine.h")).read()
    m = re.search(r"k nearest neighbours \(pct_knn_batch\*.*?\n \*\n", text, flags=re.S)
    assert m, "the k-NN contract paragraph is missing from the header comment"
    para = m.group(0)
    for phrase in ("lower index first", "bit-identical", "PCT_NO_INDEX / +inf", "NaN or infinite", "never listed", "PCT_ERR_INVALID", "PCT_ERR_EMPTY"):
        assert phrase in para, phrase
    assert "NOT index-accelerated" in text          # what PCT_ALGO_AUTO means on a rolling-map or small cloud


def test_library_exports_the_entry_points(built):
    L = C.CDLL(built.ENGINE_SO)
    missing = [n for n in KNN_FUNCTIONS if not hasattr(L, n)]
    assert not missing, missing


def test_python_binding(built):
    from pointcloudtraj_amd import engine as E
    assert E.KNN_MAX_K == 64
    assert callable(E.Cloud.knn) and callable(E.Cloud.knn_device)
    assert list(inspect.signature(E.Cloud.knn).parameters) == ["self", "queries", "k", "algo"]
    assert inspect.signature(E.Cloud.knn).parameters["algo"].default == E.ALGO_AUTO
    assert list(inspect.signature(E.Cloud.knn_device).parameters) == ["self", "q_ptr", "Q", "k", "idx_ptr", "d2_ptr", "stream", "algo"]
    L = E.lib()
    assert L.pct_knn_batch_algo.argtypes is not None and len(L.pct_knn_batch_algo.argtypes) == 7
    assert len(L.pct_knn_batch.argtypes) == 6 and len(L.pct_knn_batch_dev.argtypes) == 8


def syntax_only(source, tmp_path, name):
    p = tmp_path / name
    p.write_text(source)
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I" + INCLUDE, str(p)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr


def test_obstacle_map_header_still_compiles_as_cxx17(tmp_path):
    syntax_only('#include "pct_obstacle_map.hpp"\nint main() { return 0; }\n', tmp_path, "only_include.cpp")


def test_cxx_mirror_has_nearest_k_search(tmp_path):
    syntax_only('''#include <cstdint>
#include <vector>
#include "pct_obstacle_map.hpp"
static_assert(PCT_KNN_MAX_K == 64, "PCT_KNN_MAX_K");
void ask(pct::ObstacleMap &map, const std::vector<float> &queries, int k, std::vector<uint32_t> &index, std::vector<double> &d2)
{
    const int64_t n = (int64_t)(queries.size() / 3);
    index.resize((size_t)n * (size_t)k);
    d2.resize((size_t)n * (size_t)k);
    void (pct::ObstacleMap::*member)(const float *, int64_t, int, uint32_t *, double *) = &pct::ObstacleMap::nearestKSearch;
    (map.*member)(queries.data(), n, k, index.data(), d2.data());
    map.nearestKSearch(queries.data(), n, k, index.data(), d2.data());
    map.nearest(queries.data(), n, index.data(), d2.data());
}
''', tmp_path, "calls_nearest_k_search.cpp")
