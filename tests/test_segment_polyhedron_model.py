"""The reference model of the free-space polyhedra (tests/helpers/segment_polyhedron_model.py) against a scalar double loop, on cases
known by hand and on the guarantees the contract states -- no GPU needed.  The contract: include/pct_engine.h, paragraph
"Free-space polyhedra"."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import segment_model as M  # noqa: E402
import segment_polyhedron_model as PM  # noqa: E402
import segment_search_model as SS  # noqa: E402
from test_segment_search_model import random_case, scalar_rows  # noqa: E402

INF, NAN = np.inf, np.nan
ON_X = [[0, 0, 0, 10, 0, 0]]
DTYPES = [np.int64, np.uint32, np.float64, np.float64, np.float64]


def scalar_polyhedra(pts, segs, reach, base=0):
    """the contract, one Python double at a time, on top of the scalar capsule rows in distance order"""
    f32 = lambda v: float(np.float32(v))                                       # noqa: E731
    off, idx, d2, s = scalar_rows(pts, segs, reach, 1, base)
    P = [[float(v) for v in p] for p in np.asarray(pts, np.float32).reshape(-1, 3)]
    offsets, oi, od, os_, op = [0], [], [], [], []
    for q, seg in enumerate(np.asarray(segs, np.float64).reshape(-1, 6)):
        with np.errstate(over="ignore"):
            a, b = [f32(v) for v in seg[:3]], [f32(v) for v in seg[3:]]
        e = [b[k] - a[k] for k in range(3)]
        sup = []                                                               # (p, n) of the supports so far
        for j in range(int(off[q]), int(off[q + 1])):
            x = P[int(idx[j]) - base]
            cut = False
            for p, n in sup:
                u = [x[k] - p[k] for k in range(3)]
                h = (n[0] * u[0] + n[1] * u[1]) + n[2] * u[2]
                if h >= 0:
                    cut = True
                    break
            if cut:
                continue
            n = [(x[k] - a[k]) - float(s[j]) * e[k] for k in range(3)]
            sup.append((x, n))
            if d2[j] == 0:
                plane = [0.0, 0.0, 0.0, -1.0]
            else:
                d = math.sqrt(float(d2[j]))
                nh = [n[k] / d for k in range(3)]
                plane = nh + [(nh[0] * x[0] + nh[1] * x[1]) + nh[2] * x[2]]
            oi.append(int(idx[j])); od.append(float(d2[j])); os_.append(float(s[j])); op.append(plane)
        offsets.append(len(oi))
    return np.int64(offsets), np.uint32(oi), np.float64(od), np.float64(os_), np.float64(op).reshape(-1, 4)


def equal(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want)) and [g.dtype for g in got] == DTYPES and got[4].shape == (len(got[1]), 4)


@pytest.mark.parametrize("seed", [21, 22, 23])
def test_model_against_a_scalar_double_loop(seed):
    pts, segs = random_case(seed)
    pts[::17, 1] = NAN
    pts[5::23, 0] = INF
    pts[40] = pts[41]                                                          # a duplicate
    for reach in (0.0, 0.3, 1.5, INF, np.resize([0.2, 0.8, 3.0, NAN, -1.0], len(segs))):
        got = PM.segment_polyhedron(pts, segs, reach, 7)
        assert equal(got, scalar_polyhedra(pts, segs, reach, 7)), reach
        rows = SS.segment_search(pts, segs, reach, 1, 7)
        lens, nsup = np.diff(rows[0]), np.diff(got[0])
        assert np.all(nsup <= lens) and np.all((nsup > 0) == (lens > 0))
        first = rows[0][:-1][lens > 0]
        assert np.array_equal(got[1][got[0][:-1][lens > 0]], rows[1][first]), "the first entry of a non-empty row is a support"
    assert np.any(np.diff(PM.segment_polyhedron(pts, segs, INF)[0]) > 3)


def test_one_point_beside_the_segment():
    off, idx, d2, s, pl = PM.segment_polyhedron(np.float32([[5, 2, 0]]), ON_X, 3.0, 100)
    assert list(off) == [0, 1] and list(idx) == [100] and list(d2) == [4.0] and list(s) == [0.5]
    assert pl.tolist() == [[0.0, 1.0, 0.0, 2.0]]                               # the half-space y <= 2


def test_collinear_points_behind_each_other():
    pts = np.float32([[5, 2, 0], [5, 3, 0], [5, 2.5, 1]])
    off, idx, d2, s, pl = PM.segment_polyhedron(pts, ON_X, 5.0)
    assert list(off) == [0, 1] and list(idx) == [0]                            # both lie at or beyond the plane y = 2
    off, idx, _, _, _ = PM.segment_polyhedron(np.float32([[5, 2, 0], [5, 1.9375, 3]]), ON_X, 5.0)
    assert list(idx) == [0, 1]                                                 # y < 2: not cut, although farther away


def test_a_duplicate_point_is_cut():
    pts = np.float32([[5, 2, 0], [5, 2, 0], [1, 0, 3]])
    off, idx, _, _, _ = PM.segment_polyhedron(pts, ON_X, 5.0)
    assert list(off) == [0, 2] and list(idx) == [0, 2]                         # u = 0, h = 0: inclusive


def test_equal_d2_on_opposite_sides():
    pts = np.float32([[7, -2, 0], [3, 2, 0]])
    off, idx, d2, _, pl = PM.segment_polyhedron(pts, ON_X, 5.0)
    assert list(idx) == [0, 1] and list(d2) == [4.0, 4.0]                      # both supports, the lower index first
    assert pl.tolist() == [[0.0, -1.0, 0.0, 2.0], [0.0, 1.0, 0.0, 2.0]]


def test_a_point_on_the_segment_cuts_everything():
    pts = np.float32([[5, 2, 0], [4, 0, 0], [1, -1, 0], [4, 0, 0]])
    off, idx, d2, s, pl = PM.segment_polyhedron(pts, ON_X, 5.0)
    assert list(off) == [0, 1] and list(idx) == [1] and list(d2) == [0.0] and list(s) == [0.4]
    assert pl.tolist() == [[0.0, 0.0, 0.0, -1.0]] and not np.signbit(pl[0, :3]).any()


def test_degenerate_segment_and_a_sphere():
    rng = np.random.default_rng(31)
    d = rng.normal(size=(64, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    pts = (np.float64([3, 4, 5]) + 2.0 * d).astype(np.float32)
    seg = [[3, 4, 5, 3, 4, 5]]
    off, idx, d2, s, pl = PM.segment_polyhedron(pts, seg, 3.0)
    assert list(off) == [0, 64] and sorted(idx) == list(range(64)) and np.all(s == 0.0)      # tangent planes of a sphere cut no other point of it
    assert np.all(np.diff(d2) >= 0)
    assert np.allclose(np.linalg.norm(pl[:, :3], axis=1), 1.0, atol=1e-15)


def test_empty_and_invalid_rows():
    pts = np.float32([[1, 1, 1], [2, 2, 2]])
    segs = np.float64([[0, 0, 0, 3, 3, 0], [NAN, 0, 0, 3, 3, 3], [0, 0, 0, 3, INF, 3], [0, 0, 0, 1e39, 0, 0], [50, 50, 50, 60, 50, 50]])
    off, idx, _, _, pl = PM.segment_polyhedron(pts, segs, 2.0)
    assert list(off) == [0, 1, 1, 1, 1, 1] and list(idx) == [0] and pl.shape == (1, 4)
    for r in (NAN, -1.0, -INF):
        assert PM.segment_polyhedron(pts, segs[:1], r)[0][-1] == 0
    got = PM.segment_polyhedron(np.zeros((0, 3), np.float32), segs, INF)
    assert list(got[0]) == [0] * 6 and [len(v) for v in got[1:]] == [0] * 4 and got[4].shape == (0, 4) and [g.dtype for g in got] == DTYPES
    got = PM.segment_polyhedron(pts, np.zeros((0, 6)), 1.0)
    assert list(got[0]) == [0] and got[4].shape == (0, 4)


@pytest.mark.parametrize("seed", [41, 42])
def test_guarantees_on_tame_inputs(seed):
    """coordinates in [0, 10): (1) every sampled point of the segment lies in every half-space; (2) every candidate of the capsule
    row lies on or outside one of the row's planes"""
    rng = np.random.default_rng(seed)
    pts = (rng.random((300, 3)) * 10).astype(np.float32)
    a = rng.random((60, 3)) * 10
    b = np.clip(a + rng.normal(size=(60, 3)) * np.resize([0.0, 0.5, 2.0], 60)[:, None], 0.0, 9.999)
    segs = np.concatenate([a, b], axis=1)
    A, B = M.narrow(segs)
    for reach in (1.0, 2.5, INF):
        rows = SS.segment_search(pts, segs, reach, 1)
        off, idx, d2, s, pl = PM.from_rows(pts, segs, rows)
        assert off[-1] > 60
        t = np.linspace(0.0, 1.0, 33)[:, None]
        for q in range(60):
            P = pl[off[q]:off[q + 1]]
            if len(P) == 0:
                continue
            assert np.all(d2[off[q]:off[q + 1]] > 0)
            y = A[q] + t * (B[q] - A[q])
            assert np.all(y @ P[:, :3].T <= P[:, 3] + 1e-12 * (1 + np.abs(P[:, 3]))), "(1)"
            x = pts[rows[1][rows[0][q]:rows[0][q + 1]]].astype(np.float64)
            assert np.all((x @ P[:, :3].T - P[:, 3]).max(axis=1) >= -1e-9), "(2)"
