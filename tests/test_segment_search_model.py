"""The reference model of the capsule search (tests/helpers/segment_search_model.py) against a scalar double loop, on cases known by
hand and on the properties the contract states -- no GPU needed.  The contract: include/pct_engine.h, paragraph "Capsule search"."""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import segment_model as M  # noqa: E402
import segment_search_model as SS  # noqa: E402

INF, NAN = np.inf, np.nan
ON_X = [[0, 0, 0, 10, 0, 0]]


def scalar_rows(pts, segs, reach, order, base=0):
    """the contract, one Python double at a time (Python floats are IEEE doubles, one rounding per operation)"""
    f32 = lambda v: float(np.float32(v))                                       # noqa: E731
    offsets, idx, d2s, ss = [0], [], [], []
    for seg, r in zip(np.asarray(segs, np.float64).reshape(-1, 6), np.broadcast_to(np.asarray(reach, np.float64), (len(segs),))):
        with np.errstate(over="ignore"):
            a, b = [f32(v) for v in seg[:3]], [f32(v) for v in seg[3:]]
        row = []
        r = float(r)
        if r >= 0 and all(math.isfinite(v) for v in a + b):
            r2 = min(r * r, sys.float_info.max) if math.isfinite(r) else sys.float_info.max
            e = [b[k] - a[k] for k in range(3)]
            L2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
            for i, p in enumerate(np.asarray(pts, np.float32).reshape(-1, 3)):
                p = [float(v) for v in p]
                if any(math.isnan(v) or math.isinf(v) for v in p):
                    continue                                                   # d2 is NaN or infinite: never a candidate
                w = [p[k] - a[k] for k in range(3)]
                dot = (w[0] * e[0] + w[1] * e[1]) + w[2] * e[2]
                s = 0.0 if L2 == 0 else dot / L2
                s = 0.0 if not s > 0 else min(s, 1.0)
                c = [w[k] - s * e[k] for k in range(3)]
                d2 = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]
                if d2 <= r2:
                    row.append((d2, i + base, s))
        if order == 1:
            row.sort(key=lambda t: (t[0], t[1]))
        offsets.append(offsets[-1] + len(row))
        d2s += [t[0] for t in row]
        idx += [t[1] for t in row]
        ss += [t[2] for t in row]
    return np.int64(offsets), np.uint32(idx), np.float64(d2s), np.float64(ss)


def equal(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want)) and [g.dtype for g in got] == [np.int64, np.uint32, np.float64, np.float64]


def random_case(seed, n=300, q=60):
    rng = np.random.default_rng(seed)
    pts = (rng.random((n, 3)) * 10).astype(np.float32)
    a = rng.random((q, 3)) * 12 - 1
    d = rng.normal(size=(q, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    d[::3] = np.eye(3)[np.arange(0, q, 3) % 3]
    a[::7] = pts[(np.arange(0, q, 7) * 5) % n]
    return pts, np.concatenate([a, a + d * np.resize([0.0, 0.05, 3.0, 17.0], q)[:, None]], axis=1)


def test_hand_pinned_rows():
    pts = np.float32([[5, 0, 0], [5, 1, 0], [11, 0, 0], [-0.5, 0, 0], [11.5, 0, 0], [5, -1, 0]])
    off, idx, d2, s = SS.segment_search(pts, ON_X, 1.0, SS.ORDER_INDEX)
    assert list(off) == [0, 5] and list(idx) == [0, 1, 2, 3, 5]               # (11.5, 0, 0) is 1.5 beyond the end cap
    assert list(d2) == [0.0, 1.0, 1.0, 0.25, 1.0] and list(s) == [0.5, 0.5, 1.0, 0.0, 0.5]
    off, idx, d2, s = SS.segment_search(pts, ON_X, 1.0, SS.ORDER_DISTANCE, index_base=100)
    assert list(idx) == [100, 103, 101, 102, 105] and list(d2) == [0.0, 0.25, 1.0, 1.0, 1.0]      # equal d2 in ascending index
    assert list(SS.segment_count(pts, ON_X, 1.0)) == [5]
    assert list(SS.segment_count(pts, ON_X, np.nextafter(1.0, 0.0))) == [2]    # inclusive: d2 == reach^2 is in, just below is out


def test_model_against_a_scalar_double_loop():
    pts, segs = random_case(11)
    pts[::17, 1] = NAN
    pts[5::23, 0] = INF
    for order in (0, 1):
        for reach in (0.0, 0.3, 1.5, INF, 1e200, np.resize([0.2, 0.8, 3.0, NAN, -1.0], len(segs))):
            got = SS.segment_search(pts, segs, reach, order, 7)
            assert equal(got, scalar_rows(pts, segs, reach, order, 7)), (order, reach)
            assert np.array_equal(SS.segment_count(pts, segs, reach).astype(np.int64), np.diff(got[0]))
    assert SS.segment_search(pts, segs, 0.0, 1)[0][-1] > 0, "nothing ON a segment"
    finite = int(np.all(np.isfinite(pts), axis=1).sum())
    assert np.all(np.diff(SS.segment_search(pts, segs, INF, 0)[0]) == finite) and finite < len(pts)


def test_rows_hold_the_winner_of_the_segment_queries_first():
    pts, segs = random_case(12)
    for reach in (0.3, 1.5, INF):
        off, idx, d2, s = SS.segment_search(pts, segs, reach, 1)
        ni, nd, ns = M.segment_nn(pts, segs, reach)
        for q in range(len(segs)):
            if off[q + 1] == off[q]:
                assert ni[q] == M.NO_INDEX
            else:
                assert (idx[off[q]], d2[off[q]], s[off[q]]) == (ni[q], nd[q], ns[q])


def test_degenerate_segments_equal_the_radius_search_model():
    """a == b: the rows of the radius search's reference (tests/test_gpu_radius_search.py, ref_search) for the fp32 point a"""
    from test_gpu_radius_search import ref_search
    pts, _ = random_case(13)
    q = (np.random.default_rng(14).random((80, 3)) * 10).astype(np.float32)
    q[::9] = pts[:9]
    radii = np.resize(np.float32([0.0, 0.7, 2.5, INF]), len(q))
    segs = np.concatenate([q, q], axis=1).astype(np.float64)
    for order in (0, 1):
        ro, ri, rd = ref_search(pts, q, radii, order, 3)
        so, si, sd, s = SS.segment_search(pts, segs, radii.astype(np.float64), order, 3)
        assert ro[-1] > 0 and np.array_equal(so, ro) and np.array_equal(si, ri) and np.array_equal(sd, rd) and np.all(s == 0.0)


def test_invalid_segments_and_reaches_give_empty_rows():
    pts = np.float32([[1, 1, 1], [2, 2, 2]])
    segs = np.float64([[0, 0, 0, 3, 3, 3], [NAN, 0, 0, 3, 3, 3], [0, 0, 0, 3, INF, 3], [0, 0, 0, 1e39, 0, 0], [0, -3.5e38, 0, 3, 3, 3]])
    off, idx, _, _ = SS.segment_search(pts, segs, 0.5, 0)
    assert list(off) == [0, 2, 2, 2, 2, 2] and list(idx) == [0, 1]
    for r in (NAN, -1.0, -INF):
        assert SS.segment_search(pts, segs[:1], r, 0)[0][-1] == 0
    assert SS.segment_search(pts, segs[:1], -0.0, 0)[0][-1] == 2               # -0 is not negative
    off, idx, d2, s = SS.segment_search(np.zeros((0, 3), np.float32), segs, INF, 1)
    assert list(off) == [0] * 6 and len(idx) == len(d2) == len(s) == 0


def test_boxed_route_is_the_model_itself():
    pts, segs = random_case(15, n=2000, q=120)
    far = segs[:10].copy()
    far[:, [0, 3]] += 1e6
    segs = np.concatenate([segs, far])
    reach = np.resize(np.float64([0.0, 0.25, 0.5, 6.0, 500.0, INF, NAN]), len(segs))
    for order in (0, 1):
        assert equal(SS.segment_search_boxed(pts, segs, reach, order, 7), SS.segment_search(pts, segs, reach, order, 7))
