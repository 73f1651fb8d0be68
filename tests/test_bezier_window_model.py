"""The window forms of the certified Bezier check and the trajectory clearance as the contract states them (no GPU needed):
tests/helpers/bezier_window_model.py against the whole-curve models, against exact rational arithmetic, and the header's paragraph."""
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import bezier_certify_model as CM  # noqa: E402
import bezier_clearance_model as KM  # noqa: E402
import bezier_window_model as WM  # noqa: E402


def line3(t0, h, depth=12):
    coef, T, od, offs = CM.pack([WM.LINE3["traj"]])
    return WM.certify_window(WM.LINE3["pts"], coef, T, od, offs, [t0], [h], WM.LINE3["margin"], depth, 1000)


def test_the_table_of_the_three_metre_line():
    for t0, h, status in WM.LINE3_TABLE:
        cert, stats = line3(t0, h)
        print(t0, h, cert[0], stats)
        assert cert["status"][0] == status, (t0, h)
    # from t = 1.5 on: one round of two pieces
    cert, stats = line3(1.5, np.inf)
    assert list(stats) == [1, 2, 0] and cert["pieces"][0] == 2 and cert["depth"][0] == 0
    # [1.25, 1.75]: one piece
    cert, stats = line3(1.25, 0.5)
    assert list(stats) == [1, 1, 0] and cert["pieces"][0] == 1
    # the empty window: the sampled check's "no sample at all"
    cert, stats = line3(3.0, np.inf)
    assert list(stats) == [0, 0, 0]
    c = cert[0]
    assert c["depth"] == 0 and c["pieces"] == 0 and c["min_d2"] == np.inf and c["hit_seg"] == -1 and c["hit_idx"] == CM.NO_INDEX
    assert np.isnan(c["hit_u"]) and c["hit_d2"] == np.inf
    coef, T, od, offs = CM.pack([WM.LINE3["traj"]])
    rec, stats = WM.clearance_window(WM.LINE3["pts"], coef, T, od, offs, [3.0], [np.inf], 0.01, np.inf, 16, 1000)
    r = rec[0]
    assert r["status"] == KM.DONE and r["lo"] == np.inf and r["hi"] == np.inf and r["pieces"] == 0 and r["at_seg"] == -1 and np.isnan(r["at_u"])
    # the hit inside [0.9, 1.1] names the curve point of the whole-curve hit: the joint x = 1, as the end of segment 0 or the start of 1
    whole, _ = line3(0.0, np.inf)
    part, _ = line3(0.9, 0.2)
    x = [int(c["hit_seg"][0]) + float(c["hit_u"][0]) for c in (whole, part)]
    assert abs(x[0] - 1.0) < 1e-6 and abs(x[1] - 1.0) < 1e-6, x
    # the clearance from 1.5: the point is half a metre behind
    rec, _ = WM.clearance_window(WM.LINE3["pts"], coef, T, od, offs, [1.5], [np.inf], 0.01, np.inf, 16, 1000)
    assert rec["status"][0] == KM.DONE and rec["lo"][0] > 0.49 and rec["hi"][0] < 0.51 and rec["at_seg"][0] == 1 and rec["at_u"][0] == 0.5


def test_the_whole_window_is_the_whole_curve_model():
    pts, trajs = CM.scene()
    packed = CM.pack(trajs[:24])
    want = CM.certify(pts, *packed, CM.MARGIN, 12, 1 << 16)
    for ts, hz in ((None, None), (np.zeros(24), np.full(24, np.inf))):
        got = WM.certify_window(pts, *packed, ts, hz, CM.MARGIN, 12, 1 << 16)
        assert got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1])
    want = KM.clearances(pts, *packed, 0.05, np.inf, 16, 1 << 16)
    got = WM.clearance_window(pts, *packed, None, None, 0.05, np.inf, 16, 1 << 16)
    assert got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1])
    assert np.any(want[0]["at_seg"] > 0)


def test_covered_ends_are_exact_and_joints_belong_to_one_side():
    T = [0.3, 0.7, 0.1, 1.9]
    joints = np.cumsum(T)                                          # sequential sums, as the contract's c
    c = 0.0
    for Ti in T:
        c = c + Ti
    assert c == joints[-1]
    # covered ends are exactly 0 and 1
    for t0, h in ((0.0, np.inf), (0.1, np.inf), (0.0, 2.0), (0.35, 1.0), (joints[0], joints[2] - joints[0])):
        for w in WM.windows(T, t0, h):
            if w is not None:
                assert (w[0] == 0.0 or 0.0 < w[0] < 1.0) and (w[1] == 1.0 or 0.0 < w[1] <= 1.0) and w[0] < w[1]
    w = WM.windows(T, 0.1, np.inf)
    assert w[0][0] == 0.1 / 0.3 and w[0][1] == 1.0 and w[1:] == [(0.0, 1.0)] * 3
    # a window that ends exactly on a joint does not touch the next segment
    w = WM.windows(T, 0.0, float(joints[1]))
    assert w == [(0.0, 1.0), (0.0, 1.0), None, None]
    # one that starts exactly on a joint does not touch the previous one
    w = WM.windows(T, float(joints[1]), np.inf)
    assert w == [None, None, (0.0, 1.0), (0.0, 1.0)]
    w = WM.windows(T, float(joints[0]), float(joints[2]) - float(joints[0]))
    assert w[0] is None and w[1] == (0.0, 1.0) and w[3] is None
    # at or past the end: empty; one ulp before it: a sliver of the last segment
    assert WM.windows(T, float(joints[-1]), np.inf) == [None] * 4 and WM.windows(T, 1e9, 1.0) == [None] * 4
    w = WM.windows(T, float(np.nextafter(joints[-1], 0.0)), np.inf)
    assert w[:3] == [None] * 3 and (w[3] is None or (w[3][1] == 1.0 and w[3][0] < 1.0))
    # map_u: v itself for an uncut segment, u0 at 0 and u1 at 1
    for v in (0.0, 0.25, 65 / 128, 1.0):
        assert WM.map_u(v, 0.0, 1.0) == v
    assert WM.map_u(0.0, 0.3, 0.7) == 0.3 and WM.map_u(1.0, 0.3, 0.7) == 0.7


@pytest.mark.parametrize("t0,h", [(np.nan, 1.0), (np.inf, 1.0), (-1e-300, 1.0), (-1.0, np.inf), (0.0, 0.0), (0.0, -1.0), (0.0, np.nan), (1.0, -np.inf)])
def test_invalid_windows(t0, h):
    assert WM.windows([1.0, 1.0], t0, h) is None
    pts, trajs = CM.scene()
    packed = CM.pack(trajs[:3])
    ts, hz = np.array([0.0, t0, 0.2]), np.array([np.inf, h, 0.5])
    cert, stats = WM.certify_window(pts, *packed, ts, hz, CM.MARGIN, 12, 1 << 16)
    c = cert[1]
    assert c["status"] == CM.INVALID and c["pieces"] == 0 and c["depth"] == 0 and c["hit_seg"] == -1 and c["min_d2"] == np.inf
    rec, _ = WM.clearance_window(pts, *packed, ts, hz, 0.05, np.inf, 16, 1 << 16)
    assert rec["status"][1] == KM.INVALID and np.isnan(rec["lo"][1]) and np.isnan(rec["hi"][1]) and rec["pieces"][1] == 0
    # its neighbours do not depend on it
    alone, _ = WM.certify_window(pts, *CM.pack(trajs[2:3]), ts[2:], hz[2:], CM.MARGIN, 12, 1 << 16)
    a, b = alone[0].copy(), cert[2].copy()
    if a["hit_seg"] >= 0:
        a["hit_seg"] += 6
    assert a.tobytes() == b.tobytes()


def test_a_bad_segment_outside_the_window_still_makes_the_trajectory_invalid():
    pts, trajs = CM.scene()
    coef, T, od = trajs[0]
    T = T.copy()
    T[2] = np.nan
    cert, _ = WM.certify_window(pts, *CM.pack([(coef, T, od)]), [0.0], [0.1], CM.MARGIN, 12, 1000)
    assert cert["status"][0] == CM.INVALID


def exact_restrict(P, u0, u1):
    """the restriction of P's curve to [u0, u1] in rational arithmetic"""
    def cut(p, t):
        left, right = [p[0]], [p[-1]]
        while len(p) > 1:
            p = [(1 - t) * a + t * b for a, b in zip(p[:-1], p[1:])]
            left.append(p[0])
            right.append(p[-1])
        return left, right[::-1]
    p = [Fraction(float(v)) for v in P]
    u0, u1 = Fraction(float(u0)), Fraction(float(u1))
    if u1 < 1:
        p = cut(p, u1)[0]
    if u0 > 0:
        p = cut(p, u0 / u1)[1]
    return p


@pytest.mark.parametrize("order", (1, 3, 7, 12))
def test_restrict_against_exact_rational_de_casteljau(order):
    rng = np.random.default_rng(100 + order)
    worst = 0.0
    for trial in range(12):
        P = rng.uniform(-1000.0, 1000.0, (order + 1, 3))
        u0, u1 = sorted(rng.uniform(0.0, 1.0, 2))
        if trial % 4 == 1:
            u0 = 0.0
        elif trial % 4 == 2:
            u1 = 1.0
        elif trial % 4 == 3:
            u0 = u1 * (1.0 - 1e-9)                                 # a sliver
        got = WM.restrict(P, u0, u1)
        M0 = float(np.max(np.abs(P)))
        for k in range(3):
            want = exact_restrict(P[:, k], u0, u1)
            err = max(abs(Fraction(float(g)) - w) for g, w in zip(got[:, k], want))
            worst = max(worst, float(err) / M0)
    print(f"order {order}: restriction off the exact one by {worst:.3g} * M0 (claimed bound {WM.RESTRICT_BOUND:.3g})")
    assert worst <= WM.RESTRICT_BOUND
    # both ends covered: not cut at all
    assert WM.restrict(P, 0.0, 1.0).tobytes() == P.tobytes()


def test_header_paragraph_states_the_rules():
    text = re.sub(r"\s*\n \* ?", " ", open(os.path.join(ROOT, "include", "pct_engine.h")).read())
    m = re.search(r"Windows of a trajectory \(pct_bezier_certify_window_batch\*, pct_bezier_clearance_window_batch\*\):(.*?)All entry points need a HIP device",
                  text, flags=re.S)
    assert m, "the contract paragraph is missing"
    para = m.group(1)
    for phrase in ("batch->t_start IS read", "NULL = +inf for all", "t1 = t0 + horizon[b], one addition", "t0 is not finite or < 0",
                   "horizon is NaN or not > 0", "over ALL its segments", "t0 < cn && t1 > c", "u0 = (t0 <= c) ? 0 : (t0 - c) / T_i",
                   "u1 = (t1 >= cn) ? 1 : (t1 - c) / T_i", "!(u0 < u1)", "a covered end is exactly 0 or 1", "cut at t = u0 / u1 (one division)",
                   "q[i] = w * p[i] + t * p[i+1] with w = 1 - t computed once", "is not cut at all", "a dead slot",
                   "u = (1 - v) * u0 + v * u1", "stay indices into the packed batch", "no sample at all", "depth = pieces = 0",
                   "min_d2 = hi = lo = +inf", "348 * 2^-53 * M0", "margin + rho >= 2^-24 * M0", "da + db + ell + rho >= 2^-24 * M0",
                   "reach and L are unchanged", "nothing is written", "refused during graph capture"):
        assert phrase in para, phrase
    whole = re.search(r"Certified Bezier check \(pct_bezier_certify_batch\*\):(.*?)Trajectory clearance \(", text, flags=re.S).group(1)
    assert "t_start is NOT read" in whole
    code = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "pct_engine.h")).read(), flags=re.S)
    for name, nargs in (("pct_bezier_certify_window_batch", 9), ("pct_bezier_certify_window_batch_dev", 10), ("pct_bezier_clearance_window_batch", 10),
                        ("pct_bezier_clearance_window_batch_dev", 11)):
        m = re.search(r"int\s+" + name + r"\s*\((.*?)\)\s*;", code, flags=re.S)
        assert m and len(m.group(1).split(",")) == nargs, name


def test_python_binding_and_symbols():
    import subprocess
    from pointcloudtraj_amd import build, engine
    for name in ("bezier_certify_window", "bezier_clearance_window", "bezier_certify_window_device", "bezier_clearance_window_device"):
        assert callable(getattr(engine.Cloud, name)), name
    path = os.path.join(build.LIB, "libpct_engine.so")
    assert os.path.exists(path), f"{path} is missing: build first"
    exported = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    names = {line.split()[-1] for line in exported.splitlines() if line.strip()}
    want = {"pct_bezier_certify_window_batch", "pct_bezier_certify_window_batch_dev", "pct_bezier_clearance_window_batch",
            "pct_bezier_clearance_window_batch_dev"}
    assert want <= names, sorted(want - names)
    batch, keep, hz = engine.Cloud._window_batch(CM.scene()[1][:3], 0.25, [1.0, 2.0, np.inf])
    assert list(keep["t_start"]) == [0.25] * 3 and list(hz) == [1.0, 2.0, np.inf] and batch.B == 3
