"""CPU checks of tests/helpers/bezier_model.py, the reference model tests/test_gpu_bezier_paths.py holds every path of the sampled
Bezier check to: its sample enumeration against the oracle's (oracle/corridor_port.c ocor_bezier_samples) on a trajectory with
orders 0..12 at the edges of t_start, stop_time and dt; its positions against the oracle's wherever libm's pow is itself correctly
rounded; and the scene's own promises (planted hits, early-outs, unique nearest points)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import bezier_model as M  # noqa: E402
from oracle import oracle as O  # noqa: E402

ROWS = M.rows()


def oracle_samples(t_start, stop, dt, cap=8192):
    O.build()
    coef, T, od = M.trajectory()
    seg, tt, pos = np.zeros(cap, np.int32), np.zeros(cap), np.zeros((cap, 3))
    n = O.port_lib().ocor_bezier_samples(np.ascontiguousarray(coef), coef.shape[1], T, od, len(T), float(t_start), float(stop), float(dt),
                                         seg, tt, pos.reshape(-1), cap)
    return int(n), seg[:n], tt[:n], pos[:n]


def test_trajectory_shape():
    coef, T, od = M.trajectory()
    assert coef.shape == (13, 39) and od.tolist() == list(range(13))
    assert T.tolist() == [0.30 + 0.05 * (k % 5) for k in range(13)] and abs(T.sum() - 5.05) < 1e-12


@pytest.mark.parametrize("row", list(ROWS))
def test_enumeration_equals_the_oracles_and_gives_the_stated_count(row):
    t_start, stop, dt, want = ROWS[row]
    n, seg, tt, pos = oracle_samples(t_start, stop, dt)
    if want is None:
        assert n > 1024
    else:
        assert n == want
    res = M.case("free", "near", row)
    m = min(n, M.CAP_MAX)
    assert res["n"] == n and len(res["pos"]) == len(res["seg"]) == len(res["t"]) == m
    assert np.array_equal(res["seg"], seg[:m]) and np.array_equal(res["t"], tt[:m])          # bit for bit
    ok = res["libm_ok"]
    assert np.array_equal(res["pos"][ok], pos[:m][ok]), "model != oracle where libm's pow is correctly rounded"
    if m:
        assert ok.mean() > 0.9                                   # libm's pow misses the correct rounding on a few samples at most
        assert np.allclose(res["pos"], pos[:m], rtol=1e-13, atol=1e-13)


def test_base_row_per_segment_counts_and_boundary_rows():
    counts = [15, 18, 20, 23, 25, 15, 18, 20, 23, 25, 15, 18, 20]
    assert np.bincount(M.case("free", "near", "base")["seg"], minlength=13).tolist() == counts
    on = M.case("free", "near", "on_boundary")
    assert on["seg"][0] == 1 and on["t"][0] == 0.0               # t_s = T stays in segment 0, which then contributes nothing
    inside = M.case("free", "near", "inside_seg2")
    assert inside["seg"][0] == 2 and 0.09 < inside["t"][0] < 0.11
    T = M.trajectory()[1]                                        # dt = 0.4: t = 0 in every segment, t = 0.4 where T is 0.45 or 0.5
    assert M.case("free", "near", "dt_0.4")["seg"].tolist() == [k for k in range(13) for _ in range(2 if T[k] > 0.4 else 1)]


def test_cap_clips_the_arrays_and_the_first_hit_but_not_the_count():
    for cap, fh in ((1, -1), (19, -1), (20, -1), (21, 20), (50, 20), (254, 20), (255, 20), (256, 20)):
        r = M.case("multi", "near", "base", cap)
        assert r["n"] == 255 and len(r["pos"]) == len(r["radius"]) == len(r["idx"]) == min(255, cap) and r["first_hit"] == fh
    big = M.case("multi", "near", "dt_0.001")
    assert big["n"] == 5050 and len(big["pos"]) == 4096


def test_scene_self_checks():
    info = M.self_check()
    print(info)
    assert info["hits"][0] == 20 and min(info["late_hits"]) >= 128
    # every (cloud, parameter set, row) the GPU tests compare against: unique nearest points (asserted inside case())
    for row in ROWS:
        M.case("multi", "near", row)
    M.case("multi", "far_tail", "base")
    M.case("late", "near", "base")
