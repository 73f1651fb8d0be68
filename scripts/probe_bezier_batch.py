"""Batched Bezier check (pct_bezier_check_batch) against a loop of pct_bezier_check over the same candidates, in the same run: one JSON
line per cloud and B.

Clouds: config C5's rolling map -- a window of --window points (5 M) fed in frames of --frame, the rolling-map index live -- and
config C3's cloud -- --points (10 M) uniform points in [0,100)^3, seed 3, cell index built.
Candidates: B in {1, 16, 256, 4096} translations of a 13-segment trajectory with orders 0..12 (the one tests/helpers/bezier_model.py
describes: 5.05 s, 255 samples at dt = 0.02), spread over the cloud; sample_range is large, so every sample is searched.
Both sides are the host forms with no lists wanted, called through ctypes on structures built beforehand, and are timed on the host's
clock around the whole call (the loop's cost is its B launches and host waits): median of --reps passes after one warm-up pass.
The verdicts of the two are compared before anything is timed."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from pointcloudtraj_amd import engine as E, scenarios as S, synth

BS = (1, 16, 256, 4096)
NSEG = 13


def base_trajectory(scale):
    """13 segments, orders 0..12, control points advancing ~1.5 m per segment and axis (times `scale` per axis), stored divided by
    the segment time"""
    orders = np.arange(NSEG, dtype=np.int32)
    times = np.float64([0.30 + 0.05 * (k % 5) for k in range(NSEG)])
    r = synth.uniform01_f32(1210, 3 * NSEG * NSEG).astype(np.float64)
    coef = np.zeros((NSEG, 3 * NSEG))
    k = 0
    for s, n in enumerate(orders):
        m = int(n) + 1
        for d in range(3):
            coef[s, d * m:(d + 1) * m] = (s * 1.5 + np.linspace(0, 1.5, m) + (r[k:k + m] - 0.5) * 0.6) * scale[d]
            k += m
    return coef / times[:, None], times, orders


def candidates(B, lo, hi, scale):
    """B translations of the base trajectory, the first control point uniform in [lo, hi)"""
    coef, T, od = base_trajectory(scale)
    off = lo + synth.uniform_rows_f64(77, B, 3, 0.0, 1.0) * (np.float64(hi) - lo)
    out = []
    for b in range(B):
        c = coef.copy()
        for s, n in enumerate(od):
            m = int(n) + 1
            for d in range(3):
                c[s, d * m:(d + 1) * m] += off[b, d] / T[s]
        out.append((c, T, od))
    return out


def wall(run, reps):
    run()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        run()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), min(ms), max(ms)


def probe(name, c, lo, hi, scale, a):
    L = E.lib()
    prm = E.inflate_params((0.0, 0.0, 0.0), 1e6, 0.25, 1.5)
    for B in BS:
        cands = candidates(B, lo, hi, scale)
        batch, keep = E.pack_trajectories(cands)
        verdict = np.zeros(B, E.VERDICT_DTYPE)
        singles = [E._traj(*x) for x in cands]
        fh, ns = np.zeros(B, np.int64), np.zeros(B, np.int64)

        def run_batch():
            E._chk(L.pct_bezier_check_batch(c.handle, C.byref(batch), C.byref(prm), a.stop_time, 0.02, 4096, verdict.ctypes.data, None, 0,
                                            None, None, None, None))

        def run_loop():
            for b, (t, _) in enumerate(singles):
                E._chk(L.pct_bezier_check(c.handle, C.byref(t), C.byref(prm), 0.0, a.stop_time, 0.02,
                                          C.cast(fh.ctypes.data + 8 * b, C.POINTER(C.c_int64)), C.cast(ns.ctypes.data + 8 * b, C.POINTER(C.c_int64)),
                                          4096, None, None, None, None))

        run_batch(); run_loop()
        same = bool(np.array_equal(verdict["nsamples"], ns) and np.array_equal(verdict["first_hit"], fh))
        bm = wall(run_batch, a.reps)
        lm = wall(run_loop, a.reps if B < 4096 else 2)
        print(json.dumps(dict(cloud=name, points=len(c), B=B, samples=int(ns.sum()), colliding=int((fh >= 0).sum()), verdicts_equal=same,
                              batch_ms=dict(median=round(bm[0], 4), min=round(bm[1], 4), max=round(bm[2], 4)),
                              loop_ms=dict(median=round(lm[0], 4), min=round(lm[1], 4), max=round(lm[2], 4)),
                              loop_over_batch=round(lm[0] / bm[0], 2))), flush=True)
        del keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=int, default=5_000_000)
    ap.add_argument("--frame", type=int, default=50_000)
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--stop-time", type=float, default=100.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--skip", choices=("ring", "grid"), default=None)
    a = ap.parse_args()
    E.init(0)
    if a.skip != "ring":
        c = E.Cloud(a.window)
        c.ring_index()
        nframes = a.window // a.frame + 12
        for k in range(nframes):
            c.append(S.c5_frame(k, a.frame))
        x0 = 0.1 * (nframes - 1)
        probe("rolling window", c, (x0 - 25.0, -25.0, 0.5), (x0 + 5.0, 5.0, 1.5), (1.0, 1.0, 0.2), a)
        c.close()
    if a.skip != "grid":
        c = E.Cloud(a.points)
        c.set_input(synth.uniform_points(3, a.points, 0.0, 100.0))
        c.build_grid()
        probe("grid", c, (5.0, 5.0, 5.0), (75.0, 75.0, 75.0), (1.0, 1.0, 1.0), a)
        c.close()


if __name__ == "__main__":
    main()
