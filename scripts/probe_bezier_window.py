"""Window forms of the certified check and the clearance (pct_bezier_certify_window_batch, pct_bezier_clearance_window_batch) beside the
whole-curve calls on the candidates of scripts/probe_bezier_certify.py, in the same run: one JSON line per cloud.

Clouds and candidates as scripts/probe_bezier_clearance.py: config C5's rolling map (5 M points) and config C3's grid cloud (10 M
points), 256 translations of the 13-segment trajectory of scripts/probe_bezier_batch.py (5.05 s long).  Calls: the certified check at
margins 0.25 and 0.02 (max_depth 12) and the clearance at tol 0.01 (max_depth 16), each as the whole-curve call, as the window call
with [0, +inf), and as the window call from t = 1.0 s for 2/13 of the duration (0.777 s: a horizon of two segments' worth out of
thirteen).  Host forms through ctypes on structures built beforehand, the host's clock around the whole call; after one warm-up of
each, --reps interleaved turns; the median of each with the pieces examined.  A library without the window forms (the parent commit's
build, PCT_ENGINE_SO) is timed on the whole-curve calls alone."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np

from pointcloudtraj_amd import engine as E, scenarios as S, synth
from probe_bezier_batch import NSEG, candidates

B = 256
T_START = 1.0


def probe(name, c, lo, hi, scale, a):
    L = E.lib()
    cands = candidates(B, lo, hi, scale)
    total = float(np.sum(cands[0][1]))
    batch, keep = E.pack_trajectories(cands)
    short, keep2 = E.pack_trajectories(cands, np.full(B, T_START))
    hz = np.full(B, total * 2.0 / 13.0)
    cert = np.zeros(B, E.CERT_DTYPE)
    rec = np.zeros(B, E.CLEARANCE_DTYPE)
    stats = np.zeros(3, np.int64)
    piece_cap = max(4096, 64 * B * NSEG)
    has_window = hasattr(L, "pct_bezier_certify_window_batch")
    inf = float("inf")

    def certify(margin, which):
        def run():
            if which == "whole":
                E._chk(L.pct_bezier_certify_batch(c.handle, E.ALGO_AUTO, C.byref(batch), margin, 12, piece_cap, cert.ctypes.data, stats.ctypes.data))
            else:
                E._chk(L.pct_bezier_certify_window_batch(c.handle, E.ALGO_AUTO, C.byref(batch if which == "full" else short),
                                                         None if which == "full" else hz.ctypes.data, margin, 12, piece_cap, cert.ctypes.data, stats.ctypes.data))
        return run

    def clearance(tol, which):
        def run():
            if which == "whole":
                E._chk(L.pct_bezier_clearance_batch(c.handle, E.ALGO_AUTO, C.byref(batch), tol, inf, 16, piece_cap, rec.ctypes.data, stats.ctypes.data))
            else:
                E._chk(L.pct_bezier_clearance_window_batch(c.handle, E.ALGO_AUTO, C.byref(batch if which == "full" else short),
                                                           None if which == "full" else hz.ctypes.data, tol, inf, 16, piece_cap, rec.ctypes.data, stats.ctypes.data))
        return run

    runs = {}
    for which in ("whole", "full", "short") if has_window else ("whole",):
        runs[f"certify 0.25 {which}"] = certify(0.25, which)
        runs[f"certify 0.02 {which}"] = certify(0.02, which)
        runs[f"clearance 0.01 {which}"] = clearance(0.01, which)
    pieces, rounds = {}, {}
    for key, run in runs.items():
        run()
        pieces[key], rounds[key] = int(stats[1]), int(stats[0])
    ms = {k: [] for k in runs}
    for _ in range(a.reps):
        for key, run in runs.items():
            t0 = time.perf_counter()
            run()
            ms[key].append((time.perf_counter() - t0) * 1e3)
    out = dict(cloud=name, points=len(c), candidates=B, segments=B * NSEG, duration_s=round(total, 4), t_start=T_START, horizon_s=round(float(hz[0]), 4),
               reps=a.reps, window_forms=has_window,
               calls={k: dict(median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4), rounds=rounds[k], pieces=pieces[k])
                      for k, v in ms.items()})
    print(json.dumps(out), flush=True)
    del keep, keep2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=int, default=5_000_000)
    ap.add_argument("--frame", type=int, default=50_000)
    ap.add_argument("--points", type=int, default=10_000_000)
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
