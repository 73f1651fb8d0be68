"""Trajectory clearance (pct_bezier_clearance_batch) on the candidates of scripts/probe_bezier_certify.py, beside ONE certified check
at margin 0.02 and the sampled batched check on the same candidates, in the same run: one JSON line per cloud and tol.

Clouds: config C5's rolling map -- a window of --window points (5 M) fed in frames of --frame, the rolling-map index live -- and
config C3's cloud -- --points (10 M) uniform points in [0,100)^3, seed 3, cell index built.
Candidates: 256 translations of the 13-segment trajectory of scripts/probe_bezier_batch.py (orders 0..12), spread over the cloud.
tol: --tols, by default 0.01 and 0.001; cap +inf, max_depth --depth, piece_cap 64 per segment.
All three are the host forms, called through ctypes on structures built beforehand and timed on the host's clock around the whole
call: after one warm-up call of each, --reps turns of (clearance, certified); the median, minimum and maximum of each are printed
with the statuses, the rounds and pieces per candidate, the widest bracket, and how often the sampled check's smallest sample
distance (min_radius + margin, dt = 0.02) exceeds hi -- the sampling gap as a number.  A bisection over margins for the same figure
would cost one certified call per step."""
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
MARGIN = 0.02


def probe(name, c, lo, hi, scale, a, tol):
    L = E.lib()
    prm = E.inflate_params((0.0, 0.0, 0.0), 1e6, MARGIN, 1e6)
    cands = candidates(B, lo, hi, scale)
    batch, keep = E.pack_trajectories(cands)
    verdict = np.zeros(B, E.VERDICT_DTYPE)
    cert = np.zeros(B, E.CERT_DTYPE)
    rec = np.zeros(B, E.CLEARANCE_DTYPE)
    stats = np.zeros(3, np.int64)
    cstats = np.zeros(3, np.int64)
    piece_cap = max(4096, 64 * B * NSEG)

    def run_clearance():
        E._chk(L.pct_bezier_clearance_batch(c.handle, E.ALGO_AUTO, C.byref(batch), tol, float("inf"), a.depth, piece_cap, rec.ctypes.data, stats.ctypes.data))

    def run_certified():
        E._chk(L.pct_bezier_certify_batch(c.handle, E.ALGO_AUTO, C.byref(batch), MARGIN, 12, piece_cap, cert.ctypes.data, cstats.ctypes.data))

    run_clearance(); run_certified()
    E._chk(L.pct_bezier_check_batch(c.handle, C.byref(batch), C.byref(prm), 100.0, 0.02, 4096, verdict.ctypes.data, None, 0, None, None, None, None))
    ms = dict(clearance=[], certified=[])
    for _ in range(a.reps):
        for key, run in (("clearance", run_clearance), ("certified", run_certified)):
            t0 = time.perf_counter()
            run()
            ms[key].append((time.perf_counter() - t0) * 1e3)
    med = {k: statistics.median(v) for k, v in ms.items()}
    status = np.bincount(rec["status"], minlength=3)
    sampled = verdict["min_radius"] + MARGIN
    valid = rec["status"] != E.CLR_INVALID
    out = dict(cloud=name, points=len(c), candidates=B, segments=B * NSEG, tol=tol, max_depth=a.depth, piece_cap=piece_cap, reps=a.reps,
               clearance_ms=dict(median=round(med["clearance"], 4), min=round(min(ms["clearance"]), 4), max=round(max(ms["clearance"]), 4)),
               one_certified_call_ms=dict(median=round(med["certified"], 4), min=round(min(ms["certified"]), 4), max=round(max(ms["certified"]), 4)),
               clearance_over_one_certified_call=round(med["clearance"] / med["certified"], 3),
               done=int(status[E.CLR_DONE]), open=int(status[E.CLR_OPEN]), invalid=int(status[E.CLR_INVALID]),
               rounds=int(stats[0]), pieces=int(stats[1]), capped=int(stats[2]), pieces_per_candidate=round(int(stats[1]) / B, 2),
               deepest=int(rec["depth"].max()), widest_bracket=float(np.max((rec["hi"] - rec["lo"])[valid])), smallest_hi=float(np.min(rec["hi"][valid])),
               certified_rounds=int(cstats[0]), certified_pieces=int(cstats[1]),
               sampled_min_distance_exceeds_hi=int((sampled[valid] > rec["hi"][valid]).sum()),
               largest_excess=float(np.max(sampled[valid] - rec["hi"][valid])),
               # lo above a sample's distance would be a bug: a sample is a point of the curve
               lo_above_a_sample=int((rec["lo"][valid] > sampled[valid] + 1e-6).sum()))
    print(json.dumps(out), flush=True)
    del keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=int, default=5_000_000)
    ap.add_argument("--frame", type=int, default=50_000)
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--tols", default="0.01,0.001")
    ap.add_argument("--depth", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--skip", choices=("ring", "grid"), default=None)
    a = ap.parse_args()
    tols = [float(t) for t in a.tols.split(",")]
    E.init(0)
    if a.skip != "ring":
        c = E.Cloud(a.window)
        c.ring_index()
        nframes = a.window // a.frame + 12
        for k in range(nframes):
            c.append(S.c5_frame(k, a.frame))
        x0 = 0.1 * (nframes - 1)
        for t in tols:
            probe("rolling window", c, (x0 - 25.0, -25.0, 0.5), (x0 + 5.0, 5.0, 1.5), (1.0, 1.0, 0.2), a, t)
        c.close()
    if a.skip != "grid":
        c = E.Cloud(a.points)
        c.set_input(synth.uniform_points(3, a.points, 0.0, 100.0))
        c.build_grid()
        for t in tols:
            probe("grid", c, (5.0, 5.0, 5.0), (75.0, 75.0, 75.0), (1.0, 1.0, 1.0), a, t)
        c.close()


if __name__ == "__main__":
    main()
