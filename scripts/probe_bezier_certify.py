"""Certified Bezier check (pct_bezier_certify_batch) against the sampled batched check (pct_bezier_check_batch) on the same candidates,
in the same run, the two calls taking turns: one JSON line per cloud and margin.

Clouds: config C5's rolling map -- a window of --window points (5 M) fed in frames of --frame, the rolling-map index live -- and
config C3's cloud -- --points (10 M) uniform points in [0,100)^3, seed 3, cell index built.
Candidates: 256 translations of the 13-segment trajectory of scripts/probe_bezier_batch.py (orders 0..12, 5.05 s, 255 samples at
dt = 0.02), spread over the cloud.  Margins: --margins, by default 0.25 (the planner's; on clouds this dense every candidate collides
in round 0) and 0.02 (most candidates pass, some closely: several rounds).  The sampled check runs with search_margin = the margin and
a large sample_range, so every sample is searched; the certified check with the same margin, max_depth --depth and the default
piece_cap (64 per segment).
Both are the host forms, called through ctypes on structures built beforehand and timed on the host's clock around the whole call:
after one warm-up call of each, --reps turns of (certified, sampled); the median, minimum and maximum of each are printed with the
certificates' statuses, the pieces and rounds per candidate, and how the two verdicts relate."""
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


def probe(name, c, lo, hi, scale, a, margin):
    L = E.lib()
    prm = E.inflate_params((0.0, 0.0, 0.0), 1e6, margin, 1.5)
    cands = candidates(B, lo, hi, scale)
    batch, keep = E.pack_trajectories(cands)
    verdict = np.zeros(B, E.VERDICT_DTYPE)
    cert = np.zeros(B, E.CERT_DTYPE)
    stats = np.zeros(3, np.int64)
    piece_cap = max(4096, 64 * B * NSEG)

    def run_certified():
        E._chk(L.pct_bezier_certify_batch(c.handle, E.ALGO_AUTO, C.byref(batch), margin, a.depth, piece_cap, cert.ctypes.data, stats.ctypes.data))

    def run_sampled():
        E._chk(L.pct_bezier_check_batch(c.handle, C.byref(batch), C.byref(prm), 100.0, 0.02, 4096, verdict.ctypes.data, None, 0, None, None, None, None))

    run_certified(); run_sampled()
    ms = dict(certified=[], sampled=[])
    for _ in range(a.reps):
        for key, run in (("certified", run_certified), ("sampled", run_sampled)):
            t0 = time.perf_counter()
            run()
            ms[key].append((time.perf_counter() - t0) * 1e3)
    med = {k: statistics.median(v) for k, v in ms.items()}
    status = np.bincount(cert["status"], minlength=4)
    sampled_hit = verdict["first_hit"] >= 0
    out = dict(cloud=name, points=len(c), candidates=B, segments=B * NSEG, margin=margin, max_depth=a.depth, piece_cap=piece_cap, reps=a.reps,
               certified_ms=dict(median=round(med["certified"], 4), min=round(min(ms["certified"]), 4), max=round(max(ms["certified"]), 4)),
               sampled_ms=dict(median=round(med["sampled"], 4), min=round(min(ms["sampled"]), 4), max=round(max(ms["sampled"]), 4)),
               certified_over_sampled=round(med["certified"] / med["sampled"], 3),
               free=int(status[E.CERT_FREE]), hit=int(status[E.CERT_HIT]), undecided=int(status[E.CERT_UNDECIDED]), invalid=int(status[E.CERT_INVALID]),
               rounds=int(stats[0]), pieces=int(stats[1]), capped=int(stats[2]), pieces_per_candidate=round(int(stats[1]) / B, 2),
               deepest=int(cert["depth"].max()), samples=int(verdict["nsamples"].sum()), sampled_colliding=int(sampled_hit.sum()),
               # a FREE certificate contradicted by a sample would be a bug; a sampled "free" the certificate calls HIT is the sampling gap
               free_but_sampled_hit=int((sampled_hit & (cert["status"] == E.CERT_FREE)).sum()),
               hit_but_sampled_free=int((~sampled_hit & (cert["status"] == E.CERT_HIT)).sum()))
    print(json.dumps(out), flush=True)
    del keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=int, default=5_000_000)
    ap.add_argument("--frame", type=int, default=50_000)
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--margins", default="0.25,0.02")
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--skip", choices=("ring", "grid"), default=None)
    a = ap.parse_args()
    margins = [float(m) for m in a.margins.split(",")]
    E.init(0)
    if a.skip != "ring":
        c = E.Cloud(a.window)
        c.ring_index()
        nframes = a.window // a.frame + 12
        for k in range(nframes):
            c.append(S.c5_frame(k, a.frame))
        x0 = 0.1 * (nframes - 1)
        for m in margins:
            probe("rolling window", c, (x0 - 25.0, -25.0, 0.5), (x0 + 5.0, 5.0, 1.5), (1.0, 1.0, 0.2), a, m)
        c.close()
    if a.skip != "grid":
        c = E.Cloud(a.points)
        c.set_input(synth.uniform_points(3, a.points, 0.0, 100.0))
        c.build_grid()
        for m in margins:
            probe("grid", c, (5.0, 5.0, 5.0), (75.0, 75.0, 75.0), (1.0, 1.0, 1.0), a, m)
        c.close()


if __name__ == "__main__":
    main()
