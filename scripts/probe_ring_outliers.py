"""Radius outlier removal on the rolling map (pct_cloud_ring_remove_outliers), timed on config C5's window: one JSON line per window kind.

Window: --window points (5 M) fed in --frame-point frames (50 k), uniform and clustered, the rolling-map index live and de-dup on
(res 0.1, the lattice of the frames).  Measured: host wall time per call ended by pct_sync, [min, median, max] of --reps calls taken
in turn -- the new call, then the route a caller had before it (radius_crop read-out of the window, radius_count(ALGO_RING) over the
judged rows, ring_remove_indices of the rows below m), on the same window in the same run:
  (a) frame     newest = one frame, under a rule that removes nothing (so every repeat sees the same window)
  (b) window    every row, same rule
  (c) removal   one real removal of the whole window at --r / --m (once each: the new call on the window, the old route on a second
                cloud holding the same rows), with the rows removed
The rule that removes nothing is m = 1 with the smallest r of a ladder at which every row of the window has a neighbour.  The
early-exit share -- rows decided in their own bucket -- comes from the instrumented build of the judge kernel that set_work_counters
selects; the timed calls run the shipped one.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from pointcloudtraj_amd import engine as E, scenarios as S


def timed(fn, reps):
    ms = []
    for _ in range(reps):
        E.sync()
        t0 = time.perf_counter()
        fn()
        E.sync()
        ms.append(1e3 * (time.perf_counter() - t0))
    return [min(ms), statistics.median(ms), max(ms)]


def old_route(c, r, m, newest, remove=True):
    """what the parent commit offers: read the window out, count over the table with the judged rows as queries, remove by index"""
    idx, _, xyz = c.radius_crop((0.0, 0.0, 0.0), 1.0e9)                     # live rows in slot order (the window has not wrapped: slot order = arrival order)
    if 0 < newest < len(idx):
        idx, xyz = idx[-newest:], xyz[-newest:]
    counts = c.radius_count(xyz, np.full(len(xyz), r, np.float32), E.ALGO_RING).astype(np.int64) - 1
    doomed = idx[counts < m]
    return c.ring_remove_indices(doomed) if remove and len(doomed) else 0


def probe(a, clustered):
    make = S.c5_frame_clustered if clustered else S.c5_frame
    c = E.Cloud(a.window)
    c.ring_index()
    c.ring_dedup(0.1)
    k = 0
    while len(c) + a.frame <= a.window and k < 4 * (a.window // a.frame):  # fill without wrapping: the old route's slot order is arrival order
        c.append(make(k, a.frame))
        k += 1
    E.sync()
    info = c.ring_info()
    out = dict(kind="clustered" if clustered else "uniform", window=a.window, frame=a.frame, rows=len(c), frames=k, cell_size=info["cell_size"],
               bucket_records=info["bucket_records"], overflow_entries=info["overflow_entries"], r=a.r, m=a.m)
    safe_r = None
    for r in (0.1, 0.15, 0.2, 0.3, 0.5, 1.0, 2.0, 4.0):
        if int((c.ring_neighbour_counts(r, 1) == 0).sum()) == 0:
            safe_r = r
            break
    out["safe_r"] = safe_r
    if safe_r is not None:
        assert c.ring_remove_outliers(safe_r, 1) == 0
        out["frame_new_ms"] = timed(lambda: c.ring_remove_outliers(safe_r, 1, a.frame), a.reps)
        out["frame_old_ms"] = timed(lambda: old_route(c, safe_r, 1, a.frame), a.reps)
        out["window_new_ms"] = timed(lambda: c.ring_remove_outliers(safe_r, 1), a.reps)
        out["window_old_ms"] = timed(lambda: old_route(c, safe_r, 1, 0), max(1, a.reps // 4))
    # the early-exit share at the real rule, from the instrumented kernel (counts only: nothing is removed)
    c.set_work_counters(True)
    c.ring_neighbour_counts(a.r, a.m)
    records, walked, own = c.last_work_ex()
    c.set_work_counters(False)
    out.update(rows_walked=walked, rows_decided_in_own_bucket=own, own_bucket_share=own / max(walked, 1), records_per_row=records / max(walked, 1))
    # (c) one real removal; the old route on a twin holding the same rows
    _, _, rows = c.radius_crop((0.0, 0.0, 0.0), 1.0e9)
    twin = E.Cloud(a.window)
    twin.ring_index(info["cell_size"])
    twin.append(rows)
    E.sync()
    removed = []
    out["removal_new_ms"] = timed(lambda: removed.append(c.ring_remove_outliers(a.r, a.m)), 1)[1]
    out["removal_old_ms"] = timed(lambda: removed.append(old_route(twin, a.r, a.m, 0)), 1)[1]
    out.update(removed_new=removed[0], removed_old=removed[1], live_after=c.ring_live()[0])
    print(json.dumps(out), flush=True)
    twin.close()
    c.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--window", type=int, default=S.C5_WINDOW)
    ap.add_argument("--frame", type=int, default=S.C5_FRAME)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--r", type=float, default=0.3)
    ap.add_argument("--m", type=int, default=2)
    ap.add_argument("--kind", choices=("uniform", "clustered", "both"), default="both")
    a = ap.parse_args()
    E.init(0)
    for clustered in (False, True):
        if a.kind in ("both", "clustered" if clustered else "uniform"):
            probe(a, clustered)


if __name__ == "__main__":
    main()
