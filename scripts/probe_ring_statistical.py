"""Statistical outlier removal on the rolling map (pct_cloud_ring_remove_isolated / _remove_statistical), timed on config C5's window:
one JSON line per window kind.

Window: --window points (5 M) fed in --frame-point frames (50 k), uniform and clustered, the rolling-map index live and de-dup on
(res 0.1, the lattice of the frames).  Measured: host wall time per call ended by pct_sync, [min, median, max] of --reps calls taken
in turn after --warmup calls of each, in the same process on the same window:
  (a) frame_new   ring_remove_isolated(k, threshold, newest = one frame) under a threshold that removes nothing (the largest mean of
                  the judged rows), so that every repeat sees the same window
  (b) frame_old   the route a caller had before it for the same rows: radius_crop read-out of the window, knn(rows, k + 1, ALGO_RING)
                  with the rows as queries, the means on the host, ring_remove_indices of the rows above the threshold
  (c) window      one whole-window ring_remove_statistical at --mult (once), with its statistics and the rows removed, and the
                  instrumented kernel's records and buckets per row (set_work_counters; the timed calls run the shipped kernel)
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


def timed(fn, reps, warmup=0):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        E.sync()
        t0 = time.perf_counter()
        fn()
        E.sync()
        ms.append(1e3 * (time.perf_counter() - t0))
    return [min(ms), statistics.median(ms), max(ms)]


def host_means(idx, d2, slots, k):
    """the means of the contract from a k-NN batch of k + 1: the row's own entry dropped, or the last entry where it is absent"""
    own = idx == slots[:, None]
    drop = np.where(own.any(axis=1), own.argmax(axis=1), k)
    keep = np.ones(idx.shape, bool)
    keep[np.arange(len(idx)), drop] = False
    d = d2[keep].reshape(len(idx), k)
    s = np.zeros(len(idx))
    for e in range(k):
        s = s + np.sqrt(d[:, e])
    return np.where(np.isfinite(d[:, k - 1]), s / float(k), np.inf)


def old_route(c, k, threshold, newest, remove=True):
    """what the parent commit offers: read the window out, a k-NN batch over the table with the judged rows as queries, the means on
    the host, remove by index"""
    idx, _, xyz = c.radius_crop((0.0, 0.0, 0.0), 1.0e9)                     # live rows in slot order (the window has not wrapped: slot order = arrival order)
    if 0 < newest < len(idx):
        idx, xyz = idx[-newest:], xyz[-newest:]
    ki, kd = c.knn(xyz, k + 1, E.ALGO_RING)
    mean = host_means(ki, kd, idx, k)
    doomed = idx[mean > threshold]
    return (c.ring_remove_indices(doomed) if remove and len(doomed) else 0), mean


def probe(a, clustered):
    make = S.c5_frame_clustered if clustered else S.c5_frame
    c = E.Cloud(a.window)
    c.ring_index()
    c.ring_dedup(0.1)
    f = 0
    while len(c) + a.frame <= a.window and f < 4 * (a.window // a.frame):  # fill without wrapping: the old route's slot order is arrival order
        c.append(make(f, a.frame))
        f += 1
    E.sync()
    info = c.ring_info()
    out = dict(kind="clustered" if clustered else "uniform", window=a.window, frame=a.frame, rows=len(c), frames=f, cell_size=info["cell_size"],
               bucket_records=info["bucket_records"], overflow_entries=info["overflow_entries"], k=a.k, mult=a.mult)
    mean = c.ring_knn_mean_distances(a.k, a.frame)
    judged = mean[~np.isnan(mean)]
    threshold = float(judged[np.isfinite(judged)].max())
    out.update(frame_rows_judged=len(judged), frame_rows_unmeasured=int(np.isinf(judged).sum()), frame_threshold=threshold)
    _, route_mean = old_route(c, a.k, threshold, a.frame, remove=False)
    out["routes_agree"] = bool(np.array_equal(route_mean, judged))          # same rows, same means, bit for bit
    removed = []
    out["frame_new_ms"] = timed(lambda: removed.append(c.ring_remove_isolated(a.k, threshold, a.frame)), a.reps, a.warmup)
    out["frame_old_ms"] = timed(lambda: removed.append(old_route(c, a.k, threshold, a.frame)[0]), a.reps, a.warmup)
    out["frame_removed_during_timing"] = int(sum(removed))
    out["frame_new_below_old"] = out["frame_new_ms"][2] < out["frame_old_ms"][0]
    # the walk's cost per row over the whole window, from the instrumented kernel (nothing is removed)
    c.set_work_counters(True)
    whole = c.ring_knn_mean_distances(a.k)
    records, buckets, walked = c.last_work_ex()
    c.set_work_counters(False)
    out.update(rows_walked=walked, records_per_row=records / max(walked, 1), buckets_per_row=buckets / max(walked, 1),
               window_rows_unmeasured=int(np.isinf(whole).sum()))
    got = []
    out["window_statistical_ms"] = timed(lambda: got.append(c.ring_remove_statistical(a.k, a.mult)), 1)[1]
    out.update(window_removed=got[0][0], window_stats=got[0][1], live_after=c.ring_live()[0])
    print(json.dumps(out), flush=True)
    c.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--window", type=int, default=S.C5_WINDOW)
    ap.add_argument("--frame", type=int, default=S.C5_FRAME)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--mult", type=float, default=3.0)
    ap.add_argument("--kind", choices=("uniform", "clustered", "both"), default="both")
    a = ap.parse_args()
    E.init(0)
    for clustered in (False, True):
        if a.kind in ("both", "clustered" if clustered else "uniform"):
            probe(a, clustered)


if __name__ == "__main__":
    main()
