"""Compacting the rolling map (pct_cloud_ring_compact), timed on config C5's window: one JSON line.

Window: --window points (5 M) fed in --frame-point frames (50 k) of the clustered variant, the rolling-map index live and the ring
wrapped; then about 40 % of the rows are removed by forgetOutside-style balls (three steps, each at a quantile of the distances of the
rows still live).  Measured, host wall time, median of --reps (the window is uploaded again and thinned again before every repeat):
  (a) compact_call_ms      pct_cloud_ring_compact as the caller sees it (it returns behind its one host wait, the scatter, the copies
                           and the refile still queued), and compact_done_ms: the call and pct_sync, i.e. with all its kernels
  (b) refile_ms            the floor: an upload of the L live rows from three device arrays onto the same cloud -- three device
                           copies and ring_refile_all into the same table, waited for
  (c) relist_reupload_ms   what a caller without the call has: list the live rows (radius_crop with r = 1e4, rows read back) and
                           upload them onto the cloud again (the table is filed again), waited for
and the replan tick (pct_plan_replan_run: wall time and the wait for the graph, medians of --ticks) with the overflow-queue length
on the full window, on the thinned window (what the parent of this feature leaves a caller with) and on the compacted one.
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


def wall_ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return 1e3 * (time.perf_counter() - t0), out


def d2_to(xyz, centre):
    d = xyz.astype(np.float64) - np.asarray(centre, np.float64)
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def tick(plan, k, ticks):
    P = S.C5_PARAMS
    start, nodes, coef, T, od = S.c5_tick_queries(k)
    prm = E.inflate_params(start, P["sample_range"], P["search_margin"], P["max_radius"])
    ms, wait = [], []
    for _ in range(ticks + 2):
        ms.append(wall_ms(lambda: plan.run(prm, nodes, coef, T, od, 0.0, 2.0, 0.02, want_nn=True, copy=False))[0])
        wait.append(plan.last_run_us()[2])
    return dict(wall_ms=statistics.median(ms[2:]), wait_us=statistics.median(wait[2:]))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--window", type=int, default=S.C5_WINDOW)
    ap.add_argument("--frame", type=int, default=S.C5_FRAME)
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    E.init(0)
    c = E.Cloud(a.window)
    c.ring_index()
    mirror = S.RingMirror(a.window)
    nframes = a.window // a.frame + 12
    for k in range(nframes):
        f = S.c5_frame_clustered(k, a.frame)
        c.append(f)
        mirror.append(f)
    E.sync()
    full = mirror.live().copy()                             # slot order; the cursor stands at mirror.next
    drone = (0.1 * (nframes - 1), 0.0, 2.5)
    d2 = d2_to(full, drone)
    radii = [float(np.sqrt(np.quantile(d2, q))) for q in (0.9, 0.75, 0.6)]
    plan = E.ReplanPlan(c, S.C5_NODES, 128, S.C5_SEGMENTS)
    out = dict(window=a.window, frame=a.frame, bucket_records=c.ring_info()["bucket_records"], overflow_full=c.ring_info()["overflow_entries"],
               tick_full=tick(plan, nframes, a.ticks))

    def thin(cloud):
        return sum(cloud.ring_remove_ball(drone, r, outside=True) for r in radii)

    removed = thin(c)
    live_rows = full[d2 <= radii[-1] * radii[-1]]
    out.update(removed=removed, live=len(live_rows), dead_share=removed / a.window, overflow_thinned=c.ring_info()["overflow_entries"],
               tick_thinned=tick(plan, nframes, a.ticks))
    # (a) the call; every repeat uploads the full window again (the cursor then stands at slot 0) and thins it again
    call, done = [], []
    for rep in range(a.reps):
        if rep:
            c.set_input(full)
            assert thin(c) == removed
        E.sync()
        t0 = time.perf_counter()
        live, reclaimed = c.ring_compact()
        t1 = time.perf_counter()
        E.sync()
        t2 = time.perf_counter()
        assert (live, reclaimed) == (len(live_rows), removed)
        call.append(1e3 * (t1 - t0))
        done.append(1e3 * (t2 - t0))
    out.update(compact_call_ms=statistics.median(call[1:] or call), compact_done_ms=statistics.median(done[1:] or done), compact_first_call_ms=call[0],
               overflow_compacted=c.ring_info()["overflow_entries"], tick_compacted=tick(plan, nframes, a.ticks))
    # (c) the alternative without the call, on the same cloud (same table, same bucket size) thinned the same way
    relist = []
    for _ in range(a.reps):
        c.set_input(full)
        assert thin(c) == removed
        E.sync()

        def alt():
            _, _, xyz = c.radius_crop(drone, 1.0e4)
            c.set_input(xyz)
            E.sync()
            return len(xyz)
        ms, n = wall_ms(alt)
        assert n == len(live_rows)
        relist.append(ms)
    out["relist_reupload_ms"] = statistics.median(relist[1:] or relist)
    # (b) the floor: the live rows, already on the device, filed into the same table
    dev = [torch.from_numpy(np.ascontiguousarray(live_rows[:, k])).cuda() for k in range(3)]
    torch.cuda.synchronize()
    refile = []
    for _ in range(a.reps):
        refile.append(wall_ms(lambda: (c.set_input_device(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), len(live_rows)), E.sync()))[0])
    out.update(refile_ms=statistics.median(refile[1:] or refile), overflow_refiled=c.ring_info()["overflow_entries"])
    print(json.dumps(out), flush=True)
    plan.close()
    c.close()


if __name__ == "__main__":
    main()
