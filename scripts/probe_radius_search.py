"""Radius search with lists (pct_radius_search_batch_dev) against the radius count on the same batch: one JSON line per configuration.

Clouds: config C3's (10 M uniform points in [0,100)^3, seed 3, cell index built) and the 10 M-point clustered pillar-surface cloud.
Batches: --rotate distinct sets of 1 048 576 uniform queries over the cloud's bounding box, resident on the device, taken in turn.
Radii: r = (3 h / (4 pi rho))^(1/3) for h = 4, 32, 256 expected hits per row at the uniform cloud's density rho (points per unit
volume of its bounding box); the same radii on the pillar cloud.  The realised mean row length is printed.
Per radius and order: the median over the timed batches of the whole call -- count, scan, fill, row sort -- between two events on the
stream, and of pct_radius_count_batch_dev on the same batches in the same run (that kernel is what the search starts with, unchanged).

--rolling-map: config C5 instead -- the 5 M-point rolling window fed in 50 k-point frames (uniform and clustered variants), the
rolling-map index live, a tick batch of --tick-queries queries with r = --radius.  Per variant, for the count and for the search in
either order, one line for PCT_ALGO_RING (what PCT_ALGO_AUTO takes there) and one for PCT_ALGO_STREAM on the same cloud in the same
run: median of --batches whole calls between two events on the stream, records examined per query, overflow-queue length and
records per bucket; the results of the two are compared.
"""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from pointcloudtraj_amd import engine as E, scenarios as S, synth

HITS = (4, 32, 256)


def timed(run, rotate, batches):
    """median / min / max ms of run(b) over `batches` launches, batch b = launch mod rotate; one warm-up pass over every batch"""
    for b in range(rotate):
        run(b)
    torch.cuda.synchronize()
    ms = []
    for i in range(batches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run(i % rotate)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def rolling_window(a, clustered):
    """config C5's rolling map: a window of --window points fed in frames of --frame, a few frames beyond full so that the ring has
    wrapped (and, in the clustered variant, the buckets have grown); returns the cloud and the drone's x"""
    make = S.c5_frame_clustered if clustered else S.c5_frame
    c = E.Cloud(a.window)
    c.ring_index()
    nframes = a.window // a.frame + 12
    for k in range(nframes):
        c.append(make(k, a.frame))
    return c, 0.1 * (nframes - 1)


def tick_queries(seed, Q, x0):
    """a replan tick's batch: points of the 50 m x 50 m x 6 m slab around the drone"""
    return (synth.uniform_points(seed, Q, -1.0, 1.0).astype(np.float64) * [25.0, 25.0, 3.0] + [x0, 0.0, 3.0]).astype(np.float32)


def event_timed(run, batches):
    """median / min / max ms of the whole call between two events on the stream, after two warm-up calls"""
    run(); run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(batches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def rolling_map(a):
    dev = torch.device("cuda:0")
    cs = torch.cuda.current_stream().cuda_stream
    Q = a.tick_queries
    for clustered in (False, True):
        c, x0 = rolling_window(a, clustered)
        tq = torch.from_numpy(tick_queries(5, Q, x0)).to(dev)
        tr = torch.full((Q,), a.radius, dtype=torch.float32, device=dev)
        c.reserve_queries(Q)
        ring = c.ring_info()
        toff = torch.zeros(Q + 1, dtype=torch.int64, device=dev)
        tcnt = torch.zeros(Q, dtype=torch.int32, device=dev)
        c.radius_search_device(tq.data_ptr(), tr.data_ptr(), Q, E.ORDER_INDEX, toff.data_ptr(), 0, 0, 0, cs, E.ALGO_RING)      # sizes first
        cap = max(int(toff[Q].item()), 1)
        tidx = torch.empty(cap, dtype=torch.int32, device=dev)
        td2 = torch.empty(cap, dtype=torch.float64, device=dev)
        info = dict(cloud="c5-clustered" if clustered else "c5-uniform", points=len(c), queries=Q, radius=a.radius, mean_row=cap / Q, ring_dims=ring["dims"],
                    cell_size=ring["cell_size"], overflow_entries=ring["overflow_entries"], bucket_records=ring["bucket_records"], batches=a.batches)
        calls = [("pct_radius_count_batch_dev", None, lambda algo: c.radius_count_device(tq.data_ptr(), tr.data_ptr(), Q, tcnt.data_ptr(), cs, algo))]
        for order, oname in ((E.ORDER_INDEX, "index"), (E.ORDER_DISTANCE, "distance")):
            calls.append(("pct_radius_search_batch_dev", oname, lambda algo, order=order: c.radius_search_device(
                tq.data_ptr(), tr.data_ptr(), Q, order, toff.data_ptr(), cap, tidx.data_ptr(), td2.data_ptr(), cs, algo)))
        for call, oname, launch in calls:
            got, times = {}, {}
            for name, algo in (("PCT_ALGO_RING", E.ALGO_RING), ("PCT_ALGO_STREAM", E.ALGO_STREAM)):
                ms, ms_lo, ms_hi = event_timed(lambda: launch(algo), a.batches)
                c.set_work_counters(True)
                launch(algo)
                torch.cuda.synchronize()
                points, buckets = c.last_work()
                c.set_work_counters(False)
                got[name] = [tcnt.cpu().numpy().copy()] if oname is None else [toff.cpu().numpy().copy(), tidx.cpu().numpy().copy(), td2.cpu().numpy().copy()]
                times[name] = ms
                print(json.dumps(dict(info, call=call, order=oname, algo=name, ms_median=ms, ms_min=ms_lo, ms_max=ms_hi, records_per_query=points / Q,
                                      buckets_per_query=buckets / Q)), flush=True)
            same = all(np.array_equal(x, y) for x, y in zip(got["PCT_ALGO_RING"], got["PCT_ALGO_STREAM"]))
            print(json.dumps(dict(info, call=call, order=oname, stream_over_ring=times["PCT_ALGO_STREAM"] / times["PCT_ALGO_RING"], results_equal=bool(same))),
                  flush=True)
        c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--queries", type=int, default=1 << 20)
    ap.add_argument("--batches", type=int, default=9)
    ap.add_argument("--rotate", type=int, default=3)
    ap.add_argument("--clouds", default="uniform,clustered")
    ap.add_argument("--hits", default=",".join(str(h) for h in HITS), help="expected hits per row on the first cloud, comma-separated")
    ap.add_argument("--rolling-map", action="store_true", help="config C5's rolling window instead: PCT_ALGO_RING against PCT_ALGO_STREAM")
    ap.add_argument("--window", type=int, default=S.C5_WINDOW)
    ap.add_argument("--frame", type=int, default=S.C5_FRAME)
    ap.add_argument("--tick-queries", type=int, default=256)
    ap.add_argument("--radius", type=float, default=1.0)
    a = ap.parse_args()
    E.init(0)
    if a.rolling_map:
        a.batches = max(a.batches, 20)
        return rolling_map(a)
    dev = torch.device("cuda:0")
    Q = a.queries
    hits = [int(h) for h in a.hits.split(",")]
    radii = None
    for name in a.clouds.split(","):
        if name == "uniform":
            pts = synth.uniform_points(3, a.points, 0.0, 100.0)
        else:
            pts = synth.pillar_map_scaled(7.4 * (a.points / 10_000_000) ** 0.5)
        lo, hi = pts.min(0), pts.max(0)
        if radii is None:                                   # from the first cloud's density
            rho = len(pts) / float(np.prod((hi - lo).astype(np.float64)))
            radii = [(3.0 * h / (4.0 * math.pi * rho)) ** (1.0 / 3.0) for h in hits]
        tq = [torch.from_numpy((lo + synth.uniform01_f32(5 + b, 3 * Q).reshape(Q, 3) * (hi - lo)).astype(np.float32)).to(dev) for b in range(a.rotate)]
        cs = torch.cuda.current_stream().cuda_stream
        with E.Cloud(len(pts)) as c:
            c.set_input(pts)
            c.build_grid()
            c.reserve_queries(Q)
            info = dict(cloud=name, points=len(pts), queries=Q, grid=c.grid_info()["dims"], batches=a.batches, distinct_batches=a.rotate)
            toff = torch.zeros(Q + 1, dtype=torch.int64, device=dev)
            tcnt = torch.zeros(Q, dtype=torch.int32, device=dev)
            for h, r in zip(hits, radii):
                tr = torch.full((Q,), r, dtype=torch.float32, device=dev)
                totals = []
                for b in range(a.rotate):                   # sizes first: the device form with no room writes the offsets only
                    c.radius_search_device(tq[b].data_ptr(), tr.data_ptr(), Q, E.ORDER_INDEX, toff.data_ptr(), 0, 0, 0, cs, E.ALGO_GRID)
                    totals.append(int(toff[Q].item()))
                cap = max(totals)
                tidx = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
                td2 = torch.empty(max(cap, 1), dtype=torch.float64, device=dev)
                cnt_ms, cnt_lo, cnt_hi = timed(lambda b: c.radius_count_device(tq[b].data_ptr(), tr.data_ptr(), Q, tcnt.data_ptr(), cs, E.ALGO_GRID),
                                               a.rotate, a.batches)
                base = dict(info, expected_hits=h, radius=r, mean_row=sum(totals) / (len(totals) * Q), entries=cap)
                print(json.dumps(dict(base, call="pct_radius_count_batch_dev", ms_median=cnt_ms, ms_min=cnt_lo, ms_max=cnt_hi)), flush=True)
                for order, oname in ((E.ORDER_INDEX, "index"), (E.ORDER_DISTANCE, "distance")):
                    run = lambda b: c.radius_search_device(tq[b].data_ptr(), tr.data_ptr(), Q, order, toff.data_ptr(), cap, tidx.data_ptr(), td2.data_ptr(),
                                                           cs, E.ALGO_GRID)
                    ms, ms_lo, ms_hi = timed(run, a.rotate, a.batches)
                    print(json.dumps(dict(base, call="pct_radius_search_batch_dev", order=oname, ms_median=ms, ms_min=ms_lo, ms_max=ms_hi,
                                          ratio_to_count=ms / cnt_ms, entries_per_s=base["mean_row"] * Q / ms * 1e3,
                                          list_bytes_written=12 * totals[0])), flush=True)
                del tidx, td2, tr
        del tq


if __name__ == "__main__":
    main()
