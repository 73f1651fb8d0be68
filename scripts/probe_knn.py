"""k-NN batches (pct_knn_batch_dev) against the 1-NN batch on the same cloud and queries: one JSON line per configuration.

Clouds: config C3's (10 M uniform points in [0,100)^3, seed 3, cell index built) and the 10 M-point clustered pillar-surface cloud.
Batch: 1 048 576 uniform queries over the cloud's bounding box (seed 5), resident on the device.  Per k in 1, 4, 8, 16, 32, 64 the
cell-pruned kernel's median duration over the timed batches (HIP events around the kernel, pct_kernel_ms_history), queries/s, and the
points and cell runs examined per query (work counters, one extra instrumented batch).  Yardstick: pct_nn_batch_dev in the same run.
--stream-queries N > 0 also times the streaming kernel on N of the queries (pairs/s = N * points / kernel time; its events span the
stream kernel and the merge of its partial lists).
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from pointcloudtraj_amd import engine as E, synth

KS = (1, 4, 8, 16, 32, 64)


def timed(c, run, batches):
    run()                                                   # warm-up: code object load, workspaces
    torch.cuda.synchronize()
    for _ in range(batches):
        run()
    torch.cuda.synchronize()
    ms = c.kernel_ms_history(batches)[-batches:]
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--queries", type=int, default=1 << 20)
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--stream-queries", type=int, default=0)
    ap.add_argument("--clouds", default="uniform,clustered")
    a = ap.parse_args()
    E.init(0)
    dev = torch.device("cuda:0")
    Q = a.queries
    for name in a.clouds.split(","):
        if name == "uniform":
            pts = synth.uniform_points(3, a.points, 0.0, 100.0)
        else:
            pts = synth.pillar_map_scaled(7.4 * (a.points / 10_000_000) ** 0.5)
        lo, hi = pts.min(0), pts.max(0)
        q = (lo + synth.uniform01_f32(5, 3 * Q).reshape(Q, 3) * (hi - lo)).astype(np.float32)
        tq = torch.from_numpy(q).to(dev)
        cs = torch.cuda.current_stream().cuda_stream
        with E.Cloud(len(pts)) as c:
            c.set_input(pts)
            c.build_grid()
            c.reserve_queries(Q)
            info = dict(cloud=name, points=len(pts), queries=Q, grid=c.grid_info()["dims"], pyramid_levels=c.pyramid_info()["levels"])
            oi = torch.empty(Q, dtype=torch.int32, device=dev)
            od = torch.empty(Q, dtype=torch.float64, device=dev)
            nn_ms, nn_lo, nn_hi = timed(c, lambda: c.nn_device(tq.data_ptr(), Q, oi.data_ptr(), od.data_ptr(), cs, E.ALGO_GRID), a.batches)
            print(json.dumps(dict(info, kernel="pct_nn_batch_dev", kernel_ms_median=nn_ms, kernel_ms_min=nn_lo, kernel_ms_max=nn_hi,
                                  queries_per_s=Q / nn_ms * 1e3)), flush=True)
            nn_idx, nn_d2 = oi.cpu().numpy().view(np.uint32), od.cpu().numpy()
            for k in KS:
                ki = torch.empty((Q, k), dtype=torch.int32, device=dev)
                kd = torch.empty((Q, k), dtype=torch.float64, device=dev)
                run = lambda: c.knn_device(tq.data_ptr(), Q, k, ki.data_ptr(), kd.data_ptr(), cs, E.ALGO_GRID)
                ms, lo_ms, hi_ms = timed(c, run, a.batches)
                c.set_work_counters(True)
                run()
                torch.cuda.synchronize()
                points, runs = c.last_work()
                c.set_work_counters(False)
                row = dict(info, kernel="knn_grid_kernel", k=k, kernel_ms_median=ms, kernel_ms_min=lo_ms, kernel_ms_max=hi_ms,
                           queries_per_s=Q / ms * 1e3, points_scanned_per_query=points / Q, cell_runs_per_query=runs / Q,
                           ratio_to_nn_kernel=ms / nn_ms)
                if k == 1:
                    row["equals_nn_batch"] = bool(np.array_equal(ki.cpu().numpy().view(np.uint32)[:, 0], nn_idx) and
                                                  np.array_equal(kd.cpu().numpy()[:, 0], nn_d2))
                print(json.dumps(row), flush=True)
                del ki, kd
            if a.stream_queries > 0:
                sq = min(a.stream_queries, Q)
                for k in KS:
                    ki = torch.empty((sq, k), dtype=torch.int32, device=dev)
                    kd = torch.empty((sq, k), dtype=torch.float64, device=dev)
                    ms, lo_ms, hi_ms = timed(c, lambda: c.knn_device(tq.data_ptr(), sq, k, ki.data_ptr(), kd.data_ptr(), cs, E.ALGO_STREAM), 3)
                    print(json.dumps(dict(info, kernel="knn_stream_kernel+knn_merge_kernel", k=k, queries=sq, kernel_ms_median=ms, kernel_ms_min=lo_ms,
                                          kernel_ms_max=hi_ms, queries_per_s=sq / ms * 1e3, pairs_per_s=sq * len(pts) / ms * 1e3)), flush=True)
        del tq


if __name__ == "__main__":
    main()
