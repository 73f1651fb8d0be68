"""Depth images on the rolling map (pct_cloud_ring_carve_depth, pct_cloud_append_depth), timed on config C5's window: one JSON line.

Window: --window points (5 M) fed in --frame-point frames (50 k), the rolling-map index live and the ring wrapped.  A 640 x 480
z-depth camera stands at the drone and looks along +x.  Host wall time of the whole call, ended by pct_sync (launches, the host
waits, bookkeeping), --reps calls of each kind, the kinds taken in turn; reported as [min, median, max] in milliseconds:
  * carve_pass_ms        ring_carve_depth with an image that shows a surface 5 cm in front of the camera: the full pass over the
                         window (12 B per slot, the projection, one gather from the image), nothing removed, so it can be repeated;
  * remove_ball_pass_ms  ring_remove_ball with r = 0 on the same window: the one-pass removal this one is built beside, nothing removed;
  * carve_6m_ms          one real carve by an image that shows a surface 6 m out (the points it removes are reported);
  * append_depth_ms      append_depth of an image with depths in [2, 30]: 307 200 valid pixels un-projected on the device;
  * append_points_ms     append of the same points from host memory (3.7 MB across the bus).
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
    E.sync()
    return 1e3 * (time.perf_counter() - t0), out


def spread(ms):
    return [round(min(ms), 4), round(statistics.median(ms), 4), round(max(ms), 4)]


def unprojected(view, image):
    """the points pct_cloud_append_depth files for a z-depth image without invalid pixels (pct_engine.h, "Depth images")"""
    h, w = image.shape
    t, R = np.array(list(view.t)), np.array(list(view.R)).reshape(3, 3)
    y, x = np.divmod(np.arange(h * w), w)
    a = (x / np.float64(w) - 0.5) / view.focal
    b = (y - 0.5 * h) / np.float64(w) / view.focal
    dep = image.reshape(-1).astype(np.float64)
    return np.stack([t[k] + dep * ((a * R[k, 0] + b * R[k, 1]) + R[k, 2]) for k in range(3)], axis=1).astype(np.float32)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--window", type=int, default=S.C5_WINDOW)
    ap.add_argument("--frame", type=int, default=S.C5_FRAME)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    a = ap.parse_args()
    E.init(0)
    c = E.Cloud(a.window)
    c.ring_index()
    nframes = a.window // a.frame + 12
    for k in range(nframes):
        c.append(S.c5_frame(k, a.frame))
    E.sync()
    drone = (0.1 * (nframes - 1), 0.0, 2.5)
    view = E.depth_view(drone, S.RGBD_R, a.width, a.height, fov_hor_deg=90.0)
    near = np.full((a.height, a.width), 0.05, np.float32)
    out = dict(window=a.window, frame=a.frame, image=[a.width, a.height], reps=a.reps, live_before=c.ring_live()[0])
    for _ in range(3):                                    # warm-up: code objects, the staging buffers
        c.ring_carve_depth(view, near, 0.0)
        c.ring_remove_ball(drone, 0.0)
    carve, ball = [], []
    for _ in range(a.reps):
        ms, n = wall_ms(lambda: c.ring_carve_depth(view, near, 0.0))
        assert n == 0
        carve.append(ms)
        ms, n = wall_ms(lambda: c.ring_remove_ball(drone, 0.0))
        ball.append(ms)
    out.update(carve_pass_ms=spread(carve), remove_ball_pass_ms=spread(ball))
    ms, n = wall_ms(lambda: c.ring_carve_depth(view, np.full((a.height, a.width), 6.0, np.float32), 1.0e-3))
    out.update(carve_6m_ms=round(ms, 4), carve_6m_removed=n, live_after=c.ring_live()[0])
    rng = np.random.default_rng(5)
    image = rng.uniform(2.0, 30.0, (a.height, a.width)).astype(np.float32)
    pts = unprojected(view, image)
    for _ in range(2):
        c.append_depth(view, image)
        c.append(pts)
    E.sync()
    dep, host = [], []
    for _ in range(a.reps):
        ms, (offered, kept) = wall_ms(lambda: c.append_depth(view, image))
        assert offered == kept == len(pts)
        dep.append(ms)
        host.append(wall_ms(lambda: c.append(pts))[0])
    out.update(append_depth_ms=spread(dep), append_points_ms=spread(host), appended=len(pts))
    i, d = c.nn(pts[:: len(pts) // 64])
    assert np.all(d == 0.0)                               # the un-projected points are in the window, bit for bit
    c.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
