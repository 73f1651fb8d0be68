"""Range images on the rolling map (pct_cloud_ring_carve_range, pct_cloud_append_range) beside depth images, timed on config C5's
window: one JSON line, also written to --out when given.

Window: --window points (5 M) fed in --frame-point frames (50 k), the rolling-map index live and the ring wrapped.  A 64 x 1024
full-circle lidar and a 640 x 480 z-depth camera stand at the drone.  Host wall time of the whole call, ended by pct_sync (launches,
the host waits, bookkeeping), --reps calls of each kind, the kinds taken in turn; reported as [min, median, max] in milliseconds:
  * range_carve_pass_ms  ring_carve_range with a scan that shows a return at near_range (5 cm) everywhere: the full pass over the
                         window (12 B per slot, the projection with its two table searches, one gather from the image), nothing
                         removed, so it can be repeated;
  * depth_carve_pass_ms  ring_carve_depth with an image that shows a surface 5 cm in front of the camera, on the same window;
  * range_append_ms      append_range of a scan with ranges in [2, 30]: 65 536 valid pixels un-projected on the device;
  * depth_append_ms      append_depth of an image with depths in [2, 30]: 307 200 valid pixels;
  * range_carve_6m_ms    one real carve by a scan that shows returns 6 m out (the points it removes are reported).
The table placement (plain loads against a copy in LDS) hangs on range_carve_pass_ms against twice depth_carve_pass_ms.
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--window", type=int, default=S.C5_WINDOW)
    ap.add_argument("--frame", type=int, default=S.C5_FRAME)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rings", type=int, default=64)
    ap.add_argument("--columns", type=int, default=1024)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    E.init(0)
    c = E.Cloud(a.window)
    c.ring_index()
    nframes = a.window // a.frame + 12
    for k in range(nframes):
        c.append(S.c5_frame(k, a.frame))
    E.sync()
    drone = (0.1 * (nframes - 1), 0.0, 2.5)
    scan = E.range_view_uniform(drone, np.eye(3), 0.0, 2.0 * np.pi, -0.4, 0.4, a.columns, a.rings)
    cam = E.depth_view(drone, S.RGBD_R, 640, 480, fov_hor_deg=90.0)
    near_scan = np.full((a.rings, a.columns), 0.05, np.float32)      # = near_range: no point in the image is nearer than this
    near_cam = np.full((480, 640), 0.05, np.float32)
    out = dict(window=a.window, frame=a.frame, scan=[a.rings, a.columns], image=[640, 480], reps=a.reps, live_before=c.ring_live()[0],
               tables="plain loads (L2)")
    for _ in range(3):                                    # warm-up: code objects, the staging buffers
        c.ring_carve_range(scan, near_scan, 0.0)
        c.ring_carve_depth(cam, near_cam, 0.0)
    rc, dc = [], []
    for _ in range(a.reps):
        ms, n = wall_ms(lambda: c.ring_carve_range(scan, near_scan, 0.0))
        assert n == 0
        rc.append(ms)
        ms, n = wall_ms(lambda: c.ring_carve_depth(cam, near_cam, 0.0))
        assert n == 0
        dc.append(ms)
    out.update(range_carve_pass_ms=spread(rc), depth_carve_pass_ms=spread(dc))
    rng = np.random.default_rng(5)
    scan_img = rng.uniform(2.0, 30.0, (a.rings, a.columns)).astype(np.float32)
    cam_img = rng.uniform(2.0, 30.0, (480, 640)).astype(np.float32)
    for _ in range(2):
        c.append_range(scan, scan_img)
        c.append_depth(cam, cam_img)
    E.sync()
    ra, da = [], []
    for _ in range(a.reps):
        ms, (offered, kept) = wall_ms(lambda: c.append_range(scan, scan_img))
        assert offered == kept == scan_img.size
        ra.append(ms)
        ms, (offered, kept) = wall_ms(lambda: c.append_depth(cam, cam_img))
        assert offered == kept == cam_img.size
        da.append(ms)
    out.update(range_append_ms=spread(ra), depth_append_ms=spread(da), range_appended=int(scan_img.size), depth_appended=int(cam_img.size))
    ms, n = wall_ms(lambda: c.ring_carve_range(scan, np.full((a.rings, a.columns), 6.0, np.float32), 1.0e-3))
    out.update(range_carve_6m_ms=round(ms, 4), range_carve_6m_removed=n, live_after=c.ring_live()[0])
    c.close()
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
