"""Create / use / destroy every kind of handle repeatedly and watch the library's own count of live buffers
(pct_debug_live_buffers): device, pinned and host-mapped blocks, and their bytes."""
import os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pointcloudtraj_amd import engine as E, synth, voxel, kdtree as K, corridor, scenarios
E.init(0)
pts = synth.uniform_points(1, 300_000, 0, 50)
q = synth.uniform_points(2, 20_000, 0, 50)
cloud1 = scenarios.sensed_cloud(12.0)
prm = E.inflate_params((25, 25, 25), 100.0, 0.25, 1.5)
def once():
    c = E.Cloud(len(pts)); c.set_input(pts); c.nn(q[:100], E.ALGO_STREAM); c.build_grid(); c.nn(q, E.ALGO_GRID)
    c.radius_count(q[:500], np.float32(1.0)); c.radius_crop([25, 25, 25], 5.0)
    c.inflate(prm, q[:64].astype(np.float64))
    plan = E.NNPlan(c, 64, E.ALGO_GRID); plan.run(q[:64]); plan.close()
    o = E.Cloud(len(pts)); c.crop_to([25, 25, 25], 8.0, o); o.close(); c.close()
    v = voxel.VoxelMap(0.1, 1000); v.add_point_cloud(pts); v.close()
    t = K.KDTree(); t.insert(pts[:3000]); t.nearest(q[:5]); t.range_ids(q[0], 2.0); t.close()
    f = corridor.SafeRegionRrtStar(80000); scenarios.timed_scenario(f, cloud1); f.close() if hasattr(f, "close") else None
def rolling():
    """the rolling map: ring index, de-duplicating appends, a removal, a depth carve and append, a replan plan"""
    r = E.Cloud(60_000); r.ring_index(0.5, (50.0, 50.0, 50.0)); r.ring_dedup(0.1)
    for k in range(3):
        r.append(pts[20_000 * k:20_000 * (k + 1)])
    r.ring_remove_ball((25, 25, 25), 5.0)
    view = E.depth_view((25, 25, 25), np.eye(3), 160, 120, fov_hor_deg=90.0)
    img = np.full((120, 160), 12.0, np.float32)
    r.ring_carve_depth(view, img, 0.05); r.append_depth(view, img)
    plan = E.ReplanPlan(r, 64, 256, 4); plan.run(prm, q[:64].astype(np.float64)); plan.close()
    r.nn(q[:1000]); r.close()
once(); rolling(); E.sync()
blocks0, bytes0 = E.live_buffers()
for i in range(40):
    once(); rolling()
E.sync()
blocks1, bytes1 = E.live_buffers()
print(f"live before {blocks0} blocks / {bytes0/2**20:.1f} MiB, after 40 more rounds {blocks1} blocks / {bytes1/2**20:.1f} MiB, "
      f"delta {blocks1-blocks0} blocks / {(bytes1-bytes0)/2**20:.2f} MiB")
sys.exit(0 if (blocks1, bytes1) == (blocks0, bytes0) else 1)
