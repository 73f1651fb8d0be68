"""Workload definitions shared by tests, probes and bench.py (no oracle, no GPU code).

Config C1 corridor scenario: the clean_demo map (seed 6), start
(-10,-10,2) -> goal (9,9,2), clean_demo.launch planner constants, fixed iteration counts instead of wall-clock
limits, and a second, denser cloud for the lazy re-evaluation."""
import numpy as np

from . import synth

START, GOAL = (-10.0, -10.0, 2.0), (9.0, 9.0, 2.0)
BOUNDS = (-15.0, 15.0, -15.0, 15.0, 0.0, 4.0)
PARAMS = dict(safety_margin=0.6, search_margin=0.25, max_radius=1.5, sensing_range=30.0, max_samples=200000,
              sample_portion=0.3, goal_portion=0.1)


def sensed_cloud(radius=12.0):
    """what a 12 m sensor at the start pose has seen of the seed-6 map (shuffled, as a stream of frames would be)"""
    full = synth.pillar_map()
    crop = synth.crop_ball(full, START, radius)
    return crop[synth.shuffled_order(7, len(crop))]


def perturbed_cloud(cloud1, path):
    """a later sensor frame: the same cloud plus three new obstacle points just above the corridor's 10th, 13th and
    15th spheres -- their radii shrink (1.5 -> 1.2 / 1.3 / 1.45) but the chain stays connected and flyable"""
    extra = [path[min(k, len(path) - 1)] + np.float64([0.0, 0.0, dz]) for k, dz in ((9, 1.45), (12, 1.55), (14, 1.7))]
    return np.concatenate([cloud1, np.asarray(extra, np.float32)])


def run_scenario(finder, cloud1, cloud2=None, expand=1500, refine=400):
    """returns the (Path, Radius, status) after each planner phase; cloud2=None derives the second frame
    from the corridor found in the first phases (perturbed_cloud)"""
    p = PARAMS
    out = []
    finder.setParam(p["safety_margin"], p["search_margin"], p["max_radius"], p["sensing_range"])
    finder.setInput(cloud1)
    finder.reset()
    finder.setPt(START, GOAL, *BOUNDS, p["sensing_range"], p["max_samples"], p["sample_portion"], p["goal_portion"])
    finder.SafeRegionExpansion(expand)                 # planInitialTraj, sim_planning_demo.cpp:344-350
    out.append((*finder.getPath(), finder.status()))
    finder.SafeRegionRefine(refine)                    # planIncrementalTraj, :412
    out.append((*finder.getPath(), finder.status()))
    if cloud2 is None:
        cloud2 = perturbed_cloud(cloud1, out[-1][0])
    finder.setInput(cloud2)                            # a new sensor frame arrives (rcvPointCloudCallBack, :159-167)
    finder.SafeRegionEvaluate()                        # :413
    out.append((*finder.getPath(), finder.status()))
    finder.SafeRegionRefine(refine // 2)
    out.append((*finder.getPath(), finder.status()))
    return out


def run_commit_scenario(finder, cloud1, expand=800, refine=300, commits=3):
    """planIncrementalTraj's flow (sim_planning_demo.cpp:393-460): after the first corridor the drone commits to a point on it,
    the finder moves its root there (resetRoot), refines, and re-evaluates against the next frame -- `commits` times.  The commit
    target is the centre of the corridor's third sphere (inside the root-side spheres, as the committed trajectory end is)."""
    p = PARAMS
    out = []
    finder.setParam(p["safety_margin"], p["search_margin"], p["max_radius"], p["sensing_range"])
    finder.setInput(cloud1)
    finder.reset()
    finder.setPt(START, GOAL, *BOUNDS, p["sensing_range"], p["max_samples"], p["sample_portion"], p["goal_portion"])
    finder.SafeRegionExpansion(expand)
    finder.SafeRegionRefine(refine)
    out.append((*finder.getPath(), finder.status()))
    cloud = cloud1
    for k in range(commits):
        path, _ = finder.getPath()
        if not finder.status()["path_exists"] or len(path) < 4:
            break
        target = tuple(float(v) for v in path[2])
        finder.setStartPt(target, GOAL)
        finder.resetRoot(target)
        out.append((*finder.getPath(), finder.status()))       # the path is only re-traced by the next phase; the status moves now
        finder.SafeRegionRefine(refine // 2)
        out.append((*finder.getPath(), finder.status()))
        cloud = perturbed_cloud(cloud, finder.getPath()[0])
        finder.setInput(cloud)
        finder.SafeRegionEvaluate()
        out.append((*finder.getPath(), finder.status()))
    return out


class RingMirror:
    """host copy of a rolling window: the slot discipline of pct_cloud_append_aos (the newest frame overwrites the oldest slots,
    index of a point = its slot)"""

    def __init__(self, cap):
        self.cap, self.count, self.nxt, self.passed = int(cap), 0, 0, 0
        self.xyz = np.zeros((self.cap, 3), np.float32)

    def append(self, f):
        idx = (self.nxt + np.arange(len(f))) % self.cap
        self.xyz[idx] = f
        self.nxt = (self.nxt + len(f)) % self.cap
        self.count = min(self.cap, self.count + len(f))
        self.passed += len(f)

    def live(self):
        return self.xyz[:self.count]


def rolling_frame(full, centre, seed, radius=8.0):
    """what a `radius` m sensor at `centre` sees of the map `full`, in the shuffled order a stream of returns has"""
    crop = synth.crop_ball(full, centre, radius)
    return crop[synth.shuffled_order(seed, len(crop))]


def run_rolling_commit_scenario(finder, window=40000, expand=800, refine=300, commits=5, radius=8.0, feed="append", info=None, clock=None):
    """The planner's tick on a ROLLING map (rcvPointCloudCallBack -> SafeRegionEvaluate + SafeRegionRefine,
    sim_planning_demo.cpp:159-178, 381-422, with the frame appended to a window of `window` points instead of replacing the cloud):
    first frame = the seed-6 map within `radius` of START (order seed 7), Expansion + Refine; then `commits` times: commit to the
    centre of the corridor's third sphere (setStartPt, resetRoot, Refine(refine / 2)), sense the map within `radius` of that point
    (order seed 8 + k), append the frame, Evaluate, Refine(refine / 2).  Returns (Path, Radius, status) after every phase.

    `finder` is any object with the finder's method names.  feed = "append": one with appendInput gets the frames (the caller has
    enabled its rolling map); one without (the CPU oracle) gets setInput of a host mirror of the window.  feed = "replace": setInput
    of the mirror either way.  info (a dict, optional) receives the frame sizes, the points that passed through the window and
    whether it wrapped; clock (a list, optional) receives (phase name, seconds) per call into the finder."""
    import time
    p = PARAMS
    out = []
    full = synth.pillar_map()
    mirror = RingMirror(window)
    appends = feed == "append" and hasattr(finder, "appendInput")
    sizes = []

    def timed(name, fn, *a):
        t0 = time.perf_counter()
        fn(*a)
        if clock is not None:
            clock.append((name, time.perf_counter() - t0))

    def feed_frame(frame):
        sizes.append(len(frame))
        mirror.append(frame)
        if appends:
            timed("append", finder.appendInput, frame)
        else:
            timed("set_input", finder.setInput, mirror.live())

    def snap():
        out.append((*finder.getPath(), finder.status()))

    finder.setParam(p["safety_margin"], p["search_margin"], p["max_radius"], p["sensing_range"])
    feed_frame(rolling_frame(full, START, 7, radius))
    finder.reset()
    finder.setPt(START, GOAL, *BOUNDS, p["sensing_range"], p["max_samples"], p["sample_portion"], p["goal_portion"])
    timed("expansion", finder.SafeRegionExpansion, expand)
    snap()
    timed("refine", finder.SafeRegionRefine, refine)
    snap()
    for k in range(commits):
        path, _ = finder.getPath()
        if not finder.status()["path_exists"] or len(path) < 4:
            break
        target = tuple(float(v) for v in path[2])
        finder.setStartPt(target, GOAL)
        finder.resetRoot(target)
        timed("refine", finder.SafeRegionRefine, refine // 2)
        snap()
        feed_frame(rolling_frame(full, target, 8 + k, radius))
        timed("evaluate", finder.SafeRegionEvaluate)
        snap()
        timed("refine", finder.SafeRegionRefine, refine // 2)
        snap()
    if info is not None:
        info.update(frames=sizes, passed=mirror.passed, wrapped=mirror.passed > mirror.cap, window=mirror.live().copy())
    return out


def run_lidar_window_scenario(finder, window=40000, expand=800, refine=300, commits=5, radius=8.0, info=None, clock=None):
    """The planner's tick in the reference's LIDAR mode: every frame the planner's cloud is crop(global map, drone, max_dist)
    (camera_sensor.cpp:133-145), handed to setInput as a replacement (sim_planning_demo.cpp:159-167), so points that leave the
    sensing range vanish.  Same phases, frames and commit points as run_rolling_commit_scenario.

    A finder with forgetOutside (its rolling map enabled by the caller, with setRollingDedup on) keeps a window instead: per frame
    appendInput(frame) -> forgetOutside(sensor position, radius) -> Evaluate -> Refine -- the window then holds that frame's points
    without being replaced.  A finder without it (the CPU oracle) gets setInput(frame): the reference's lidar mode itself.
    info (a dict, optional) receives the frame sizes and the points forgotten per frame; clock as in run_rolling_commit_scenario."""
    import time
    p = PARAMS
    out = []
    full = synth.pillar_map()
    rolling = hasattr(finder, "forgetOutside")
    sizes, forgotten = [], []

    def timed(name, fn, *a):
        t0 = time.perf_counter()
        r = fn(*a)
        if clock is not None:
            clock.append((name, time.perf_counter() - t0))
        return r

    def feed_frame(centre, seed):
        frame = rolling_frame(full, centre, seed, radius)
        sizes.append(len(frame))
        if rolling:
            timed("append", finder.appendInput, frame)
            forgotten.append(timed("forget", finder.forgetOutside, centre, radius))
        else:
            timed("set_input", finder.setInput, frame)

    def snap():
        out.append((*finder.getPath(), finder.status()))

    finder.setParam(p["safety_margin"], p["search_margin"], p["max_radius"], p["sensing_range"])
    feed_frame(START, 7)
    finder.reset()
    finder.setPt(START, GOAL, *BOUNDS, p["sensing_range"], p["max_samples"], p["sample_portion"], p["goal_portion"])
    timed("expansion", finder.SafeRegionExpansion, expand)
    snap()
    timed("refine", finder.SafeRegionRefine, refine)
    snap()
    for k in range(commits):
        path, _ = finder.getPath()
        if not finder.status()["path_exists"] or len(path) < 4:
            break
        target = tuple(float(v) for v in path[2])
        finder.setStartPt(target, GOAL)
        finder.resetRoot(target)
        timed("refine", finder.SafeRegionRefine, refine // 2)
        snap()
        feed_frame(target, 8 + k)
        timed("evaluate", finder.SafeRegionEvaluate)
        snap()
        timed("refine", finder.SafeRegionRefine, refine // 2)
        snap()
    if info is not None:
        info.update(frames=sizes, forgotten=forgotten)
    return out


# ---- the rgbd window: a camera at the origin looking along +x, a back wall, and an obstacle that leaves ---------------------------
RGBD = dict(width=64, height=48, fov_hor_deg=90.0, wall_x=8.0, wall_size=(16.0, 12.0), obstacle_x=5.0, obstacle_size=2.0, lattice=0.1,
            obstacle_frames=3, cap=40000, res=0.1, margin=1.0e-3, extent=(10.0, 18.0, 14.0))
# camera axes in world, one per column: image right = -y, image down = -z, optical axis = +x
RGBD_R = ((0.0, 0.0, 1.0), (-1.0, 0.0, 0.0), (0.0, -1.0, 0.0))


def rgbd_view():
    """the scenario's pct_depth_view (engine.DepthView), metric Z"""
    from . import engine
    return engine.depth_view((0.0, 0.0, 0.0), RGBD_R, RGBD["width"], RGBD["height"], fov_hor_deg=RGBD["fov_hor_deg"])


def _lattice(x, size_y, size_z, step):
    ny, nz = int(round(size_y / step)), int(round(size_z / step))
    y = (np.arange(ny + 1) - ny / 2.0) * step
    z = (np.arange(nz + 1) - nz / 2.0) * step
    yy, zz = np.meshgrid(y, z, indexing="ij")
    return np.stack([np.full(yy.size, x), yy.ravel(), zz.ravel()], axis=1).astype(np.float32)


def rgbd_wall():
    """the back wall: a 0.1 m lattice at x = 8 covering the frustum, 16 m x 12 m"""
    return _lattice(RGBD["wall_x"], *RGBD["wall_size"], RGBD["lattice"])


def rgbd_obstacle():
    """the obstacle: a 2 m x 2 m lattice at x = 5, centred on the optical axis"""
    return _lattice(RGBD["obstacle_x"], RGBD["obstacle_size"], RGBD["obstacle_size"], RGBD["lattice"])


def rgbd_scene(frame):
    """the world at frame `frame`: the wall, and the obstacle while it is there (frames 0 to 2)"""
    return np.concatenate([rgbd_wall(), rgbd_obstacle()]) if frame < RGBD["obstacle_frames"] else rgbd_wall()


def run_rgbd_window_scenario(window, render, frames=6, carve=True, images=None, each=None):
    """The reference's rgbd mode on a window that is never replaced: every frame the sensor hands over a depth image of the scene
    (render(view, points) -> float32 [height, width], +inf where nothing is seen: a test-side renderer, the library renders
    nothing), and the window takes it as clearSeenThrough(view, image, margin) then appendDepthImage(view, image) with de-dup on --
    carve first, then append.  `window` is a SafeRegionRrtStar with its rolling map and setRollingDedup on, or anything with the
    same two members and live_set().  carve = False leaves the carve out: the window then keeps the obstacle after it has left.
    Returns the live set (a set of (x, y, z) tuples) after every frame; `images` (a list, optional) receives the images; `each`
    (optional) is called as each(frame index, window) after every frame."""
    view = rgbd_view()
    out = []
    for k in range(frames):
        image = render(view, rgbd_scene(k))
        if images is not None:
            images.append(image)
        if carve:
            window.clearSeenThrough(view, image, RGBD["margin"])
        window.appendDepthImage(view, image, float("inf"))
        if hasattr(window, "live_set"):
            out.append(window.live_set())
        else:
            _, _, xyz = window.cloud().radius_crop((0.0, 0.0, 0.0), 1.0e4)
            out.append(set(map(tuple, xyz.tolist())))
        if each is not None:
            each(k, window)
    return out


# ---- the same window seen by a lidar: a 90 degree sector scan of the wall and of the obstacle that leaves ---------------------------
# sensor axes = world axes (x azimuth 0, y azimuth +90 degrees, z up); the sector starts at azimuth -45 degrees, which
# engine.range_view_uniform folds into the view's R so that azimuth 0 is the sector's lower edge, not inside its span
LIDAR_SCAN = dict(width=64, height=48, az_start_deg=-45.0, az_span_deg=90.0, el_lo_deg=-33.0, el_hi_deg=33.0, near_range=0.05)


def lidar_range_view():
    """the scenario's pct_range_view (engine.RangeView) with its four tables"""
    from . import engine
    g = LIDAR_SCAN
    rad = np.pi / 180.0
    return engine.range_view_uniform((0.0, 0.0, 0.0), np.eye(3), g["az_start_deg"] * rad, g["az_span_deg"] * rad, g["el_lo_deg"] * rad,
                                     g["el_hi_deg"] * rad, g["width"], g["height"], g["near_range"])


def run_lidar_range_window_scenario(window, render, frames=6, carve=True, images=None, each=None):
    """run_rgbd_window_scenario with a lidar for a sensor: every frame the sensor hands over a range image of the same scene
    (render(view, points) -> float32 [height, width], the nearest return per beam cell, +inf where none: a test-side renderer), and
    the window takes it as clearSeenThroughRange(view, image, margin) then appendRangeImage(view, image) with de-dup on -- carve
    first, then append.  `window` is a SafeRegionRrtStar with its rolling map and setRollingDedup on, or anything with the same two
    members and live_set().  Returns the live set after every frame, as run_rgbd_window_scenario does."""
    view = lidar_range_view()
    out = []
    for k in range(frames):
        image = render(view, rgbd_scene(k))
        if images is not None:
            images.append(image)
        if carve:
            window.clearSeenThroughRange(view, image, RGBD["margin"])
        window.appendRangeImage(view, image, float("inf"))
        if hasattr(window, "live_set"):
            out.append(window.live_set())
        else:
            _, _, xyz = window.cloud().radius_crop((0.0, 0.0, 0.0), 1.0e4)
            out.append(set(map(tuple, xyz.tolist())))
        if each is not None:
            each(k, window)
    return out


# ---- the rgbd window with a noisy sensor: speckle pixels in free space, withdrawn by the radius rule in the frame that brought them ----
# Every frame `speckles` pixels of the image read `depth` metres in front of the wall instead of what is there.  The pixels come from a
# fixed list -- a lattice with a pitch of 8 pixels that starts 4 pixels off the border, walked with a stride coprime to its length -- so
# no pixel is used twice, any two are at least 8 pixels apart and no library's random numbers are involved.  A wall point (0.25 m a
# pixel at 8 m) or an obstacle point (0.16 m a pixel at 5 m) has at least 2 other points within 0.3 m, also beside a speckle's hole;
# a speckle point has none (the next one is 8 pixels = 1.5 m away, the obstacle 1 m, the wall 2 m): r = 0.3, min_neighbours = 2.
RGBD_SPECKLE = dict(speckles=4, depth=2.0, r=0.3, min_neighbours=2, pitch=8, border=4, stride=11)


def rgbd_speckle_pixels(frame, speckles=None):
    """the (column, row) pixels that frame `frame` corrupts"""
    k = RGBD_SPECKLE["speckles"] if speckles is None else int(speckles)
    pitch, border = RGBD_SPECKLE["pitch"], RGBD_SPECKLE["border"]
    nu = (RGBD["width"] - 2 * border - 1) // pitch + 1
    nv = (RGBD["height"] - 2 * border - 1) // pitch + 1
    if (frame + 1) * k > nu * nv:
        raise ValueError("the speckle list has no unused pixel left for this frame")
    cells = [(RGBD_SPECKLE["stride"] * j) % (nu * nv) for j in range(frame * k, (frame + 1) * k)]
    return [(border + pitch * (c % nu), border + pitch * (c // nu)) for c in cells]


def rgbd_pixel_point(view, u, v, dep):
    """the fp32 point pixel (u, v) holding `dep` un-projects to (include/pct_engine.h, paragraph "Depth images"), operation by operation"""
    t, Rm = np.array(list(view.t), np.float64), np.array(list(view.R), np.float64).reshape(3, 3)
    w, h, focal, dep = np.float64(view.width), np.float64(view.height), np.float64(view.focal), np.float64(np.float32(dep))
    a = (np.float64(u) / w - 0.5) / focal
    b = (np.float64(v) - 0.5 * h) / w / focal
    return np.array([t[k] + dep * ((a * Rm[k, 0] + b * Rm[k, 1]) + Rm[k, 2]) for k in range(3)], np.float64).astype(np.float32)


def run_rgbd_speckle_scenario(window, render, frames=6, filter=True, speckles=None, r=None, min_neighbours=None, images=None, each=None):
    """run_rgbd_window_scenario with a noisy sensor: the tick is clearSeenThrough -> appendDepthImage -> removeOutliers(r,
    min_neighbours, newest = the points the append kept), de-dup on.  filter = False leaves the last step out: the window then holds
    every speckle until a later image sees through it.  `window` is a SafeRegionRrtStar with its rolling map and setRollingDedup on,
    or anything with the same three members and live_set().  Returns the live set after every frame; `images` (a list, optional)
    receives the corrupted images; each(frame index, window, dict(speckle = that frame's speckle points fp32 [k, 3], kept, removed))
    is called after every frame."""
    view = rgbd_view()
    r = RGBD_SPECKLE["r"] if r is None else r
    m = RGBD_SPECKLE["min_neighbours"] if min_neighbours is None else min_neighbours
    dep = np.float32(RGBD["wall_x"] - RGBD_SPECKLE["depth"])
    out = []
    for k in range(frames):
        image = np.array(render(view, rgbd_scene(k)), np.float32)
        pix = rgbd_speckle_pixels(k, speckles)
        for u, v in pix:
            image[v, u] = dep
        if images is not None:
            images.append(image)
        window.clearSeenThrough(view, image, RGBD["margin"])
        kept = window.appendDepthImage(view, image, float("inf"))
        removed = window.removeOutliers(r, m, kept) if filter and kept > 0 else 0
        if hasattr(window, "live_set"):
            out.append(window.live_set())
        else:
            _, _, xyz = window.cloud().radius_crop((0.0, 0.0, 0.0), 1.0e4)
            out.append(set(map(tuple, xyz.tolist())))
        if each is not None:
            each(k, window, dict(speckle=np.stack([rgbd_pixel_point(view, u, v, dep) for u, v in pix]), kept=kept, removed=removed))
    return out


def run_rgbd_speckle_scenario_statistical(window, render, frames=6, k=4, stddev_mult=3.0, speckles=None, images=None, each=None):
    """run_rgbd_speckle_scenario with the statistical rule in place of the radius rule.  With de-dup on, the rows a frame keeps from
    the second frame on are almost only its speckles, whose own statistics condemn nothing, so the threshold is taken once and used
    from then on: frame 0 calls removeStatisticalOutliers(k, stddev_mult, 0) over the whole window and keeps its threshold, every
    later frame calls removeIsolated(k, threshold, newest = the points the append kept).  `window` is a SafeRegionRrtStar with its
    rolling map and setRollingDedup on, or anything with the same four members and live_set().  Returns the live set after every
    frame; each(frame index, window, dict(speckle, kept, removed, threshold, stats = frame 0's statistics or None)) is called after
    every frame."""
    view = rgbd_view()
    dep = np.float32(RGBD["wall_x"] - RGBD_SPECKLE["depth"])
    out = []
    threshold = float("inf")
    for f in range(frames):
        image = np.array(render(view, rgbd_scene(f)), np.float32)
        pix = rgbd_speckle_pixels(f, speckles)
        for u, v in pix:
            image[v, u] = dep
        if images is not None:
            images.append(image)
        window.clearSeenThrough(view, image, RGBD["margin"])
        kept = window.appendDepthImage(view, image, float("inf"))
        stats = None
        if f == 0:
            removed, stats = window.removeStatisticalOutliers(k, stddev_mult, 0)
            threshold = stats["threshold"]
        else:
            removed = window.removeIsolated(k, threshold, kept) if kept > 0 else 0
        if hasattr(window, "live_set"):
            out.append(window.live_set())
        else:
            _, _, xyz = window.cloud().radius_crop((0.0, 0.0, 0.0), 1.0e4)
            out.append(set(map(tuple, xyz.tolist())))
        if each is not None:
            each(f, window, dict(speckle=np.stack([rgbd_pixel_point(view, u, v, dep) for u, v in pix]), kept=kept, removed=removed,
                                 threshold=threshold, stats=stats))
    return out


# ---- the rgbd window with a partial view: a camera that pans round a room whose obstacles come and go --------------------------------
# A camera at the origin turns by 90 degrees per frame (four headings a lap, fov 90: the views tile the circle) inside a square room
# with walls 6 m away.  In every heading a 4 m x 4 m obstacle stands 4 m away during the even laps, a little further along the wall
# each time, and is gone during the odd laps: every lap the carve withdraws what left and the append files what is new, so the
# number of points ever filed grows while the number of live points does not.  `cap` is deliberately small: it holds the live points
# and one image, not what a window that never reclaims removed slots needs -- such a window evicts live wall points BEHIND the camera,
# which the partial view does not sense again until the camera has come round.
RGBD_PAN = dict(width=32, height=24, fov_hor_deg=90.0, wall_x=6.0, wall_size=(16.0, 12.0), obstacle_x=4.0, obstacle_size=4.0, shift=0.7,
                lattice=0.1, laps=6, cap=5000, big_cap=12000, fraction=0.05, res=0.1, margin=1.0e-3, extent=(14.0, 14.0, 14.0))


def rgbd_pan_view(heading):
    """the pct_depth_view (engine.DepthView) of heading 0..3: the optical axis turned by heading * 90 degrees about z, metric Z"""
    from . import engine
    c, s = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))[heading % 4]
    Rm = ((s, 0.0, c), (-c, 0.0, s), (0.0, -1.0, 0.0))          # columns: image right, image down, optical axis
    return engine.depth_view((0.0, 0.0, 0.0), Rm, RGBD_PAN["width"], RGBD_PAN["height"], fov_hor_deg=RGBD_PAN["fov_hor_deg"])


def rgbd_pan_scene(frame):
    """what the camera of frame `frame` can see: the wall of its heading and, during the even laps, that lap's obstacle in front"""
    heading, lap = frame % 4, frame // 4
    pts = _lattice(RGBD_PAN["wall_x"], *RGBD_PAN["wall_size"], RGBD_PAN["lattice"])
    if lap % 2 == 0:
        ob = _lattice(RGBD_PAN["obstacle_x"], RGBD_PAN["obstacle_size"], RGBD_PAN["obstacle_size"], RGBD_PAN["lattice"])
        ob[:, 1] += np.float32(RGBD_PAN["shift"] * (lap // 2) - 1.0)
        pts = np.concatenate([pts, ob])
    c, s = ((1, 0), (0, 1), (-1, 0), (0, -1))[heading]
    return np.stack([c * pts[:, 0] - s * pts[:, 1], s * pts[:, 0] + c * pts[:, 1], pts[:, 2]], axis=1).astype(np.float32)


def run_rgbd_pan_scenario(window, render, laps=None, images=None, each=None):
    """The rgbd tick -- clearSeenThrough(view, image, margin) then appendDepthImage(view, image), de-dup on -- for the panning camera
    above, on whatever window the caller configured: small or large, with setRollingCompact (autocompact) on or off.  `window` has
    the two camelCase members and live_set() (the numpy models), or is a SafeRegionRrtStar.  Returns the live set after every
    frame; `images` (a list, optional) receives (view, image) per frame; each(frame index, window) is called after every frame."""
    out = []
    for k in range(4 * (RGBD_PAN["laps"] if laps is None else laps)):
        view = rgbd_pan_view(k % 4)
        image = render(view, rgbd_pan_scene(k))
        if images is not None:
            images.append((view, image))
        window.clearSeenThrough(view, image, RGBD_PAN["margin"])
        window.appendDepthImage(view, image, float("inf"))
        if hasattr(window, "live_set"):
            out.append(window.live_set())
        else:
            _, _, xyz = window.cloud().radius_crop((0.0, 0.0, 0.0), 1.0e4)
            out.append(set(map(tuple, xyz.tolist())))
        if each is not None:
            each(k, window)
    return out


def timed_scenario(finder, cloud1, expand=1500, refine=400):
    """run_scenario with wall-clock milliseconds per planner phase (bench.py / scripts/probe_corridor.py)"""
    import time
    p = PARAMS
    t = [time.perf_counter()]
    finder.setParam(p["safety_margin"], p["search_margin"], p["max_radius"], p["sensing_range"])
    finder.setInput(cloud1); t.append(time.perf_counter())
    finder.reset()
    finder.setPt(START, GOAL, *BOUNDS, p["sensing_range"], p["max_samples"], p["sample_portion"], p["goal_portion"])
    finder.SafeRegionExpansion(expand); t.append(time.perf_counter())
    finder.SafeRegionRefine(refine); t.append(time.perf_counter())
    path, _ = finder.getPath()
    cloud2 = perturbed_cloud(cloud1, path)
    t.append(time.perf_counter())
    finder.setInput(cloud2); t.append(time.perf_counter())
    finder.SafeRegionEvaluate(); t.append(time.perf_counter())
    finder.SafeRegionRefine(refine // 2); t.append(time.perf_counter())
    d = [1e3 * (b - a) for a, b in zip(t[:-1], t[1:])]
    out = {"set_input_ms": d[0], "expansion_ms": d[1], "refine_ms": d[2], "set_input_2_ms": d[4], "evaluate_ms": d[5], "refine_2_ms": d[6]}
    out["total_ms"] = sum(out.values())
    out["status"] = finder.status()
    out["path_len"] = len(finder.getPath()[0])
    return out


# ---- config C5: rolling window fed one sensor frame per tick ------------------------------------------
C5_WINDOW, C5_FRAME = 5_000_000, 50_000
C5_NODES, C5_SEGMENTS, C5_ORDER = 64, 3, 6
C5_PARAMS = dict(sample_range=30.0, search_margin=0.25, max_radius=1.5)


def c5_frame(k, frame=C5_FRAME, tunnel=0.0, step=0.1):
    """sensor frame k: `frame` points uniform in a 60 m cube around a drone moving +`step` m per frame along x (seed 8),
    flattened to a 6 m slab above the ground (|z| * 0.2).  tunnel > 0 (test variant): points closer than `tunnel` to the
    flight axis (y = 0, z = 2.5) are moved sideways by 2 * tunnel, so the corridor ahead of the drone is free space and the
    inflation radii are not all negative."""
    p = synth.uniform_points(8, frame, -30.0, 30.0, offset=k * frame)
    p[:, 0] += np.float32(step * k)
    p[:, 2] = np.abs(p[:, 2]) * np.float32(0.2)
    if tunnel > 0:
        near = np.hypot(p[:, 1], p[:, 2] - np.float32(2.5)) < tunnel
        p[near, 1] += np.where(p[near, 1] >= 0, np.float32(2 * tunnel), np.float32(-2 * tunnel))
    return p


def c5_frame_clustered(k, frame=C5_FRAME, step=0.1):
    """sensor frame k of config C5's CLUSTERED variant (points on 0.1-grid pillar surfaces, as map_generator.cpp makes them): the
    same window around the same moving drone, but every point lies on a face of a square pillar -- pillars on a 3 m lattice, 0.6-1.4 m wide by
    a hash of their lattice cell, 0-6 m tall -- snapped to the 0.1 m lattice.  Frames re-sense the same surface points again and again (exact
    duplicates across frames, as the reference's rgbd mode accumulates them, camera_sensor.cpp:160-166); the corridor along the flight
    axis holds no pillar."""
    u = synth.uniform01_f32(8, 3 * frame, offset=3 * k * frame).reshape(frame, 3).astype(np.float64)
    v = synth.uniform01_f32(18, 2 * frame, offset=2 * k * frame).reshape(frame, 2).astype(np.float64)
    x0 = step * k
    px, py = u[:, 0] * 60.0 - 30.0 + x0, u[:, 1] * 60.0 - 30.0
    ci, cj = np.floor(px / 3.0), np.floor(py / 3.0)                       # the pillar's lattice cell
    cj = np.where(np.abs(cj * 3.0 + 1.5) <= 1.5, cj + np.where(py >= 0, 1.0, -1.0), cj)     # the two rows beside the flight axis move out: |y| < 3.8 m stays free
    hsh = (ci.astype(np.int64) * 73856093) ^ (cj.astype(np.int64) * 19349663)
    w = 0.6 + 0.1 * ((hsh >> 3) & 7).astype(np.float64)                   # 0.6 .. 1.3 m
    cx, cy = ci * 3.0 + 1.5, cj * 3.0 + 1.5
    face = (u[:, 2] * 4.0).astype(np.int64) & 3
    along = (v[:, 0] - 0.5) * w
    x = np.where(face == 0, cx - w / 2, np.where(face == 1, cx + w / 2, cx + along))
    y = np.where(face == 2, cy - w / 2, np.where(face == 3, cy + w / 2, cy + along))
    z = v[:, 1] * 6.0
    p = np.stack([x, y, z], 1)
    return (np.round(p * 10.0) / 10.0).astype(np.float32)


def c5_tick_queries(k):
    """what tick k asks of the cloud: the drone's pose, 64 corridor-node centres ahead of it (seed 9) and the committed
    trajectory -- 3 segments of order 6, 1 s each, control points jittered by +-0.3 m (seed 9) around a straight 12 m run;
    returns (start, nodes f64 [64,3], polycoef f64 [3,21] (control points / T as the optimizer stores them), seg_time, orders)"""
    x0 = 0.1 * k
    nodes = (synth.uniform_points(9, C5_NODES, -1.0, 1.0, offset=k * C5_NODES).astype(np.float64) * [8.0, 3.0, 1.0] + [x0 + 6.0, 0.0, 2.5])
    m = C5_ORDER + 1
    seg_time = np.ones(C5_SEGMENTS)
    orders = np.full(C5_SEGMENTS, C5_ORDER, np.int32)
    coef = np.zeros((C5_SEGMENTS, 3 * m))
    ctrl = synth.uniform_points(9, C5_SEGMENTS * m, -0.3, 0.3, offset=1_000_000 + k * C5_SEGMENTS * m).astype(np.float64)
    for sgm in range(C5_SEGMENTS):
        for d in range(3):
            for j in range(m):
                w = (sgm + j / float(C5_ORDER)) / C5_SEGMENTS
                base = [x0 + 12.0 * w, 0.0, 2.5][d]
                coef[sgm, d * m + j] = (base + (ctrl[sgm * m + j, d] if 0 < j < C5_ORDER else 0.0)) / seg_time[sgm]
    return (x0, 0.0, 2.5), nodes, coef, seg_time, orders
