"""Corridor generation on the ROLLING map, timed: scenarios.run_rolling_commit_scenario at the reference's scale (12 m sensing
radius, a window of 80 000 points, 1500 Expansion + 400 Refine iterations, five commits), speculation 64 and 256.

Three ways to feed the same frames, alternating in ONE process (one warm-up pass, then 5 repetitions each, interleaved):
  fused    rolling map, appendInput, one launch per speculative batch (rrt_expand_kernel<true>)
  staged   rolling map, appendInput, setFusedExpansion(False): three launches + three round trips per batch -- what a ring-indexed
           cloud got before the fused step could search the rolling-map index
  static   no rolling map: setInput of the whole window per frame with a cell-index rebuild -- how a caller had to feed frames before
           the finder took them
Prints ONE JSON line: per feed and speculation the per-phase milliseconds (medians), median / min / max of the total, fused launches
in the first Expansion and overall, milliseconds per appendInput; and scenarios.timed_scenario (config C1, static cloud) on the same
machine for scale."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pointcloudtraj_amd import corridor, engine, scenarios

RADIUS, WINDOW, EXPAND, REFINE, REPS = 12.0, 80000, 1500, 400, 5


class Counting:
    """the finder, plus the number of fused launches its first Expansion made"""

    def __init__(self, finder):
        self._f = finder
        self.first_expansion_launches = 0

    def __getattr__(self, name):
        return getattr(self._f, name)

    def SafeRegionExpansion(self, n):
        r = self._f.SafeRegionExpansion(n)
        self.first_expansion_launches = self._f.expansionLaunches()
        return r


def one_run(feed, speculation):
    f = corridor.SafeRegionRrtStar(WINDOW)
    if feed != "static":
        f.enableRollingMap()
    f.setSpeculation(speculation)
    f.setFusedExpansion(feed != "staged")
    w = Counting(f)
    clock, info = [], {}
    phases = scenarios.run_rolling_commit_scenario(w, WINDOW, expand=EXPAND, refine=REFINE, radius=RADIUS,
                                                   feed="replace" if feed == "static" else "append", info=info, clock=clock)
    ms = {}
    for name, sec in clock:
        ms[name] = ms.get(name, 0.0) + 1e3 * sec
    feeds = [1e3 * sec for name, sec in clock if name in ("append", "set_input")]
    out = dict(phase_ms=ms, total_ms=sum(ms.values()), feed_ms_each=statistics.median(feeds), launches_first_expansion=w.first_expansion_launches,
               launches=f.expansionLaunches(), repair_batches=f.repairBatches(), phases=len(phases), frames=info["frames"],
               final=phases[-1][2])
    f.close()
    return out


def summarise(runs):
    tot = [r["total_ms"] for r in runs]
    names = sorted(runs[0]["phase_ms"])
    return dict(total_ms_median=round(statistics.median(tot), 3), total_ms_min=round(min(tot), 3), total_ms_max=round(max(tot), 3),
                phase_ms_median={n: round(statistics.median(r["phase_ms"][n] for r in runs), 3) for n in names},
                feed_ms_each_median=round(statistics.median(r["feed_ms_each"] for r in runs), 4),
                launches_first_expansion=runs[0]["launches_first_expansion"], launches=runs[0]["launches"],
                repair_batches=runs[0]["repair_batches"])


def main():
    engine.init(0)
    feeds = ("fused", "staged", "static")
    res = dict(probe="corridor_rolling", radius=RADIUS, window=WINDOW, expand=EXPAND, refine=REFINE, reps=REPS, by_speculation={})
    for K in (64, 256):
        runs = {fd: [] for fd in feeds}
        shape = None
        for rep in range(REPS + 1):                       # pass 0 warms up (allocations, code objects) and is dropped
            for fd in feeds:
                r = one_run(fd, K)
                key = (r["phases"], tuple(r["frames"]), json.dumps(r["final"], sort_keys=True))
                shape = shape or key
                assert key == shape, f"{fd}: a different corridor ({key} vs {shape})"        # every feed computes the same thing
                if rep:
                    runs[fd].append(r)
        res["by_speculation"][str(K)] = {fd: summarise(runs[fd]) for fd in feeds}
        res["frames"], res["phases"] = list(shape[1]), shape[0]
    c1 = []
    cloud1 = scenarios.sensed_cloud(12.0)
    for rep in range(4):
        f = corridor.SafeRegionRrtStar(80000)
        f.setSpeculation(64)
        t = scenarios.timed_scenario(f, cloud1)
        f.close()
        if rep:
            c1.append(t["total_ms"])
    res["c1_static_timed_scenario_total_ms"] = dict(median=round(statistics.median(c1), 3), min=round(min(c1), 3), max=round(max(c1), 3))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
