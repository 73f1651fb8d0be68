"""Trajectory generation (pct_bezier_generate_batch): the time of one batch of 256 candidates, one JSON line per segment count.

Candidates: 256 different corridors of --segments spheres each (8 and 13 by default) from the generator of the tests
(tests/helpers/trajgen_model.py: a random walk of overlapping spheres, radii 0.6..1.4), order 7, minimum jerk, no limits unless
--max-vel is given, eps 1e-5, automatic rho, at most --max-iter iterations.  The host form is timed on the host's clock around the whole
call (copies in, one launch, copies out, one wait): after one warm-up call, --reps calls; the median, minimum and maximum are printed
with the statuses and the iterations the candidates took.  The launch is as long as its slowest candidate.
--scipy N: instead, the time scipy's SLSQP takes on the first N of those corridors, one at a time on the CPU, for scale (no GPU needed)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import numpy as np

import trajgen_model as M

B = 256


def corridors(m, count=B):
    out = []
    for seed in range(count):
        c, r, T, od = M.generator_corridor(1000 + seed, m)
        out.append(dict(centres=c, radius=r, seg_time=T, orders=od, start=M.rest(c[0]), end=M.rest(c[-1])))
    return out


def slsqp_seconds(cand, prm):
    from scipy.optimize import minimize
    pb = M.Problem(cand["centres"], cand["radius"], cand["seg_time"], cand["orders"], cand["start"], cand["end"], prm)
    N, I3 = pb.N, np.eye(3)
    c, rr = pb.c[pb.seg_of], (pb.r - prm["margin"])[pb.seg_of]
    X = lambda v: v.reshape(N, 3)
    JE = np.kron(pb.E, I3)

    def ball_jac(v):
        J = np.zeros((N, 3 * N))
        d = -2.0 * (X(v) - c)
        for i in range(N):
            J[i, 3 * i:3 * i + 3] = d[i]
        return J
    cons = [dict(type="eq", fun=lambda v: (pb.E @ X(v) - pb.b).ravel(), jac=lambda v: JE),
            dict(type="ineq", fun=lambda v: rr * rr - np.sum((X(v) - c) ** 2, axis=1), jac=ball_jac)]
    t0 = time.perf_counter()
    r = minimize(lambda v: 0.5 * np.sum(X(v) * (pb.Q @ X(v))), c.ravel(), jac=lambda v: (pb.Q @ X(v)).ravel(), constraints=cons, method="SLSQP",
                 options=dict(maxiter=2000, ftol=1e-14))
    return time.perf_counter() - t0, bool(r.success), int(r.nit)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", default="8,13")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-iter", type=int, default=20000)
    ap.add_argument("--max-vel", type=float, default=0.0)
    ap.add_argument("--scipy", type=int, default=0)
    a = ap.parse_args()
    prm = M.params(max_iter=a.max_iter, max_vel=a.max_vel)
    for m in [int(v) for v in a.segments.split(",")]:
        if a.scipy:
            runs = [slsqp_seconds(c, prm) for c in corridors(m, a.scipy)]
            print(json.dumps(dict(solver="scipy SLSQP, one problem at a time, CPU", segments=m, problems=a.scipy,
                                  seconds=[round(s, 3) for s, _, _ in runs], success=[ok for _, ok, _ in runs], iterations=[n for _, _, n in runs])), flush=True)
            continue
        from pointcloudtraj_amd import engine as E
        E.init(0)
        packed = E.pack_corridors(corridors(m))
        p = E.gen_params(**prm)
        E.bezier_generate(packed, p, 24)
        ms = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            _, res = E.bezier_generate(packed, p, 24)
            ms.append((time.perf_counter() - t0) * 1e3)
        it = np.sort(res["iterations"])
        print(json.dumps(dict(candidates=B, segments=m, order=7, minimize_order=3, eps=prm["eps"], max_vel=a.max_vel, reps=a.reps,
                              batch_ms=dict(median=round(statistics.median(ms), 3), min=round(min(ms), 3), max=round(max(ms), 3)),
                              ok=int(np.sum(res["status"] == E.GEN_OK)), not_converged=int(np.sum(res["status"] == E.GEN_NOT_CONVERGED)),
                              invalid=int(np.sum(res["status"] == E.GEN_INVALID)),
                              iterations=dict(min=int(it[0]), median=int(it[len(it) // 2]), max=int(it[-1])),
                              us_per_iteration_of_the_slowest=round(statistics.median(ms) * 1e3 / int(it[-1]), 3))), flush=True)


if __name__ == "__main__":
    main()
