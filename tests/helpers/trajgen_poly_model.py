"""numpy restatement of the trajectory generator in polyhedra (include/pct_trajgen.h, the paragraph "Trajectory generation in
polyhedra"), built on trajgen_model.py: the problem, the iteration, the rho rule and the stop test are that module's solve(), run
here on a Problem whose set is a list of half-spaces per segment instead of a ball.  What is restated here is what the header
adds: the normalisation of the planes, the pinned projection (v itself; active sets of one, two, three planes in ascending order;
the fallback) with its two constants, the corridor slack, and what makes a candidate invalid.  Also the case table the CPU and GPU
tests share and the text form tests/host/trajgen_poly_check.cpp reads."""
import math

import numpy as np

import trajgen_model as M

OK, NOT_CONVERGED, INVALID = M.OK, M.NOT_CONVERGED, M.INVALID
MAX_PLANES = 24
ACCEPT = 1e-9          # a candidate may stand this far outside a plane that is not in its active set
DET_MIN = 1e-8         # Gram determinants below this: near-parallel, skipped
GEN_RESULT_DTYPE = M.GEN_RESULT_DTYPE
params = M.params
rest = M.rest


def pdot(n, y):
    """nh . y in the header's order; n is [..., 3] (or [3]), y is [3] or [..., 3]"""
    return (n[..., 0] * y[..., 0] + n[..., 1] * y[..., 1]) + n[..., 2] * y[..., 2]


class Polytope:
    """The normalised planes of one segment and what the enumeration needs of them, computed once: the pairs and triples that are
    not skipped, in the pinned order, with their Gram entries."""

    def __init__(self, planes, margin):
        p = np.asarray(planes, np.float64).reshape(-1, 4)
        self.cnt = len(p)
        ln = np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2])
        self.len = ln
        with np.errstate(all="ignore"):
            self.nh = p[:, :3] / ln[:, None]
            self.o = p[:, 3] / ln - margin
        c = self.cnt
        I, J = np.triu_indices(c, 1) if c else (np.zeros(0, int), np.zeros(0, int))      # i outer, j inner, ascending
        with np.errstate(all="ignore"):
            a = pdot(self.nh[I], self.nh[J]) if c else np.zeros(0)
        keep = (1.0 - a * a) >= DET_MIN
        self.pI, self.pJ, self.pA = I[keep], J[keep], a[keep]
        self.pDet = 1.0 - self.pA * self.pA
        ti, tj, tk, ta = [], [], [], []
        for i, j, aa in zip(self.pI, self.pJ, self.pA):
            k = np.arange(j + 1, c)
            ti.append(np.full(len(k), i)); tj.append(np.full(len(k), j)); tk.append(k); ta.append(np.full(len(k), aa))
        cat = lambda v, dt: np.concatenate(v).astype(dt) if v else np.zeros(0, dt)
        ti, tj, tk, ta = cat(ti, int), cat(tj, int), cat(tk, int), cat(ta, np.float64)
        with np.errstate(all="ignore"):
            b, cc = pdot(self.nh[ti], self.nh[tk]), pdot(self.nh[tj], self.nh[tk])
            det = ((1.0 + 2.0 * ((ta * b) * cc)) - (ta * ta + b * b)) - cc * cc
        keep = det >= DET_MIN
        self.tI, self.tJ, self.tK, self.tA, self.tB, self.tC, self.tDet = ti[keep], tj[keep], tk[keep], ta[keep], b[keep], cc[keep], det[keep]

    def viol(self, y, two_eps):
        return pdot(self.nh, np.asarray(y, np.float64)) - (self.o - two_eps)

    def project(self, v, two_eps, stage=None):
        """the pinned projection of one point.  stage (a list, optional) receives 0 = inside, 1 / 2 / 3 = the size of the accepted
        active set, -1 = the fallback."""
        v = np.asarray(v, np.float64)
        g = self.viol(v, two_eps)
        if not np.any(g > 0.0):
            if stage is not None:
                stage.append(0)
            return v.copy()
        nh = self.nh
        best, z = math.inf, v.copy()

        def worst(y, skip):
            gy = self.viol(y, two_eps)
            gy[list(skip)] = -math.inf
            return float(np.max(gy))

        for i in range(self.cnt):
            if not g[i] >= 0.0:
                continue
            y = v - g[i] * nh[i]
            w = worst(y, (i,))
            if w < best - ACCEPT:
                best, z = w, y
                if w <= ACCEPT:
                    if stage is not None:
                        stage.append(1)
                    return z
        if len(self.pI):
            I, J, a, det = self.pI, self.pJ, self.pA, self.pDet
            li, lj = (g[I] - a * g[J]) / det, (g[J] - a * g[I]) / det
            for e in np.nonzero((li >= 0.0) & (lj >= 0.0))[0]:
                y = (v - li[e] * nh[I[e]]) - lj[e] * nh[J[e]]
                w = worst(y, (I[e], J[e]))
                if w < best - ACCEPT:
                    best, z = w, y
                    if w <= ACCEPT:
                        if stage is not None:
                            stage.append(2)
                        return z
        if len(self.tI):
            I, J, K, a, b, c, det = self.tI, self.tJ, self.tK, self.tA, self.tB, self.tC, self.tDet
            gi, gj, gk = g[I], g[J], g[K]
            li = (((1.0 - c * c) * gi + (b * c - a) * gj) + (a * c - b) * gk) / det
            lj = (((b * c - a) * gi + (1.0 - b * b) * gj) + (a * b - c) * gk) / det
            lk = (((a * c - b) * gi + (a * b - c) * gj) + (1.0 - a * a) * gk) / det
            for e in np.nonzero((li >= 0.0) & (lj >= 0.0) & (lk >= 0.0))[0]:
                y = ((v - li[e] * nh[I[e]]) - lj[e] * nh[J[e]]) - lk[e] * nh[K[e]]
                w = worst(y, (I[e], J[e], K[e]))
                if w < best - ACCEPT:
                    best, z = w, y
                    if w <= ACCEPT:
                        if stage is not None:
                            stage.append(3)
                        return z
        if stage is not None:
            stage.append(-1)
        return z


class PolyProblem(M.Problem):
    """trajgen_model.Problem with polytopes for balls: `c` (the start iterate) holds the anchors, project_ball and measures are the
    polytope's.  planes: one [k, 4] array per segment."""

    def __init__(self, anchors, planes, seg_time, orders, start, end, prm, stages=None):
        self.planes = [np.asarray(p, np.float64).reshape(-1, 4) for p in planes]
        self.stages = stages
        self.poly = None
        m = len(np.asarray(seg_time).reshape(-1))
        super().__init__(anchors, np.zeros(m), seg_time, orders, start, end, prm)
        if self.valid:
            self.two_eps = 2.0 * prm["eps"]

    def _valid(self):
        p = self.prm
        if not (1 <= self.m <= M.MAX_SEG) or len(self.planes) != self.m:
            return False
        if not (np.all(np.isfinite(self.c)) and np.all(np.isfinite(self.T)) and np.all(np.isfinite(self.start)) and np.all(np.isfinite(self.end))):
            return False
        if np.any(self.T <= 0) or np.any(self.n < M.MIN_ORDER) or np.any(self.n > M.MAX_ORDER) or np.any(self.n - 2 < p["minimize_order"]):
            return False
        if any(len(q) > MAX_PLANES for q in self.planes):
            return False
        self.poly = [Polytope(q, p["margin"]) for q in self.planes]
        for q, poly in zip(self.planes, self.poly):
            if not (np.all(np.isfinite(poly.len)) and np.all(poly.len > 0.0) and np.all(np.isfinite(q[:, 3]))):
                return False
        return True

    def project_ball(self, v):
        out = np.empty_like(v)
        for r in range(len(v)):
            out[r] = self.poly[self.seg_of[r]].project(v[r], self.two_eps, self.stages)
        return out

    def slack(self, x):
        s = math.inf
        for r in range(len(x)):
            poly = self.poly[self.seg_of[r]]
            if poly.cnt:
                s = min(s, float(np.min(poly.o - pdot(poly.nh, x[r]))))
        return s

    def measures(self, x):
        cost = 0.5 * float(np.sum(x * (self.P @ x)))
        vmax = float(np.max(np.abs(self.D1 @ x) * self.fv[:, None]))
        amax = float(np.max(np.abs(self.D2 @ x) * self.fa[:, None]))
        return cost, self.slack(x), vmax, amax


def solve(anchors, planes, seg_time, orders, start, end, prm, row_stride=39, force_iterations=None, trace=None, stages=None):
    """One candidate, by trajgen_model.solve on a PolyProblem (that function builds its Problem by name; the name is pointed at the
    polytope problem for the length of the call).  Returns (rows, record as a dict, x or None)."""
    keep = M.Problem
    M.Problem = lambda c, r, T, od, s, e, p: PolyProblem(c, planes, T, od, s, e, p, stages)
    try:
        return M.solve(anchors, None, seg_time, orders, start, end, prm, row_stride, force_iterations, trace)
    finally:
        M.Problem = keep


def run_case(case, **kw):
    return solve(case["anchors"], case["planes"], case["seg_time"], case["orders"], case["start"], case["end"], case["prm"], **kw)


def problem(case, prm=None):
    return PolyProblem(case["anchors"], case["planes"], case["seg_time"], case["orders"], case["start"], case["end"], prm or case["prm"])


# ---------------------------------------------------------------------------------------------------------------------------------
# polytopes and the shared case table

def box_planes(lo, hi):
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    out = []
    for a in range(3):
        n = np.zeros(3); n[a] = 1.0
        out.append(np.concatenate([n, [hi[a]]]))
        out.append(np.concatenate([-n, [-lo[a]]]))
    return np.array(out)


def tube_planes(p0, p1, half, extra=0, cut=None, seed=0):
    """a box of half width `half` around the edge p0 -> p1 (reaching `half` past its ends), in the edge's own frame, and `extra`
    planes tangent to the capsule of radius `cut` around the edge, with normals of random direction and length"""
    p0, p1 = np.asarray(p0, np.float64), np.asarray(p1, np.float64)
    d = p1 - p0
    L = float(np.linalg.norm(d))
    d = d / L
    h = np.array([0.0, 0.0, 1.0]) if abs(d[2]) < 0.9 else np.array([1.0, 0.0, 0.0])
    e1 = np.cross(d, h); e1 /= np.linalg.norm(e1)
    e2 = np.cross(d, e1)
    mid = 0.5 * (p0 + p1)
    out = []
    for n, reach in ((d, L / 2 + half), (-d, L / 2 + half), (e1, half), (-e1, half), (e2, half), (-e2, half)):
        out.append(np.concatenate([n, [float(n @ mid) + reach]]))
    rng = np.random.default_rng(seed)
    for _ in range(extra):
        n = rng.normal(0, 1, 3)
        n /= np.linalg.norm(n)
        off = float(n @ mid) + abs(float(n @ d)) * L / 2 + cut
        f = rng.uniform(0.2, 5.0)
        out.append(np.concatenate([n * f, [off * f]]))
    return np.array(out)


def capsule_box(a, b, reach):
    """six planes of a box inside the capsule (segment a -> b, reach): half width reach / sqrt(3) across the segment, the same past
    its ends, so that its farthest corners are `reach` from the segment -- what turns a row of supports into a bounded polytope"""
    return tube_planes(a, b, reach / math.sqrt(3.0))


def route_polytopes(waypoints, support_offsets, support_planes, reach, margin):
    """the polytopes of a route's edges from the rows of a segment-polyhedron query over them (offsets [m + 1], planes [total, 4]):
    every support plane moved in by `margin`, then the box.  An empty list for an edge whose nearest support is within `margin`
    cannot be told from the planes alone, so the caller passes the rows' d2 where it matters (pillar_world does)."""
    w = np.asarray(waypoints, np.float64).reshape(-1, 3)
    out = []
    for i in range(len(w) - 1):
        sup = np.asarray(support_planes, np.float64).reshape(-1, 4)[support_offsets[i]:support_offsets[i + 1]].copy()
        sup[:, 3] -= margin
        out.append(np.concatenate([sup, capsule_box(w[i], w[i + 1], reach)]))
    return out


def pillar_world():
    """two pillars (3 x 3 points on a 0.1 m lattice, 3 m tall: 558 points) whose faces stand 1.0 m to either side of a three-edge
    route, and a second route whose middle edge passes the first pillar at 0.15 m.  Returns (cloud float32 [558, 3], route, grazing
    route, reach, margin)."""
    pts = []
    for cx, cy in ((1.5, 1.1), (3.0, -1.1)):
        for ix in (-1, 0, 1):
            for iy in (-1, 0, 1):
                for iz in range(31):
                    pts.append((cx + ix * 0.1, cy + iy * 0.1, iz * 0.1))
    route = np.array([[0, 0, 1.5], [1.5, 0, 1.5], [3.0, 0, 1.5], [4.5, 0, 1.5]], np.float64)
    graze = np.array([[0, 0, 1.5], [1.5, 0.85, 1.5], [3.0, 0.85, 1.5], [4.5, 0, 1.5]], np.float64)
    return np.array(pts, np.float32), route, graze, 1.5, 0.2


def route_case(waypoints, planes, seg_time, order, start=None, end=None, prm=None):
    w = np.asarray(waypoints, np.float64).reshape(-1, 3)
    m = len(w) - 1
    return dict(anchors=0.5 * (w[:-1] + w[1:]), planes=[np.asarray(p, np.float64).reshape(-1, 4) for p in planes],
                seg_time=np.asarray(seg_time, np.float64), orders=np.full(m, order, np.int32) if np.isscalar(order) else np.asarray(order, np.int32),
                start=rest(w[0]) if start is None else np.asarray(start, np.float64), end=rest(w[-1]) if end is None else np.asarray(end, np.float64),
                prm=prm or params())


def sixteen_route(seed=4):
    """17 waypoints on the random walk of trajgen_model.generator_corridor, 16 edges of order 12, 24 planes on every one"""
    c, _, _, _ = M.generator_corridor(seed, 17)
    planes = [tube_planes(c[i], c[i + 1], 0.8, extra=18, cut=1.0, seed=100 * seed + i) for i in range(16)]
    T = np.array([max(float(np.linalg.norm(c[i + 1] - c[i])), 0.5) for i in range(16)])
    return route_case(c, planes, T, 12)


def cases():
    """name -> dict(anchors, planes, seg_time, orders, start, end, prm); every one is solved to OK well inside its max_iter.  A
    single quintic is fixed by its end states, so its plane can only be inactive; the single segments with active planes have order 7."""
    out = {}
    out["quintic_plane"] = dict(anchors=np.array([[0.0, 0, 0]]), planes=[np.array([[0.0, 3.0, 0, 3.0]])], seg_time=np.array([2.0]), orders=np.array([5], np.int32),
                                start=np.array([-1, 0.5, 0, 0.3, 0.2, 0, 0, 0, 0.1]), end=np.array([1.5, -0.5, 0.4, 0, 0.1, 0, 0.05, 0, 0]), prm=params())
    # one segment, one active plane: the start velocity carries the two free control points to y = 1.057, past the plane y = 1.02
    out["face"] = dict(anchors=np.array([[0.2, 0.5, 0]]), planes=[np.array([[0.0, 2.0, 0, 2.04]])], seg_time=np.array([2.0]), orders=np.array([7], np.int32),
                       start=np.array([0, 0, 0, 0.3, 1.5, 0, 0, 0, 0]), end=rest([0.5, 1.0, 0]), prm=params())
    # two edges at a right angle, boxes of half width 0.5: the joint wants to cut the corner and ends on y = 0.5 of the first box and
    # x = 1.5 of the second
    out["bend"] = route_case([[0, 0, 0], [2, 0, 0], [2, 2, 0]], [box_planes([-0.5, -0.5, -0.5], [2.5, 0.5, 0.5]), box_planes([1.5, -0.5, -0.5], [2.5, 2.5, 0.5])],
                             [1.5, 1.5], 7)
    # everything on the diagonal: the start velocity carries the two free control points to 1.057 on every axis, past the corner
    # (1.02, 1.02, 1.02) of the box
    out["vertex"] = dict(anchors=np.array([[0.5, 0.5, 0.5]]), planes=[box_planes([-1, -1, -1], [1.02, 1.02, 1.02])], seg_time=np.array([2.0]), orders=np.array([7], np.int32),
                         start=np.array([0, 0, 0, 1.5, 1.5, 1.5, 0, 0, 0]), end=rest([1.0, 1.0, 1.0]), prm=params())
    # no plane at all on the first segment, far planes on the second: the KKT solution
    c = np.array([[0.0, 0, 0], [2.0, 0.3, 0.1], [4.0, 1.2, 0.2]])
    out["free2"] = route_case(c, [np.zeros((0, 4)), box_planes([-50, -50, -50], [50, 50, 50])], [1.0, 1.6], 7, start=rest(c[0] + [-0.5, 0.2, 0]), end=rest(c[-1] + [0.4, 0, 0.1]))
    return out


def invalid_cases():
    base = cases()["bend"]
    many = dict(base, planes=[tube_planes([0, 0, 0], [2, 0, 0], 0.5, extra=19, cut=0.8, seed=1), base["planes"][1]])
    zero = dict(base, planes=[base["planes"][0], np.vstack([base["planes"][1], [[0.0, 0.0, 0.0, 1.0]]])])
    return dict(planes25=many, zero_norm=zero)


def quintic_touch_case():
    """m = 1, order 5, one ACTIVE plane.  A single quintic is fixed by its end states (its largest y is 0.66, at the third control
    point), so a plane can be active only by passing within 2 eps of a control point: y <= 0.66 + 5e-6 leaves that point inside the
    plane (slack 5e-6) and 1.5e-5 outside the shrunk one, the projection moves z off x on every iteration, and the candidate ends
    PCT_GEN_NOT_CONVERGED with r_prim = 1.5e-5 > eps = 1e-5."""
    return dict(cases()["quintic_plane"], planes=[np.array([[0.0, 1.0, 0.0, 0.66 + 5e-6]])])


def empty_case():
    """x <= -1 and x >= 1 on the second segment: no point satisfies both"""
    base = cases()["bend"]
    return dict(base, planes=[base["planes"][0], np.array([[1.0, 0, 0, -1.0], [-1.0, 0, 0, -1.0], [0, 1.0, 0, 2.5]])])


# ---------------------------------------------------------------------------------------------------------------------------------
# batches

def pack(cands):
    """a list of case dicts -> the arrays of a pct_trajgen_poly_batch"""
    nseg = [len(np.asarray(c["seg_time"]).reshape(-1)) for c in cands]
    offs = np.zeros(len(cands) + 1, np.int32)
    offs[1:] = np.cumsum(nseg)
    cat = lambda key, dt, w: (np.concatenate([np.asarray(c[key], dt).reshape(-1, w) for c in cands]) if cands else np.zeros((0, w), dt))
    per_seg = [np.asarray(p, np.float64).reshape(-1, 4) for c in cands for p in c["planes"]]
    po = np.zeros(len(per_seg) + 1, np.int32)
    po[1:] = np.cumsum([len(p) for p in per_seg])
    planes = np.concatenate(per_seg) if per_seg else np.zeros((0, 4))
    return dict(anchors=np.ascontiguousarray(cat("anchors", np.float64, 3)), planes=np.ascontiguousarray(planes), plane_offsets=po,
                seg_time=np.ascontiguousarray(cat("seg_time", np.float64, 1).reshape(-1)), orders=np.ascontiguousarray(cat("orders", np.int32, 1).reshape(-1)),
                seg_offsets=offs, start_state=np.ascontiguousarray(cat("start", np.float64, 9)), end_state=np.ascontiguousarray(cat("end", np.float64, 9)))


def solve_batch(cands, prm, row_stride=39, force_iterations=None, stages=None):
    res = np.zeros(len(cands), GEN_RESULT_DTYPE)
    rows = []
    for b, c in enumerate(cands):
        fi = None if force_iterations is None else int(force_iterations[b])
        r, rec, _ = solve(c["anchors"], c["planes"], c["seg_time"], c["orders"], c["start"], c["end"], prm, row_stride, force_iterations=fi, stages=stages)
        rows.append(r)
        for name in GEN_RESULT_DTYPE.names:
            res[b][name] = rec[name]
    return (np.concatenate(rows) if rows else np.zeros((0, row_stride))), res


def write_batch_text(path, cands, prm, row_stride):
    a = pack(cands)
    with open(path, "w") as f:
        f.write(f"{len(cands)} {len(a['seg_time'])} {len(a['planes'])} {row_stride}\n")
        f.write(f"{prm['minimize_order']} {prm['max_iter']} {prm['check_every']} " + " ".join(repr(float(prm[k])) for k in ("max_vel", "max_acc", "margin", "eps", "rho")) + "\n")
        for key in ("seg_offsets", "orders", "plane_offsets"):
            f.write(" ".join(str(int(v)) for v in a[key]) + "\n")
        for key in ("seg_time", "anchors", "planes", "start_state", "end_state"):
            f.write(" ".join(repr(float(v)) for v in a[key].reshape(-1)) + "\n")


read_result_text = M.read_result_text
