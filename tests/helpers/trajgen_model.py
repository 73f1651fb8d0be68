"""numpy restatement of the trajectory generator (include/pct_trajgen.h, the paragraph "Trajectory generation"): the problem, the
ADMM iteration, the rho rule, the check cadence, the stop test and the shrunk projection radius, as the header states them -- with
dense matrices and LAPACK solves where the kernel runs block Cholesky factors in LDS.  Also the case table the CPU and GPU tests
share, and the direct restatement of the reference's time allocation."""
import math

import numpy as np

OK, NOT_CONVERGED, INVALID = 0, 1, 2
MIN_ORDER, MAX_ORDER, MAX_SEG = 5, 12, 16
ALPHA = 1.6                       # over-relaxation
RHO_AUTO = 1e-5                   # start of the automatic rho, relative to max|P| = 1
RHO_MIN, RHO_MAX = 1e-9, 1e3
RHO_STEP = 5.0                    # rho moves only when the rule asks for more than this factor, either way

GEN_RESULT_DTYPE = np.dtype([("status", np.int32), ("iterations", np.int32), ("cost", np.float64), ("duration", np.float64),
                             ("r_prim", np.float64), ("r_dual", np.float64), ("sphere_slack", np.float64),
                             ("max_vel_ctrl", np.float64), ("max_acc_ctrl", np.float64)])


def params(minimize_order=3, max_iter=4000, check_every=25, max_vel=0.0, max_acc=0.0, margin=0.0, eps=1e-5, rho=0.0):
    return dict(minimize_order=int(minimize_order), max_iter=int(max_iter), check_every=int(check_every), max_vel=float(max_vel),
                max_acc=float(max_acc), margin=float(margin), eps=float(eps), rho=float(rho))


def cost_matrix(n, k):
    """M_k(n): c^T M c = the integral over [0, 1] of the squared k-th derivative of the Bezier curve with control values c"""
    q = n - k
    D = np.zeros((q + 1, n + 1))
    for a in range(q + 1):
        for i in range(k + 1):
            D[a, a + i] = (-1.0) ** (k - i) * math.comb(k, i)
    G = np.array([[math.comb(q, a) * math.comb(q, b) / math.comb(2 * q, a + b) / (2 * q + 1) for b in range(q + 1)] for a in range(q + 1)])
    f = float(math.factorial(n) // math.factorial(q))
    return f * f * (D.T @ G @ D)


BASE_L = np.array([[1.0, 0.0, 0.0], [-1.0, 1.0, 0.0], [1.0, -2.0, 1.0]])      # value, first and second difference at a segment's start
BASE_R = np.array([[1.0, 0.0, 0.0], [1.0, -1.0, 0.0], [1.0, -2.0, 1.0]])      # the same at its end, counted back from the last point


class Problem:
    """One candidate: the matrices of the header's problem, dense, per axis (they are the same for x, y and z)"""

    def __init__(self, centres, radius, seg_time, orders, start, end, prm):
        self.c = np.asarray(centres, np.float64).reshape(-1, 3)
        self.r = np.asarray(radius, np.float64).reshape(-1)
        self.T = np.asarray(seg_time, np.float64).reshape(-1)
        self.n = np.asarray(orders, np.int64).reshape(-1)
        self.start = np.asarray(start, np.float64).reshape(3, 3)       # rows p, v, a
        self.end = np.asarray(end, np.float64).reshape(3, 3)
        self.prm = prm
        self.m = len(self.T)
        self.valid = self._valid()
        if not self.valid:
            return
        k, m = prm["minimize_order"], self.m
        self.off = np.concatenate([[0], np.cumsum(self.n + 1)])
        self.N = N = int(self.off[-1])
        self.seg_of = np.concatenate([np.full(n + 1, s) for s, n in enumerate(self.n)])
        P = np.zeros((N, N))
        for s in range(m):
            a, b = self.off[s], self.off[s + 1]
            P[a:b, a:b] = 2.0 * self.T[s] ** (1 - 2 * k) * cost_matrix(int(self.n[s]), k)
        self.P = P
        self.scale = 1.0 / np.abs(P).max()
        self.Q = P * self.scale
        self.use_v = math.isfinite(prm["max_vel"]) and prm["max_vel"] > 0
        self.use_a = math.isfinite(prm["max_acc"]) and prm["max_acc"] > 0
        # first and second differences inside every segment; physical value = difference * fv (fa)
        D1, D2, fv, fa = [], [], [], []
        for s in range(m):
            n, a = int(self.n[s]), int(self.off[s])
            for l in range(n):
                row = np.zeros(N); row[a + l], row[a + l + 1] = -1.0, 1.0
                D1.append(row); fv.append(n / self.T[s])
            for l in range(n - 1):
                row = np.zeros(N); row[a + l], row[a + l + 1], row[a + l + 2] = 1.0, -2.0, 1.0
                D2.append(row); fa.append(n * (n - 1) / self.T[s] ** 2)
        self.D1, self.D2, self.fv, self.fa = np.array(D1), np.array(D2), np.array(fv), np.array(fa)
        self.bv = prm["max_vel"] / self.fv if self.use_v else None
        self.ba = prm["max_acc"] / self.fa if self.use_a else None
        self.rb = self.r - prm["margin"] - 2.0 * prm["eps"]
        # equalities: group 0 = start, groups 1..m-1 = joints, group m = end; rows value / first / second difference
        ne = 3 * (m + 1)
        E, b = np.zeros((ne, N)), np.zeros((ne, 3))
        for g in range(m + 1):
            for rt in range(3):
                row = 3 * g + rt
                if g >= 1:
                    s = g - 1
                    n = int(self.n[s])
                    for e in range(3):
                        E[row, self.off[s] + n - e] += BASE_R[rt, e]
                if g <= m - 1:
                    s = g
                    cl = 1.0 if g == 0 else -self.gamma(g)[rt]
                    for l in range(3):
                        E[row, self.off[s] + l] += cl * BASE_L[rt, l]
        n0, T0, nl, Tl = int(self.n[0]), self.T[0], int(self.n[-1]), self.T[-1]
        b[0], b[1], b[2] = self.start[0], self.start[1] * (T0 / n0), self.start[2] * (T0 * T0 / (n0 * (n0 - 1)))
        b[3 * m], b[3 * m + 1], b[3 * m + 2] = self.end[0], self.end[1] * (Tl / nl), self.end[2] * (Tl * Tl / (nl * (nl - 1)))
        self.E, self.b = E, b

    def gamma(self, g):
        """joint g between segments g-1 and g: the right segment's differences in units of the left one's"""
        n, T, n2, T2 = float(self.n[g - 1]), self.T[g - 1], float(self.n[g]), self.T[g]
        return np.array([1.0, (n2 / T2) * (T / n), (n2 * (n2 - 1.0) / (T2 * T2)) * (T * T / (n * (n - 1.0)))])

    def _valid(self):
        p = self.prm
        if not (1 <= self.m <= MAX_SEG):
            return False
        if not (np.all(np.isfinite(self.c)) and np.all(np.isfinite(self.r)) and np.all(np.isfinite(self.T)) and np.all(np.isfinite(self.start))
                and np.all(np.isfinite(self.end))):
            return False
        if np.any(self.T <= 0) or np.any(self.n < MIN_ORDER) or np.any(self.n > MAX_ORDER) or np.any(self.n - 2 < p["minimize_order"]):
            return False
        return bool(np.all(self.r - p["margin"] - 2.0 * p["eps"] > 0))

    def Hmat(self, rho):
        A = np.eye(self.N)
        if self.use_v:
            A = A + self.D1.T @ self.D1
        if self.use_a:
            A = A + self.D2.T @ self.D2
        return self.Q + rho * A

    def project_ball(self, v):
        d = v - self.c[self.seg_of]
        dist = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        rb = self.rb[self.seg_of]
        f = np.where(dist > rb, rb / np.where(dist > 0, dist, 1.0), 1.0)
        return np.where((dist > rb)[:, None], self.c[self.seg_of] + d * f[:, None], v)

    def measures(self, x):
        """the final pass on x itself: cost, sphere_slack, the largest velocity and acceleration control values"""
        cost = 0.5 * float(np.sum(x * (self.P @ x)))
        d = x - self.c[self.seg_of]
        slack = float(np.min((self.r[self.seg_of] - self.prm["margin"]) - np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])))
        vmax = float(np.max(np.abs(self.D1 @ x) * self.fv[:, None]))
        amax = float(np.max(np.abs(self.D2 @ x) * self.fa[:, None]))
        return cost, slack, vmax, amax

    def rows(self, x, row_stride):
        out = np.zeros((self.m, row_stride))
        for s in range(self.m):
            n = int(self.n[s])
            for d in range(3):
                out[s, d * (n + 1):(d + 1) * (n + 1)] = x[self.off[s]:self.off[s + 1], d] / self.T[s]
        return out


def solve(centres, radius, seg_time, orders, start, end, prm, row_stride=39, force_iterations=None, trace=None):
    """One candidate.  Returns (rows [m, row_stride], result record as a dict, x [N, 3] or None).  force_iterations: run exactly that
    many iterations whatever the stop test says (the position comparison of the GPU tests)."""
    pb = Problem(centres, radius, seg_time, orders, start, end, prm)
    m = pb.m
    if not pb.valid:
        res = dict(status=INVALID, iterations=0, cost=math.nan, duration=math.nan, r_prim=math.nan, r_dual=math.nan, sphere_slack=math.nan,
                   max_vel_ctrl=math.nan, max_acc_ctrl=math.nan)
        return np.full((m, row_stride), np.nan), res, None
    eps, adaptive = prm["eps"], prm["rho"] <= 0
    rho = RHO_AUTO if adaptive else prm["rho"]
    x = pb.c[pb.seg_of].copy()
    z1, u1 = x.copy(), np.zeros_like(x)
    zv = uv = za = ua = None
    if pb.use_v:
        zv, uv = pb.D1 @ x, np.zeros((len(pb.D1), 3))
    if pb.use_a:
        za, ua = pb.D2 @ x, np.zeros((len(pb.D2), 3))

    def factor(rho):
        H = pb.Hmat(rho)
        Hi = np.linalg.inv(H)
        return Hi, pb.E @ Hi @ pb.E.T

    def At(y1, yv, ya):
        g = y1.copy()
        if pb.use_v:
            g = g + pb.D1.T @ yv
        if pb.use_a:
            g = g + pb.D2.T @ ya
        return g

    Hi, S = factor(rho)
    r_prim = r_dual = math.inf
    it, done = 0, False
    last = force_iterations if force_iterations is not None else prm["max_iter"]
    while it < last and not done:
        it += 1
        rhs = rho * At(z1 - u1, None if zv is None else zv - uv, None if za is None else za - ua)
        w = Hi @ rhs
        nu = np.linalg.solve(S, pb.E @ w - pb.b)
        x = w - Hi @ (pb.E.T @ nu)
        check = it % prm["check_every"] == 0 or it == last
        if check:
            g_old = At(z1, zv, za)
        rp = 0.0
        v = ALPHA * x + (1.0 - ALPHA) * z1 + u1
        z1 = pb.project_ball(v)
        u1 = v - z1
        rp = max(rp, float(np.max(np.abs(x - z1))))
        nax, nz = float(np.max(np.abs(x))), float(np.max(np.abs(z1)))
        if pb.use_v:
            d = pb.D1 @ x
            v = ALPHA * d + (1.0 - ALPHA) * zv + uv
            zv = np.clip(v, -pb.bv[:, None], pb.bv[:, None])
            uv = v - zv
            rp = max(rp, float(np.max(np.abs(d - zv))))
            nax, nz = max(nax, float(np.max(np.abs(d)))), max(nz, float(np.max(np.abs(zv))))
        if pb.use_a:
            d = pb.D2 @ x
            v = ALPHA * d + (1.0 - ALPHA) * za + ua
            za = np.clip(v, -pb.ba[:, None], pb.ba[:, None])
            ua = v - za
            rp = max(rp, float(np.max(np.abs(d - za))))
            nax, nz = max(nax, float(np.max(np.abs(d)))), max(nz, float(np.max(np.abs(za))))
        if not check:
            continue
        r_prim = rp
        r_dual = rho * float(np.max(np.abs(At(z1, zv, za) - g_old)))
        if trace is not None:
            trace.append((it, rho, r_prim, r_dual))
        if force_iterations is None and r_prim <= eps and r_dual <= eps:
            done = True
        elif adaptive and it < last:
            nq = float(np.max(np.abs(pb.Q @ x)))
            ny = rho * float(np.max(np.abs(At(u1, uv, ua))))
            num = r_prim / max(nax, nz, 1e-300)
            den = r_dual / max(nq, ny, 1e-300)
            ratio = math.sqrt(num / den) if den > 0 else math.inf
            new = min(max(rho * ratio, RHO_MIN), RHO_MAX) if math.isfinite(ratio) else RHO_MAX
            if new > rho * RHO_STEP or new * RHO_STEP < rho:
                f = rho / new
                u1 = u1 * f
                if pb.use_v:
                    uv = uv * f
                if pb.use_a:
                    ua = ua * f
                rho = new
                Hi, S = factor(rho)
    cost, slack, vmax, amax = pb.measures(x)
    ok = r_prim <= eps and r_dual <= eps and slack >= 0
    res = dict(status=OK if ok else NOT_CONVERGED, iterations=it, cost=cost, duration=float(np.sum(pb.T)), r_prim=r_prim, r_dual=r_dual,
               sphere_slack=slack, max_vel_ctrl=vmax, max_acc_ctrl=amax, rho=rho)
    return pb.rows(x, row_stride), res, x


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference's time allocation, restated directly (sim_planning_demo.cpp:603-686)

def time_allocation(centres, radius, start, end, init_vel, vel_mean, acc_mean, branches=None):
    """branches (a list, optional) receives per leg 0 = cannot slow down, 1 = cannot reach vel_mean, 2 = cruises"""
    c = np.asarray(centres, np.float64).reshape(-1, 3)
    r = np.asarray(radius, np.float64).reshape(-1)
    n = len(r)
    pts = [np.asarray(start, np.float64)]
    for i in range(1, n):
        delta = c[i] - c[i - 1]
        dist = math.sqrt(delta[0] * delta[0] + delta[1] * delta[1] + delta[2] * delta[2])
        pts.append(delta * (dist + r[i - 1] - r[i]) / (2.0 * dist) + c[i - 1])
    pts.append(np.asarray(end, np.float64))
    out = np.zeros(n)
    for k in range(n):
        d = pts[k + 1] - pts[k]
        v0 = np.asarray(init_vel, np.float64) if k == 0 else np.zeros(3)
        D = math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
        V0 = float(v0[0] * (d[0] / D) + v0[1] * (d[1] / D) + v0[2] * (d[2] / D))
        aV0 = abs(V0)
        sgn = 1.0 if vel_mean > V0 else -1.0
        acct = (vel_mean - V0) / acc_mean * sgn
        accd = V0 * acct + (acc_mean * acct * acct / 2) * sgn
        dcct = vel_mean / acc_mean
        dccd = acc_mean * dcct * dcct / 2
        if D < aV0 * aV0 / (2 * acc_mean):
            out[k] = (2.0 * aV0 / acc_mean if V0 < 0 else 0.0) + aV0 / acc_mean
            which = 0
        elif D < accd + dccd:
            t1 = 2.0 * aV0 / acc_mean if V0 < 0 else 0.0
            t2 = (-aV0 + math.sqrt(aV0 * aV0 + acc_mean * D - aV0 * aV0 / 2)) / acc_mean
            out[k] = t1 + t2 + (aV0 + acc_mean * t2) / acc_mean
            which = 1
        else:
            out[k] = acct + (D - accd - dccd) / vel_mean + dcct
            which = 2
        if branches is not None:
            branches.append((which, V0))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the shared case table

def chain(points, radius, speed=1.0, order=7):
    """spheres along a polyline of centres, one segment each; times = centre spacing / speed (first and last: the sphere's radius)"""
    c = np.asarray(points, np.float64).reshape(-1, 3)
    r = np.full(len(c), radius, np.float64) if np.isscalar(radius) else np.asarray(radius, np.float64)
    T = np.zeros(len(c))
    for i in range(len(c)):
        a = c[max(i - 1, 0)]
        b = c[min(i + 1, len(c) - 1)]
        T[i] = max(np.linalg.norm(b - a) / 2.0, r[i] / 2.0) / speed
    return c, r, T, np.full(len(c), order, np.int32)


def rest(p):
    return np.concatenate([np.asarray(p, np.float64), np.zeros(6)])


def generator_corridor(seed, m, order=7):
    """the prototype's generator: m overlapping spheres on a random walk, radii 0.6..1.4, neighbours overlap by 40..60 %"""
    rng = np.random.default_rng(seed)
    c, r = [np.zeros(3)], [rng.uniform(0.6, 1.4)]
    heading = np.array([1.0, 0.0, 0.0])
    for _ in range(m - 1):
        heading = heading + rng.normal(0, 0.5, 3)
        heading /= np.linalg.norm(heading)
        rn = rng.uniform(0.6, 1.4)
        c.append(c[-1] + heading * (r[-1] + rn) * rng.uniform(0.4, 0.6))
        r.append(rn)
    c, r = np.array(c), np.array(r)
    T = np.array([max(np.linalg.norm(c[min(i + 1, m - 1)] - c[max(i - 1, 0)]) / 2.0, 0.5) for i in range(m)])
    return c, r, T, np.full(m, order, np.int32)


def cases():
    """name -> dict(centres, radius, seg_time, orders, start, end, prm); every one is solved to OK well inside its max_iter"""
    out = {}
    c, r, T, od = chain([[0, 0, 0]], 5.0, order=5)
    out["quintic"] = dict(centres=c, radius=r, seg_time=np.array([2.0]), orders=od, start=np.array([-1, 0.5, 0, 0.3, 0.2, 0, 0, 0, 0.1]),
                          end=np.array([1.5, -0.5, 0.4, 0, 0.1, 0, 0.05, 0, 0]), prm=params())
    for m in (2, 3):
        c, r, T, od = chain([[2.0 * i, 0.3 * i * i, 0.1 * i] for i in range(m)], 50.0)
        out[f"big{m}"] = dict(centres=c, radius=r, seg_time=np.linspace(1.0, 1.6, m), orders=od, start=rest(c[0] + [-0.5, 0.2, 0]),
                              end=rest(c[-1] + [0.4, 0, 0.1]), prm=params())
    bend = [[0, 0, 0], [2, 0, 0], [2, 2, 0]]
    c, r, T, od = chain(bend, [1.4, 0.9, 1.4])
    out["bend"] = dict(centres=c, radius=r, seg_time=np.array([1.5, 1.2, 1.5]), orders=od, start=rest([-1.0, 0.3, 0]), end=rest([2.3, 3.0, 0]),
                       prm=params())
    c, r, T, od = generator_corridor(5, 5)
    s5, e5 = rest(c[0] - [0.3, 0, 0.1]), rest(c[-1] + [0.1, 0.2, 0])
    out["gen5"] = dict(centres=c, radius=r, seg_time=T, orders=od, start=s5, end=e5, prm=params())
    out["gen5_vel"] = dict(centres=c, radius=r, seg_time=T, orders=od, start=s5, end=e5, prm=params(max_vel=1.6))
    out["gen5_acc"] = dict(centres=c, radius=r, seg_time=T, orders=od, start=s5, end=e5, prm=params(max_acc=5.0))
    return out


def run_case(case, **kw):
    return solve(case["centres"], case["radius"], case["seg_time"], case["orders"], case["start"], case["end"], case["prm"], **kw)


# ---------------------------------------------------------------------------------------------------------------------------------
# batches: the packing the binding uses, the model over a batch, and the text form tests/host/trajgen_check.cpp reads and writes

def pack(cands):
    """a list of dicts (centres, radius, seg_time, orders, start, end) -> the arrays of a pct_trajgen_batch"""
    nseg = [len(np.asarray(c["seg_time"]).reshape(-1)) for c in cands]
    offs = np.zeros(len(cands) + 1, np.int32)
    offs[1:] = np.cumsum(nseg)
    cat = lambda key, dt, w: (np.concatenate([np.asarray(c[key], dt).reshape(-1, w) for c in cands]) if cands else np.zeros((0, w), dt))
    return dict(centres=np.ascontiguousarray(cat("centres", np.float64, 3)), radius=np.ascontiguousarray(cat("radius", np.float64, 1).reshape(-1)),
                seg_time=np.ascontiguousarray(cat("seg_time", np.float64, 1).reshape(-1)), orders=np.ascontiguousarray(cat("orders", np.int32, 1).reshape(-1)),
                seg_offsets=offs, start_state=np.ascontiguousarray(cat("start", np.float64, 9)), end_state=np.ascontiguousarray(cat("end", np.float64, 9)))


def solve_batch(cands, prm, row_stride=39, force_iterations=None):
    res = np.zeros(len(cands), GEN_RESULT_DTYPE)
    rows = []
    for b, c in enumerate(cands):
        fi = None if force_iterations is None else int(force_iterations[b])
        r, rec, _ = solve(c["centres"], c["radius"], c["seg_time"], c["orders"], c["start"], c["end"], prm, row_stride, force_iterations=fi)
        rows.append(r)
        for name in GEN_RESULT_DTYPE.names:
            res[b][name] = rec[name]
    return (np.concatenate(rows) if rows else np.zeros((0, row_stride))), res


def write_batch_text(path, cands, prm, row_stride):
    a = pack(cands)
    with open(path, "w") as f:
        f.write(f"{len(cands)} {len(a['seg_time'])} {row_stride}\n")
        f.write(f"{prm['minimize_order']} {prm['max_iter']} {prm['check_every']} " + " ".join(repr(float(prm[k])) for k in ("max_vel", "max_acc", "margin", "eps", "rho")) + "\n")
        for key in ("seg_offsets", "orders"):
            f.write(" ".join(str(int(v)) for v in a[key]) + "\n")
        for key in ("seg_time", "radius", "centres", "start_state", "end_state"):
            f.write(" ".join(repr(float(v)) for v in a[key].reshape(-1)) + "\n")


def read_result_text(path, B, row_stride):
    tok = open(path).read().split()
    res = np.zeros(B, GEN_RESULT_DTYPE)
    for b in range(B):
        rec = tok[9 * b:9 * b + 9]
        res[b] = (int(rec[0]), int(rec[1])) + tuple(float(v) for v in rec[2:])
    rows = np.array([float(v) for v in tok[9 * B:]]).reshape(-1, row_stride)
    return rows, res
