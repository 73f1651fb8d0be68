"""The numpy model of the trajectory generator (tests/helpers/trajgen_model.py) against things that do not share its algorithm: the
closed-form quintic, the KKT system of the equality-constrained problem, scipy's SLSQP on the cases with active constraints,
numerical quadrature of the cost, and -- for the library's host function -- the direct restatement of the reference's time allocation.
No GPU needed."""
import math
import os
import sys

import numpy as np
import pytest
from scipy.optimize import minimize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import trajgen_model as M  # noqa: E402

CASES = M.cases()
# The largest relative gap (model cost - SLSQP cost) / SLSQP cost measured over ACTIVE at eps = 1e-5 was 1.11e-4 (gen5; bend 3.3e-5,
# gen5_vel 8.7e-5, gen5_acc -3.5e-4: the model may use the eps * n(n-1)/T^2 the limits are not guaranteed by).  The gap is the price
# of projecting onto spheres shrunk by 2 eps and scales with eps; the table is small, hence the factor 10.
COST_TOL = 1.2e-3
ACTIVE = ("bend", "gen5", "gen5_vel", "gen5_acc")


def problem(case):
    return M.Problem(case["centres"], case["radius"], case["seg_time"], case["orders"], case["start"], case["end"], case["prm"])


def test_single_quintic_is_the_hermite_solution():
    case = CASES["quintic"]
    rows, res, x = M.run_case(case)
    assert res["status"] == M.OK
    T = float(case["seg_time"][0])
    p0, v0, a0 = case["start"].reshape(3, 3)
    p1, v1, a1 = case["end"].reshape(3, 3)
    want = np.zeros((6, 3))
    want[0] = p0
    want[1] = p0 + v0 * T / 5
    want[2] = 2 * want[1] - p0 + a0 * T * T / 20
    want[5] = p1
    want[4] = p1 - v1 * T / 5
    want[3] = 2 * want[4] - p1 + a1 * T * T / 20
    assert np.abs(x - want).max() < 1e-9
    assert np.allclose(rows[0, :18].reshape(3, 6).T * T, x, rtol=0, atol=1e-15) and np.all(rows[0, 18:] == 0)


@pytest.mark.parametrize("name", ["big2", "big3"])
def test_inactive_constraints_give_the_kkt_solution(name):
    case = CASES[name]
    _, res, x = M.run_case(case)
    assert res["status"] == M.OK
    pb = problem(case)
    ne = len(pb.E)
    K = np.block([[pb.Q, pb.E.T], [pb.E, np.zeros((ne, ne))]])
    want = np.linalg.solve(K, np.concatenate([np.zeros((pb.N, 3)), pb.b]))[:pb.N]
    cost = 0.5 * float(np.sum(want * (pb.P @ want)))
    assert pb.measures(want)[1] > 1.0, "the spheres are meant to be inactive"
    assert abs(res["cost"] - cost) <= 1e-9 * cost
    assert np.abs(x - want).max() < 1e-6


def slsqp(pb):
    """the same problem (the full radius r - margin, no shrink) through an independent solver, analytic Jacobians"""
    N, I3 = pb.N, np.eye(3)
    c, rr = pb.c[pb.seg_of], (pb.r - pb.prm["margin"])[pb.seg_of]
    X = lambda v: v.reshape(N, 3)
    JE = np.kron(pb.E, I3)
    cons = [dict(type="eq", fun=lambda v: (pb.E @ X(v) - pb.b).ravel(), jac=lambda v: JE)]

    def ball_jac(v):
        J = np.zeros((N, 3 * N))
        d = -2.0 * (X(v) - c)
        for i in range(N):
            J[i, 3 * i:3 * i + 3] = d[i]
        return J
    cons.append(dict(type="ineq", fun=lambda v: rr * rr - np.sum((X(v) - c) ** 2, axis=1), jac=ball_jac))
    for use, D, bound in ((pb.use_v, pb.D1, pb.bv), (pb.use_a, pb.D2, pb.ba)):
        if use:
            JD = np.kron(D, I3)
            cons.append(dict(type="ineq", fun=lambda v, D=D, bound=bound: (bound[:, None] - D @ X(v)).ravel(), jac=lambda v, JD=JD: -JD))
            cons.append(dict(type="ineq", fun=lambda v, D=D, bound=bound: (bound[:, None] + D @ X(v)).ravel(), jac=lambda v, JD=JD: JD))
    r = minimize(lambda v: 0.5 * np.sum(X(v) * (pb.Q @ X(v))), c.ravel(), jac=lambda v: (pb.Q @ X(v)).ravel(), constraints=cons, method="SLSQP",
                 options=dict(maxiter=2000, ftol=1e-14))
    assert r.success, r.message
    return X(r.x)


@pytest.mark.parametrize("name", ACTIVE)
def test_active_constraints_against_slsqp(name):
    case = CASES[name]
    prm = case["prm"]
    _, res, x = M.run_case(case)
    pb = problem(case)
    assert res["status"] == M.OK and res["iterations"] < prm["max_iter"], res
    # feasibility as guaranteed
    assert res["sphere_slack"] >= 0 and res["r_prim"] <= prm["eps"] and res["r_dual"] <= prm["eps"]
    assert np.abs(pb.E @ x - pb.b).max() < 1e-9
    if pb.use_v:
        assert np.all(np.abs(pb.D1 @ x) <= pb.bv[:, None] + prm["eps"])
    if pb.use_a:
        assert np.all(np.abs(pb.D2 @ x) <= pb.ba[:, None] + prm["eps"])
    # the independent solver: its point is feasible for the model's constraints, and the model's cost is no worse than tol above it
    xs = slsqp(pb)
    cost_s, slack_s, _, _ = pb.measures(xs)
    assert np.abs(pb.E @ xs - pb.b).max() < 1e-8 and slack_s > -1e-8
    if pb.use_v:
        assert np.all(np.abs(pb.D1 @ xs) <= pb.bv[:, None] + 1e-8)
    if pb.use_a:
        assert np.all(np.abs(pb.D2 @ xs) <= pb.ba[:, None] + 1e-8)
    gap = (res["cost"] - cost_s) / cost_s
    print(f"{name}: iterations {res['iterations']}, model cost {res['cost']:.9g}, SLSQP {cost_s:.9g}, relative gap {gap:.3e}")
    assert res["cost"] <= cost_s * (1 + COST_TOL)
    # the case is what its name says: something is active at the optimum
    if name == "bend":
        pb2 = problem(dict(case, radius=np.full(3, 50.0)))
        K = np.block([[pb2.Q, pb2.E.T], [pb2.E, np.zeros((len(pb2.E),) * 2)]])
        free = np.linalg.solve(K, np.concatenate([np.zeros((pb2.N, 3)), pb2.b]))[:pb2.N]
        assert pb.measures(free)[1] < -0.01, "the unconstrained solution is meant to leave the middle sphere"
    if name == "gen5_vel":
        assert res["max_vel_ctrl"] > prm["max_vel"] * (1 - 1e-3) and CASES["gen5"]["prm"]["max_vel"] == 0
    if name == "gen5_acc":
        assert res["max_acc_ctrl"] > prm["max_acc"] * (1 - 1e-3)


@pytest.mark.parametrize("n", [5, 7, 12])
@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_cost_matrix_against_quadrature(n, k):
    from numpy.polynomial import Polynomial as Poly
    rng = np.random.default_rng(100 * n + k)
    c = rng.normal(0, 1, n + 1)
    t, one_t = Poly([0, 1]), Poly([1, -1])
    curve = sum(float(c[j]) * math.comb(n, j) * t ** j * one_t ** (n - j) for j in range(n + 1))
    dk = curve.deriv(k)
    nodes, weights = np.polynomial.legendre.leggauss(16)          # exact to degree 31 >= 2 (n - k)
    u = 0.5 * (nodes + 1.0)
    want = 0.5 * float(np.sum(weights * dk(u) ** 2))
    got = float(c @ M.cost_matrix(n, k) @ c)
    assert abs(got - want) <= 1e-9 * abs(want)


def test_time_allocation_against_the_restatement():
    from pointcloudtraj_amd import engine
    seen = set()
    corridors = [
        # three spheres, a start velocity along the first leg: the long legs cruise
        (np.array([[0, 0, 0], [3.0, 0.5, 0], [6.0, 0, 0.5]]), np.array([2.0, 1.8, 2.0]), [-1.5, 0, 0], [7.5, 0, 0.5], [0.5, 0, 0], 1.0, 1.0),
        # short legs (cannot reach vel_mean) and a start velocity pointing backwards (negative projection)
        (np.array([[0, 0, 0], [0.8, 0, 0], [1.6, 0.2, 0], [2.4, 0.2, 0.1]]), np.array([0.7, 0.6, 0.6, 0.7]), [-0.3, 0, 0], [2.8, 0.2, 0.1], [-0.4, 0.1, 0], 2.0, 1.5),
        # a first leg too short to slow down on: fast start, close first joint
        (np.array([[0, 0, 0], [0.5, 0, 0]]), np.array([0.45, 0.6]), [0.1, 0, 0], [0.9, 0, 0], [3.0, 0, 0], 1.0, 1.0),
    ]
    for c, r, s, e, v, vm, am in corridors:
        br = []
        want = M.time_allocation(c, r, s, e, v, vm, am, branches=br)
        got = engine.time_allocation(c, r, s, e, v, vm, am)
        assert got.shape == want.shape and np.all(np.isfinite(want)) and np.all(want > 0)
        assert np.array_equal(got, want), (got, want)
        seen |= {b for b, _ in br}
        if v[0] < 0:
            assert br[0][1] < 0, "the projected start velocity is meant to be negative"
    assert seen == {0, 1, 2}, seen
