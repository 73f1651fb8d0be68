"""The numpy model of the trajectory generator in polyhedra (tests/helpers/trajgen_poly_model.py) against things that do not share
its algorithm: the pinned projection against scipy's SLSQP on the 3-D problem, the route without an active plane against the KKT
system of the equality-constrained problem, and the routes with active faces, a joint on an edge of two polytopes and a vertex
against SLSQP on the same QP.  No GPU needed."""
import os
import sys

import numpy as np
import pytest
from scipy.optimize import minimize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import trajgen_poly_model as PM  # noqa: E402

CASES = PM.cases()
# The relative gaps (model cost - SLSQP cost) / SLSQP cost measured over ACTIVE at eps = 1e-5: face 2.8e-5, bend 5.1e-5,
# vertex 3.2e-5.  The gap is the price of projecting onto polytopes shrunk by 2 eps and scales with eps; the table is small, hence
# the factor 10 on the largest, as tests/test_trajgen_model.py has it for the balls.
COST_TOL = 5.2e-4
ACTIVE = ("face", "bend", "vertex")
# SLSQP on the 3-D projection stops within about 1e-9 of the point; the model's accept tolerance is 1e-9 (metres)
PROJ_TOL = 1e-7
CUBE = PM.box_planes([-1, -1, -1], [1, 1, 1])


def reference_projection(planes, v):
    """min |y - v|^2 s.t. nh . y <= o, by SLSQP from a point of the set (the origin in every polytope used here)"""
    p = np.asarray(planes, np.float64).reshape(-1, 4)
    if len(p) == 0:
        return np.asarray(v, np.float64)
    ln = np.linalg.norm(p[:, :3], axis=1)
    nh, o = p[:, :3] / ln[:, None], p[:, 3] / ln
    assert np.all(o >= 0), "the origin is meant to be inside"
    r = minimize(lambda y: 0.5 * np.sum((y - v) ** 2), np.zeros(3), jac=lambda y: y - v, method="SLSQP",
                 constraints=[dict(type="ineq", fun=lambda y: o - nh @ y, jac=lambda y: -nh)], options=dict(maxiter=500, ftol=1e-14))
    assert r.success, r.message
    return r.x


def project(planes, v, stage=None):
    return PM.Polytope(planes, 0.0).project(np.asarray(v, np.float64), 0.0, stage)


def random_polytope(rng, cuts):
    """the cube and `cuts` random planes at distance 0.3 .. 1.2 from the origin, with normals of random length"""
    out = [CUBE]
    for _ in range(cuts):
        n = rng.normal(0, 1, 3)
        n /= np.linalg.norm(n)
        f = rng.uniform(0.1, 10.0)
        out.append(np.concatenate([n * f, [rng.uniform(0.3, 1.2) * f]])[None])
    return np.concatenate(out)


@pytest.mark.parametrize("cuts", [0, 3, 8, 18])
def test_projection_on_random_polytopes(cuts):
    rng = np.random.default_rng(7 + cuts)
    seen = set()
    for _ in range(6):
        planes = random_polytope(rng, cuts)
        assert len(planes) == 6 + cuts <= PM.MAX_PLANES
        for _ in range(12):
            v = rng.normal(0, 1.2, 3)
            st = []
            z = project(planes, v, st)
            seen.add(st[0])
            want = reference_projection(planes, v)
            assert np.abs(z - want).max() < PROJ_TOL, (planes, v, z, want, st)
            poly = PM.Polytope(planes, 0.0)
            assert np.all(poly.viol(z, 0.0) <= PM.ACCEPT)
            if st[0] == 0:
                assert np.array_equal(z, v)
    assert -1 not in seen and {0, 1, 2} <= seen, seen
    if cuts == 18:
        assert 3 in seen, seen


@pytest.mark.parametrize("v, want, stage", [
    ([0.3, -0.2, 0.9], [0.3, -0.2, 0.9], 0),
    ([2.0, 0.3, 0.2], [1.0, 0.3, 0.2], 1),             # a face
    ([2.0, -3.0, 0.1], [1.0, -1.0, 0.1], 2),           # an edge
    ([2.0, 5.0, -1.5], [1.0, 1.0, -1.0], 3),           # a vertex
    ([1.0, 0.0, 0.0], [1.0, 0.0, 0.0], 0),             # exactly on a plane: inside, returned as it is
])
def test_projection_ends_where_it_is_built_to(v, want, stage):
    st = []
    z = project(CUBE, v, st)
    assert st == [stage] and np.abs(z - np.array(want)).max() <= 4e-16, (z, st)
    assert np.abs(z - reference_projection(CUBE, np.array(v))).max() < PROJ_TOL


def test_projection_with_a_duplicated_plane():
    planes = np.concatenate([CUBE, CUBE[:1], 3.0 * CUBE[2:3]])          # x <= 1 twice, y <= 1 again with a longer normal
    for v, want in (([2.0, 0.1, 0.2], [1.0, 0.1, 0.2]), ([2.0, 2.0, 0.0], [1.0, 1.0, 0.0]), ([3.0, 2.0, 4.0], [1.0, 1.0, 1.0])):
        st = []
        z = project(planes, v, st)
        assert st[0] > 0 and np.abs(z - np.array(want)).max() <= 4e-16, (v, z, st)


def test_projection_with_two_near_parallel_planes():
    """x <= 1 and a plane turned from it by 1e-6 rad: their Gram determinant is 1e-12, below the threshold, so the pair is never
    solved; the point is found on one of them"""
    t = 1e-6
    planes = np.concatenate([CUBE, [[np.cos(t), np.sin(t), 0.0, 1.0]]])
    poly = PM.Polytope(planes, 0.0)
    assert not np.any((poly.pI == 0) & (poly.pJ == 6)), "the near-parallel pair is meant to be skipped"
    for v in ([2.0, 0.5, 0.0], [2.0, -0.5, 0.3], [3.0, 0.0, 0.0], [2.0, 2.0, 2.0]):
        st = []
        z = poly.project(np.array(v), 0.0, st)
        want = reference_projection(planes, np.array(v))
        assert st[0] in (1, 2, 3) and np.abs(z - want).max() < PROJ_TOL, (v, z, want, st)


def test_projection_with_24_planes_and_with_none():
    planes = PM.tube_planes([0, 0, 0], [1.0, 0.4, 0.2], 0.8, extra=18, cut=1.0, seed=3)
    assert len(planes) == PM.MAX_PLANES
    rng = np.random.default_rng(11)
    mid = np.array([0.5, 0.2, 0.1])
    shifted = planes.copy()
    shifted[:, 3] -= planes[:, :3] @ mid                             # the same polytope with the edge's midpoint at the origin
    stages = []
    for _ in range(40):
        v = rng.normal(0, 1.5, 3)
        z = project(shifted, v, stages)
        assert np.abs(z - reference_projection(shifted, v)).max() < PROJ_TOL
    assert {1, 2, 3} <= set(stages) and -1 not in stages, stages
    v = rng.normal(0, 100.0, 3)
    st = []
    assert np.array_equal(project(np.zeros((0, 4)), v, st), v) and st == [0]


def test_fallback_on_an_empty_set_returns_the_least_violating_candidate():
    planes = np.array([[1.0, 0, 0, -1.0], [-1.0, 0, 0, -1.0]])      # x <= -1 and x >= 1
    st = []
    z = project(planes, [0.25, 3.0, 4.0], st)
    assert st == [-1] and np.array_equal(z, [-1.0, 3.0, 4.0])       # both candidates are 2 m outside the other plane: the first is kept


def test_route_without_an_active_plane_gives_the_kkt_solution():
    case = CASES["free2"]
    st = []
    _, res, x = PM.run_case(case, stages=st)
    assert res["status"] == PM.OK and set(st) == {0}
    pb = PM.problem(case)
    ne = len(pb.E)
    K = np.block([[pb.Q, pb.E.T], [pb.E, np.zeros((ne, ne))]])
    want = np.linalg.solve(K, np.concatenate([np.zeros((pb.N, 3)), pb.b]))[:pb.N]
    cost = 0.5 * float(np.sum(want * (pb.P @ want)))
    assert pb.slack(want) > 1.0, "the planes are meant to be inactive"
    assert abs(res["cost"] - cost) <= 1e-9 * cost
    assert np.abs(x - want).max() < 1e-6


def slsqp(pb):
    """the same problem (the planes moved in by the margin, no shrink) through an independent solver, analytic Jacobians"""
    N, I3 = pb.N, np.eye(3)
    X = lambda v: v.reshape(N, 3)
    JE = np.kron(pb.E, I3)
    cons = [dict(type="eq", fun=lambda v: (pb.E @ X(v) - pb.b).ravel(), jac=lambda v: JE)]
    rows, offs = [], []
    for r in range(N):
        poly = pb.poly[pb.seg_of[r]]
        for q in range(poly.cnt):
            row = np.zeros(3 * N)
            row[3 * r:3 * r + 3] = poly.nh[q]
            rows.append(row); offs.append(poly.o[q])
    G, h = np.array(rows), np.array(offs)
    cons.append(dict(type="ineq", fun=lambda v: h - G @ v, jac=lambda v: -G))
    for use, D, bound in ((pb.use_v, pb.D1, pb.bv), (pb.use_a, pb.D2, pb.ba)):
        if use:
            JD = np.kron(D, I3)
            cons.append(dict(type="ineq", fun=lambda v, D=D, bound=bound: (bound[:, None] - D @ X(v)).ravel(), jac=lambda v, JD=JD: -JD))
            cons.append(dict(type="ineq", fun=lambda v, D=D, bound=bound: (bound[:, None] + D @ X(v)).ravel(), jac=lambda v, JD=JD: JD))
    r = minimize(lambda v: 0.5 * np.sum(X(v) * (pb.Q @ X(v))), pb.c[pb.seg_of].ravel(), jac=lambda v: (pb.Q @ X(v)).ravel(), constraints=cons, method="SLSQP",
                 options=dict(maxiter=2000, ftol=1e-14))
    assert r.success, r.message
    return X(r.x)


def active_planes(pb, x, tol=1e-4):
    """per control point the number of its planes it lies on (within tol)"""
    return np.array([int(np.sum(pb.poly[pb.seg_of[r]].o - PM.pdot(pb.poly[pb.seg_of[r]].nh, x[r]) < tol)) for r in range(len(x))])


@pytest.mark.parametrize("name", ACTIVE)
def test_active_planes_against_slsqp(name):
    case = CASES[name]
    prm = case["prm"]
    st = []
    _, res, x = PM.run_case(case, stages=st)
    pb = PM.problem(case)
    assert res["status"] == PM.OK and res["iterations"] < prm["max_iter"], res
    assert res["sphere_slack"] >= 0 and res["r_prim"] <= prm["eps"] and res["r_dual"] <= prm["eps"]
    assert abs(res["sphere_slack"] - pb.slack(x)) == 0.0
    assert np.abs(pb.E @ x - pb.b).max() < 1e-9
    xs = slsqp(pb)
    cost_s = pb.measures(xs)[0]
    assert np.abs(pb.E @ xs - pb.b).max() < 1e-8 and pb.slack(xs) > -1e-8
    gap = (res["cost"] - cost_s) / cost_s
    print(f"{name}: iterations {res['iterations']}, model cost {res['cost']:.9g}, SLSQP {cost_s:.9g}, relative gap {gap:.3e}, stages {sorted(set(st))}")
    assert res["cost"] <= cost_s * (1 + COST_TOL)
    # the case is what its name says
    act = active_planes(pb, x)
    if name == "face":
        assert act.max() == 1 and 1 in st
    if name == "vertex":
        assert act.max() == 3 and 3 in st
    if name == "bend":
        last0, first1 = pb.off[1] - 1, pb.off[1]
        assert np.array_equal(x[last0], x[first1]) or np.abs(x[last0] - x[first1]).max() < 1e-12
        assert act[last0] >= 1 and act[first1] >= 1, "the joint is meant to lie on a plane of either polytope"
        assert abs(x[last0][1] - 0.5) < 1e-4 and abs(x[first1][0] - 1.5) < 1e-4
    free = dict(case, planes=[np.zeros((0, 4)) for _ in case["planes"]])
    _, _, xf = PM.run_case(free)
    assert pb.slack(xf) < -0.01, "the unconstrained solution is meant to leave the polytope"


def test_invalid_and_infeasible_candidates():
    for name, case in PM.invalid_cases().items():
        rows, res, x = PM.run_case(case)
        assert res["status"] == PM.INVALID and x is None and np.all(np.isnan(rows)), name
    prm = PM.params(max_iter=300)
    _, res, _ = PM.run_case(dict(PM.empty_case(), prm=prm))
    assert res["status"] == PM.NOT_CONVERGED and res["r_prim"] > prm["eps"] and res["sphere_slack"] < 0
    bend = CASES["bend"]
    outside = dict(bend, start=PM.rest([-1.0, 0, 0]), prm=prm)           # the start point 0.5 m outside the first box
    _, res, _ = PM.run_case(outside)
    assert res["status"] == PM.NOT_CONVERGED and res["sphere_slack"] < -0.4
    apart = dict(bend, planes=[bend["planes"][0], PM.box_planes([3.0, -0.5, -0.5], [4.0, 2.5, 0.5])], prm=prm)     # no common point
    _, res, _ = PM.run_case(apart)
    assert res["status"] == PM.NOT_CONVERGED
