"""GPU tests of the trajectory generator in polyhedra (pct_bezier_generate_poly_batch, pct_bezier_generate_poly_batch_dev;
include/pct_trajgen.h, paragraph "Trajectory generation in polyhedra") against the numpy restatement in
tests/helpers/trajgen_poly_model.py and against its own guarantees.

status and iterations are compared exactly.  Rows and record fields are compared with the model at the same iteration count.
Measured on the first GPU run over the table of tests/test_trajgen_poly_host.py (150 iterations) and the converged table: the largest
difference of a row entry from the model 2.6e-9 (the sixteen-segment candidate, stopped far from convergence; the converged
candidates are below 2.3e-11) and of a record field 1.9e-8 relative to max(1, |model|) (its cost); the tolerances are 100 x those, the
rule tests/test_gpu_trajgen.py states for itself.  The route without an active plane against the sphere form under spheres of 50 m
around the same anchors: both kernels run the same statements on the same numbers there (the projections are the identity), and the
measured difference of rows and records is 0; the test asks for equal bytes."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import trajgen_poly_model as PM  # noqa: E402
from test_trajgen_poly_host import host_table  # noqa: E402

pytestmark = pytest.mark.gpu

ROW_TOL = 2.6e-7          # 100 x the measured 2.6e-9 (rows are control points / seg_time: metres per second)
REC_TOL = 1.9e-6          # 100 x the measured 1.9e-8, relative to max(1, |model|)
EQ_TOL = 8.2e-10          # |E x - b|: 100 x the model's own 8.2e-12 (the quintic, whose points come through a factor conditioned like 1 / rho)
STRIDE = 39
GUARD = 3                 # rows / records of sentinel on either side of the device buffers
SENTINEL = -7.25
PCT_ERR_INVALID = 2
FORMS = ("host", "dev")
FIELDS = ("cost", "duration", "r_prim", "r_dual", "sphere_slack", "max_vel_ctrl", "max_acc_ctrl")
HOST_PRM = PM.params(max_vel=6.0, max_acc=12.0, max_iter=150)
FAN_SCALES = (0.8, 1.0, 1.5, 2.0)


@pytest.fixture(scope="module")
def E():
    from pointcloudtraj_amd import engine
    engine.init(0)
    return engine


def run(E, form, cands, prm, stride=STRIDE, stream=None, arrays=None):
    """one call of either form; the device form runs into sentinel-framed buffers and the frame is checked.  Returns (rows, results)."""
    p = E.gen_params(**prm)
    if form == "host":
        return E.bezier_generate_poly(cands if arrays is None else (E.TrajGenPolyBatch(*[arrays[k].ctypes.data for k in E.POLY_FIELDS], len(cands)), arrays), p, stride)
    import torch
    dev = torch.device("cuda", 0)
    arr = E.pack_poly_corridors(cands)[1] if arrays is None else arrays
    B, total = len(cands), len(arr["seg_time"])
    t = {k: torch.from_numpy(v).to(dev) for k, v in arr.items()}
    coef = torch.full((total + 2 * GUARD, stride), SENTINEL, dtype=torch.float64, device=dev)
    res = torch.full((B + 2 * GUARD, 64), 0x5A, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    try:
        E.bezier_generate_poly_device(t, p, coef[GUARD:GUARD + total], res[GUARD:GUARD + B], stream=stream)
    finally:
        torch.cuda.synchronize()
        hc, hr = coef.cpu().numpy(), res.cpu().numpy()
        run.last = (hc, hr)
    assert np.all(hc[:GUARD] == SENTINEL) and np.all(hc[GUARD + total:] == SENTINEL), "the guard band around d_polycoef was written"
    assert np.all(hr[:GUARD] == 0x5A) and np.all(hr[GUARD + B:] == 0x5A), "the guard band around d_res was written"
    return hc[GUARD:GUARD + total].copy(), hr[GUARD:GUARD + B].copy().reshape(-1).view(E.GEN_RESULT_DTYPE)


# ---- the model's side, computed once and left unchanged

@pytest.fixture(scope="module")
def tables():
    """[(names, candidates, params, model rows, model records)]: the host check's ragged batch at 150 iterations, and the five
    candidates of it that converge under the default parameters"""
    names, cands, _ = host_table()
    out = [(names, cands, HOST_PRM) + PM.solve_batch(cands, HOST_PRM, STRIDE)]
    out.append((names[:5], cands[:5], PM.params()) + PM.solve_batch(cands[:5], PM.params(), STRIDE))
    return out


def compare(names, cands, rows, res, mrows, mres, label):
    assert np.array_equal(res["status"], mres["status"]) and np.array_equal(res["iterations"], mres["iterations"]), (label, res, mres)
    offs = PM.pack(cands)["seg_offsets"]
    worst_row = worst_rec = 0.0
    for b, name in enumerate(names):
        a, e = offs[b], offs[b + 1]
        if mres["status"][b] == PM.INVALID:
            assert np.all(np.isnan(rows[a:e])) and all(np.isnan(res[f][b]) for f in FIELDS) and res["iterations"][b] == 0, name
            continue
        gap = float(np.abs(rows[a:e] - mrows[a:e]).max())
        rec = max(abs(res[f][b] - mres[f][b]) / max(1.0, abs(mres[f][b])) for f in FIELDS)
        print(f"{label} {name}: status {res['status'][b]} iterations {res['iterations'][b]} row gap {gap:.3e} record gap {rec:.3e}")
        worst_row, worst_rec = max(worst_row, gap), max(worst_rec, rec)
    print(f"{label}: largest row gap {worst_row:.3e}, largest record gap {worst_rec:.3e}")
    return worst_row, worst_rec


@pytest.mark.parametrize("form", FORMS)
def test_case_table_matches_the_model(E, tables, form):
    worst = [0.0, 0.0]
    for t, (names, cands, prm, mrows, mres) in enumerate(tables):
        rows, res = run(E, form, cands, prm)
        got = compare(names, cands, rows, res, mrows, mres, f"{form} table {t}")
        worst = [max(a, b) for a, b in zip(worst, got)]
    assert list(tables[0][4]["status"]) == [0, 0, 0, 0, 0, 1, 2, 2, 1, 1] and np.all(tables[1][4]["status"] == PM.OK)
    assert worst[0] <= ROW_TOL and worst[1] <= REC_TOL, worst


def test_guarantees_from_the_returned_rows(E, tables):
    """independent of the model's iteration: every control point of an OK candidate inside every plane moved in by the margin, the
    slack, and E x = b, recomputed in fp64 from the rows"""
    names, cands = tables[1][0], tables[1][1]
    margin = 0.01          # the face and vertex cases keep their fixed control points 0.02 m inside their planes
    prm = PM.params(margin=margin)
    rows, res = run(E, "host", cands, prm)
    offs = PM.pack(cands)["seg_offsets"]
    for b, case in enumerate(cands):
        assert res["status"][b] == PM.OK, (names[b], res[b])
        pb = PM.problem(case, prm)
        mine = rows[offs[b]:offs[b + 1]]
        x = np.concatenate([mine[s, :3 * (n + 1)].reshape(3, n + 1).T * case["seg_time"][s] for s, n in enumerate(case["orders"])])
        slack = np.inf
        for r in range(len(x)):
            poly = pb.poly[pb.seg_of[r]]
            if poly.cnt:
                d = poly.o - PM.pdot(poly.nh, x[r])          # o already has the margin taken off
                assert np.all(d >= 0.0), f"{names[b]}: a control point outside a plane moved in by the margin"
                slack = min(slack, float(d.min()))
        print(f"{names[b]}: slack {res['sphere_slack'][b]:.6e} recomputed {slack:.6e}, |E x - b| {np.abs(pb.E @ x - pb.b).max():.3e}")
        # the kernel measured x itself; the rows are x / T, so the recomputation differs by the rounding of that division and product
        assert slack == res["sphere_slack"][b] or abs(slack - res["sphere_slack"][b]) <= 1e-14 * max(1.0, float(np.abs(x).max()))
        assert np.abs(pb.E @ x - pb.b).max() <= EQ_TOL
        for s, n in enumerate(case["orders"]):
            assert np.all(mine[s, 3 * (n + 1):] == 0.0)


def test_ragged_batch_candidates_do_not_see_each_other(E):
    names, cands, want = host_table()
    cands, want = cands[:8], want[:8]                      # B = 8: the rest of the table runs in the table test
    prm = PM.params(max_iter=200, max_vel=6.0)
    rows, res = run(E, "dev", cands, prm)
    rows_h, res_h = run(E, "host", cands, prm)
    assert rows.tobytes() == rows_h.tobytes() and res.tobytes() == res_h.tobytes(), "the two forms differ"
    offs = PM.pack(cands)["seg_offsets"]
    for b, cand in enumerate(cands):
        mine, rec = rows[offs[b]:offs[b + 1]], res[b]
        if want[b] == PM.INVALID:
            assert rec["status"] == PM.INVALID and np.all(np.isnan(mine)) and np.isnan(rec["cost"]), b
            continue
        one_rows, one_res = run(E, "host", [cand], prm)
        assert one_rows.tobytes() == mine.tobytes() and one_res.tobytes() == rec.tobytes(), f"candidate {names[b]} differs from its own run"
        assert rec["status"] in (PM.OK, PM.NOT_CONVERGED) and np.all(np.isfinite(mine))
    assert np.sum(res["status"] == PM.OK) >= 5
    # B == 0: PCT_OK, nothing written
    r0, s0 = run(E, "dev", [], prm)
    assert len(r0) == 0 and len(s0) == 0
    r0, s0 = E.bezier_generate_poly([], E.gen_params(**prm), STRIDE)
    assert len(r0) == 0 and len(s0) == 0


def test_bad_params_and_bad_offsets_are_refused_with_nothing_written(E):
    case = PM.cases()["bend"]
    for bad in (dict(minimize_order=0), dict(minimize_order=5), dict(max_iter=0), dict(eps=0.0), dict(check_every=0)):
        with pytest.raises(E.EngineError) as e:
            run(E, "dev", [case], PM.params(**bad))
        assert e.value.code == PCT_ERR_INVALID
        hc, hr = run.last
        assert np.all(hc == SENTINEL) and np.all(hr == 0x5A), "a refused call wrote something"
    with pytest.raises(E.EngineError) as e:
        E.bezier_generate_poly([case], E.gen_params(), 3 * 8 - 1)                      # row_stride below 3 * (7 + 1)
    assert e.value.code == PCT_ERR_INVALID
    # the host form reads the offsets: plane_offsets[0] != 0, and a descent anywhere
    for where, value in ((0, 1), (2, 3)):
        arr = E.pack_poly_corridors([case, case])[1]
        arr["plane_offsets"][where] = value
        coef = np.full((4, STRIDE), SENTINEL)
        res = np.full(2, 0x5A5A5A5A, np.int64).repeat(8).view(E.GEN_RESULT_DTYPE)
        batch = E.TrajGenPolyBatch(*[arr[k].ctypes.data for k in E.POLY_FIELDS], 2)
        p = E.gen_params()
        import ctypes as C
        st = E.lib().pct_bezier_generate_poly_batch(C.byref(batch), C.byref(p), coef.ctypes.data_as(C.POINTER(C.c_double)), STRIDE, res.ctypes.data)
        assert st == PCT_ERR_INVALID and np.all(coef == SENTINEL) and np.all(res.view(np.int64) == 0x5A5A5A5A)
    # the device form cannot: a descent inside a candidate makes that candidate INVALID and leaves its neighbour alone
    arr = E.pack_poly_corridors([case, case])[1]
    arr["plane_offsets"][1] = 13                                                      # segment 1 of candidate 0 would own [13, 12)
    rows, res = run(E, "dev", [case, case], PM.params(), arrays=arr)
    alone, alone_res = run(E, "dev", [case], PM.params())
    assert res["status"][0] == PM.INVALID and np.all(np.isnan(rows[:2]))
    assert res["status"][1] == PM.OK and rows[2:].tobytes() == alone.tobytes() and res[1:].tobytes() == alone_res.tobytes()


def test_route_without_an_active_plane_agrees_with_the_sphere_form(E):
    case = PM.cases()["free2"]
    m = len(case["seg_time"])
    sphere = dict(centres=case["anchors"], radius=np.full(m, 50.0), seg_time=case["seg_time"], orders=case["orders"], start=case["start"], end=case["end"])
    for prm in (PM.params(), PM.params(max_vel=6.0, max_acc=12.0)):
        rows, res = run(E, "host", [case], prm)
        srows, sres = E.bezier_generate([sphere], E.gen_params(**prm), STRIDE)
        assert res["status"][0] == sres["status"][0] == PM.OK and res["iterations"][0] == sres["iterations"][0]
        print(f"largest row difference {np.abs(rows - srows).max():.3e}; cost {res['cost'][0]!r} against {sres['cost'][0]!r}")
        assert rows.tobytes() == srows.tobytes()
        for f in ("status", "iterations", "cost", "duration", "r_prim", "r_dual", "max_vel_ctrl", "max_acc_ctrl"):
            assert res[f][0] == sres[f][0], f
        assert res["sphere_slack"][0] > 40.0 and sres["sphere_slack"][0] > 40.0           # the one field that means another thing


def pillar_candidates(E, c, route, reach, margin, scales):
    """segment_polyhedron on the route's edges plus the box planes -> the fan of poly corridors, or None when an edge collides"""
    segs = np.concatenate([route[:-1], route[1:]], axis=1)
    offs, _, d2, _, planes = c.segment_polyhedron(segs, reach)
    for i in range(len(segs)):
        if offs[i + 1] > offs[i] and d2[offs[i]] <= margin * margin:
            return None
    base = PM.route_case(route, PM.route_polytopes(route, offs, planes, reach, margin), [1.6, 1.2, 1.6], 7)
    return E.corridor_fan(base, scales)


def test_pipeline_polytopes_generate_certify_on_the_device(E):
    """two pillars beside a three-edge route, four time scales: the polytopes from the cloud, then generate and certify on the same
    device buffers, no host copy of the coefficients in between"""
    import torch
    cloud, route, graze, reach, margin = PM.pillar_world()
    assert 200 <= len(cloud) <= 900
    prm = E.gen_params(**PM.params(max_vel=2.0, max_iter=2000))
    dev = torch.device("cuda", 0)
    with E.Cloud(len(cloud)) as c:
        c.set_input(cloud)
        c.build_grid()
        assert pillar_candidates(E, c, graze, reach, margin, FAN_SCALES) is None, "the grazing route is meant to yield no polytope"
        cands = pillar_candidates(E, c, route, reach, margin, FAN_SCALES)
        assert cands is not None and all(6 < len(p) <= E.trajgen_max_planes() for p in cands[0]["planes"])
        _, arr = E.pack_poly_corridors(cands)
        B, total, piece_cap = len(cands), len(arr["seg_time"]), 4096
        t = {k: torch.from_numpy(v).to(dev) for k, v in arr.items()}
        coef = torch.zeros((total, STRIDE), dtype=torch.float64, device=dev)
        res = torch.zeros((B, 64), dtype=torch.uint8, device=dev)
        cert = torch.zeros((B * 48,), dtype=torch.uint8, device=dev)
        c.reserve_queries(2 * piece_cap)
        torch.cuda.synchronize()
        stream = torch.cuda.current_stream().cuda_stream
        E.bezier_generate_poly_device(t, prm, coef, res)
        bz = E.BezierBatch(coef.data_ptr(), STRIDE, t["seg_time"].data_ptr(), t["orders"].data_ptr(), t["seg_offsets"].data_ptr(), None, B)
        c.bezier_certify_device(bz, 0.15, 12, piece_cap, cert.data_ptr(), 0, stream)
        torch.cuda.synchronize()
    gen = res.cpu().numpy().reshape(-1).view(E.GEN_RESULT_DTYPE)
    cer = cert.cpu().numpy().view(E.CERT_DTYPE)
    good = [b for b in range(B) if gen["status"][b] == E.GEN_OK and cer["status"][b] == E.CERT_FREE]
    print("pipeline:", list(gen["status"]), list(gen["iterations"]), list(cer["status"]), "good", good)
    assert good, (gen, cer)
    # the host form gives the same trajectories
    rows_h, res_h = E.bezier_generate_poly(cands, prm, STRIDE)
    assert rows_h.tobytes() == coef.cpu().numpy().tobytes() and res_h.tobytes() == gen.tobytes()


def test_cxx_mirror_flies_the_polytopes_and_refuses_the_grazing_route():
    """examples/trajectory_polyhedra.cpp: the same world through ObstacleMap::generateSafeTrajectoryInPolyhedra -- its guarantees
    against a host loop, its choice against the shortest candidate that is OK and certified free, -1 for the grazing route"""
    from pointcloudtraj_amd import build
    exe = os.path.join(build.LIB, "trajectory_polyhedra")
    assert os.path.exists(exe), "the example is not built: build first"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
    assert "grazing route: -1" in r.stdout and "polytopes: candidate" in r.stdout


def test_device_form_captured_in_a_graph(E):
    """captured once on a side stream and replayed twice: the bytes of the eager call both times.  The process keeps its default
    queue count."""
    import torch
    cands = E.corridor_fan(PM.cases()["bend"], FAN_SCALES[:3])
    prm = E.gen_params(**PM.params(max_vel=2.0))
    dev = torch.device("cuda", 0)
    _, arr = E.pack_poly_corridors(cands)
    B, total = len(cands), len(arr["seg_time"])
    t = {k: torch.from_numpy(v).to(dev) for k, v in arr.items()}
    coef = torch.zeros((total, STRIDE), dtype=torch.float64, device=dev)
    res = torch.zeros((B, 64), dtype=torch.uint8, device=dev)
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    E.bezier_generate_poly_device(t, prm, coef, res, stream=side.cuda_stream)          # eager
    side.synchronize()
    want = (coef.cpu().numpy().tobytes(), res.cpu().numpy().tobytes())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        E.bezier_generate_poly_device(t, prm, coef, res, stream=side.cuda_stream)
    for _ in range(2):
        coef.zero_()
        res.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert (coef.cpu().numpy().tobytes(), res.cpu().numpy().tobytes()) == want
    assert np.all(res.cpu().numpy().reshape(-1).view(E.GEN_RESULT_DTYPE)["status"] == E.GEN_OK)
    del g
