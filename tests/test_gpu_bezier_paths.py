"""GPU tests of the sampled Bezier check on every path that implements it, against the reference model of
tests/helpers/bezier_model.py (exactly rounded Bernstein powers, exhaustive nearest neighbour) on a trajectory with orders 0..12:

    plain, grid, ring              pct_bezier_check on an un-indexed, a cell-sorted and a rolling-map cloud (host loop + bezier_eval_kernel
                                   or bezier_block_kernel up to 1024 samples, the staged kernels above; replan_block_kernel<true> on the ring)
    plain_dev, grid_dev, ring_dev  pct_bezier_check_dev: torch buffers, a side stream (always the staged kernels)
    plan_grid, plan_ring           the captured replan batch (pct_plan_create_replan) with no corridor nodes and max_samples = cap

Bars: everything exact -- n and first_hit ==, positions, radii, squared distances and indices np.array_equal.  Every evaluator uses
pow_uint_cr and the reference's term order, and the scene has one nearest point per sample, so there is nothing
to tolerate and no sample to leave out.  The contract under test (include/pct_engine.h): nsamples is the unclipped count; first_hit
and the arrays cover the first min(nsamples, cap, 4096) samples.

An empty cloud takes no cell index (pct_cloud_build_grid: PCT_ERR_EMPTY), so on the `empty` cloud the grid kinds assert that refusal
and check the cloud as it stands, and plan_grid asserts that no plan can be made."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import bezier_model as M  # noqa: E402

pytestmark = pytest.mark.gpu

KINDS = ("plain", "grid", "ring", "plain_dev", "grid_dev", "ring_dev", "plan_grid", "plan_ring")
HOST_KINDS = ("plain", "grid", "ring")
ROWS = M.rows()
EXPRESS_ROWS = [r for r, v in ROWS.items() if v[3] is not None and v[3] <= 1024]
GUARD = 64
PCT_ERR_INVALID, PCT_ERR_EMPTY = 2, 5


@pytest.fixture(scope="module")
def E():
    from pointcloudtraj_amd import engine
    engine.init(0)
    return engine


def base_of(kind):
    return "grid" if "grid" in kind else "ring" if "ring" in kind else "plain"


def new_cloud(E, base, name):
    pts = M.scene()["clouds"][name]
    c = E.Cloud(max(len(pts), 1))
    if base == "ring":
        if len(pts):
            c.ring_index()
            c.set_input(pts)
        else:
            c.ring_index(extent=(32.0, 32.0, 32.0))              # an indexed window with nothing appended
        assert c.has_ring_index
    elif len(pts):
        c.set_input(pts)
        if base == "grid":
            c.build_grid()
    elif base == "grid":
        with pytest.raises(E.EngineError) as ei:
            c.build_grid()
        assert ei.value.code == PCT_ERR_EMPTY
    c.reserve_queries(M.CAP_MAX)
    return c


class Rig:
    """the module's clouds (one per index kind and cloud of the scene), captured plans and device buffers, made on first use"""

    def __init__(self, E):
        self.E, self.clouds, self.plans, self.dev = E, {}, {}, None

    def cloud(self, kind, name):
        key = (base_of(kind), name)
        if key not in self.clouds:
            self.clouds[key] = new_cloud(self.E, *key)
        return self.clouds[key]

    def plan(self, kind, name, cap):
        key = (kind, name, cap)
        if key not in self.plans:
            self.plans[key] = self.E.ReplanPlan(self.cloud(kind, name), 0, cap, M.NSEG)
        return self.plans[key]

    def buffers(self):
        import torch
        if self.dev is None:
            dev = torch.device("cuda", 0)
            n = M.CAP_MAX + GUARD
            self.dev = dict(pos=torch.empty(3 * n, dtype=torch.float64, device=dev), rad=torch.empty(n, dtype=torch.float64, device=dev),
                            d2=torch.empty(n, dtype=torch.float64, device=dev), idx=torch.empty(n, dtype=torch.int32, device=dev),
                            fh=torch.empty(1, dtype=torch.int64, device=dev), ns=torch.empty(1, dtype=torch.int32, device=dev),
                            stream=torch.cuda.Stream(device=dev))
        return self.dev

    def close(self):
        for p in self.plans.values():
            p.close()
        for c in self.clouds.values():
            c.close()


@pytest.fixture(scope="module")
def rig(E):
    r = Rig(E)
    yield r
    r.close()


def host_call(E, c, prm, traj, t_start, stop, dt, cap):
    """pct_bezier_check as Cloud.bezier_check calls it, into arrays filled with a sentinel and GUARD words more than cap: returns
    the first min(n, cap) entries after asserting that nothing behind them was written"""
    coef, T, od = traj
    bt, keep = E._traj(coef, T, od)
    pos = np.full(3 * (cap + GUARD), -7.25, np.float64); rad = np.full(cap + GUARD, -7.25, np.float64)
    d2 = np.full(cap + GUARD, -7.25, np.float64); idx = np.full(cap + GUARD, 0xABCD1234, np.uint32)
    fh, ns = C.c_int64(-99), C.c_int64(-99)
    E._chk(E.lib().pct_bezier_check(c.handle, C.byref(bt), C.byref(prm), float(t_start), float(stop), float(dt), C.byref(fh), C.byref(ns),
                                    cap, pos.ctypes.data, rad.ctypes.data, d2.ctypes.data, idx.ctypes.data))
    m = min(ns.value, cap)
    assert m >= 0
    assert np.all(pos[3 * m:] == -7.25) and np.all(rad[m:] == -7.25) and np.all(d2[m:] == -7.25) and np.all(idx[m:] == 0xABCD1234), \
        f"entries behind the first {m} were written (cap {cap})"
    return ns.value, fh.value, pos[:3 * m].reshape(m, 3), rad[:m], d2[:m], idx[:m]


def run_path(rig, kind, cloud="multi", params="near", row="base", cap=M.CAP_MAX, guard=False, c=None):
    """n, first_hit, pos, radius, d2, idx of one check along `kind`.  guard: host kinds go through the raw entry point with sentinel
    arrays (host_call) instead of Cloud.bezier_check.  c: a cloud of the caller's instead of the module's."""
    import torch
    E, S = rig.E, M.scene()
    coef, T, od = S["traj"]
    p = S["params"][params]
    prm = E.inflate_params(p["start"], p["sample_range"], p["search_margin"], p["max_radius"])
    t_start, stop, dt, _ = ROWS[row]
    if c is None:
        c = rig.cloud(kind, cloud)
    if kind in HOST_KINDS:
        if guard:
            return host_call(E, c, prm, S["traj"], t_start, stop, dt, cap)
        r = c.bezier_check(prm, coef, T, od, t_start, stop, dt=dt, cap=cap)
        return r["n"], r["first_hit"], r["pos"], r["radius"], r["d2"], r["idx"]
    if kind.endswith("_dev"):
        b = rig.buffers()
        for k in ("pos", "rad", "d2"):
            b[k].fill_(-7.25)
        b["idx"].fill_(0x2BCD1234); b["fh"].fill_(-99); b["ns"].fill_(-99)
        torch.cuda.synchronize()
        keep = c.bezier_check_device(prm, coef, T, od, t_start, stop, dt, cap, b["pos"].data_ptr(), b["rad"].data_ptr(), b["d2"].data_ptr(),
                                     b["idx"].data_ptr(), b["fh"].data_ptr(), b["ns"].data_ptr(), b["stream"].cuda_stream)
        b["stream"].synchronize()
        del keep
        n, fh = int(b["ns"].item()), int(b["fh"].item())
        m = min(n, cap)
        pos, rad, d2, idx = (b[k].cpu().numpy() for k in ("pos", "rad", "d2", "idx"))
        assert np.all(pos[3 * cap:] == -7.25) and np.all(rad[cap:] == -7.25) and np.all(d2[cap:] == -7.25) and np.all(idx[cap:] == 0x2BCD1234), \
            f"device entries behind cap {cap} were written"
        return n, fh, pos[:3 * m].reshape(m, 3), rad[:m], d2[:m], idx[:m].view(np.uint32)
    plan = rig.plan(kind, cloud, cap)
    r = plan.run(prm, np.zeros((0, 3)), coef, T, od, t_start, stop, dt)
    assert r["nctrl"] > 0                                        # the control points of the segments from t_start on ride along
    return r["nsamples"], r["first_hit_sample"], r["sample_pos"], r["sample_radius"], r["sample_d2"], r["sample_idx"]


def check(E, got, want, tag):
    n, fh, pos, rad, d2, idx = got
    print(f"{tag}: n {n} (model {want['n']}), first_hit {fh} (model {want['first_hit']}), {len(pos)} entries, "
          f"pos off {int(np.any(pos != want['pos'], axis=1).sum()) if len(pos) == len(want['pos']) else '?'}")
    assert n == want["n"], tag
    assert len(pos) == len(rad) == len(d2) == len(idx) == len(want["pos"]), tag
    assert np.array_equal(pos, want["pos"]), f"{tag}: positions"
    assert np.array_equal(d2, want["d2"]), f"{tag}: squared distances"
    assert np.array_equal(idx.astype(np.int64), np.where(want["idx"] < 0, np.int64(E.NO_INDEX), want["idx"])), f"{tag}: indices"
    assert np.array_equal(rad, want["radius"]), f"{tag}: radii"
    assert fh == want["first_hit"], tag


def plan_grid_on_empty(rig, kind, cloud):
    """no cell index on an empty cloud, hence no captured plan over one: assert the refusal (module docstring)"""
    if kind == "plan_grid" and cloud == "empty":
        with pytest.raises(rig.E.EngineError) as ei:
            rig.E.ReplanPlan(rig.cloud(kind, cloud), 0, 64, M.NSEG)
        assert ei.value.code == PCT_ERR_INVALID
        return True
    return False


# ---- 1. every order, every path ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_every_order_on_every_path(E, rig, kind):
    """every row of the table with at most 1024 samples (what the one-launch form takes), cap 4096, on `multi`"""
    for row in EXPRESS_ROWS:
        check(E, run_path(rig, kind, "multi", "near", row), M.case("multi", "near", row), f"{kind} {row}")


# ---- 2. the boundary between the one-launch and the staged form --------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("plain", "grid"))
def test_staged_boundary_host(E, rig, kind):
    """1010 samples run the one-launch form, 1265 and 5050 the staged kernels, told apart by the work counters: on an un-indexed
    cloud the streaming NN behind either form reports Q x n from the host with Q = the samples evaluated (one-launch form) or
    Q = cap (staged); on a cell-sorted cloud bezier_block_kernel leaves the counters alone while the staged form's cell search
    counts its work from zero.  5050 samples: n reports them all, the arrays hold 4096."""
    c = rig.cloud(kind, "multi")
    N = len(M.scene()["clouds"]["multi"])
    c.set_work_counters(True)
    try:
        c.nn(np.zeros((1, 3), np.float32), E.ALGO_STREAM)        # a known figure to start from
        assert c.last_work() == (N, 0)
        for row, staged in (("dt_0.005", False), ("dt_0.004", True), ("dt_0.005", False), ("dt_0.001", True)):
            before = c.last_work()
            want = M.case("multi", "near", row)
            got = run_path(rig, kind, "multi", "near", row, guard=True)
            work = c.last_work()
            print(f"{kind} {row}: last_work {before} -> {work}")
            check(E, got, want, f"{kind} {row}")
            if kind == "plain":
                assert work == ((M.CAP_MAX if staged else want["n"]) * N, 0), (row, work)
            elif staged:
                assert work[0] > 0 and work != (N, 0), (row, work)       # the cell search of the staged inflation counted, from zero
                c.nn(np.zeros((1, 3), np.float32), E.ALGO_STREAM)
            else:
                assert work == before == (N, 0), (row, work)     # bezier_block_kernel: nothing counted
        assert M.case("multi", "near", "dt_0.004")["n"] > 1024
        big = M.case("multi", "near", "dt_0.001")
        assert big["n"] == 5050 and len(big["pos"]) == 4096
    finally:
        c.set_work_counters(False)


def test_staged_rows_on_the_ring(E, rig):
    check(E, run_path(rig, "ring", "multi", "near", "dt_0.005", guard=True), M.case("multi", "near", "dt_0.005"), "ring dt_0.005")
    check(E, run_path(rig, "ring", "multi", "near", "dt_0.004", guard=True), M.case("multi", "near", "dt_0.004"), "ring dt_0.004")
    check(E, run_path(rig, "ring", "multi", "near", "dt_0.001", guard=True), M.case("multi", "near", "dt_0.001"), "ring dt_0.001")


@pytest.mark.parametrize("kind", ("plain_dev", "grid_dev", "ring_dev", "plan_grid", "plan_ring"))
def test_staged_rows_device_and_plan(E, rig, kind):
    """the same three rows where no host loop is involved; the device form takes at most 4096 entries and rejects a larger cap"""
    for row in ("dt_0.005", "dt_0.004"):
        check(E, run_path(rig, kind, "multi", "near", row), M.case("multi", "near", row), f"{kind} {row}")
    if kind.endswith("_dev"):
        with pytest.raises(E.EngineError) as ei:
            run_path(rig, kind, "multi", "near", "dt_0.001", cap=M.CAP_MAX + 1)
        assert ei.value.code == PCT_ERR_INVALID
    check(E, run_path(rig, kind, "multi", "near", "dt_0.001"), M.case("multi", "near", "dt_0.001"), f"{kind} dt_0.001")


# ---- 3. truncation ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_truncation_contract(E, rig, kind):
    """n is the unclipped count; the arrays hold min(n, cap) entries with the words behind them untouched; first_hit covers the
    samples [0, min(n, cap)) only: the first planted obstacle is at sample 20"""
    for cap in (1, 19, 20, 21, 50, 254, 255, 256):
        want = M.case("multi", "near", "base", cap)
        assert want["n"] == 255 and len(want["pos"]) == min(255, cap) and want["first_hit"] == (-1 if cap <= 20 else 20)
        got = run_path(rig, kind, "multi", "near", "base", cap=cap, guard=True)
        check(E, got, want, f"{kind} cap {cap}")
        assert got[0] == 255 and len(got[2]) == min(255, cap) and got[1] == (-1 if cap <= 20 else 20)


# ---- 4. the answer does not depend on the calls before ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("ring", "grid"))
def test_first_hit_does_not_depend_on_earlier_calls(E, rig, kind):
    """`late`: the only obstacle on the path sits at sample 150.  A ring cloud answers from a context it keeps between calls, made
    for max(cap, 128) samples and grown on demand; a call with cap 50 must report no hit before and after a call with cap 2048 has
    grown it (the fused batch used to evaluate, and report hits among, as many samples as the context held)."""
    c = new_cloud(E, kind, "late")
    try:
        small, large = M.case("late", "near", "base", 50), M.case("late", "near", "base", 2048)
        assert small["first_hit"] == -1 and large["first_hit"] >= 128
        check(E, run_path(rig, kind, "late", cap=50, guard=True, c=c), small, f"{kind} cap 50, fresh cloud")
        check(E, run_path(rig, kind, "late", cap=2048, guard=True, c=c), large, f"{kind} cap 2048")
        check(E, run_path(rig, kind, "late", cap=50, guard=True, c=c), small, f"{kind} cap 50 after cap 2048")
    finally:
        c.close()


# ---- 5. zero samples ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cloud", ("multi", "empty"))
@pytest.mark.parametrize("kind", KINDS)
def test_zero_samples(E, rig, kind, cloud):
    """t_start at and past the end, stop_time 0 and below dt: n = 0, first_hit = -1, status OK, no output entry written (host
    kinds: the sentinel arrays of host_call), and the next ordinary call on the same cloud is still right"""
    if plan_grid_on_empty(rig, kind, cloud):
        return
    for row in M.ZERO_ROWS:
        want = M.case(cloud, "near", row)
        assert want["n"] == 0 and want["first_hit"] == -1
        got = run_path(rig, kind, cloud, "near", row, guard=True)
        check(E, got, want, f"{kind} {cloud} {row}")
        assert got[0] == 0 and got[1] == -1 and len(got[2]) == 0
        check(E, run_path(rig, kind, cloud, "near", "window", guard=True), M.case(cloud, "near", "window"), f"{kind} {cloud} window after {row}")


# ---- 6. empty cloud, early-out ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_empty_cloud_and_partial_early_out(E, rig, kind):
    """no obstacle at all: every sample gets max_radius - search_margin, no index, d2 = inf.  far_tail (sample_range 3): the first
    ~27 samples are searched, the rest take the early-out -- among them the obstacle planted at sample 150, which must not be
    reported, while the one at sample 20 is."""
    far = M.case("multi", "far_tail", "base")
    assert (far["idx"] < 0).any() and (far["idx"] >= 0).any() and far["first_hit"] == 20
    check(E, run_path(rig, kind, "multi", "far_tail", "base", guard=True), far, f"{kind} far_tail")
    if plan_grid_on_empty(rig, kind, "empty"):
        return
    want = M.case("empty", "near", "base")
    assert np.all(want["radius"] == 1.25) and np.all(want["idx"] == -1) and np.all(np.isinf(want["d2"]))
    check(E, run_path(rig, kind, "empty", "near", "base", guard=True), want, f"{kind} empty")


# ---- 7. argument checks -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", HOST_KINDS)
def test_argument_checks(E, rig, kind):
    """order 13, a row stride below 3 * (order + 1), dt = 0 / NaN, cap = 0, nseg = 0: PCT_ERR_INVALID, and the cloud still answers"""
    S = M.scene()
    coef, T, od = S["traj"]
    p = S["params"]["near"]
    prm = E.inflate_params(p["start"], p["sample_range"], p["search_margin"], p["max_radius"])
    c = rig.cloud(kind, "multi")
    od13 = od.copy(); od13[5] = 13
    bad = {
        "order 13": dict(orders=od13),
        "row_stride 38": dict(polycoef=np.ascontiguousarray(coef[:, :38])),
        "dt 0": dict(dt=0.0),
        "dt nan": dict(dt=float("nan")),
        "cap 0": dict(cap=0),
        "nseg 0": dict(polycoef=np.zeros((0, M.ROW_STRIDE)), seg_time=np.zeros(0), orders=np.zeros(0, np.int32)),
    }
    for name, over in bad.items():
        a = dict(polycoef=coef, seg_time=T, orders=od, dt=0.02, cap=512)
        a.update(over)
        with pytest.raises(E.EngineError) as ei:
            c.bezier_check(prm, a["polycoef"], a["seg_time"], a["orders"], 0.0, 100.0, dt=a["dt"], cap=a["cap"])
        assert ei.value.code == PCT_ERR_INVALID, name
        check(E, run_path(rig, kind, "multi", "near", "window", guard=True), M.case("multi", "near", "window"), f"{kind} after {name}")
