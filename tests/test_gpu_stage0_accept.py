"""Stage 0 of the dense NN batch kernel: the termination test (kernels.hpp stage0_accept_threshold, block_leaves_undecided) and the one
load instruction for the eight run bounds (coop_stage0).

The quick accept is computed from the query's fractional cell position alone, before the record loads; the exact test recomputes the
block's bounds from the query (stage0_block) where it is needed.  Every case compares the cell-pruned search with the all-fp64 brute force
(ALGO_STREAM_EXACT) on the same cloud, indices and fp64 squared distances bit for bit, on the arrival-order path (a partial batch: Q no
multiple of 32) and on the counting-sorted one (just above 16384 queries).  All clouds are built with PCT_PYRAMID=0 so that the dense kernel
runs.  The class of input a case is about is counted on the CPU with the kernel's fp32 arithmetic (the model of
test_stage0_accept_model.py, the helpers of test_gpu_stage0_tails.py / test_gpu_stage0_addressing.py) and the count asserted non-zero.
"""
import numpy as np
import pytest

from pointcloudtraj_amd import synth

import test_gpu_stage0_addressing as A
import test_gpu_stage0_tails as T0
import test_stage0_accept_model as M

pytestmark = pytest.mark.gpu

SORTED_Q = T0.SORTED_Q
E = A.E                   # the engine fixture
F32 = np.float32


def grid_arrays(info, n):
    o = np.tile(np.asarray(info["origin"], F32), (n, 1))
    h = np.full(n, info["cell_size"], F32)
    g = np.tile(np.array(info["dims"], np.int64), (n, 1))
    return o, h, g


def block_best(info, pts, q):
    """fp64 squared distance to the nearest record of every query's 2x2x2 block (+inf for an empty block): what stage 0 finds"""
    o, h, g = grid_arrays(info, len(q))
    inv_h = (F32(1) / h).astype(F32)
    _, _, lo, hi = M.block_of(o, inv_h, g, q)
    po, _, pg = grid_arrays(info, len(pts))
    with np.errstate(invalid="ignore"):
        pc = np.fmin(np.fmax(np.floor((pts - po) * inv_h[0]), F32(0)), (pg - 1).astype(F32)).astype(np.int64)
    bd = np.empty(len(q))
    for s in range(0, len(q), 256):
        e = min(s + 256, len(q))
        inb = np.all((pc[None] >= lo[s:e, None]) & (pc[None] <= hi[s:e, None]), axis=2)
        with np.errstate(invalid="ignore", over="ignore"):
            d2 = ((pts[None].astype(np.float64) - q[s:e, None].astype(np.float64)) ** 2).sum(axis=2)
        bd[s:e] = np.where(inb & ~np.isnan(d2), d2, np.inf).min(axis=1)
    return bd


def classes(info, pts, q):
    """how stage 0's termination test ends for every query: 'quick' (the fp32 accept), 'band' (only the exact test accepts), 'undecided';
    plus f, the block bounds and whether the |f| < 2 guard holds"""
    o, h, g = grid_arrays(info, len(q))
    inv_h, hd = (F32(1) / h).astype(F32), h.astype(np.float64)
    with np.errstate(invalid="ignore"):
        f, c, lo, hi = M.block_of(o, inv_h, g, q)
        bn = M.new_threshold(f, hd)
        whole, be = M.exact_bound(o, hd, g, q, lo, hi)
        guard = M.guard(f)
    bd = block_best(info, pts, q)
    quick = M.accept(bn, bd)
    exact = whole | ((be > 0.0) & (bd <= be * be))
    assert not (quick & ~exact).any()
    return dict(quick=quick, band=~quick & exact, undecided=~exact, f=f, c=c, lo=lo, hi=hi, guard=guard, whole=whole, bd=bd)


def both_paths(E, c, q, what, n_arrival=4099):
    """the arrival-order path on a partial batch and the sorted path just above SORTED_Q; returns the reference answers of the first len(q)"""
    assert n_arrival % 32 != 0 and n_arrival < SORTED_Q
    ri, rd = T0.check_against_exact(E, c, T0.padded(q, n_arrival), what + ", arrival order")
    T0.check_against_exact(E, c, T0.padded(q, SORTED_Q + 3), what + ", sorted")
    return ri[:len(q)], rd[:len(q)]


def uniform_cloud(seed, dims, h, origin, ppc=6.0):
    """uniform points at ppc per cell over dims cells of size h from origin, two corner points pinning the bounding box (the last cell of
    every axis is 0.9 h deep, so the dims come out as given)"""
    dims, origin = np.asarray(dims, np.float64), np.asarray(origin, np.float64)
    ext = (dims - 0.1) * h
    n = max(2, int(round(ppc * dims.prod())))
    pts = (origin + synth.uniform_points(seed, n, 0.0, 1.0).astype(np.float64) * ext).astype(F32)
    pts[0] = origin
    pts[1] = origin + ext
    return pts


def ulp_neighbours(x, k=2):
    """[2k + 1, ...]: x and its k fp32 neighbours to either side"""
    out, lo, hi = [x], x, x
    for _ in range(k):
        lo, hi = np.nextafter(lo, F32(-np.inf)), np.nextafter(hi, F32(np.inf))
        out += [lo, hi]
    return np.stack(out)


@pytest.mark.parametrize("h,origin", [(1.0, (0.0, 0.0, 0.0)), (0.7, (0.3, -11.1, 5.7))], ids=["unit_cells", "cells_of_0.7"])
def test_a_half_cell_planes(E, monkeypatch, h, origin):
    """queries on the planes f = 0.5 of every axis and one and two ulps to either side: the side of the block flips there, and the bounds the
    exact test recomputes must be those of the block that was scanned.  With unit cells from the origin f is exactly 0.5 on the plane."""
    dims = (8, 7, 6)
    pts = uniform_cloud(8101, dims, h, origin)
    c, info = A.sparse_grid(E, monkeypatch, pts, h)
    assert info["dims"] == dims and np.allclose(info["origin"], origin)
    o32, h32 = np.asarray(info["origin"], F32), F32(info["cell_size"])
    qs = []
    for axis in range(3):
        base = (o32 + synth.uniform_points(8110 + axis, 5 * 8 * 20, 0.0, 1.0) * (np.array(dims, F32) * h32)).astype(F32).reshape(5, 160, 3)
        cell = np.arange(160) % dims[axis]
        plane = (o32[axis] + (cell.astype(F32) + F32(0.5)) * h32).astype(F32)
        base[:, :, axis] = ulp_neighbours(plane)
        qs.append(base.reshape(-1, 3))
    q = np.concatenate(qs).astype(F32)
    cl = classes(info, pts, q)
    near = np.abs(cl["f"] - F32(0.5)) < F32(1e-5)
    counts = {"low side": int((near & (cl["f"] < F32(0.5))).sum()), "high side": int((near & (cl["f"] >= F32(0.5))).sum()),
              "exactly 0.5": int((cl["f"] == F32(0.5)).sum()), "exact test": int((cl["band"] | cl["undecided"]).sum()), "quick": int(cl["quick"].sum())}
    print(counts)
    assert counts["low side"] >= 500 and counts["high side"] >= 500 and counts["exact test"] >= 20 and counts["quick"] >= 500, counts
    assert counts["exactly 0.5"] >= 400 or h != 1.0, counts
    both_paths(E, c, q, f"half-cell planes, h = {h}")
    c.close()


@pytest.mark.parametrize("where", ["quick", "band", "undecided"])
def test_b_single_near_point(E, monkeypatch, where):
    """8^3 unit cells, the cells 1..5 of every axis empty but for one point 0.675 / 0.69 / 0.71 below queries around (3.3, 3.3, 3.3) in x:
    the block's nearest face is 0.7 away, the quick accept reaches 0.6844, the exact test 0.6961.  'undecided' adds a point just outside
    the block, 0.7005 away: the true neighbour, which only the fallback finds."""
    d = {"quick": 0.675, "band": 0.69, "undecided": 0.71}[where]
    fill = [(x + 0.5, y + 0.5, z + 0.5) for z in range(8) for y in range(8) for x in range(8) if not all(1 <= v <= 5 for v in (x, y, z))]
    own = [(3.3 - d, 3.3, 3.3)] + ([(4.0005, 3.3, 3.3)] if where == "undecided" else [])
    pts = np.array([(0.0, 0.0, 0.0), (7.9, 7.9, 7.9)] + fill + own, F32)
    c, info = A.sparse_grid(E, monkeypatch, pts, 1.0)
    assert info["dims"] == (8, 8, 8) and info["origin"] == (0.0, 0.0, 0.0) and info["cell_size"] == 1.0
    q = (np.array([3.3, 3.3, 3.3], F32) + synth.uniform_points(8201, 1024, -0.002, 0.002)).astype(F32)
    cl = classes(info, pts, q)
    n = {k: int(cl[k].sum()) for k in ("quick", "band", "undecided")}
    print(where, n)
    assert n[where] == len(q), n
    ri, rd = both_paths(E, c, q, f"single near point, {where}")
    if where == "undecided":
        assert np.all(ri == len(pts) - 1) and np.all(A.winner_run(info, pts, q, ri) == -1) and np.all(rd < cl["bd"])
    else:
        assert np.all(ri == len(pts) - 1) and np.array_equal(rd, cl["bd"])
    c.close()


def test_c_border_cells_and_outside(E, monkeypatch):
    """queries in the border cells of every face and 0.5, 1.5 and 2.5 cells outside it: |f| = 0.5 and 1.5 pass the guard (|f| < 2), 2.5 (and
    3.5 on the upper sides, where f counts from the last cell's lower face) fail it"""
    dims, h = (8, 7, 6), 1.0
    pts = uniform_cloud(8301, dims, h, (0.0, 0.0, 0.0))
    c, info = A.sparse_grid(E, monkeypatch, pts, h)
    assert info["dims"] == dims
    qs, side = [], []
    for axis in range(3):
        for upper in (0, 1):
            for k, off in enumerate((None, 0.5, 1.5, 2.5)):
                b = (synth.uniform_points(8310 + 8 * axis + 4 * upper + k, 96, 0.0, 1.0) * np.array(dims, F32)).astype(F32)
                if off is None:
                    b[:, axis] = b[:, axis] / F32(dims[axis]) + F32(upper * (dims[axis] - 1))
                else:
                    b[:, axis] = F32(dims[axis] + off) if upper else F32(-off)
                qs.append(b)
                side += [(axis, upper, k)] * len(b)
    q, side = np.concatenate(qs).astype(F32), np.array(side)
    cl = classes(info, pts, q)
    outside = side[:, 2] > 0
    for axis in range(3):
        for upper in (0, 1):
            m = (side[:, 0] == axis) & (side[:, 1] == upper)
            cnt = {"border cell": int((m & ~outside).sum()), "outside, guard holds": int((m & outside & cl["guard"]).sum()),
                   "outside, guard fails": int((m & outside & ~cl["guard"]).sum()), "outside, quick": int((m & outside & cl["quick"]).sum()),
                   "border, quick": int((m & ~outside & cl["quick"]).sum())}
            print(axis, upper, cnt)
            assert cnt["border cell"] == 96 and cnt["outside, guard holds"] >= 96 and cnt["outside, guard fails"] >= 96 and cnt["border, quick"] >= 48, cnt
    assert int((outside & cl["quick"]).sum()) >= 20 and not (cl["quick"] & ~cl["guard"]).any()
    both_paths(E, c, q, "border cells and outside")
    c.close()


@pytest.mark.parametrize("dims", [(1, 9, 8), (9, 1, 8), (9, 8, 1), (1, 1, 1)], ids=["x", "y", "z", "one_point"])
def test_d_one_cell_thick(E, monkeypatch, dims):
    """grids of one cell along x, along y and along z (both rows of that axis coincide: disabled rows, no face with cells behind it on that
    axis) and a cloud of one point (the block is the grid); queries from a box one cell wider"""
    one = dims == (1, 1, 1)
    pts = np.array([(2.0, 3.0, 4.0)], F32) if one else uniform_cloud(8401, dims, 1.0, (0.0, 0.0, 0.0))
    c, info = A.sparse_grid(E, monkeypatch, pts, 1.0)
    assert info["dims"] == dims
    lo = np.asarray(info["origin"], F32)
    q = (lo - F32(1) + synth.uniform_points(8410, 2048, 0.0, 1.0) * (np.array(dims, F32) + F32(2))).astype(F32)
    cl = classes(info, pts, q)
    _, _, ok = A.stage0_runs(info, pts, q)
    cnt = {"quick": int(cl["quick"].sum()), "exact test": int((~cl["quick"]).sum()), "disabled rows": int((~ok).any(axis=1).sum()),
           "block is the grid": int(cl["whole"].sum())}
    print(dims, cnt)
    thin = dims.index(1)
    assert np.all(cl["lo"][:, thin] == 0) and np.all(cl["hi"][:, thin] == 0)
    assert cnt["quick"] >= 100 and cnt["exact test"] >= 100 and (thin == 0 or cnt["disabled rows"] == len(q)), cnt
    assert cnt["block is the grid"] == (len(q) if one else 0) and (not one or int(cl["undecided"].sum()) == 0), cnt
    both_paths(E, c, q, f"grid {dims}")
    c.close()


@pytest.mark.parametrize("n,m", [(60, 6), (5, 5), (3, 2)])
def test_e_disabled_rows_and_empty_runs(E, monkeypatch, n, m):
    """points on the anti-diagonal of an m^3 cube: the blocks at the low corner hold empty runs at the start of the record array, those at the
    high corner empty runs at its end, the blocks on the faces disabled rows (ya == yb or za == zb), whose end must be the start's own
    address -- for the run bounds fetched by one load instruction, starts in lanes 0..3 and ends in lanes 4..7"""
    pts = A.antidiagonal_cloud(n, m, 8500 + n)
    c, info = A.sparse_grid(E, monkeypatch, pts)
    assert info["dims"] == (m, m, m)
    q = np.concatenate([A.corner_queries(8510 + n, 1024, m), synth.uniform_points(8520 + n, 2048, -1.0, m + 1.0)]).astype(F32)
    rs, re, ok = A.stage0_runs(info, pts, q)
    cl = classes(info, pts, q)
    both = ((cl["lo"][:, 1] == cl["hi"][:, 1]) & (cl["lo"][:, 2] == cl["hi"][:, 2]))
    cnt = {"a == b == 0": int(((rs == 0) & (re == 0)).any(axis=1).sum()), "a == b == n": int(((rs == n) & (re == n)).any(axis=1).sum()),
           "ya == yb": int((cl["lo"][:, 1] == cl["hi"][:, 1]).sum()), "za == zb": int((cl["lo"][:, 2] == cl["hi"][:, 2]).sum()), "both": int(both.sum()),
           "no row disabled": int(ok.all(axis=1).sum())}
    print(n, m, cnt)
    assert min(cnt.values()) >= 100, cnt
    both_paths(E, c, q, f"anti-diagonal cloud of {n} points")
    c.close()


def test_f_nonfinite_queries(E, monkeypatch):
    """NaN, +inf and -inf in one, two or all coordinates among ordinary queries: (no index, +inf) as the brute force answers, and the
    ordinary queries of the same waves untouched.  A NaN f drops out of the quick accept's minimum; all three NaN give no accept."""
    dims = (8, 7, 6)
    pts = uniform_cloud(8601, dims, 1.0, (0.0, 0.0, 0.0))
    c, info = A.sparse_grid(E, monkeypatch, pts, 1.0)
    q = (synth.uniform_points(8610, 2048, 0.0, 1.0) * np.array(dims, F32)).astype(F32)
    bad = []
    for v in (np.nan, np.inf, -np.inf):
        for mask in range(1, 8):
            bad.append([v if mask >> a & 1 else 3.3 for a in range(3)])
    bad += [[np.inf, -np.inf, np.nan], [np.nan, 4.5, np.inf], [-np.inf, np.nan, np.nan]]
    bad = np.array(bad, F32)
    pos = (np.arange(len(bad) * 8) * 5 + 3) % len(q)
    q[pos] = np.tile(bad, (8, 1))
    for Q in (4099, SORTED_Q + 3):                              # (check_against_exact compares indices as they come: "none" is -1 here, 2^32 - 1 there)
        qq = T0.padded(q, Q)
        ri, rd = c.nn(qq, E.ALGO_STREAM_EXACT)
        gi, gd = T0.nn_device(E, c, qq, E.ALGO_GRID)
        ri, gi = ri.astype(np.int64), gi.astype(np.int64)
        assert np.array_equal(gd, rd), Q
        assert np.array_equal(np.where(gi == 0xFFFFFFFF, -1, gi), np.where(ri == 0xFFFFFFFF, -1, ri)), Q
    ri, rd = ri[:len(q)], rd[:len(q)]
    assert len(np.unique(pos)) == len(pos) and np.all(rd[pos] == np.inf) and np.all((ri[pos] < 0) | (ri[pos] == 0xFFFFFFFF))
    assert np.all(np.isfinite(rd[np.setdiff1d(np.arange(len(q)), pos)]))
    c.close()


# points scanned and runs scanned by the instrumented kernel for the batch of test_g, recorded from a run of the commit before this change
PARENT_WORK = (204917, 18919)


def test_g_work_counters(E, monkeypatch):
    """the instrumented build (COUNT) reports what it reported before: 4096 seeded queries from a box one cell wider than a 6-per-cell cloud
    (stage 0 plus the fallback of the undecided ones); the run bounds now come from one load, the count from lanes 0..3 and their partners"""
    dims = (12, 11, 10)
    pts = uniform_cloud(8701, dims, 1.0, (0.0, 0.0, 0.0))
    c, info = A.sparse_grid(E, monkeypatch, pts, 1.0)
    assert info["dims"] == dims
    q = (F32(-1) + synth.uniform_points(8710, 4096, 0.0, 1.0) * (np.array(dims, F32) + F32(2))).astype(F32)
    c.set_work_counters(True)
    gi, gd = T0.nn_device(E, c, q, E.ALGO_GRID)
    work = c.last_work()
    c.set_work_counters(False)
    ri, rd = c.nn(q, E.ALGO_STREAM_EXACT)
    assert np.array_equal(gd, rd) and np.array_equal(gi, ri.astype(np.int64))
    rs, re, ok = A.stage0_runs(info, pts, q)
    stage0 = (int((re - rs).sum()), int(ok.sum()))
    print("work", work, "stage 0 alone", stage0)
    assert work[0] >= stage0[0] and work[1] >= stage0[1]
    assert tuple(work) == PARENT_WORK
    c.close()
