"""Stage 0 of the dense NN batch kernel: the termination test's quick accept, modelled on the CPU in the kernel's own arithmetic.

Three tests decide whether a query's 2x2x2 block of cells settles it, given the best squared distance bd found in the block
(kernels.hpp: stage0_block, stage0_accept_threshold, block_leaves_undecided):

    new      bc = min over the axes of max(f, 1 - f), b = (bc - 1/64) * h * 0.999999 in fp32 (0 unless max |f| < 2); accept iff
             b > 0 and bd <= b * b -- from the query's fractional cell position f alone
    present  the form it replaced: bc = the minimum over the block's faces that have cells behind them, face by face from the block's
             bounds, same margin, same guard; it declines when no face has cells behind it
    exact    the six fp64 face distances less h/256; accepts everything when the block covers the whole grid

The kernel is exact only if  new => exact.  The design rests on the stronger chain  new => present => exact,  where "present" counts the
blocks that cover the whole grid as accepted: there the present form merely handed the query to the exact test, which accepts all of them
(asserted below).  Everything here is numpy with fp32 where the kernel has fp32 and fp64 where it has fp64; no GPU.
"""
import numpy as np

F32 = np.float32
INF32 = F32(np.inf)


def block_of(o, inv_h, g, q):
    """the kernel's stage0_block: (f [N,3] fp32, c, lo, hi [N,3] int64) for origin o [N,3] fp32, inv_h [N] fp32, dims g [N,3], query q [N,3] fp32"""
    t = ((q - o) * inv_h[:, None]).astype(F32)
    cf = np.fmin(np.fmax(np.floor(t), F32(0)), (g - 1).astype(F32))
    f = (t - cf).astype(F32)
    c = cf.astype(np.int64)
    low = f < F32(0.5)
    lo = np.maximum(np.where(low, c - 1, c), 0)
    hi = np.minimum(np.where(low, c, c + 1), g - 1)
    return f, c, lo, hi


def guard(f):
    return np.fmax(np.fmax(np.abs(f[:, 0]), np.abs(f[:, 1])), np.abs(f[:, 2])) < F32(2)


def threshold(bc, hd):
    """(bc - 1/64) * (float)hd * 0.999999f in fp32, widened"""
    b = ((bc - F32(0.015625)) * hd.astype(F32)).astype(F32) * F32(0.999999)
    return b.astype(F32).astype(np.float64)


def new_threshold(f, hd):
    m = np.fmax(f, (F32(1) - f).astype(F32))
    bc = np.fmin(np.fmin(m[:, 0], m[:, 1]), m[:, 2])
    return np.where(guard(f), threshold(bc, hd), 0.0)


def present_threshold(f, c, lo, hi, g, hd):
    """the face-by-face form; 0 where it declines (no face with cells behind it, or the guard)"""
    with np.errstate(invalid="ignore"):
        below = np.where(lo > 0, (f + (c - lo).astype(F32)).astype(F32), INF32)
        above = np.where(hi < g - 1, ((hi + 1 - c).astype(F32) - f).astype(F32), INF32)
    bc = np.fmin(below, above)
    bc = np.fmin(np.fmin(bc[:, 0], bc[:, 1]), bc[:, 2])
    ok = (bc < INF32) & guard(f)
    return np.where(ok, threshold(np.where(ok, bc, F32(1)), hd), 0.0)


def exact_bound(o, hd, g, q, lo, hi):
    """(whole [N] bool: the block covers the grid, bound [N] fp64: nearest face with cells behind it, less h/256)"""
    od, qd, h = o.astype(np.float64), q.astype(np.float64), hd[:, None]
    below = np.where(lo > 0, qd - (od + lo.astype(np.float64) * h), np.inf)
    above = np.where(hi < g - 1, (od + (hi + 1).astype(np.float64) * h) - qd, np.inf)
    bound = np.minimum(below, above).min(axis=1)
    whole = bound == np.inf
    return whole, bound - hd * (1.0 / 256.0)


def accept(b, bd):
    return (b > 0.0) & (bd <= b * b)


def check_chain(o, h, g, q, bds, what):
    """assert new => present => exact (and new => exact) for every bd in bds ([N] arrays or callables of the three thresholds)"""
    hf = h.astype(F32)
    inv_h = (F32(1) / hf).astype(F32)
    hd = hf.astype(np.float64)
    f, c, lo, hi = block_of(o, inv_h, g, q)
    bn = new_threshold(f, hd)
    bp = present_threshold(f, c, lo, hi, g, hd)
    whole, be = exact_bound(o, hd, g, q, lo, hi)
    n_new = 0
    for bd in bds:
        bd = bd(bn, bp, be) if callable(bd) else bd
        a_new = accept(bn, bd)
        a_pre = accept(bp, bd) | whole
        a_exa = whole | ((be > 0.0) & (bd <= be * be))
        bad = a_new & ~a_pre
        assert not bad.any(), f"{what}: new accepts, present does not: {int(bad.sum())} cases, first g={g[bad][0]} f={f[bad][0]} bd={bd[bad][0]!r}"
        bad = a_pre & ~a_exa
        assert not bad.any(), f"{what}: present accepts, exact does not: {int(bad.sum())} cases, first g={g[bad][0]} f={f[bad][0]} bd={bd[bad][0]!r}"
        bad = a_new & ~a_exa
        assert not bad.any(), f"{what}: new accepts, exact does not: {int(bad.sum())} cases"
        n_new += int(a_new.sum())
    # the new threshold never exceeds the present one where the present one is in force
    assert np.all((bn <= bp) | (bp == 0.0)), what
    return n_new


def threshold_bds():
    """bd at both quick thresholds squared and at the exact bound squared, each with its two fp64 neighbours"""
    out = []
    for pick in (lambda bn, bp, be: bn * bn, lambda bn, bp, be: bp * bp, lambda bn, bp, be: np.where(be > 0.0, be * be, 0.0)):
        out.append(pick)
        out.append(lambda bn, bp, be, pick=pick: np.nextafter(pick(bn, bp, be), np.inf))
        out.append(lambda bn, bp, be, pick=pick: np.nextafter(pick(bn, bp, be), -np.inf))
    return out


def random_grids(rng, n):
    dims = np.array([1, 2, 3, 4, 7, 32, 217, 1024])
    g = dims[rng.integers(0, len(dims), (n, 3))]
    h = np.exp(rng.uniform(np.log(0.01), np.log(10.0), n)).astype(F32)
    o = rng.uniform(-100.0, 100.0, (n, 3)).astype(F32)
    return o, h, g


def test_inclusion_random():
    """more than 10^6 random (grid, query, bd) triples: dims 1 .. 1024 per axis, queries up to 3 cells outside on every side, bd random
    around the thresholds and at the fp64 neighbours of the new, the present and the exact threshold"""
    rng = np.random.default_rng(7001)
    n = 1 << 20
    o, h, g = random_grids(rng, n)
    u = rng.uniform(0.0, 1.0, (n, 3)) * (g + 6.0) - 3.0           # cell units, [-3, g + 3)
    q = (o.astype(np.float64) + u * h.astype(np.float64)[:, None]).astype(F32)
    r = rng.uniform(0.0, 1.3, n) * h.astype(np.float64)
    n_new = check_chain(o, h, g, q, [r * r] + threshold_bds(), "random triples")
    assert n_new > n // 4, "the random triples hardly ever reach the quick accept"


def test_inclusion_half_cell_planes():
    """f at 0, 0.5 and 1 and the fp32 values next to them: grids with origin 0 and a power-of-two cell, where f is exact; in cell 0 the
    queries' neighbours ARE f's fp32 neighbours, in the other cells the nearest f that a query can have.  f = 1 is the query on the grid's
    upper face (clamped to the last cell)."""
    rows = []
    for gdim in (1, 2, 3, 8, 1024):
        for hval in (1.0, 0.5, 4.0):
            cells = sorted({0, 1, gdim // 2, gdim - 2, gdim - 1} & set(range(gdim)))
            for cidx in cells:
                for frac in (0.0, 0.5, 1.0):
                    x = F32((cidx + frac) * hval)
                    for k in range(-3, 4):
                        v = x
                        for _ in range(abs(k)):
                            v = np.nextafter(v, F32(np.inf) if k > 0 else F32(-np.inf))
                        rows.append((gdim, hval, v))
    rows = np.array(rows, np.float64)
    n = len(rows)
    rng = np.random.default_rng(7002)
    for axis in range(3):
        for other in (1, 2, 5):
            g = np.full((n, 3), other, np.int64)
            g[:, axis] = rows[:, 0].astype(np.int64)
            h = rows[:, 1].astype(F32)
            o = np.zeros((n, 3), F32)
            q = (rng.uniform(0.0, 1.0, (n, 3)) * other * rows[:, 1][:, None]).astype(F32)
            q[:, axis] = rows[:, 2].astype(F32)
            r = rng.uniform(0.0, 1.3, n) * rows[:, 1]
            check_chain(o, h, g, q, [r * r] + threshold_bds(), f"half-cell planes, axis {axis}")
    f, _, _, _ = block_of(np.zeros((n, 3), F32), (F32(1) / rows[:, 1].astype(F32)).astype(F32), np.tile(rows[:, :1].astype(np.int64), (1, 3)),
                          np.tile(rows[:, 2:3].astype(F32), (1, 3)))
    for v in (0.0, 0.5, 1.0):
        x = F32(v)
        for w in (x, np.nextafter(x, F32(np.inf)), np.nextafter(x, F32(-np.inf))):
            if w >= 0:
                assert (f[:, 0] == w).any(), f"f = {w!r} does not occur"


def test_inclusion_thin_grids():
    """grids of 1 and 2 cells along one, two or all three axes (a block that covers the whole grid among them)"""
    rng = np.random.default_rng(7003)
    n = 1 << 16
    for dims in ((1, 9, 9), (9, 1, 9), (9, 9, 1), (2, 9, 9), (9, 2, 9), (9, 9, 2), (1, 1, 9), (1, 2, 1), (1, 1, 1), (2, 2, 2), (2, 1, 2), (3, 2, 1)):
        o, h, _ = random_grids(rng, n)
        g = np.tile(np.array(dims, np.int64), (n, 1))
        u = rng.uniform(0.0, 1.0, (n, 3)) * (g + 6.0) - 3.0
        q = (o.astype(np.float64) + u * h.astype(np.float64)[:, None]).astype(F32)
        r = rng.uniform(0.0, 1.3, n) * h.astype(np.float64)
        check_chain(o, h, g, q, [r * r] + threshold_bds(), f"grid {dims}")
        if max(dims) <= 2:                                        # blocks that ARE the grid: the present form declines, the exact test accepts all
            hf = h.astype(F32)
            f, c, lo, hi = block_of(o, (F32(1) / hf).astype(F32), g, q)
            whole, _ = exact_bound(o, hf.astype(np.float64), g, q, lo, hi)
            assert whole.any() and (max(dims) > 1 or whole.all())
            assert np.all(present_threshold(f, c, lo, hi, g, hf.astype(np.float64))[whole] == 0.0)
            assert (new_threshold(f, hf.astype(np.float64))[whole] > 0.0).any()


def test_fast_route_kept():
    """uniform queries inside the grid at 6 points per cell: the new test accepts at least 95 % of what the present one accepts (they differ
    only where the block touches the grid's border, where the present form ignores the face without cells behind it).  A 10^3 grid, where
    half the cells are border cells; on the headline's 217^3 the share of such cells is 3 %."""
    rng = np.random.default_rng(7004)
    gd, ppc, nq = 10, 6, 8192
    pts = rng.uniform(0.0, gd, (gd ** 3 * ppc, 3)).astype(F32)
    q = rng.uniform(0.0, gd, (nq, 3)).astype(F32)
    g = np.tile(np.array([gd, gd, gd], np.int64), (nq, 1))
    o, h = np.zeros((nq, 3), F32), np.ones(nq, F32)
    hd = h.astype(np.float64)
    f, c, lo, hi = block_of(o, h, g, q)
    pc = np.minimum(np.floor(pts).astype(np.int64), gd - 1)
    bd = np.empty(nq)
    for s in range(0, nq, 512):
        e = min(s + 512, nq)
        inb = np.all((pc[None, :, :] >= lo[s:e, None, :]) & (pc[None, :, :] <= hi[s:e, None, :]), axis=2)
        d2 = ((pts[None, :, :].astype(np.float64) - q[s:e, None, :].astype(np.float64)) ** 2).sum(axis=2)
        bd[s:e] = np.where(inb, d2, np.inf).min(axis=1)
    a_new = accept(new_threshold(f, hd), bd)
    a_pre = accept(present_threshold(f, c, lo, hi, g, hd), bd)
    assert not (a_new & ~a_pre).any()
    share = a_new.sum() / a_pre.sum()
    interior = np.all((c >= 1) & (c <= gd - 2), axis=1)
    print(f"present accepts {a_pre.mean():.4f} of the queries, new {a_new.mean():.4f}: {share:.4f} of the present; interior cells: "
          f"{a_pre[interior].mean():.4f} / {a_new[interior].mean():.4f}")
    assert np.array_equal(a_new[interior], a_pre[interior]), "away from the border the two forms are the same test"
    assert share >= 0.95
