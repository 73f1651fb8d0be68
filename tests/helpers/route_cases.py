"""Inputs for the tests of the routed search's device phases: the same tables feed tests/test_route_model.py (the numpy model against a
scalar loop, no GPU) and tests/test_gpu_route_phases.py (the kernels against the model).  Everything is seeded and small."""
import numpy as np

NO_INDEX = 0xFFFFFFFF
INF, NAN = np.inf, np.nan
F32 = np.float32


def cuts_for(world, variant):
    """world + 1 boundaries, the inner ones fp32-representable and ascending, 0.0 among them; variant 1 repeats cuts (slabs no query
    can own)"""
    rng = np.random.default_rng(100 * world + variant)
    n = world - 1
    if n == 0:
        inner = np.empty(0)
    elif variant == 0 and n <= 32:
        inner = np.sort(rng.choice(np.arange(-16, 17) * 0.25, n, replace=False))      # distinct
        inner[np.argmin(np.abs(inner))] = 0.0
    else:
        inner = np.sort(rng.choice(np.arange(-16, 17) * 0.25, n, replace=True))       # 33 values: repeats whenever n > 1
        inner[np.argmin(np.abs(inner))] = 0.0
        if n > 1:
            inner[n // 2 - 1 if n // 2 else 0] = inner[n // 2]                                # at least one pair coincides
        inner = np.sort(inner)
    cuts = np.concatenate([[-INF], inner, [INF]]).astype(np.float64)
    assert (np.diff(cuts[1:-1]) >= 0).all() and (cuts[1:-1].astype(F32).astype(np.float64) == cuts[1:-1]).all()
    return cuts


def edge_coordinates(cuts):
    """every distinct inner cut, one fp32 ulp below it and one above; -0.0 (against the cut at 0.0); +-inf; NaN"""
    e = []
    for c in np.unique(cuts[1:-1]):
        c = F32(c)
        e += [c, np.nextafter(c, F32(-INF)), np.nextafter(c, F32(INF))]
    e += [F32(-0.0), F32(INF), F32(-INF), F32(NAN), F32(0.0)]
    return np.array(e, F32)


def owner_queries(cuts, axis, Q, seed):
    """Q x 3 fp32: random rows, the first ones carrying the edge coordinates on `axis`, some with NaN / inf on the OTHER axes (which
    must not matter, and must be copied bit for bit)"""
    rng = np.random.default_rng(seed)
    q = rng.uniform(-5, 5, (Q, 3)).astype(F32)
    e = edge_coordinates(cuts)
    if Q:
        k = min(Q, len(e))
        start = seed % len(e) if Q < len(e) else 0                 # a short batch still meets a different edge per seed
        q[:k, axis] = np.roll(e, -start)[:k]
        if Q > len(e):
            q[len(e):, axis] = np.where(rng.random(Q - len(e)) < 0.3, rng.choice(e, Q - len(e)), q[len(e):, axis])
        other = (axis + 1) % 3
        q[1::13, other] = F32(NAN)
        q[2::17, (axis + 2) % 3] = F32(-INF)
    return q


EDGE_VARIANTS = [(-1.3, 2.7), (-INF, 2.7), (-1.3, INF), (-INF, INF)]     # halo edges, not fp32-representable where finite


def certify_case(m, axis, edges, seed):
    """m rows cycling through the table below; returns the arguments of certify by name"""
    lo, hi = edges
    rng = np.random.default_rng(seed)
    G = 4096
    gid = rng.integers(0, 2 ** 31 - 1, G, dtype=np.int64).astype(np.uint32)      # non-identity, values up to 2^31 - 2
    gid[0], gid[1], gid[G - 1] = 2 ** 31 - 2, 0, 2 ** 31 - 2
    a, b = (lo if np.isfinite(lo) else -40.0), (hi if np.isfinite(hi) else 40.0)
    x = rng.uniform(a + 0.01, b - 0.01, m).astype(F32)                          # inside the halo's edges
    lidx = rng.integers(0, G, m, dtype=np.int64).astype(np.uint32)
    lidx[::5] = rng.choice([0, 1, G - 1], len(lidx[::5]))
    ld2 = np.empty(m, np.float64)
    NCASE = 14
    for i in range(m):
        c = i % NCASE
        if c == 4:                                                              # outside: margin < 0
            x[i] = F32(lo - 0.75) if np.isfinite(lo) else (F32(hi + 0.75) if np.isfinite(hi) else x[i])
        elif c == 7:
            x[i] = F32(NAN)
        elif c == 8:
            x[i] = F32(INF)
        elif c == 9:
            x[i] = F32(-INF)
    # (a query exactly ON an edge needs an fp32-representable edge: certify_on_the_edge below)
    xd = x.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        margin = np.fmin(xd - lo, hi - xd)
        m2 = margin * margin
    for i in range(m):
        c = i % NCASE
        t = m2[i] if np.isfinite(m2[i]) else 6.25
        if c == 0:
            ld2[i] = t                                                          # exactly margin * margin: NOT certified
        elif c == 1:
            ld2[i] = np.nextafter(t, 0.0)                                       # just below: certified
        elif c == 2:
            ld2[i] = np.nextafter(t, INF)
        elif c == 5:
            ld2[i] = 0.0                                                        # on top of a point, margin > 0
        elif c == 6:
            lidx[i] = NO_INDEX                                                  # nothing found, whatever d2 says
            ld2[i] = [0.0, 1e-3, INF][(i // NCASE) % 3]
        elif c == 11:
            ld2[i] = INF                                                        # found, infinitely far
        elif c == 12:
            ld2[i] = t * rng.uniform(0.0, 0.999)
        elif c == 13:
            ld2[i] = t * rng.uniform(1.001, 3.0)
        else:
            ld2[i] = rng.uniform(0.0, 0.01)
    mine_ids = rng.permutation(3 * m + 5)[:m].astype(np.uint32)
    return dict(axis=axis, lo_edge=float(lo), hi_edge=float(hi), mine_q=_rows(x, axis, rng), mine_ids=mine_ids, lidx=lidx, ld2=ld2, gid=gid)


def certify_on_the_edge(axis, seed=3):
    """margin == 0 exactly: fp32-representable edges, queries ON them (d2 = 0: 0 < 0 * 0 is false, and margin > 0 is false) and one
    ulp inside (d2 = 0 is then certified)"""
    rng = np.random.default_rng(seed)
    lo, hi = -1.25, 2.5
    x = np.array([lo, hi, np.nextafter(F32(lo), F32(INF)), np.nextafter(F32(hi), F32(-INF)), np.nextafter(F32(lo), F32(-INF)),
                  np.nextafter(F32(hi), F32(INF))], F32)
    m = len(x)
    gid = (np.arange(16, dtype=np.uint32) * 7 + 3)
    return dict(axis=axis, lo_edge=lo, hi_edge=hi, mine_q=_rows(x, axis, rng), mine_ids=np.arange(m, dtype=np.uint32)[::-1].copy(),
                lidx=np.arange(m, dtype=np.uint32), ld2=np.zeros(m), gid=gid)


def _rows(x, axis, rng):
    q = rng.uniform(-50, 50, (len(x), 3)).astype(F32)
    q[:, axis] = x
    q[::9, (axis + 1) % 3] = F32(NAN)                                           # the other axes do not matter
    return q


def records(n, n_out, flagged, seed):
    """n answer records in a random order, one per query of a random n-subset of [0, n_out); `flagged` is "none", "all" or "some"
    (about 1 %): those carry NO_INDEX and d2 = -1"""
    from route_model import RECORD
    rng = np.random.default_rng(seed)
    rec = np.empty(n, RECORD)
    rec["query"] = rng.permutation(n_out)[:n].astype(np.uint32)
    rec["gid"] = rng.integers(0, 2 ** 31 - 1, n, dtype=np.int64).astype(np.uint32)
    rec["d2"] = rng.uniform(0, 100, n)
    if n:
        rec["d2"][rng.integers(0, n)] = 0.0                                     # d2 == 0 is an answer, not a flag
    f = np.zeros(n, bool) if flagged == "none" else np.ones(n, bool) if flagged == "all" else rng.random(n) < 0.01
    rec["gid"][f] = NO_INDEX
    rec["d2"][f] = -1.0
    return rec
