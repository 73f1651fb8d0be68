"""The arithmetic contract of include/pct_engine.h at the edges of the fp32 range: the shared case generator (imported by
tests/test_gpu_numeric_edges.py) and the CPU tests that pin what "right" means there before any GPU is involved.

The contract: coordinates are fp32, every deciding distance is the fp64 value ((dx*dx + dy*dy) + dz*dz) of the widened operands
with one rounding per operation, lowest index on ties, d2 <= (double)r * (double)r inclusive.  That value is finite for every pair
of finite floats (at most 3 * (2 * FLT_MAX)^2 ~ 1.4e78), so the answer is defined for ANY finite cloud and query; for non-finite
operands it is what the comparisons imply (a NaN or infinite d2 is never < +inf and never <= a finite r*r).

Every case is a fixed-seed (cloud, queries, radii) triple.  Families (CASES below): scale ladder, far queries, sentinels, tiny,
radii; the non-finite families (NONFINITE_QUERY_CASES, NONFINITE_ROW_CASES) are kept apart because the engine answers some of
their index builds with an error status.  The conditions a case must satisfy to keep biting are assertions in the tests below.
"""
import functools
from fractions import Fraction

import numpy as np
import pytest

FLT_MAX = np.float32(3.4028234663852886e38)
SQRT_FLT_MAX = 1.8446743e19          # fp32 squared distances overflow beyond this separation
NO_INDEX = -1                        # oracle's "no point" (the engine reports PCT_NO_INDEX = 0xFFFFFFFF)
SCALES = [1e-30, 1e-12, 1.0, 1e6, 1e12, 1e18, 3e19, 1e25, 1e38]


class Case:
    """One cloud with its queries.  radii: one per query.  inside: queries drawn inside the cloud's bounding box (cheap for the
    cell-pruned search, the ones batch-size variants replicate).  meta: what the family's conditions are checked against."""

    def __init__(self, name, family, pts, queries, radii, inside, **meta):
        self.name, self.family = name, family
        self.pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
        self.queries = np.ascontiguousarray(queries, np.float32).reshape(-1, 3)
        self.radii = np.ascontiguousarray(radii, np.float32).reshape(-1)
        self.inside = np.ascontiguousarray(inside, bool).reshape(-1)
        self.meta = meta
        assert len(self.radii) == len(self.queries) == len(self.inside)

    def __repr__(self):
        return self.name


# ---- the reference, twice ----------------------------------------------------------------------------------------------------

def numpy_d2(pts, q):
    """[len(q), len(pts)] fp64 squared distances in the contract's operation order (numpy evaluates each ufunc with one rounding)"""
    P = pts.astype(np.float64)
    Q = q.astype(np.float64)
    with np.errstate(all="ignore"):
        dx = P[None, :, 0] - Q[:, None, 0]
        s = dx * dx
        dy = P[None, :, 1] - Q[:, None, 1]
        s = s + dy * dy
        dz = P[None, :, 2] - Q[:, None, 2]
        s = s + dz * dz
    return s


def numpy_nearest(pts, q, chunk=16):
    """(idx, d2) by the contract: minimum over s < best starting from best = +inf, lowest index among equal minima; a query no
    point is < +inf from (NaN / infinite operands) gets (-1, +inf)"""
    idx = np.empty(len(q), np.int64)
    d2 = np.empty(len(q), np.float64)
    for a in range(0, len(q), chunk):
        s = numpy_d2(pts, q[a:a + chunk])
        s = np.where(np.isnan(s), np.inf, s)
        i = np.argmin(s, axis=1)                       # first occurrence = lowest index
        m = s[np.arange(len(i)), i]
        idx[a:a + chunk] = np.where(m < np.inf, i, NO_INDEX)
        d2[a:a + chunk] = m
    return idx, d2


def numpy_count(pts, q, r, chunk=16):
    r2 = r.astype(np.float64) * r.astype(np.float64)
    out = np.empty(len(q), np.int64)
    for a in range(0, len(q), chunk):
        with np.errstate(all="ignore"):
            out[a:a + chunk] = (numpy_d2(pts, q[a:a + chunk]) <= r2[a:a + chunk, None]).sum(axis=1)
    return out


def numpy_ties(pts, q, chunk=16):
    """how many points attain each query's minimum"""
    out = np.empty(len(q), np.int64)
    for a in range(0, len(q), chunk):
        s = numpy_d2(pts, q[a:a + chunk])
        s = np.where(np.isnan(s), np.inf, s)
        out[a:a + chunk] = (s == s.min(axis=1, keepdims=True)).sum(axis=1)
    return out


def exact_chain_d2(p, q):
    """the same chain in rational arithmetic, rounded to fp64 after every operation (float(Fraction) rounds correctly)"""
    sq = []
    for k in range(3):
        d = float(Fraction(float(p[k])) - Fraction(float(q[k])))
        sq.append(float(Fraction(d) * Fraction(d)))
    s = float(Fraction(sq[0]) + Fraction(sq[1]))
    return float(Fraction(s) + Fraction(sq[2]))


# ---- building blocks -----------------------------------------------------------------------------------------------------------

def _scale12(s):
    """s as an fp32 with a 12-bit significand: products with integers below 4096 are exact, so a dyadic lattice stays a lattice
    (and its mirror-image ties stay exact) at every rung of the ladder"""
    m, e = np.frexp(np.float64(np.float32(s)))
    return np.float32(np.ldexp(np.floor(m * 4096.0) / 4096.0, e))


def _f32_finite(a):
    a = np.asarray(a, np.float64)
    assert np.all(np.abs(a) <= float(FLT_MAX)), "generator bug: coordinate beyond the fp32 range"
    return a.astype(np.float32)


def _radii_for(pts, q, rng):
    """per-query radii that bite: the fp32 neighbours of the exact NN distance (the inclusive boundary), a multiple of it, zero"""
    _, d2 = numpy_nearest(pts, q)
    with np.errstate(all="ignore"):
        d = np.sqrt(d2)
    r = np.minimum(d, float(FLT_MAX)).astype(np.float32)
    kind = rng.integers(0, 4, len(q))
    with np.errstate(all="ignore"):
        r = np.where(kind == 1, np.nextafter(r, np.float32(np.inf)), r)
        r = np.where(kind == 2, np.minimum(r.astype(np.float64) * 3.0, float(FLT_MAX)).astype(np.float32), r)
    r = np.where(kind == 3, np.float32(0.0), r)
    return np.where(np.isfinite(r), r, FLT_MAX).astype(np.float32)


def ordinary_cloud(seed, n, ext):
    """uniform points in [0, ext]^3 with a few bulk duplicates at the end"""
    rng = np.random.default_rng(seed)
    p = (rng.random((n, 3)) * ext).astype(np.float32)
    ndup = min(16, n // 4)
    if ndup:
        p[n - ndup:] = p[rng.integers(0, n - ndup, ndup)]
    return p


def _ordinary_queries(pts, rng, n_in=16, n_on=8):
    """queries inside the box (unique minimisers, generically) and on points (the duplicated rows among them: exact ties)"""
    lo, hi = pts.min(0).astype(np.float64), pts.max(0).astype(np.float64)
    inside = (lo + rng.random((n_in, 3)) * (hi - lo)).astype(np.float32)
    on = np.concatenate([pts[-(n_on // 2):], pts[rng.integers(0, len(pts), n_on - n_on // 2)]])
    return np.concatenate([inside, on])


# ---- family: scale ladder ------------------------------------------------------------------------------------------------------

def _unit_pattern(n_uniform=30_000):
    """unit pattern in [-1, 1]^3, as (fp64 coordinates of the rounded rows, integer numerators of the dyadic rows):
    uniform points, a 0.1-lattice (8^3 nodes), a dyadic lattice k/64 (5^3 nodes, mirror-symmetric: exact ties at every scale) and
    64 duplicated rows"""
    rng = np.random.default_rng(20250101)
    uni = rng.random((n_uniform, 3)) * 2.0 - 1.0
    k = np.arange(8) - 4
    lat = np.stack(np.meshgrid(k, k, k, indexing="ij"), -1).reshape(-1, 3) * 0.1 + 0.05
    m = np.arange(-2, 3) * 16                                  # numerators of k / 64: -32 .. 32
    dy = np.stack(np.meshgrid(m, m, m, indexing="ij"), -1).reshape(-1, 3)
    return rng, uni, lat, dy


@functools.lru_cache(maxsize=None)
def scale_ladder_case(s, offset):
    rng, uni, lat, dy = _unit_pattern()
    s12 = np.float64(_scale12(s))
    off = 1.0 if offset else 0.0                               # an offset of the same order: the pattern then spans [0, 2] s
    body = _f32_finite((np.concatenate([uni, lat]) + off) * s12)
    dyad = _f32_finite((dy + 64.0 * off) * (s12 / 64.0))       # exact: integers below 4096 times a 12-bit significand
    assert np.array_equal(dyad.astype(np.float64), (dy + 64.0 * off) * (s12 / 64.0))
    pts = np.concatenate([body, dyad])
    dup = pts[rng.integers(0, len(pts), 64)]
    pts = np.concatenate([pts, dup])
    lo, hi = (off - 1.0) * s12, (off + 1.0) * s12
    inside = _f32_finite(lo + rng.random((24, 3)) * (hi - lo))
    on = np.concatenate([dup[:4], body[rng.integers(0, len(body), 4)]])
    # midpoints between two dyadic neighbours along x (numerators -8 and +8 around 0, +-16 the neighbours): equidistant, exact
    mid_num = np.array([[-8, 0, 0], [8, 16, -16], [24, -32, 32], [-24, 32, 0]], np.float64)
    mid = _f32_finite((mid_num + 64.0 * off) * (s12 / 64.0))
    q = [inside, on, mid]
    n_out = 0
    if 82.0 * s12 <= float(FLT_MAX):                           # 40 extents outside, where that is still finite
        out = _f32_finite((off + rng.choice([-1.0, 1.0], (6, 3)) * 80.0 * rng.random((6, 3)).clip(0.5)) * s12)
        q.append(out)
        n_out = len(out)
    q = np.concatenate(q)
    ins = np.zeros(len(q), bool)
    ins[:len(inside) + len(on) + len(mid)] = True
    name = f"ladder/s={s:g}/{'offset' if offset else 'centred'}" + ("" if n_out else "/no-outside-queries(overflow)")
    return Case(name, "ladder", pts, q, _radii_for(pts, q, rng), ins, scale=s, n_inside=len(inside), n_outside=n_out)


# ---- family: far queries -------------------------------------------------------------------------------------------------------

def far_distances():
    """1e18, sqrt(FLT_MAX) -/+ a few ulp-scale steps (2^64 and its fp32 neighbours), 3e19, 1e30, FLT_MAX"""
    t = np.float32(2.0 ** 64)
    steps = [t]
    lo = hi = t
    for _ in range(3):
        lo, hi = np.nextafter(lo, np.float32(0)), np.nextafter(hi, np.float32(np.inf))
        steps += [lo, hi]
    return np.float32([1e18] + sorted(steps) + [3e19, 1e30, FLT_MAX])


def _far_queries(pts):
    """far along +x sharing row 0's y and z (both signs for small clouds would need two extreme rows: the sign is +x, and row 0
    is the extreme row along +x), along the diagonal, and with only y far"""
    D = far_distances()
    y0, z0 = pts[0, 1], pts[0, 2]
    axis = np.stack([D, np.full_like(D, y0), np.full_like(D, z0)], 1)
    diag = np.stack([D, D, D], 1)
    mid = pts[len(pts) // 2]
    one = np.stack([np.full_like(D, mid[0]), -D, np.full_like(D, mid[2])], 1)
    return axis, diag, one


@functools.lru_cache(maxsize=None)
def far_query_case(n, ext):
    rng = np.random.default_rng(4000 + n + int(ext))
    pts = ordinary_cloud(500 + n, n, ext)
    i = int(np.argmax(pts[:, 0]))                              # row 0 := THE extreme row along +x (strictly: no other row shares its x)
    pts[[0, i]] = pts[[i, 0]]
    pts[0, 0] = np.nextafter(pts[:, 0].max(), np.float32(np.inf))
    axis, diag, one = _far_queries(pts)
    near = _ordinary_queries(pts, rng) if n >= 17 else np.concatenate([pts[:1], pts[-1:] + np.float32(0.25)])
    q = np.concatenate([near, axis, diag, one])
    ins = np.zeros(len(q), bool)
    ins[:len(near)] = True
    name = f"far/n={n}/ext={ext:g}" + ("/no-tie(one point)" if n == 1 else "")
    return Case(name, "far", pts, q, _radii_for(pts, q, rng), ins, n_near=len(near), n_axis=len(axis), small=n <= 100)


# ---- family: sentinels ---------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def sentinel_case(kind):
    """an ordinary cloud plus "invalid return" rows at the edge of the fp32 range"""
    rng = np.random.default_rng({"fltmax-all-1": 7001, "fltmax-x-64": 7002, "1e38-all-64": 7003, "fltmax-mixed-5": 7004}[kind])
    base = ordinary_cloud(611, 30_000, 10.0)
    if kind == "fltmax-all-1":
        sent, at = np.float32([[FLT_MAX, FLT_MAX, FLT_MAX]]), "end"
    elif kind == "fltmax-x-64":
        sent = base[rng.integers(0, len(base), 64)].copy()
        sent[:, 0] = np.where(np.arange(64) % 2 == 0, FLT_MAX, -FLT_MAX)
        at = "inside"
    elif kind == "1e38-all-64":
        sent = (rng.choice([-1.0, 1.0], (64, 3)) * 1e38).astype(np.float32)
        at = "start"
    else:
        sent = np.float32([[FLT_MAX, 0, 0], [-FLT_MAX, -FLT_MAX, -FLT_MAX], [0, 1e38, 0], [1e38, -1e38, FLT_MAX], [0, 0, -FLT_MAX]])
        at = "inside"
    if at == "start":
        pts = np.concatenate([sent, base])
    elif at == "end":
        pts = np.concatenate([base, sent])
    else:
        pts = np.concatenate([base[:12_345], sent, base[12_345:]])
    near = _ordinary_queries(base, rng, 24, 8)
    # around the sentinels: a little inside of each of (up to) 6 of them, and between them (the origin-side middle of the range)
    pick = sent[:: max(1, len(sent) // 6)][:6].astype(np.float64)
    around = _f32_finite(pick * (1.0 - 2.0 ** -20 * rng.integers(1, 64, (len(pick), 1))))
    between = np.float32([[1e37, -2e37, 3e37], [-5e37, 5e37, 5e37], [1e38, 0, 0], [0, -3e38, 1.0]])
    q = np.concatenate([near, around, between])
    ins = np.zeros(len(q), bool)
    ins[:len(near)] = True
    return Case(f"sentinels/{kind}/{at}", "sentinels", pts, q, _radii_for(pts, q, rng), ins, n_near=len(near))


# ---- family: tiny --------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def tiny_case(kind):
    rng = np.random.default_rng({"extent-1e-30": 8001, "subnormal": 8002}[kind])
    if kind == "extent-1e-30":
        s12 = np.float64(_scale12(1e-30))
        uni = _f32_finite(rng.random((2000, 3)) * s12)
        k = np.arange(0, 65, 16)
        dy = np.stack(np.meshgrid(k, k, k, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
        dyad = _f32_finite(dy * (s12 / 64.0))
        pts = np.concatenate([uni, dyad, uni[:16]])
        mid = _f32_finite(np.float64([[8, 0, 0], [24, 16, 48], [56, 64, 32]]) * (s12 / 64.0))
        q = np.concatenate([_f32_finite(rng.random((16, 3)) * s12), pts[-4:], uni[100:104], mid])
        name = "tiny/extent-1e-30"
    else:
        # integer multiples of the smallest subnormal 2^-149 (all arithmetic on them is exact in fp64), both signs, and signed
        # zeros: rows 3 and 7 are (0, 0, 0) and (-0, -0, -0) -- they must tie, for queries of either sign
        u = np.float64(2.0 ** -149)
        k = rng.integers(-1000, 1001, (1500, 3)).astype(np.float64)
        pts = (k * u).astype(np.float32)
        pts[3] = np.float32([0.0, 0.0, 0.0])
        pts[7] = np.float32([-0.0, -0.0, -0.0])
        pts[-8:] = pts[100:108]
        assert np.array_equal(pts[8:-8].astype(np.float64), (k * u)[8:-8]), "multiples of 2^-149 are exact in fp32"
        zq = np.float32([[0.0, 0.0, 0.0], [-0.0, -0.0, -0.0], [-0.0, 0.0, -0.0]])
        q = np.concatenate([(rng.integers(-1200, 1201, (16, 3)) * u).astype(np.float32), zq, pts[-4:], pts[200:204]])
        name = "tiny/subnormal+signed-zeros"
    return Case(name, "tiny", pts, q, _radii_for(pts, q, rng), np.ones(len(q), bool))


# ---- family: radii -------------------------------------------------------------------------------------------------------------

SPECIAL_RADII = np.float32([0.0, 1e-42, 1e19, 1e30, FLT_MAX, np.inf, np.nan, -1.5, -1e30, -np.inf])


@functools.lru_cache(maxsize=None)
def radii_case(n):
    """every special radius for queries inside and far; r = +inf and NaN are part of the contract (d2 <= +inf holds for every
    finite d2, nothing is <= NaN), a negative radius enters only squared"""
    rng = np.random.default_rng(9000 + n)
    pts = ordinary_cloud(9100 + n, n, 10.0)
    base = np.concatenate([_ordinary_queries(pts, rng, 3, 2), np.float32([[1e19, 5, 5], [3e19, 3e19, 3e19], [FLT_MAX, 0, 0], [5, -1e30, 5]])])
    q = np.repeat(base, len(SPECIAL_RADII), axis=0)
    r = np.tile(SPECIAL_RADII, len(base))
    ins = np.repeat(np.arange(len(base)) < 5, len(SPECIAL_RADII))
    return Case(f"radii/n={n}", "radii", pts, q, r, ins)


def finite_cases():
    cs = [scale_ladder_case(s, o) for s in SCALES for o in (False, True)]
    cs += [far_query_case(n, ext) for n, ext in ((1, 10.0), (2, 10.0), (17, 10.0), (100, 10.0), (30_000, 10.0), (200_000, 3000.0))]
    cs += [sentinel_case(k) for k in ("fltmax-all-1", "fltmax-x-64", "1e38-all-64", "fltmax-mixed-5")]
    cs += [tiny_case(k) for k in ("extent-1e-30", "subnormal")]
    cs += [radii_case(n) for n in (100, 30_000)]
    return cs


CASES = finite_cases()
CASE_IDS = [c.name for c in CASES]


# ---- non-finite families -------------------------------------------------------------------------------------------------------

def nonfinite_triples():
    """NaN / +inf / -inf in one, two or all coordinates"""
    out = []
    for v in (np.nan, np.inf, -np.inf):
        for mask in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 1, 1)):
            out.append([v if m else 4.5 for m in mask])
    out += [[np.inf, -np.inf, np.nan], [np.nan, 4.5, np.inf]]
    return np.float32(out)


def nonfinite_positions(Q):
    """first, last, every 8th of the first two waves' worth of queries, and a run of 64 (two blocks of the batch kernel)"""
    pos = {0, Q - 1} | set(range(8, 129, 8))
    start = min(1000, Q // 2)
    pos |= set(range(start, min(start + 64, Q - 1)))
    return np.array(sorted(p for p in pos if 0 <= p < Q), np.int64)


@functools.lru_cache(maxsize=None)
def nonfinite_query_case(Q):
    """a batch of ordinary queries with non-finite ones mixed in; meta: where they sit, and the batch without them"""
    rng = np.random.default_rng(10_000 + Q)
    pts = ordinary_cloud(10_100, 30_000, 10.0)
    q = (rng.random((Q, 3)) * 10.0).astype(np.float32)
    q[: min(4, Q)] = pts[-4:][: min(4, Q)]
    pos = nonfinite_positions(Q)
    bad = nonfinite_triples()
    clean = q.copy()
    q[pos] = bad[np.arange(len(pos)) % len(bad)]
    r = np.full(Q, 0.7, np.float32)
    return Case(f"nonfinite-queries/Q={Q}", "nonfinite-queries", pts, q, r, ~np.isin(np.arange(Q), pos), positions=pos, clean=clean)


NONFINITE_QUERY_CASES = [nonfinite_query_case(Q) for Q in (7, 600, 2048, 20_000)]      # express, express, unbinned, binned batches


@functools.lru_cache(maxsize=None)
def nonfinite_rows_case(k, where):
    rng = np.random.default_rng(11_000 + k)
    base = ordinary_cloud(11_100, 30_000, 10.0)
    bad = nonfinite_triples()[np.arange(k) % len(nonfinite_triples())]
    bad = np.where(bad == np.float32(4.5), base[:k], bad).astype(np.float32)     # finite coordinates of a bad row: those of a real point
    at = {"start": 0, "end": len(base), "inside": 17_001}[where]
    pts = np.concatenate([base[:at], bad, base[at:]])
    q = np.concatenate([_ordinary_queries(base, rng, 24, 8), base[:4] + np.float32(1e-3), np.float32([[40, -30, 5], [1e19, 5, 5]])])
    r = np.concatenate([np.full(len(q) - 4, 0.7, np.float32), np.float32([np.inf, -np.inf, 1e30, FLT_MAX])])
    ins = np.ones(len(q), bool)
    ins[-2:] = False
    return Case(f"nonfinite-rows/k={k}/{where}", "nonfinite-rows", pts, q, r, ins, bad_rows=np.arange(at, at + k))


NONFINITE_ROW_CASES = [nonfinite_rows_case(1, "start"), nonfinite_rows_case(64, "inside"), nonfinite_rows_case(5, "end")]


# ---- expected results (shared with the GPU file) --------------------------------------------------------------------------------

_expected = {}


def expected(case, O):
    """(idx int64 with -1 = none, d2, counts) from the C oracle, cached per case"""
    if case.name not in _expected:
        i, d = O.brute_nearest(case.pts, case.queries)
        c = O.brute_count(case.pts, case.queries, case.radii)
        _expected[case.name] = (i.astype(np.int64), d, c.astype(np.int64))
    return _expected[case.name]


# ================================================================================================================================
# CPU tests
# ================================================================================================================================

ALL_CASES = CASES + NONFINITE_QUERY_CASES + NONFINITE_ROW_CASES


@pytest.mark.parametrize("case", ALL_CASES, ids=[c.name for c in ALL_CASES])
def test_oracle_equals_numpy_fp64(oracle, case):
    """oracle.brute_nearest / brute_count (oracle/kdtree_port.c) against an independent numpy evaluation of the same chain"""
    ei, ed, ec = expected(case, oracle)
    ni, nd = numpy_nearest(case.pts, case.queries)
    assert np.array_equal(ed, nd), case.name
    assert np.array_equal(ei, ni), case.name
    assert np.array_equal(ec, numpy_count(case.pts, case.queries, case.radii)), case.name
    if case in CASES:
        assert np.all(np.isfinite(case.pts)) and np.all(np.isfinite(case.queries)), "a finite family must be finite"
        assert np.all(np.isfinite(ed)) and np.all(ei >= 0), "every finite pair has a finite fp64 d2 (<= 1.4e78)"


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_fp64_value_is_the_correctly_rounded_chain(oracle, case):
    """a sample of (query, winner) and (query, arbitrary row) pairs in exact rational arithmetic, rounded after every operation:
    the oracle's d2 is that value, not an artefact of the C compiler (x87 excess precision, contraction) or of numpy"""
    ei, ed, _ = expected(case, oracle)
    rng = np.random.default_rng(5)
    for j in rng.choice(len(case.queries), min(12, len(case.queries)), replace=False):
        assert exact_chain_d2(case.pts[ei[j]], case.queries[j]) == ed[j], (case.name, j)
        k = int(rng.integers(0, len(case.pts)))
        assert exact_chain_d2(case.pts[k], case.queries[j]) == numpy_d2(case.pts[k:k + 1], case.queries[j:j + 1])[0, 0]
        assert exact_chain_d2(case.pts[k], case.queries[j]) >= ed[j]


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_every_case_has_a_unique_minimiser_and_an_exact_tie(case):
    """... between DIFFERENT indices, except where the family makes that impossible (the case's name says so)"""
    ties = numpy_ties(case.pts, case.queries)
    assert np.any(ties == 1), f"{case.name}: no query with a unique minimiser"
    if "no-tie" in case.name:
        assert len(case.pts) == 1
    else:
        assert np.any(ties >= 2), f"{case.name}: no query with an exact fp64 tie"


def test_scale_ladder_covers_the_rungs_and_overflows_fp32_where_it_should():
    names = {(c.meta["scale"], "offset" in c.name) for c in CASES if c.family == "ladder"}
    assert names == {(s, o) for s in SCALES for o in (False, True)}
    for c in (c for c in CASES if c.family == "ladder"):
        n_in = c.meta["n_inside"]
        _, d2 = numpy_nearest(c.pts, c.queries[:n_in])
        over = float(np.mean(d2 > float(FLT_MAX)))
        if c.meta["scale"] >= 1e25:
            assert over >= 0.5, f"{c.name}: only {over:.0%} of the queries inside the cloud have a NN d2 beyond FLT_MAX"
        if c.meta["scale"] <= 1e18:
            assert over == 0.0
        if c.meta["scale"] <= 1e-30:                       # every fp32 screening distance underflows below the near-tie band's 2^-90
            assert np.all(d2 < 2.0 ** -90)
        assert (c.meta["n_outside"] > 0) == (82.0 * c.meta["scale"] <= float(FLT_MAX))


def test_far_query_family_conditions():
    far = [c for c in CASES if c.family == "far"]
    assert sorted(len(c.pts) for c in far) == [1, 2, 17, 100, 30_000, 200_000]
    D = far_distances()
    assert D[0] == np.float32(1e18) and D[-1] == FLT_MAX and np.float32(2.0 ** 64) in D
    assert np.sum(D.astype(np.float64) ** 2 > float(FLT_MAX)) >= 6 and np.sum(D.astype(np.float64) ** 2 <= float(FLT_MAX)) >= 4
    for c in far:
        if c.meta["small"]:
            # at most 3 cells per axis at 6 points per cell over a roughly cubic cloud (engine.hip: h = cbrt(vol * 6 / n))
            ext = (c.pts.max(0) - c.pts.min(0)).astype(np.float64)
            if len(c.pts) > 1:
                d = max(ext.max(), 1e-6)
                h = np.cbrt(np.prod(np.maximum(ext, d * 1e-3)) * 6.0 / len(c.pts))
                assert np.all(np.floor(ext / h) + 1 <= 3), c.name
            continue
        a0 = c.meta["n_near"]
        axis = c.queries[a0:a0 + c.meta["n_axis"]]
        assert np.all(c.pts[0, 0] > c.pts[1:, 0]), "row 0 is the extreme row along +x"
        assert np.all(axis[:, 1] == c.pts[0, 1]) and np.all(axis[:, 2] == c.pts[0, 2]) and np.all(axis[:, 0] > c.pts[0, 0])
        ai, _ = numpy_nearest(c.pts, axis)
        ties = numpy_ties(c.pts, axis)
        assert np.all(ai == 0), "the all-points tie is won by index 0, the row in the cell the query is clamped to"
        # extent 10: every point is at ONE fp64 distance from a query 1e18 or more away (the coordinates vanish below the ulp of
        # the difference); extent 3000: thousands of rows still tie at 1e18 (ulp 128), all of them from 1e30 on
        assert np.all(ties >= 1000) and np.all(ties[axis[:, 0] >= 1e30] == len(c.pts))
        if np.ptp(c.pts[:, 0]) <= 10.0:
            assert np.all(ties == len(c.pts))


def test_sentinel_and_tiny_family_conditions():
    for c in (c for c in CASES if c.family == "sentinels"):
        big = np.abs(c.pts).max(axis=1) >= 1e38
        assert 1 <= big.sum() <= 64 and len(c.pts) - big.sum() == 30_000
        i, _ = numpy_nearest(c.pts, c.queries)
        assert np.any(big[i]) and np.any(~big[i]), "queries around the sentinels and around the ordinary part"
    sub = tiny_case("subnormal")
    assert np.all(np.abs(sub.pts) < np.finfo(np.float32).tiny) and np.any(np.signbit(sub.pts[7])) and not np.any(np.signbit(sub.pts[3]))
    i, d = numpy_nearest(sub.pts, np.float32([[0.0, 0.0, 0.0], [-0.0, -0.0, -0.0], [-0.0, 0.0, -0.0]]))
    assert np.all(i == 3) and np.all(d == 0.0), "-0.0 and 0.0 tie: the lower index wins whatever the signs"
    tiny = tiny_case("extent-1e-30")
    assert np.all(numpy_d2(tiny.pts, tiny.queries).astype(np.float32) == 0), "every fp32 squared distance underflows to 0"


def test_oracle_on_nonfinite_operands(oracle):
    """what the contract's comparisons imply, asserted explicitly"""
    for c in NONFINITE_QUERY_CASES:
        ei, ed, ec = expected(c, oracle)
        pos = c.meta["positions"]
        assert not np.any(np.isfinite(c.queries[pos]).all(axis=1)) and np.isfinite(np.delete(c.queries, pos, 0)).all()
        assert np.all(ei[pos] == NO_INDEX) and np.all(ed[pos] == np.inf), "no point is < +inf from a NaN / infinite query"
        assert np.all(ec[pos] == 0), "and none is within a finite radius"
        ci, cd = oracle.brute_nearest(c.pts, c.meta["clean"])
        keep = c.inside
        assert np.array_equal(ei[keep], ci[keep]) and np.array_equal(ed[keep], cd[keep]), "the ordinary queries are unaffected"
        has_nan = np.isnan(c.queries[pos]).any(axis=1)
        cinf = oracle.brute_count(c.pts, c.queries[pos], np.inf)
        assert np.all(cinf[has_nan] == 0), "NaN <= +inf is false"
        assert np.all(cinf[~has_nan] == len(c.pts)), "an infinite query without a NaN term: d2 = +inf <= r*r = +inf for every point"
    for c in NONFINITE_ROW_CASES:
        ei, ed, ec = expected(c, oracle)
        bad = c.meta["bad_rows"]
        good = np.delete(c.pts, bad, axis=0)
        gi, gd = oracle.brute_nearest(good, c.queries)
        remap = np.delete(np.arange(len(c.pts)), bad)
        assert not np.any(np.isin(ei, bad)), "a NaN / infinite row is never the winner"
        assert np.array_equal(ed, gd) and np.array_equal(ei, remap[gi])
        gc = oracle.brute_count(good, c.queries, c.radii).astype(np.int64)
        r2inf = np.isinf(c.radii.astype(np.float64) ** 2)
        assert np.array_equal(ec[~r2inf], gc[~r2inf]), "... and is never counted under a finite r*r"
        n_inf_rows = int((~np.isnan(c.pts[bad]).any(axis=1)).sum())            # infinite without a NaN: d2 = +inf <= +inf
        assert np.array_equal(ec[r2inf], gc[r2inf] + n_inf_rows)
    c = radii_case(100)
    _, _, ec = expected(c, oracle)
    r = c.radii
    assert np.all(ec[np.isnan(r)] == 0), "NaN radius: nothing is inside"
    assert np.all(ec[np.isinf(r)] == len(c.pts)), "r*r = +inf: every finite d2 is inside"
    neg = oracle.brute_count(c.pts, c.queries, -np.abs(r))
    pos_ = oracle.brute_count(c.pts, c.queries, np.abs(r))
    assert np.array_equal(neg, pos_), "a negative radius counts as |r|"
    inside_q = c.inside & (r == 0)
    assert np.all(ec[inside_q] <= 16 + 1)


def test_planner_points_beyond_fp32_narrow_to_infinity():
    """pct_inflate_batch narrows fp64 planner points to fp32: |p| > FLT_MAX becomes +/-inf, i.e. a non-finite query"""
    with np.errstate(over="ignore"):
        p = np.float64([3.5e38, -1e300, 3.4028234e38]).astype(np.float32)
    assert np.isposinf(p[0]) and np.isneginf(p[1]) and np.isfinite(p[2])
