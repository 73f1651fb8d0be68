"""CPU test: the batch sort's bin of a query (csrc/query_bin.hpp), by the shipped function compiled for the host and reached through
pct_debug_query_bins (no device is touched), against a numpy-float32 restatement of the definition:

    cell_coord = int(fmin(fmax(floor((v - o) * inv_h), 0), g - 1))  per axis,  c >>= shift,
    s, yin = cy // strip, cy % strip,   bin = ((s * bz + cz) * strip + yin) * bx + cx        (32-bit unsigned)

The host chooses between two forms per grid (the definition, and one without division or 32-bit multiplies for grids whose row count
and bx stay below 2^24); both must give the definition's bin bit for bit for every fp32 query, and every bin must be below nbins: the
sort kernels index a histogram with it.  (Dimensions are kept to those whose g - 1 is an fp32 number: beyond 2^24 + 1 cells per axis
the definition's own clamp (float)(g - 1) can round up past the last cell; the index build makes at most 1025 cells per axis.)"""
import ctypes as C
import itertools

import numpy as np
import pytest

F32 = np.float32
FLT_MAX = np.finfo(np.float32).max
DENORM = np.float32(1e-45)


@pytest.fixture(scope="module")
def lib():
    from pointcloudtraj_amd import build, engine
    build.build_all()
    return engine.lib()


def shipped_bins(lib, dims, origin, inv_h, shift, strip, q):
    d = (C.c_int32 * 3)(*dims)
    o = (C.c_float * 3)(*[float(v) for v in origin])
    q = np.ascontiguousarray(q, dtype=np.float32)
    bins = np.full(len(q), 0xFFFFFFFF, dtype=np.uint32)
    nbins, fast = C.c_uint32(0), C.c_int(-1)
    rc = lib.pct_debug_query_bins(d, o, C.c_float(float(inv_h)), int(shift), int(strip), q.ctypes.data, len(q), bins.ctypes.data,
                                  C.byref(nbins), C.byref(fast))
    assert rc == 0
    return bins, nbins.value, fast.value


def layout(dims, shift, strip):
    shift = min(max(shift, 0), 4)
    bx, by, bz = [((g - 1) >> shift) + 1 for g in dims]
    strip = min(max(strip, 1), by)
    rows = (by + strip - 1) // strip * strip * bz
    return shift, bx, by, bz, strip, rows


def reference_bins(dims, origin, inv_h, shift, strip, q):
    shift, bx, by, bz, strip, rows = layout(dims, shift, strip)
    c = []
    with np.errstate(all="ignore"):
        for a in range(3):
            t = np.floor((q[:, a].astype(F32) - F32(origin[a])) * F32(inv_h))
            assert t.dtype == np.float32
            t = np.fmin(np.fmax(t, F32(0)), F32(dims[a] - 1))          # fmax / fmin drop a NaN, as fmaxf / fminf do
            c.append(t.astype(np.int64) >> shift)
    cx, cy, cz = c
    s, yin = cy // strip, cy % strip
    return ((((s * bz + cz) * strip + yin) * bx + cx) & 0xFFFFFFFF).astype(np.uint32), (bx * rows) & 0xFFFFFFFF


def expected_fast(dims, inv_h, shift, strip):
    """the documented rule: rows <= 2^24 and bx < 2^24 (multiplicands), bins < 2^32 (products), inv_h * 2^-shift normal and exact"""
    shift, bx, by, bz, strip, rows = layout(dims, shift, strip)
    cs = np.ldexp(F32(inv_h), -shift)
    scale_ok = bool(np.isfinite(cs)) and abs(float(cs)) >= float(np.finfo(np.float32).tiny) and np.ldexp(cs, shift) == F32(inv_h)
    return int(scale_ok and rows <= (1 << 24) and bx < (1 << 24) and bx * rows < (1 << 32))


def axis_values(g, o, inv_h, shift):
    """cell borders +- 1 ulp (first, last, bin borders, the middle), the faces, values outside, the ends of the fp32 range"""
    h = 1.0 / float(inv_h)
    cells = {0, 1, 2, g // 2, g - 2, g - 1, g, g + 1, 1 << shift, (1 << shift) + 1, 3 << shift, 16 << shift, 17 << shift}
    vals = []
    for k in sorted(k for k in cells if 0 <= k <= g + 1):
        b = F32(float(o) + k * h)
        vals += [np.nextafter(b, F32(-np.inf)), b, np.nextafter(b, F32(np.inf))]
    far = F32(float(o) + (g + 1000) * h)
    vals += [F32(float(o) - 1000 * h), far, F32(o), F32(0.0), F32(-0.0), DENORM, -DENORM, F32(FLT_MAX), F32(-FLT_MAX), F32(3e38), F32(-3e38),
             F32(np.inf), F32(-np.inf), F32(np.nan)]
    return np.unique(np.array(vals, dtype=np.float32).view(np.uint32)).view(np.float32)          # by bit pattern: keeps -0.0 and NaN


def queries_for(dims, origin, inv_h, shift, rng, cap=12):
    """every combination of the per-axis values (thinned at random to `cap` per axis where the grid has many borders)"""
    per_axis = []
    for a in range(3):
        v = axis_values(dims[a], origin[a], inv_h, shift)
        if len(v) > cap:
            keep = np.isnan(v) | np.isinf(v) | (np.abs(v) >= F32(3e38))
            rest = np.flatnonzero(~keep)
            v = np.concatenate([v[keep], v[rng.choice(rest, cap - int(keep.sum()), replace=False)]])
        per_axis.append(v)
    return np.array(list(itertools.product(*per_axis)), dtype=np.float32)


def check(lib, dims, origin, inv_h, shift, strip, q, want_fast=None):
    got, nbins, fast = shipped_bins(lib, dims, origin, inv_h, shift, strip, q)
    ref, ref_nbins = reference_bins(dims, origin, inv_h, shift, strip, q)
    assert nbins == ref_nbins
    assert fast == expected_fast(dims, inv_h, shift, strip)
    if want_fast is not None:
        assert fast == want_fast
    assert np.array_equal(got, ref), (dims, shift, strip, q[np.flatnonzero(got != ref)[:4]])
    assert int(got.max()) < nbins
    return fast


SMALL_GRIDS = [
    ((1, 1, 1), (0.0, 0.0, 0.0), 1.0),
    ((40, 1, 30), (-3.0, 2.0, 0.5), 2.5),                        # flat: by = 1
    ((40, 3, 30), (-3.0, 2.0, 0.5), 2.5),                        # by = 3 at shift 0
    ((33, 15, 9), (1.25, -7.0, 0.0), 1.0 / 0.37),                # by = 15
    ((9, 17, 33), (1.25, -7.0, 0.0), 1.0 / 0.37),                # by = 17: two strips of 16, the second one mostly padding
    ((118, 118, 118), (-0.0004, -0.0004, -0.0004), 1.0 / 0.0848),  # the headline's grid
    ((300, 200, 100), (-50.0, -50.0, -5.0), 3.0),
]


@pytest.mark.parametrize("dims,origin,inv_h", SMALL_GRIDS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) and isinstance(v[0], int) else None)
def test_every_shift_and_strip_matches_the_definition(lib, dims, origin, inv_h):
    rng = np.random.default_rng(7)
    for shift in range(5):
        by = ((dims[1] - 1) >> shift) + 1
        q = queries_for(dims, origin, inv_h, shift, rng)
        for strip in sorted({1, 3, 7, 16, by}):
            check(lib, dims, origin, inv_h, shift, strip, q, want_fast=1)


def test_random_queries_on_the_headline_grid(lib):
    rng = np.random.default_rng(11)
    q = rng.uniform(-0.5, 10.5, size=(200_000, 3)).astype(np.float32)
    check(lib, (118, 118, 118), (-0.0004, -0.0004, -0.0004), 1.0 / 0.0848, 1, 16, q, want_fast=1)


@pytest.mark.parametrize("dims,shift,strip,want_fast", [
    ((1 << 24, 1, 1), 0, 16, 0),              # bx = 2^24: one past the 24-bit multiplicand
    (((1 << 24) - 1, 1, 1), 0, 16, 1),
    (((1 << 25) - 1, 1, 1), 1, 16, 0),        # bx = 2^24: the limit is on the bins, not the cells
    (((1 << 25) - 2, 1, 1), 1, 16, 1),
    ((3, 4096, 4096), 0, 16, 1),              # rows = 2^24: the last row is 2^24 - 1
    ((3, 4096, 4097), 0, 16, 0),
    ((3, 4097, 4096), 0, 16, 0),              # 257 strips of 16: the padding counts
    ((3, 4090, 4096), 0, 7, 1),               # 585 strips of 7 = 4095 padded rows per plane
    ((3, 4096, 4096), 0, 7, 0),               # 586 strips of 7 = 4102
    ((255, 4096, 4096), 0, 16, 1),            # 255 * 2^24 bins: the largest count of bins with rows at their limit (2^32 bins wrap nbins itself)
    ((70000, 70000, 3), 4, 16, 1),
])
def test_both_sides_of_the_24_bit_limit(lib, dims, shift, strip, want_fast):
    rng = np.random.default_rng(3)
    origin, inv_h = (-100.0, 3.0, 0.25), 4.0
    q = queries_for(dims, origin, inv_h, shift, rng, cap=14)
    extent = np.array(dims, dtype=np.float64) / inv_h
    r = (np.array(origin) + rng.uniform(-0.01, 1.01, size=(20_000, 3)) * extent).astype(np.float32)
    check(lib, dims, origin, inv_h, shift, strip, np.concatenate([q, r]), want_fast=want_fast)


def test_a_scale_that_leaves_the_normal_range_keeps_the_definition(lib):
    """inv_h * 2^-shift must be a normal number that scales back exactly; 2^-124 / 16 is not"""
    dims, origin, inv_h = (16, 16, 16), (0.0, 0.0, 0.0), float(np.ldexp(F32(1.0), -124))
    vals = np.array([0.0, -0.0, 1e-45, 1.0, 3e37, 1e38, 2.1e38, 3e38, FLT_MAX, -FLT_MAX, np.inf, -np.inf, np.nan, -3e38], dtype=np.float32)
    q = np.array(list(itertools.product(vals, repeat=3)), dtype=np.float32)
    assert check(lib, dims, origin, inv_h, 1, 16, q) == 1
    assert check(lib, dims, origin, inv_h, 2, 3, q) == 1          # 2^-126: the smallest normal
    assert check(lib, dims, origin, inv_h, 3, 3, q) == 0
    assert check(lib, dims, origin, inv_h, 4, 16, q) == 0


def test_knobs_are_clamped_and_bad_arguments_refused(lib):
    q = np.array([[0.5, 0.5, 0.5], [7.5, 3.2, 9.9]], dtype=np.float32)
    dims, origin = (10, 10, 10), (0.0, 0.0, 0.0)
    a = shipped_bins(lib, dims, origin, 1.0, 9, 1000, q)
    b = shipped_bins(lib, dims, origin, 1.0, 4, 1, q)             # shift 4: by = 1, so the strip is 1
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]
    a = shipped_bins(lib, dims, origin, 1.0, -3, 0, q)
    b = shipped_bins(lib, dims, origin, 1.0, 0, 1, q)
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]
    d = (C.c_int32 * 3)(10, 0, 10)
    o = (C.c_float * 3)(0, 0, 0)
    assert lib.pct_debug_query_bins(d, o, C.c_float(1.0), 1, 16, q.ctypes.data, 2, None, None, None) != 0
