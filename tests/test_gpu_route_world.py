"""The routed multi-GPU search with every rank in ONE process (include/pct_shard.h: pct_shard_local_world,
pct_shard_route_build_world, pct_shard_route_nn_world, pct_shard_route_nn_partitioned_world), in this process through ctypes, against
the exhaustive ORACLE -- not against the engine's own single cloud: every rank's indices and fp64 squared distances must equal
oracle.brute_nearest(points, queries) bit for bit, the lowest global index on ties; a query with a NaN or infinite coordinate
answers (PCT_NO_INDEX, +inf) as the single cloud documents (tests/test_gpu_numeric_edges.py).

The clouds are the unfriendly ones: a 0.5 lattice appended to itself in shuffled order (exact duplicates on different ranks, exact
ties between different points at the midpoint queries), a cloud of identical points (a zero-width layout), thin slabs whose longest
axis is y or z, a tight cluster with one far outlier (nearly every histogram bin empty, coinciding cuts), clouds of 0, 1 and 3
points under 8 ranks (owners without points); dealt to the ranks evenly, unevenly and with ranks that hold nothing."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

pytestmark = pytest.mark.gpu

F32 = np.float32
QMAX = 5000
LATTICE = (40, 16, 12)          # x 0.5: 20 x 8 x 6, the longest axis is x


@pytest.fixture(scope="module")
def A():
    import route_abi
    route_abi.shard()
    return route_abi


# ---- clouds -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cloud(name):
    rng = np.random.default_rng(sum(name.encode()))
    if name == "uniform":
        return rng.uniform(0, 30, (20_000, 3)).astype(F32)
    if name == "lattice":
        g = np.stack(np.meshgrid(*[np.arange(n) * 0.5 for n in LATTICE], indexing="ij"), -1).reshape(-1, 3).astype(F32)
        g = g[rng.permutation(len(g))]
        return np.concatenate([g, g])                                    # every point twice, 7680 rows apart
    if name == "identical":
        return np.tile(np.array([[3.25, -1.5, 7.0]], F32), (5000, 1))
    if name == "thin_y":
        return rng.uniform([0, 0, 0], [2, 40, 3], (12_000, 3)).astype(F32)
    if name == "thin_z":
        return rng.uniform([0, 0, 0], [3, 2, 40], (12_000, 3)).astype(F32)
    if name == "cluster":
        p = rng.uniform(10, 10.01, (6001, 3)).astype(F32)
        p[3000] = [500, 10, 10]
        return p
    raise KeyError(name)


def nonfinite_rows(rng, n, lo, hi):
    q = rng.uniform(lo, hi, (n, 3)).astype(F32)
    vals = np.array([np.nan, np.inf, -np.inf], F32)
    for i in range(n):
        q[i, rng.integers(0, 3)] = vals[i % 3]
        if i % 5 == 0:
            q[i, rng.integers(0, 3)] = vals[(i // 5) % 3]
    return q


@functools.lru_cache(maxsize=None)
def queries(name):
    """QMAX rows in a shuffled order: inside the box, (a few) far outside it, exactly on points, at midpoints of lattice neighbours (the
    lattice) or of random pairs, and 60 rows with NaN / +-inf coordinates"""
    pts = cloud(name)
    rng = np.random.default_rng(1 + sum(name.encode()))
    lo, hi = pts.min(0).astype(np.float64), pts.max(0).astype(np.float64)
    if name == "cluster":
        hi = lo + 0.01                                                   # around the cluster; the road to the outlier gets a few rows below
    pad = 0.05 * max((hi - lo).max(), 1.0)
    parts = [nonfinite_rows(rng, 60, lo, hi), pts[rng.integers(0, len(pts), 700)]]
    ext = np.maximum(hi - lo, 1.0)
    far = rng.uniform(lo - 3 * ext, hi + 3 * ext, (16, 3))
    far[:, 0] = np.where(rng.random(16) < 0.5, lo[0] - 3 * ext[0], hi[0] + 3 * ext[0])
    parts.append(far.astype(F32))
    if name == "lattice":
        nx, ny, nz = LATTICE
        mids = [[(i + 0.5) * 0.5, (i % ny) * 0.5, (i % nz) * 0.5] for i in range(nx - 1)]           # between x neighbours, at EVERY x position
        mids += [[(i % nx) * 0.5, (j + 0.5) * 0.5, 1.0] for i in range(7) for j in range(ny - 1)]   # between y neighbours
        mids += [[(i % nx) * 0.5 + 0.25, 2.25, (i % (nz - 1)) * 0.5 + 0.25] for i in range(100)]     # cell centres: eight-way ties
        parts.append(np.array(mids, F32))
    else:
        a, b = pts[rng.integers(0, len(pts), 200)], pts[rng.integers(0, len(pts), 200)]
        parts.append(((a.astype(np.float64) + b) / 2).astype(F32))
    if name == "cluster":
        parts.append(np.linspace([10, 10, 10], [500, 10, 10], 40).astype(F32))
    n = QMAX - sum(len(p) for p in parts)
    parts.append(rng.uniform(lo - pad, hi + pad, (n, 3)).astype(F32))
    q = np.concatenate(parts)
    q = q[rng.permutation(len(q))]
    assert q.shape == (QMAX, 3)
    return q


_want = {}


def want(oracle, name, pts=None, q=None):
    """(idx int64 with -1 = none, d2) for the cloud's whole query set, computed once: the oracle on the finite rows, the documented
    (PCT_NO_INDEX, +inf) on rows with a NaN or infinite coordinate"""
    if name not in _want:
        pts = cloud(name) if pts is None else pts
        q = queries(name) if q is None else q
        wi, wd = oracle.brute_nearest(pts, q)
        wi, wd = wi.astype(np.int64), wd.copy()
        bad = ~np.isfinite(q).all(1)
        wi[bad], wd[bad] = -1, np.inf
        wi.setflags(write=False)
        wd.setflags(write=False)
        _want[name] = (wi, wd, bad)
    return _want[name]


def deal(n, world, how, seed=0):
    """how many rows each rank holds (rows stay in global order): even, uneven, or with ranks that hold nothing"""
    if how == "even":
        return [n * (k + 1) // world - n * k // world for k in range(world)]
    rng = np.random.default_rng(seed + world)
    w = rng.uniform(0.1, 1.0, world) ** 3
    if how == "zeros" and world > 1:
        w[rng.permutation(world)[:max(1, world // 2)]] = 0.0
    if w.sum() == 0:
        w[-1] = 1.0
    c = np.floor(np.cumsum(w) / w.sum() * n + 0.5).astype(np.int64)
    c[-1] = n
    return np.diff(np.concatenate([[0], c])).tolist()


def split(pts, counts):
    e = np.cumsum(counts)
    return [pts[e[k] - counts[k]:e[k]] for k in range(len(counts))]


def check(A, res, wi, wd, what):
    """every rank's answers equal the expected ones bit for bit; the guard tails are untouched"""
    Q = len(wi)
    for k, (gi, gd) in enumerate(res):
        assert A.untouched(gi[Q:]) and A.untouched(gd[Q:]), (what, k)
        gi = np.where(gi[:Q] == A.NO_INDEX, -1, gi[:Q].astype(np.int64))
        bad = (gi != wi) | (gd[:Q].view(np.uint64) != wd.view(np.uint64))
        if bad.any():
            j = int(np.nonzero(bad)[0][0])
            raise AssertionError(f"{what}, rank {k}: {int(bad.sum())}/{Q} answers wrong, first at {j}: got ({gi[j]}, {gd[j]!r}) want ({wi[j]}, {wd[j]!r})")


def check_stats(st, total_queries, batches):
    assert sum(s["owned"] for s in st) == total_queries, st
    assert all(s["batches"] == batches for s in st), st
    assert len({s["uncertified"] for s in st}) == 1, st
    return st[0]["uncertified"]


CLOUDS = ["uniform", "lattice", "identical", "thin_y", "thin_z", "cluster"]
HOW = ["even", "uneven", "zeros"]


@pytest.mark.parametrize("halo", [0.0, 0.5, 4.0])
@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("name", CLOUDS)
def test_replicated_batches_equal_the_oracle(A, oracle, name, world, halo):
    """Q = 5000, 257 and 1 on one set of routes.  Statistics: summed over the ranks, owned == Q x batches; every rank counts the same
    uncertified answers; one rank alone cannot certify exactly the non-finite queries; the lattice at halo 0 must enter the second
    round -- queries sit at the midpoint between x neighbours at EVERY x position, 0.25 from both, so whatever the cut, one of them is
    at most 0.25 from it and its d2 = 0.0625 is not below margin^2."""
    pts, q = cloud(name), queries(name)
    wi, wd, bad = want(oracle, name)
    case = CLOUDS.index(name) + world + int(halo * 2)
    counts = deal(len(pts), world, HOW[case % 3], seed=case)
    assert sum(counts) == len(pts) and (HOW[case % 3] != "zeros" or world == 1 or 0 in counts)
    with A.local_world(split(pts, counts), stride=(12, 16)[(case // 3) % 2], halo=halo) as w:
        total = nonfinite = 0
        for Q in (QMAX, 257, 1):
            rc, res = w.nn(q[:Q])
            assert rc == A.OK
            check(A, res, wi[:Q], wd[:Q], f"{name} world {world} halo {halo} Q {Q}")
            total += Q
            nonfinite += int(bad[:Q].sum())
        st = w.stats()
        unc = check_stats(st, total, 3)
        if world == 1:
            assert unc == nonfinite and st[0]["slab_points"] == len(pts)
        else:
            assert unc >= nonfinite
        if name == "lattice" and halo == 0.0 and world > 1:
            assert unc > nonfinite


def test_uniform_cloud_at_halo_4_certifies_everything(A, oracle):
    """world 2, finite queries inside the box: the owner's margin is at least the halo (4 mean point spacings, spacing = cbrt(box
    volume / N)) and every query has its nearest point well inside that -- checked here, on the oracle's distances -- so nothing may
    reach the second round"""
    pts = cloud("uniform")
    q = np.random.default_rng(77).uniform(0.5, 29.5, (QMAX, 3)).astype(F32)
    wi, wd, bad = want(oracle, "uniform/inside", pts, q)
    spacing = float(np.cbrt(np.prod(pts.max(0).astype(np.float64) - pts.min(0)) / len(pts)))
    assert not bad.any() and np.sqrt(wd.max()) < 3.9 * spacing
    with A.local_world(split(pts, deal(len(pts), 2, "uneven", 5)), stride=16, halo=4.0) as w:
        rc, res = w.nn(q)
        assert rc == A.OK
        check(A, res, wi, wd, "uniform inside, world 2 halo 4")
        assert check_stats(w.stats(), QMAX, 1) == 0


@pytest.mark.parametrize("halo", [0.0, 0.5, 4.0])
@pytest.mark.parametrize("N", [0, 1, 3])
def test_tiny_clouds_under_8_ranks(A, oracle, N, halo):
    """empty slabs and owners without points; N = 0: every answer is (PCT_NO_INDEX, +inf)"""
    rng = np.random.default_rng(N)
    pts = rng.uniform(-1, 1, (N, 3)).astype(F32)
    q = np.concatenate([rng.uniform(-2, 2, (240, 3)).astype(F32), nonfinite_rows(rng, 12, -1, 1), pts, pts[:2] + F32(0.5)])[:257]
    q = np.concatenate([q, rng.uniform(-2, 2, (257 - len(q), 3)).astype(F32)])
    wi, wd, bad = want(oracle, f"tiny/{N}", pts, q)
    if N == 0:
        assert (wi == -1).all() and np.isinf(wd).all()
    counts = [0] * 8
    for i in range(N):
        counts[(2 + 3 * i) % 8] += 1
    with A.local_world(split(pts, counts), stride=12 if N != 1 else 16, halo=halo) as w:
        for Q in (257, 1):
            rc, res = w.nn(q[:Q])
            assert rc == A.OK
            check(A, res, wi[:Q], wd[:Q], f"N {N} halo {halo} Q {Q}")
        unc = check_stats(w.stats(), 258, 2)
        assert sum(s["slab_points"] for s in w.stats()) >= N
        if N == 0:
            assert unc == 258


def test_64_ranks(A, oracle):
    pts, q = cloud("thin_y"), queries("thin_y")
    wi, wd, bad = want(oracle, "thin_y")
    with A.local_world(split(pts, deal(len(pts), 64, "zeros", 9)), stride=12, halo=0.5) as w:
        rc, res = w.nn(q[:2000])
        assert rc == A.OK
        check(A, res, wi[:2000], wd[:2000], "64 ranks")
        check_stats(w.stats(), 2000, 1)


def test_an_empty_batch_writes_nothing(A):
    pts = cloud("lattice")
    with A.local_world(split(pts, deal(len(pts), 3, "even")), halo=0.5) as w:
        rc, res = w.nn(np.empty((0, 3), F32))                            # the result arrays are 64 filled elements long
        assert rc == A.OK and all(A.untouched(gi) and A.untouched(gd) for gi, gd in res)
        assert all(s["batches"] == 0 and s["owned"] == 0 for s in w.stats())


PART_SIZES = [0, 257, 1300, 1, 0, 700, 64, 5]


def partitioned_batches(name, world, shift=0):
    q = queries(name)
    sizes = [PART_SIZES[(k + shift) % len(PART_SIZES)] for k in range(world)]
    begins = [(311 * k + 97 * shift) % (QMAX - 1300) for k in range(world)]
    return [slice(b, b + n) for b, n in zip(begins, sizes)]


@pytest.mark.parametrize("world", [3, 8])
@pytest.mark.parametrize("name,halo", [("lattice", 0.0), ("uniform", 4.0)])
def test_partitioned_batches_equal_the_oracle(A, oracle, name, halo, world):
    """every rank brings its own batch, of its own size (0 for some ranks; then 0 for all): each rank's answers against the oracle on
    that rank's queries"""
    pts, q = cloud(name), queries(name)
    wi, wd, bad = want(oracle, name)
    with A.local_world(split(pts, deal(len(pts), world, "uneven", world)), stride=16, halo=halo) as w:
        total = 0
        for shift in (0, 3):
            sl = partitioned_batches(name, world, shift)
            assert 0 in [s.stop - s.start for s in sl]
            rc, res = w.nn_partitioned([q[s] for s in sl])
            assert rc == A.OK
            for k, s in enumerate(sl):
                check(A, [res[k]], wi[s], wd[s], f"{name} world {world} partitioned, batch of rank {k}")
            total += sum(s.stop - s.start for s in sl)
        rc, res = w.nn_partitioned([q[:0]] * world)
        assert rc == A.OK and all(A.untouched(gi) and A.untouched(gd) for gi, gd in res)
        st = w.stats()
        assert sum(s["owned"] for s in st) == total, st
        if halo == 0.0:
            assert sum(s["uncertified"] for s in st) > 0


def test_workspaces_are_reused_across_batch_sizes_and_forms(A, oracle):
    """one set of routes: Q = 100, then 5000, then 7, then a partitioned batch, then a replicated one"""
    pts, q = cloud("lattice"), queries("lattice")
    wi, wd, bad = want(oracle, "lattice")
    with A.local_world(split(pts, deal(len(pts), 3, "zeros", 1)), stride=12, halo=0.5) as w:
        for b, Q in ((0, 100), (0, QMAX), (4000, 7)):
            rc, res = w.nn(q[b:b + Q])
            assert rc == A.OK
            check(A, res, wi[b:b + Q], wd[b:b + Q], f"replicated Q {Q}")
        sl = partitioned_batches("lattice", 3, 1)
        rc, res = w.nn_partitioned([q[s] for s in sl])
        assert rc == A.OK
        for k, s in enumerate(sl):
            check(A, [res[k]], wi[s], wd[s], f"partitioned, rank {k}")
        rc, res = w.nn(q[1000:1257])
        assert rc == A.OK
        check(A, res, wi[1000:1257], wd[1000:1257], "replicated after partitioned")
