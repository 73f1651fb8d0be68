"""The fp64-query layer of the engine's C ABI, asked directly: pct_nn_batch_q64, pct_nn_batch_q64_ties, pct_radius_indices_q64,
pct_radius_indices_r2_q64 and pct_radius_indices_batch_q64 (include/pct_engine.h) -- the searches under the kd_* drop-in and the
corridor finder's tree queries.

Reference: numpy in fp64 with one ufunc call per operation (tests/helpers/q64_cases.py): the first index of the minimum, the tie
count (s == s.min()).sum(), the hit set s <= r2.  Everything is exact by contract -- ((dx*dx + dy*dy) + dz*dz) on the float-widened
points, no fused multiply-add -- so every comparison is bit for bit.

Sizes straddle every dispatch of the layer: 16384 points (nn_small_kernel / nn_small_batch_kernel against the streaming kernels),
65536 points (radius_small_kernel against the crop compaction; the limit of the batched range kernel), 1 / 4 / 1024 queries (single,
all-fp64 against fp32-filtered, block-per-query), and 16384 queries (two part_q slices).  The queries are genuine doubles of the four
classes of q64_cases: random, lattice (heavy ties), cell centres moved by 2^-40 (doubles that still tie), one axis at 1e17.
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import q64_cases as QC  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = (1, 5, 1003, 16384, 16385, 65536, 65537)
FORMS = ("uniform", "lattice")
MANY_Q = (1, 2, 3, 4, 5, 8, 9, 1024, 1025)
NN_CASES = [(n, Q) for n in SIZES for Q in (MANY_Q if n in (1003, 16385) else (1, 5))] + [(1003, 16384 + 5)]
PCT_ERR_INVALID = 2


@pytest.fixture(scope="module")
def clouds():
    """(fp32 points, resident E.Cloud without an index) per (n, form), made on first use and shared by the module"""
    from pointcloudtraj_amd import engine as E
    E.init(0)
    made = []

    @functools.lru_cache(maxsize=None)
    def get(n, form):
        pts = QC.cloud(1000 + n, n, lattice=(form == "lattice"))
        c = E.Cloud(n)
        c.set_input(pts)
        made.append(c)
        return pts, c
    yield get
    for c in made:
        c.close()


def check_nn(c, pts, q, counted):
    """idx and d2 equal numpy's; ties == the tie count where the path counts (one query, at most 16384 points), 0 or the count
    elsewhere; the forms without a ties array give the same rows"""
    want_i, want_d, want_c = QC.nn_reference(pts, q)
    idx, d2, ties = c.nn_q64_ties(q)
    assert np.array_equal(d2, want_d)
    assert np.array_equal(idx, want_i)
    if counted:
        assert np.array_equal(ties, want_c)
    else:
        assert np.all((ties == 0) | (ties == want_c))
    i2, dd2 = c.nn_q64(q)
    i3, dd3, none = c.nn_q64_ties(q, want_ties=False)
    assert none is None and np.array_equal(i2, want_i) and np.array_equal(dd2, want_d) and np.array_equal(i3, want_i) and np.array_equal(dd3, want_d)
    return want_i, want_d, want_c


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n,Q", NN_CASES)
def test_nn_q64_mixed_double_queries(clouds, n, Q, form):
    pts, c = clouds(n, form)
    if Q == 1:                                                    # the single-query kernel meets every class
        for k in range(4):
            q, _ = QC.queries(7000 + n + k, 1, first_class=k)
            check_nn(c, pts, q, counted=n <= 16384)
        return
    q, _ = QC.queries(7000 + n + Q, Q)
    assert QC.genuine_double(q).any()
    check_nn(c, pts, q, counted=False)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", SIZES)
def test_nn_q64_where_no_distance_is_finite(clouds, n, form):
    """a NaN or infinite coordinate, or |q| = 1e160: (PCT_NO_INDEX, +inf) (reported_index, kernels.hpp) as a batch and one by one;
    the ordinary query among them is answered as without them"""
    pts, c = clouds(n, form)
    nf = QC.non_finite_queries()
    want_i, _, _ = check_nn(c, pts, nf, counted=False)
    assert (want_i == QC.NO_INDEX).sum() == len(nf) - 1
    for qq in nf:
        check_nn(c, pts, qq[None], counted=n <= 16384)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", SIZES)
def test_nn_q64_filtered_and_all_fp64_paths_agree_with_numpy(clouds, n, form):
    """five queries that are fp32 values throughout take the fp32-filtered kernels beyond 16384 points; one fp64 ulp on one
    coordinate of the last query sends the same batch to the all-fp64 kernel"""
    pts, c = clouds(n, form)
    rng = np.random.default_rng(7100 + n)
    q = np.concatenate([np.round(rng.uniform(QC.LO, QC.HI, (2, 3)) * 2) / 2, QC.cloud(7200 + n, 3, False).astype(np.float64)])
    assert len(q) == 5 and not QC.genuine_double(q).any()
    check_nn(c, pts, q, counted=False)
    check_nn(c, pts, q[:4], counted=False)                          # four of them: below the filtered path's batch size
    q[-1, 1] = np.nextafter(q[-1, 1], np.inf)
    assert QC.genuine_double(q).sum() == 1
    check_nn(c, pts, q, counted=False)


def centres(n):
    """one centre of each class 0 .. 2 inside the box"""
    return np.concatenate([QC.queries(7300 + n + k, 1, first_class=k)[0] for k in range(3)])


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", (16385, 65536, 65537))
def test_radius_indices_q64_full_lists(clouds, n, form):
    pts, c = clouds(n, form)
    for qq in centres(n):
        for r in (0.0, 0.5, 1.5, np.inf, np.nan):
            got, hits = c.radius_indices_q64(qq, r)
            want = QC.hits_reference(pts, qq, r * r)
            assert hits == len(want) and np.array_equal(got, want), f"centre {qq} r {r}"
        got, hits = c.radius_indices_q64(qq, -1.5)                  # r enters as r * r: a negative r lists the rows of |r|
        assert hits == len(got) and np.array_equal(got, QC.hits_reference(pts, qq, 2.25))
        got, hits = c.radius_indices_r2_q64(qq, 2.25)
        assert hits == len(got) and np.array_equal(got, QC.hits_reference(pts, qq, 2.25))
    # r2 = the d2 a nearest-neighbour query returned: the tied set, as kd_nearest fetches it beyond 16384 nodes
    q, _ = QC.queries(7400 + n, 12)
    want_i, want_d, want_c = QC.nn_reference(pts, q)
    _, d2 = c.nn_q64(q)
    assert np.array_equal(d2, want_d)
    for k in range(len(q)):
        got, hits = c.radius_indices_r2_q64(q[k], d2[k])
        tied = np.flatnonzero(QC.d2_rows(pts.astype(np.float64), q[k])[0] == want_d[k]).astype(np.uint32)
        assert hits == want_c[k] == len(tied) and np.array_equal(got, tied), f"query {k}"
    assert (want_c > 1).sum() >= 3                                   # the three queries with an axis at 1e17 tie on any cloud


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", (16385, 65536, 65537))
def test_radius_indices_q64_truncated_list_is_the_lowest_indices(clouds, n, form):
    """cap < hits: *n_out is the number of hits all the same, and what is written is the `cap` lowest indices, ascending -- on both
    sides of 65536 points (one-block kernel with arrival-order slots / order-preserving compaction)"""
    pts, c = clouds(n, form)
    for qq, r in zip(centres(n), (3.0, np.inf, 2.5)):
        want = QC.hits_reference(pts, qq, r * r)
        assert len(want) >= 9
        for cap in (len(want) // 3, 1, 0):
            for got, hits in (c.radius_indices_q64(qq, r, cap=cap), c.radius_indices_r2_q64(qq, r * r, cap=cap)):
                assert hits == len(want)
                assert np.array_equal(got, want[:cap]), f"centre {qq} r {r} cap {cap}"


BATCH_RADII = {1003: (0.0, 0.5, 3.0, 5.0, 5.5, 6.5, 9.0, np.inf, np.nan, -3.0),
               65536: (0.0, 0.5, 1.0, 1.3, 1.4, 1.6, 2.5, np.inf, np.nan, -1.0)}


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", (1003, 65536))
@pytest.mark.parametrize("K", (1, 7, 1024))
def test_radius_indices_batch_q64(clouds, K, n, form):
    """rows in arrival order: sorted, a row that fits equals numpy's hit set; a row beyond min(cap_per_query, 65536 / K) reports
    -(hits) and holds distinct true hits"""
    pts, c = clouds(n, form)
    cap = 100
    eff = min(cap, 65536 // K)                                       # K = 1024: the library's own 64 per row
    rounds = [(QC.queries(7500 + n + K, K)[0], np.float64([BATCH_RADII[n][i % 10] for i in range(K)]))]
    if K == 1:                                                       # one row that fits, one that overflows
        rounds = [(centres(n)[:1], np.float64([BATCH_RADII[n][2]])), (centres(n)[:1], np.float64([np.inf]))]
    fits = overflows = 0
    for q, r in rounds:
        ids, counts = c.radius_indices_batch_q64(q, r, cap)
        for k in range(K):
            want = QC.hits_reference(pts, q[k], r[k] * r[k])
            if len(want) <= eff:
                assert counts[k] == len(want) and np.array_equal(np.sort(ids[k, :len(want)]), want), f"row {k}"
                fits += 1
            else:
                assert counts[k] == -len(want), f"row {k}"
                stored = ids[k, :eff]
                assert len(set(stored.tolist())) == eff and np.all(np.isin(stored, want)), f"row {k}"
                overflows += 1
    assert fits >= 1 and overflows >= 1


def test_radius_indices_batch_q64_limits(clouds):
    from pointcloudtraj_amd import engine as E
    pts, c = clouds(1003, "uniform")
    q, _ = QC.queries(7600, 1025)
    with pytest.raises(E.EngineError) as e:
        c.radius_indices_batch_q64(q, 1.0, 8)                        # more than 1024 queries
    assert e.value.code == PCT_ERR_INVALID
    _, big = clouds(65537, "uniform")
    with pytest.raises(E.EngineError) as e:
        big.radius_indices_batch_q64(q[:7], 1.0, 8)                  # more than 65536 points
    assert e.value.code == PCT_ERR_INVALID
    with E.Cloud(64) as empty:
        ids, counts = empty.radius_indices_batch_q64(q[:7], np.inf, 8)
        assert np.array_equal(counts, np.zeros(7, np.int64))
        got, hits = empty.radius_indices_q64(q[0], np.inf)
        assert hits == 0 and len(got) == 0
