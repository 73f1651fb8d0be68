"""The device phases of the routed multi-GPU search (include/pct_engine.h: pct_route_*_dev, pct_merge_finish_dev,
pct_cloud_upload_aos_dev), each called directly through the C ABI and compared EXACTLY with the numpy model of
tests/helpers/route_model.py.  The two comparisons the routed form's correctness rests on are met head on: a query exactly on a
cut (and one fp32 ulp either side of it) in the owner kernels, and d2 exactly margin * margin (and one fp64 ulp either side) in the
certification.  Every output buffer has its documented size, a guard tail that must stay untouched, and a fill that tells "not
written" from "written with 0"; every entry point runs twice on the same buffers (its counters are re-zeroed per call)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import route_cases as RC  # noqa: E402
import route_model as M  # noqa: E402

pytestmark = pytest.mark.gpu

U32, F32, F64, U8 = np.uint32, np.float32, np.float64, np.uint8
WORLDS = [(1, 0), (2, 0), (3, 0), (3, 1), (64, 1)]                      # (world, cut variant: 1 = repeated cuts)
QS = [0, 1, 255, 256, 257, 1000, 70_001]                                # around one block; many blocks (LDS histogram + global atomics)


@pytest.fixture(scope="module")
def A():
    import route_abi
    route_abi.engine()
    return route_abi


def bits(a):
    return np.ascontiguousarray(a).view(U8)


def call_owner(A, cuts, world, axis, rank, dq, Q, bufs):
    return A.engine().pct_route_owner_dev(A.host_ptr(cuts), world, axis, rank, A.ptr(dq), Q, *[A.ptr(b) for b in bufs], A.stream())


@pytest.mark.parametrize("Q", QS)
@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("world,variant", WORLDS)
def test_owner_owner_all_and_partition(A, world, variant, axis, Q):
    L = A.engine()
    cuts = RC.cuts_for(world, variant)
    q = RC.owner_queries(cuts, axis, Q, seed=7 * world + axis + Q)
    qb = q.view(U32)
    own, counts = M.owner(cuts, axis, q)
    dq = A.dev(q)
    empty = np.nonzero(counts == 0)[0]
    ranks = sorted({0, world - 1, int(np.argmax(counts))} | ({int(empty[len(empty) // 2])} if len(empty) else set()))
    for rank in ranks:                                                   # pct_route_owner_dev: counts of every owner, this rank's share compacted
        bufs = [A.out(world, U32), A.out(Q, U32), A.out(3 * Q, F32)]
        for _ in range(2):
            assert call_owner(A, cuts, world, axis, rank, dq, Q, bufs) == A.OK
            c, ids, mq = A.host(bufs[0], U32), A.host(bufs[1], U32), A.host(bufs[2], U32)
            assert (c[:world] == counts).all() and A.untouched(c[world:])
            m = int(counts[rank])
            assert (np.sort(ids[:m]) == M.mine(own, rank)).all()
            assert A.untouched(ids[m:])
            assert (mq[:3 * m].reshape(-1, 3) == qb[ids[:m]]).all() and A.untouched(mq[3 * m:])
    d_counts, d_owner = A.out(world, U32), A.out(Q, U8)                  # pct_route_owner_all_dev: the owner of every query as a byte
    for _ in range(2):
        assert L.pct_route_owner_all_dev(A.host_ptr(cuts), world, axis, A.ptr(dq), Q, A.ptr(d_counts), A.ptr(d_owner), A.stream()) == A.OK
        c, o = A.host(d_counts, U32), A.host(d_owner, U8)
        assert (c[:world] == counts).all() and A.untouched(c[world:])
        assert (o[:Q] == own).all() and A.untouched(o[Q:])
    off = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(U32)      # pct_route_partition_dev: the queries grouped by owner, with their slots
    d_cur, d_xyz, d_slot = A.out(world, U32), A.out(3 * Q, F32), A.out(Q, U32)
    for _ in range(2):
        assert L.pct_route_partition_dev(A.host_ptr(off), world, A.ptr(d_owner), A.ptr(dq), Q, A.ptr(d_cur), A.ptr(d_xyz), A.ptr(d_slot), A.stream()) == A.OK
        cur, xyz, slot = A.host(d_cur, U32), A.host(d_xyz, U32), A.host(d_slot, U32)
        assert (cur[:world] == counts).all() and A.untouched(cur[world:])
        assert A.untouched(slot[Q:]) and A.untouched(xyz[3 * Q:])
        assert (np.sort(slot[:Q]) == np.arange(Q)).all()                 # every slot once
        for k, (o, want) in enumerate(M.partition(off, own, q)):
            assert set(slot[o:o + int(counts[k])].tolist()) == want, k
        assert (xyz[:3 * Q].reshape(-1, 3) == qb[slot[:Q]]).all()


def test_owner_phases_refuse_bad_arguments_and_write_nothing(A):
    L = A.engine()
    Q = 300
    cuts = np.concatenate([[-np.inf], np.linspace(-1, 1, 64), [np.inf]])          # long enough for every world tried
    off = np.zeros(65, U32)
    dq = A.dev(RC.owner_queries(cuts[:4], 0, Q, seed=1))
    bufs = [A.out(64, U32), A.out(Q, U32), A.out(3 * Q, F32)]
    d_owner, d_xyz, d_slot = A.out(Q, U8), A.out(3 * Q, F32), A.out(Q, U32)
    p = [A.ptr(b) for b in bufs]
    st = A.stream()
    cp = A.host_ptr(cuts)
    bad = []
    for world, axis, rank in [(0, 0, 0), (65, 0, 0), (3, 3, 0), (3, -1, 0), (3, 0, 3), (3, 0, -1)]:
        bad.append(L.pct_route_owner_dev(cp, world, axis, rank, A.ptr(dq), Q, *p, st))
    bad.append(L.pct_route_owner_dev(None, 3, 0, 0, A.ptr(dq), Q, *p, st))
    bad.append(L.pct_route_owner_dev(cp, 3, 0, 0, None, Q, *p, st))
    for k in range(3):
        bad.append(L.pct_route_owner_dev(cp, 3, 0, 0, A.ptr(dq), Q, *[None if j == k else p[j] for j in range(3)], st))
    bad.append(L.pct_route_owner_dev(cp, 3, 0, 0, A.ptr(dq), -1, *p, st))
    for world, axis in [(0, 0), (65, 0), (3, 3)]:
        bad.append(L.pct_route_owner_all_dev(cp, world, axis, A.ptr(dq), Q, p[0], A.ptr(d_owner), st))
    bad.append(L.pct_route_owner_all_dev(None, 3, 0, A.ptr(dq), Q, p[0], A.ptr(d_owner), st))
    bad.append(L.pct_route_owner_all_dev(cp, 3, 0, None, Q, p[0], A.ptr(d_owner), st))
    bad.append(L.pct_route_owner_all_dev(cp, 3, 0, A.ptr(dq), Q, None, A.ptr(d_owner), st))
    bad.append(L.pct_route_owner_all_dev(cp, 3, 0, A.ptr(dq), Q, p[0], None, st))
    op = A.host_ptr(off)
    own = A.dev(np.zeros(Q, U8))
    for world in (0, 65):
        bad.append(L.pct_route_partition_dev(op, world, A.ptr(own), A.ptr(dq), Q, p[0], A.ptr(d_xyz), A.ptr(d_slot), st))
    bad.append(L.pct_route_partition_dev(None, 3, A.ptr(own), A.ptr(dq), Q, p[0], A.ptr(d_xyz), A.ptr(d_slot), st))
    args = [A.ptr(own), A.ptr(dq), Q, p[0], A.ptr(d_xyz), A.ptr(d_slot)]
    for k in (0, 1, 3, 4, 5):
        bad.append(L.pct_route_partition_dev(op, 3, *[None if j == k else args[j] for j in range(6)], st))
    assert bad == [A.INVALID] * len(bad), bad
    for b in bufs + [d_owner, d_xyz, d_slot]:
        assert A.untouched(A.host(b, U8))


CERTIFY = [(m, axis, e) for m in (1, 257, 5000) for axis in (0, 1, 2) for e in range(len(RC.EDGE_VARIANTS))]


def run_certify(A, a):
    m = len(a["lidx"])
    d = {k: A.dev(a[k]) for k in ("mine_q", "mine_ids", "lidx", "ld2", "gid")}
    d_ans = A.out(m, M.RECORD)
    want = M.certify(**a)
    for _ in range(2):
        rc = A.engine().pct_route_certify_dev(a["axis"], a["lo_edge"], a["hi_edge"], A.ptr(d["mine_q"]), A.ptr(d["mine_ids"]), m, A.ptr(d["lidx"]), A.ptr(d["ld2"]),
                                              A.ptr(d["gid"]), A.ptr(d_ans), A.stream())
        assert rc == A.OK
        got = A.host(d_ans, M.RECORD)
        assert A.untouched(got[m:])
        for f in ("query", "gid"):
            assert (got[f][:m] == want[f]).all(), f
        assert (got["d2"][:m].view(np.uint64) == want["d2"].view(np.uint64)).all()
    return want


@pytest.mark.parametrize("m,axis,e", CERTIFY)
def test_certify(A, m, axis, e):
    """d2 exactly margin * margin and one ulp either side, margin < 0, d2 == 0, nothing found, NaN / +-inf coordinates, halo edges at
    +-inf, a non-identity table of global indices up to 2^31 - 2: records read back through the structured dtype, all three fields"""
    want = run_certify(A, RC.certify_case(m, axis, RC.EDGE_VARIANTS[e], seed=1000 * m + 10 * axis + e))
    if m >= 257:
        assert (want["d2"] < 0).any() and (want["d2"] >= 0).any()


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_certify_with_the_query_on_the_halo_edge(A, axis):
    """margin == 0 exactly (fp32-representable edges): not certified even at d2 == 0; one ulp inside it is"""
    want = run_certify(A, RC.certify_on_the_edge(axis))
    assert (want["d2"] == [-1, -1, 0, 0, -1, -1]).all()


def test_certify_refuses_bad_arguments(A):
    a = RC.certify_case(40, 0, RC.EDGE_VARIANTS[0], seed=2)
    d = [A.dev(a[k]) for k in ("mine_q", "mine_ids")] + [40] + [A.dev(a[k]) for k in ("lidx", "ld2", "gid")] + [A.out(40, M.RECORD)]
    p = [v if isinstance(v, int) else A.ptr(v) for v in d]
    L = A.engine()
    bad = [L.pct_route_certify_dev(3, -1.0, 1.0, *p, A.stream()), L.pct_route_certify_dev(-1, -1.0, 1.0, *p, A.stream())]
    for k in (0, 1, 3, 4, 5, 6):
        bad.append(L.pct_route_certify_dev(0, -1.0, 1.0, *[None if j == k else p[j] for j in range(7)], A.stream()))
    assert bad == [A.INVALID] * len(bad), bad
    assert A.untouched(A.host(d[-1], U8))
    assert L.pct_route_certify_dev(0, -1.0, 1.0, None, None, 0, None, None, None, None, A.stream()) == A.OK      # m == 0: a no-op


def guarded(a, dtype):
    """an in/out array followed by the guard fill, as one host array"""
    return np.concatenate([np.asarray(a, dtype), np.frombuffer(bytes([0xA5]) * (64 * np.dtype(dtype).itemsize), dtype)])


@pytest.mark.parametrize("flagged", ["none", "all", "some"])
@pytest.mark.parametrize("n", [0, 1, 257, 5000])
def test_scatter_gather_to_global_put_back_and_merge_finish(A, n, flagged):
    L = A.engine()
    st = A.stream()
    n_out = n + 37                                                        # the result arrays are longer than the batch
    rng = np.random.default_rng(3 * n + len(flagged))
    # scatter: records in a random order -> result arrays; the flagged ones counted and listed
    rec = RC.records(n, n_out, flagged, seed=n + len(flagged))
    d_rec = A.dev(rec)
    d_idx, d_d2, d_fc, d_fid = A.out(n_out, U32), A.out(n_out, F64), A.out(1, U32), A.out(n, U32)
    wi, wd, wf = M.scatter(rec, A.host(d_idx, U32), A.host(d_d2, F64))    # the model on the filled arrays: untouched slots keep the fill
    assert len(wf) == {"none": 0, "all": n}.get(flagged, len(wf))
    for _ in range(2):
        assert L.pct_route_scatter_dev(A.ptr(d_rec), n, A.ptr(d_idx), A.ptr(d_d2), A.ptr(d_fc), A.ptr(d_fid), st) == A.OK
        gi, gd, fc, fid = A.host(d_idx, U32), A.host(d_d2, F64), A.host(d_fc, U32), A.host(d_fid, U32)
        assert (gi == wi).all() and (bits(gd) == bits(wd)).all()          # guard tails included
        assert fc[0] == len(wf) and A.untouched(fc[1:])                   # n == 0: the count is still set (to 0); nothing else is written
        assert set(fid[:fc[0]].tolist()) == wf and len(set(fid[:fc[0]].tolist())) == fc[0]
        assert A.untouched(fid[fc[0]:])
    # gather: the rows of a permutation subset
    q = rng.uniform(-9, 9, (n_out, 3)).astype(F32)
    q[::7, 1] = np.nan
    ids = rng.permutation(n_out)[:n].astype(U32)
    d_q, d_ids, d_out = A.dev(q), A.dev(ids), A.out(3 * n, F32)
    for _ in range(2):
        assert L.pct_route_gather_queries_dev(A.ptr(d_q), A.ptr(d_ids), n, A.ptr(d_out), st) == A.OK
        g = A.host(d_out, U32)
        assert (g[:3 * n] == M.gather_queries(q, ids).view(U32).reshape(-1)).all() and A.untouched(g[3 * n:])
    # to_global: in place, PCT_NO_INDEX stays
    G = 777
    gid = rng.integers(0, 2 ** 31 - 1, G, dtype=np.int64).astype(U32)
    gid[0] = 2 ** 31 - 2
    lidx = rng.integers(0, G, n, dtype=np.int64).astype(U32)
    lidx[::3] = A.NO_INDEX
    lidx[1::5] = 0
    d_l, d_gid = A.dev(guarded(lidx, U32)), A.dev(gid)
    assert L.pct_route_to_global_dev(A.ptr(d_l), n, A.ptr(d_gid), st) == A.OK
    got = A.host(d_l, U32)
    assert (got[:n] == M.to_global(lidx, gid)).all() and A.untouched(got[n:])
    # put_back: merged second-round answers into the slots of a permutation subset
    vi, vd = rng.integers(0, 2 ** 31 - 1, n, dtype=np.int64).astype(U32), rng.uniform(0, 9, n)
    if n:
        vi[0], vd[0] = A.NO_INDEX, np.inf
    d_vi, d_vd, d_oi, d_od = A.dev(vi), A.dev(vd), A.out(n_out, U32), A.out(n_out, F64)
    wi, wd = M.put_back(ids, vi, vd, A.host(d_oi, U32), A.host(d_od, F64))
    for _ in range(2):
        assert L.pct_route_put_back_dev(A.ptr(d_ids), n, A.ptr(d_vi), A.ptr(d_vd), A.ptr(d_oi), A.ptr(d_od), st) == A.OK
        assert (A.host(d_oi, U32) == wi).all() and (bits(A.host(d_od, F64)) == bits(wd)).all()
    # merge_finish: INT32_MAX -> PCT_NO_INDEX, everything else as it is
    cand = np.resize(np.array([0, 1, 2 ** 31 - 2, 0x7FFFFFFF], np.int32), n)
    d_c, d_o = A.dev(cand), A.out(n, U32)
    assert L.pct_merge_finish_dev(A.ptr(d_c), A.ptr(d_o), n, st) == A.OK
    got = A.host(d_o, U32)
    assert (got[:n] == M.merge_finish(cand)).all() and A.untouched(got[n:])
    if n >= 4:
        assert got[:4].tolist() == [0, 1, 2 ** 31 - 2, 0xFFFFFFFF]


def test_second_round_phases_refuse_null_pointers(A):
    L = A.engine()
    st = A.stream()
    b = A.out(8, F64)
    p = A.ptr(b)
    bad = [L.pct_route_scatter_dev(None, 4, p, p, p, p, st), L.pct_route_scatter_dev(p, 4, None, p, p, p, st), L.pct_route_scatter_dev(p, 4, p, p, None, p, st),
           L.pct_route_scatter_dev(p, -1, p, p, p, p, st), L.pct_route_gather_queries_dev(None, p, 4, p, st), L.pct_route_gather_queries_dev(p, p, 4, None, st),
           L.pct_route_to_global_dev(None, 4, p, st), L.pct_route_to_global_dev(p, 4, None, st), L.pct_route_put_back_dev(None, 4, p, p, p, p, st),
           L.pct_route_put_back_dev(p, 4, p, p, p, None, st), L.pct_merge_finish_dev(None, p, 4, st), L.pct_merge_finish_dev(p, None, 4, st)]
    assert bad == [A.INVALID] * len(bad), bad
    assert A.untouched(A.host(b, U8))


@pytest.fixture(scope="module")
def upload_case(oracle):
    rng = np.random.default_rng(42)
    pts = rng.uniform(0, 20, (5003, 3)).astype(F32)
    pts[100:200] = pts[:100]                                              # duplicates: the lowest index wins
    q = np.concatenate([rng.uniform(-2, 22, (900, 3)).astype(F32), pts[50:150]])
    return pts, q, oracle.brute_nearest(pts, q)


@pytest.mark.parametrize("stride", [12, 16, 32])
def test_cloud_upload_from_device_records(A, upload_case, stride):
    """pct_cloud_upload_aos_dev: x, y, z at the start of every `stride`-byte record in DEVICE memory; the cloud then answers like one
    filled from the host -- bit-equal to the exhaustive oracle"""
    pts, q, (wi, wd) = upload_case
    n = len(pts)
    rec = np.full((n, stride // 4), F32(-3e33), F32)
    rec[:, :3] = pts
    d = A.dev(rec)
    L = A.engine()
    c = A.E.Cloud(n)
    try:
        assert L.pct_cloud_upload_aos_dev(c.handle, A.ptr(d), n, stride) == A.OK
        assert len(c) == n
        gi, gd = c.nn(q)
        assert (gi.astype(np.int64) == wi).all() and (gd.view(np.uint64) == wd.view(np.uint64)).all()
        for bad_stride in (8, 14):
            assert L.pct_cloud_upload_aos_dev(c.handle, A.ptr(d), n, bad_stride) == A.INVALID
        assert L.pct_cloud_upload_aos_dev(c.handle, None, n, stride) == A.INVALID
        assert L.pct_cloud_upload_aos_dev(None, A.ptr(d), n, stride) == A.INVALID
        big = A.dev(np.zeros((n + 1, stride // 4), F32))
        assert L.pct_cloud_upload_aos_dev(c.handle, A.ptr(big), n + 1, stride) == A.CAPACITY
        assert len(c) == n                                                # a refused upload leaves the cloud as it was
        gi, gd = c.nn(q[:64])
        assert (gi.astype(np.int64) == wi[:64]).all() and (gd.view(np.uint64) == wd[:64].view(np.uint64)).all()
        assert L.pct_cloud_upload_aos_dev(c.handle, A.ptr(d), 17, stride) == A.OK       # fewer rows than the capacity: the size is n
        assert len(c) == 17
        assert L.pct_cloud_upload_aos_dev(c.handle, None, 0, stride) == A.OK            # n == 0 leaves an empty cloud
        assert len(c) == 0
    finally:
        c.close()
