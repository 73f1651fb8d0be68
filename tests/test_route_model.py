"""The numpy model of the routed search's device phases (tests/helpers/route_model.py) against scalar Python loops written from the
contract in include/pct_engine.h, on a few hundred rows that hold every edge the GPU tests use (tests/helpers/route_cases.py): queries
on a cut and one fp32 ulp either side, -0.0 against a cut at 0.0, +-inf and NaN; d2 at, just below and just above margin * margin;
margin zero, negative and infinite; nothing found; 2^31 - 2 as a global index.  No GPU needed."""
import math
import os
import struct
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import route_cases as RC  # noqa: E402
import route_model as M  # noqa: E402

NO = 0xFFFFFFFF


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def scalar_owner(cuts, x):
    """the number of inner cuts at or below x; every comparison with NaN is false"""
    k = 0
    for j in range(1, len(cuts) - 1):
        if x >= cuts[j]:
            k += 1
    return k


def c_fmin(a, b):
    """C's fmin: a NaN operand is ignored unless both are NaN"""
    if math.isnan(a):
        return b
    if math.isnan(b):
        return a
    return min(a, b)


@pytest.mark.parametrize("world,variant", [(1, 0), (2, 0), (3, 0), (3, 1), (64, 1)])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_owner_counts_and_partition(world, variant, axis):
    cuts = RC.cuts_for(world, variant)
    assert len(cuts) == world + 1 and cuts[0] == -np.inf and cuts[-1] == np.inf
    if world > 1:
        assert 0.0 in cuts[1:-1]
    if variant == 1:
        assert (np.diff(cuts[1:-1]) == 0).any()
    q = RC.owner_queries(cuts, axis, 300, seed=world + axis)
    own, counts = M.owner(cuts, axis, q)
    want = [scalar_owner(cuts.tolist(), float(q[i, axis])) for i in range(len(q))]
    assert own.dtype == np.uint8 and own.tolist() == want
    assert counts.dtype == np.uint32 and counts.tolist() == [want.count(k) for k in range(world)]
    for r in range(world):
        assert M.mine(own, r).tolist() == [i for i, o in enumerate(want) if o == r]
    off = np.concatenate([[0], np.cumsum(counts)[:-1]])
    segs = M.partition(off, own, q)
    assert [s[0] for s in segs] == off.tolist()
    assert [s[1] for s in segs] == [{i for i, o in enumerate(want) if o == k} for k in range(world)]
    # the edges themselves, spelled out: on a cut -> the slab above, one ulp below -> the slab below, -0.0 is on the cut at 0.0, NaN -> 0
    if world == 2:
        e = np.zeros((6, 3), np.float32)
        e[:, axis] = [0.0, -0.0, np.nextafter(np.float32(0), np.float32(-1)), np.nan, np.inf, -np.inf]
        assert M.owner(cuts, axis, e)[0].tolist() == [1, 1, 0, 0, 1, 0]


def test_owner_of_an_empty_batch_and_of_cuts_at_infinity():
    own, counts = M.owner(RC.cuts_for(3, 0), 1, np.empty((0, 3), np.float32))
    assert len(own) == 0 and counts.tolist() == [0, 0, 0]
    cuts = np.array([-np.inf, np.inf, np.inf, np.inf])               # the layout of an empty cloud
    q = np.array([[0, 0, 0], [np.inf, 0, 0], [np.nan, 0, 0], [-np.inf, 0, 0]], np.float32)
    assert M.owner(cuts, 0, q)[0].tolist() == [0, 2, 0, 0]


@pytest.mark.parametrize("edges", RC.EDGE_VARIANTS + ["on_the_edge"])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_certify(edges, axis):
    a = RC.certify_on_the_edge(axis) if edges == "on_the_edge" else RC.certify_case(300, axis, edges, seed=11 + axis)
    got = M.certify(**a)
    assert got.dtype == M.RECORD and got.dtype.itemsize == 16
    ncert = 0
    for i in range(len(got)):
        x = float(a["mine_q"][i, axis])
        margin = c_fmin(x - a["lo_edge"], a["hi_edge"] - x)
        d2 = float(a["ld2"][i])
        found = int(a["lidx"][i]) != NO
        cert = found and margin > 0.0 and d2 < margin * margin
        ncert += cert
        want = (int(a["mine_ids"][i]), int(a["gid"][a["lidx"][i]]) if cert else NO, d2 if cert else -1.0)
        assert (int(got["query"][i]), int(got["gid"][i])) == want[:2], i
        assert struct.pack("<d", float(got["d2"][i])) == struct.pack("<d", want[2]), i
    assert 0 < ncert < len(got)                                        # both verdicts occur in every table
    if edges == "on_the_edge":
        assert (got["d2"] == [-1, -1, 0, 0, -1, -1]).all()             # on the edge and outside: not certified; one ulp inside: certified
    else:
        t = np.arange(len(got)) % 14
        finite_x = np.isfinite(a["mine_q"][:, axis])
        assert (got["d2"][(t == 6) | (t == 11)] == -1.0).all()         # nothing found; found infinitely far
        inside = (t == 1) | (t == 5)
        assert (got["d2"][inside & finite_x] >= 0.0).all() and (got["gid"][inside] != NO).all()
        if np.isfinite(edges[0]) or np.isfinite(edges[1]):             # a finite margin: d2 at and above its square, and margin < 0
            assert (got["d2"][(t == 0) | (t == 2) | (t == 4)] == -1.0).all()
        assert (got["d2"][t == 7] == -1.0).all()                       # a NaN coordinate: margin is NaN
        assert int(a["gid"].max()) == 2 ** 31 - 2


@pytest.mark.parametrize("flagged", ["none", "all", "some"])
@pytest.mark.parametrize("n", [0, 1, 300])
def test_scatter_gather_to_global_put_back(n, flagged):
    n_out = n + 37
    rec = RC.records(n, n_out, flagged, seed=n + len(flagged))
    idx0, d20 = np.full(n_out, 0xA5A5A5A5, np.uint32), np.full(n_out, 7.5)
    idx, d2, fl = M.scatter(rec, idx0, d20)
    wi, wd, wf = idx0.copy(), d20.copy(), set()
    for r in rec:
        wi[r["query"]], wd[r["query"]] = r["gid"], r["d2"]
        if r["d2"] < 0.0:
            wf.add(int(r["query"]))
    assert (idx == wi).all() and (bits(d2) == bits(wd)).all() and fl == wf
    assert (idx0 == 0xA5A5A5A5).all() and (d20 == 7.5).all()          # arguments stay as they were
    assert len(fl) == {"none": 0, "all": n}.get(flagged, len(fl))
    rng = np.random.default_rng(n)
    q = rng.uniform(-1, 1, (n_out, 3)).astype(np.float32)
    q[::7, 1] = np.nan
    ids = rng.permutation(n_out)[:n].astype(np.uint32)
    g = M.gather_queries(q, ids)
    assert g.shape == (n, 3) and all(bits(g[i]).tolist() == bits(q[ids[i]]).tolist() for i in range(n))
    gid = rng.integers(0, 2 ** 31 - 1, 64).astype(np.uint32)
    lidx = rng.integers(0, 64, n).astype(np.uint32)
    lidx[::3] = NO
    assert M.to_global(lidx, gid).tolist() == [NO if v == NO else int(gid[v]) for v in lidx.tolist()]
    vi, vd = rng.integers(0, 2 ** 31 - 1, n).astype(np.uint32), rng.uniform(0, 9, n)
    oi, od = M.put_back(ids, vi, vd, idx0, d20)
    wi, wd = idx0.copy(), d20.copy()
    for i in range(n):
        wi[ids[i]], wd[ids[i]] = vi[i], vd[i]
    assert (oi == wi).all() and (bits(od) == bits(wd)).all()


def test_merge_finish():
    cand = np.array([0, 1, 2 ** 31 - 2, 0x7FFFFFFF, 5, 0x7FFFFFFF], np.int32)
    got = M.merge_finish(cand)
    assert got.dtype == np.uint32 and got.tolist() == [0, 1, 2 ** 31 - 2, NO, 5, NO]
    assert len(M.merge_finish(np.empty(0, np.int32))) == 0
