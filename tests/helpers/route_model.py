"""numpy model (fp64) of the device phases of the routed multi-GPU search, written from the contract in include/pct_engine.h
("device helpers of the spatially routed multi-GPU form") and include/pct_shard.h, not from the kernels:

  slab k of `world` is [cuts[k], cuts[k + 1]) along `axis`, cuts[0] = -inf, cuts[world] = +inf; a query belongs to the slab its
  coordinate falls into (a NaN coordinate compares below every cut: slab 0); an answer record is {uint32 query, uint32 global index,
  double d2}, d2 < 0 = "not certified by its owner".

Every function takes and returns host arrays and leaves its arguments unchanged."""
import numpy as np

NO_INDEX = 0xFFFFFFFF
INT32_MAX = 0x7FFFFFFF
RECORD = np.dtype([("query", "<u4"), ("gid", "<u4"), ("d2", "<f8")])
assert RECORD.itemsize == 16


def owner(cuts, axis, q):
    """(owner[Q] uint8, counts[world] uint32): the number of cuts[1 .. world - 1] that are <= (double) q[:, axis]; NaN -> 0"""
    cuts = np.asarray(cuts, np.float64)
    world = len(cuts) - 1
    x = np.asarray(q, np.float32).reshape(-1, 3)[:, axis].astype(np.float64)
    own = np.searchsorted(cuts[1:world], x, side="right")        # inner cuts ascend (repeats allowed); side="right" counts cuts <= x
    own = np.where(np.isnan(x), 0, own).astype(np.uint8)         # searchsorted sorts NaN last; the contract sends it to slab 0
    return own, np.bincount(own, minlength=world).astype(np.uint32)


def mine(own, rank):
    """the query ids a rank owns, ascending (the device lists them in any order)"""
    return np.nonzero(np.asarray(own) == rank)[0].astype(np.uint32)


def partition(offsets, own, q):
    """per owner: (first slot of its segment, the set of query slots that belong there)"""
    own = np.asarray(own)
    return [(int(o), set(np.nonzero(own == k)[0].tolist())) for k, o in enumerate(offsets)]


def certify(axis, lo_edge, hi_edge, mine_q, mine_ids, lidx, ld2, gid):
    """records of the owner's answers: certified iff a point was found, the query lies strictly inside the halo's edges and the point
    is strictly nearer than the nearer edge (margin = fmin(x - lo_edge, hi_edge - x): a NaN operand is ignored unless both are)"""
    x = np.asarray(mine_q, np.float32).reshape(-1, 3)[:, axis].astype(np.float64)
    lidx = np.asarray(lidx, np.uint32)
    ld2 = np.asarray(ld2, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        margin = np.fmin(x - np.float64(lo_edge), np.float64(hi_edge) - x)
        cert = (lidx != NO_INDEX) & (margin > 0.0) & (ld2 < margin * margin)
    out = np.empty(len(x), RECORD)
    out["query"] = np.asarray(mine_ids, np.uint32)
    out["gid"] = NO_INDEX
    out["d2"] = -1.0
    out["gid"][cert] = np.asarray(gid, np.uint32)[lidx[cert]]
    out["d2"][cert] = ld2[cert]
    return out


def scatter(records, idx, d2):
    """(idx, d2, flagged): every record written to its query's slot; flagged = the set of queries whose d2 < 0"""
    idx, d2 = np.array(idx, np.uint32), np.array(d2, np.float64)
    idx[records["query"]] = records["gid"]
    d2[records["query"]] = records["d2"]
    return idx, d2, set(records["query"][records["d2"] < 0.0].tolist())


def gather_queries(q, ids):
    return np.asarray(q, np.float32).reshape(-1, 3)[np.asarray(ids, np.int64)]


def to_global(lidx, gid):
    """local -> global indices; NO_INDEX stays"""
    lidx = np.asarray(lidx, np.uint32)
    found = lidx != NO_INDEX
    out = lidx.copy()
    out[found] = np.asarray(gid, np.uint32)[lidx[found]]
    return out


def put_back(ids, idx, d2, out_idx, out_d2):
    out_idx, out_d2 = np.array(out_idx, np.uint32), np.array(out_d2, np.float64)
    out_idx[np.asarray(ids, np.int64)] = idx
    out_d2[np.asarray(ids, np.int64)] = d2
    return out_idx, out_d2


def merge_finish(cand):
    """merged int32 candidates -> uint32 indices, INT32_MAX ("no shard holds a point") -> NO_INDEX"""
    cand = np.asarray(cand, np.int32)
    return np.where(cand == INT32_MAX, NO_INDEX, cand.astype(np.int64)).astype(np.uint32)
