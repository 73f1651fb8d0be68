"""Reference model of the voxel de-duplication (include/pct_voxel.h, voxel.hip) and of its key table's hash (vox_key.hpp).

    q = float64(p) / res                             a true fp64 division, never a multiplication by 1 / res
    r = round half away from zero of q               WITHOUT adding 0.5: t = trunc(q); |q - t| >= 0.5 -> t += sign(q).  q - t is exact
                                                     (Sterbenz for |q| >= 1, q itself below), so no double near a tie is misjudged;
                                                     floor(q + 0.5) is not: 0.49999999999999994 + 0.5 rounds up to 1.0
    accepted  <=>  -2^20 <= r < 2^20 on all three axes (a NaN or infinite quotient fails it)
    ids in first-seen order over the ACCEPTED points only; a skipped point reports is_new = 0, voxel_index = -1
    centres   float64(i) * res, and that product narrowed to float32

The tables of adversarial coordinates the GPU tests and the CPU check of this model against oracle/voxel_port.c share are here too."""
import numpy as np

LIM = 1 << 20


def quotient(p, res):
    return np.asarray(p).astype(np.float64) / np.float64(res)


def round_half_away(q):
    """C's round() on float64 arrays; NaN and +-inf pass through"""
    q = np.asarray(q, np.float64)
    with np.errstate(invalid="ignore"):
        t = np.trunc(q)
        up = np.abs(q - t) >= 0.5
    return np.where(up, t + np.sign(q), t)


def coords(pts, res):
    """(rounded quotients float64 [n, 3], accepted [n])"""
    r = round_half_away(quotient(np.asarray(pts)[:, :3], res))
    with np.errstate(invalid="ignore"):
        ok = np.all((r >= -LIM) & (r < LIM), axis=1)
    return r, ok


class VoxelModel:
    """sequential voxel_map / voxel_value_map over the accepted points"""

    def __init__(self, res):
        self.res = float(res)
        self.ids = {}
        self.key_list = []

    def __len__(self):
        return len(self.key_list)

    def clear(self):
        self.ids.clear()
        self.key_list.clear()

    def add(self, pts):
        """(n_new, is_new uint8 [n], voxel_index int32 [n], accepted bool [n])"""
        pts = np.asarray(pts)
        n = len(pts)
        is_new, index = np.zeros(n, np.uint8), np.full(n, -1, np.int32)
        if n == 0:
            return 0, is_new, index, np.zeros(0, bool)
        r, ok = coords(pts, self.res)
        k = np.where(ok[:, None], r, 0.0).astype(np.int64)
        before = len(self.key_list)
        ids, keys = self.ids, self.key_list
        for i in np.nonzero(ok)[0].tolist():
            key = (int(k[i, 0]), int(k[i, 1]), int(k[i, 2]))
            got = ids.get(key)
            if got is None:
                got = ids[key] = len(keys)
                keys.append(key)
                is_new[i] = 1
            index[i] = got
        return len(keys) - before, is_new, index, ok

    def keys(self):
        return np.asarray(self.key_list, np.int32).reshape(-1, 3)

    def cloud_f64(self):
        return self.keys().astype(np.float64) * np.float64(self.res)

    def cloud_f32(self):
        return self.cloud_f64().astype(np.float32)


# ---- the key table's hash (vox_key.hpp), restated -------------------------------------------------------------------------------------
def vox_pack(k):
    """vox_pack of int keys [n, 3] -> uint64 [n]: 21 bits per axis, biased by 2^20"""
    b = (np.asarray(k, np.int64) + LIM).astype(np.uint64)
    return b[:, 0] | (b[:, 1] << np.uint64(21)) | (b[:, 2] << np.uint64(42))


def vox_hash(key):
    """the murmur3 finaliser, low 32 bits"""
    k = np.asarray(key, np.uint64).copy()
    with np.errstate(over="ignore"):
        k ^= k >> np.uint64(33)
        k *= np.uint64(0xff51afd7ed558ccd)
        k ^= k >> np.uint64(33)
        k *= np.uint64(0xc4ceb9fe1a85ec53)
        k ^= k >> np.uint64(33)
    return (k & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def colliding_voxels(count=300, low_bits=16, value=0xFFFF):
    """`count` lattice keys [count, 3] (int32) whose hashes agree with `value` in their low `low_bits` bits, drawn in lattice order from
    a 288^3 block (2.4 x 10^7 keys, ~360 of them hit) around the origin: in any table of up to 2^low_bits slots they share one home
    slot -- the LAST one for value = all ones, so that their probe chain wraps to slot 0"""
    side = 288
    ax = np.arange(side, dtype=np.int64) - side // 2
    out = []
    for z in ax:                                                      # a z-slab at a time keeps the working set small
        k = np.empty((side * side, 3), np.int64)
        k[:, 0] = np.tile(ax, side)
        k[:, 1] = np.repeat(ax, side)
        k[:, 2] = z
        hit = (vox_hash(vox_pack(k)) & np.uint32((1 << low_bits) - 1)) == np.uint32(value)
        out.extend(k[hit].tolist())
        if len(out) >= count:
            break
    assert len(out) >= count
    return np.asarray(out[:count], np.int32)


# ---- adversarial coordinates -----------------------------------------------------------------------------------------------------------
def _around(v, dtype, steps=1):
    """v and `steps` neighbours on each side, in dtype"""
    v = dtype(v)
    out, lo, hi = [v], v, v
    for _ in range(steps):
        lo, hi = np.nextafter(lo, dtype(-np.inf)), np.nextafter(hi, dtype(np.inf))
        out += [lo, hi]
    return out


def tie_values(dtype):
    """coordinates on and beside the ties of res = 0.1 (and off-tie for 0.25 and 1/3): k * 0.05 for k = 0..40 as the fp64 product and
    as the decimal's nearest double k / 20 (0.15 is the latter, 0.15000000000000002 the former), then held in `dtype` (the fp32
    table reaches the kernel widened), and 0.049999999999999996 -- whose quotient by 0.1 is 0.49999999999999994, the double below
    one half -- each with its nextafter neighbours on both sides, both signs, and -0.0"""
    base = sorted(set([k * 0.05 for k in range(41)] + [k / 20.0 for k in range(41)])) + [0.049999999999999996]
    vals = []
    for b in base:
        for v in _around(b, dtype):
            vals += [v, -v]
    vals.append(dtype(-0.0))
    return np.asarray(vals, dtype)


def tie_points(dtype):
    """[n, 3] points: each tie value on each axis in turn, the other two axes on fixed off-tie coordinates, then all three axes
    equal; ~250 distinct values -> ~1000 points with many repeated voxels"""
    v = tie_values(dtype)
    rows = []
    for ax in range(3):
        p = np.empty((len(v), 3), dtype)
        p[:] = dtype(0.52), dtype(-1.31), dtype(2.04)
        p[:, ax] = v
        rows.append(p)
    rows.append(np.stack([v, v, v], axis=1))
    return np.concatenate(rows)


RANGE_TARGETS = (LIM - 1, LIM, -LIM, -LIM - 1)


def range_values(res, dtype, steps=3):
    """coordinates whose rounded quotient by res is 2^20 - 1, 2^20 (the first one out), -2^20 (the last one in) and -2^20 - 1: the
    doubles (floats) within `steps` nextafter steps of +-2^20 * res and of the rounding boundaries (+-2^20 -+ 0.5) * res,
    (-2^20 - 0.5) * res; asserts that all four quotients occur"""
    vals = []
    for c in (LIM - 0.5, float(LIM), -(LIM - 0.5), -float(LIM), -(LIM + 0.5)):
        vals += _around(c * res, dtype, steps)
    vals = np.asarray(vals, dtype)
    r = round_half_away(quotient(vals, res))
    assert set(RANGE_TARGETS) <= set(r.astype(np.int64).tolist()), (res, dtype)
    return vals


def wild_values(dtype):
    """non-finite and huge coordinates: always skipped"""
    v = [np.inf, -np.inf, np.nan, 3e38, -3e38]
    if dtype == np.float64:
        v += [1e300, -1e300]
    return np.asarray(v, dtype)


def on_each_axis(vals, dtype, rest=(0.3, -0.7, 1.2)):
    """every value on x, then on y, then on z, the other two coordinates valid"""
    vals = np.asarray(vals, dtype)
    rows = []
    for ax in range(3):
        p = np.empty((len(vals), 3), dtype)
        p[:] = [dtype(x) for x in rest]
        p[:, ax] = vals
        rows.append(p)
    return np.concatenate(rows)
