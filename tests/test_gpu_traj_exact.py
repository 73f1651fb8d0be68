"""GPU tests of the trajectory evaluators (traj.hip through include/pct_traj.h) against the exact-power model of
tests/helpers/traj_exact_model.py, which tests/test_traj_exact_model.py holds to the oracle port and to rational arithmetic.

Bars: every comparison is np.array_equal on the BITS of the doubles (.view(np.uint64), so -0.0 and 0.0 are told apart) or == on
integers; there is no tolerance in this file.  All three kernels take their powers from pct::pow_uint_cr, which is correctly
rounded, and follow the reference's order of operations without contraction, so nothing is left to tolerate.

    pct_bezier_state_batch     one-hot rows (single Bernstein terms that cannot cancel) and rows of mixed magnitude for every order
                               1..12 at the edges of u; n across the block size of 256 and the workspace floor of 4096; wide rows
    pct_traj_wire_sample       five trajectories x 2, 3, 11, 257, 1001 samples: positions and step lengths; either output alone
    pct_traj_segm_index,       at the adjacent doubles where the model's answer changes (bisected), at both zeros, a negative length,
    pct_traj_nearest_voxels    NaN, infinity; the voxel cloud against the model's positions through tests/helpers/voxel_exact_model.py
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import traj_exact_model as M  # noqa: E402
import voxel_exact_model as VM  # noqa: E402

pytestmark = pytest.mark.gpu

PCT_ERR_INVALID = 2
TRAJ = M.trajectories()
SENTINEL = -7.25e77

U_EDGES = np.float64([
    0.0, -0.0, 1.0, 2.0 ** -1074, 2.0 ** -1022, 2.0 ** -30, 0.5, np.nextafter(0.5, 0.0), np.nextafter(0.5, 1.0), 1.0 / 3.0,
    1.0 - 2.0 ** -53, (2.0 ** 27 - 1) * 2.0 ** -27,       # the last one's square is an exact tie of the rounding
    *M.LIBM_MISS_U,                                       # glibc's pow is one ulp off at these
    -0.25, 1.25,                                          # outside [0, 1]: the reference evaluates them like any other
])


@pytest.fixture(scope="module")
def E():
    from pointcloudtraj_amd import engine
    engine.init(0)
    return engine


@pytest.fixture(scope="module")
def T(E):
    from pointcloudtraj_amd import traj
    traj._lib()
    return traj


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------ pct_bezier_state_batch
def one_hot_rows():
    """a segment for every order n = 1..12 and every j = 0..n: 1.0 at control point j of one axis (the axis moves with n + j),
    0.0 elsewhere -- 90 segments, each of whose nine outputs is a single Bernstein term or an exact zero"""
    rows, orders = [], []
    for n in range(1, 13):
        for j in range(n + 1):
            r = np.zeros(39)
            r[((n + j) % 3) * (n + 1) + j] = 1.0
            rows.append(r)
            orders.append(n)
    return np.asarray(rows), np.ones(len(rows)), np.int32(orders)


def mixed_rows():
    """orders 1..12, every row mixing coordinates of magnitude 1e-3, 1 and 1e4"""
    rng = np.random.default_rng(20261021)
    orders = np.arange(1, 13, dtype=np.int32)
    pc = np.zeros((12, 39))
    scale = np.float64([1e-3, 1.0, 1e4])
    for s, n in enumerate(orders):
        k = 3 * (int(n) + 1)
        pc[s, :k] = rng.uniform(-1, 1, k) * scale[(np.arange(k) + s) % 3]
    return pc, np.linspace(0.6, 1.7, 12), orders


@pytest.mark.parametrize("rows", ["one_hot", "mixed"])
def test_state_is_the_model_bit_for_bit_at_the_edges_of_u(T, rows):
    pc, times, orders = one_hot_rows() if rows == "one_hot" else mixed_rows()
    seg = np.repeat(np.arange(len(orders)), len(U_EDGES)).astype(np.int32)
    u = np.tile(U_EDGES, len(orders))
    want, _ = M.state(pc, orders, seg, u)
    got = T.get_state_from_bezier(pc, times, orders, seg, u)
    assert same_bits(got[:, :3], want[:, :3])                          # positions
    assert same_bits(got[:, 3:6], want[:, 3:6]) and same_bits(got[:, 6:9], want[:, 6:9])
    if rows == "one_hot":
        assert np.count_nonzero(want[:, :3]) > 0 and np.count_nonzero(want[:, 6:9]) > 0
    else:
        mag = np.abs(want[:, :3])
        assert mag.max() > 1e3 and mag[mag > 0].min() < 1e-2          # what a tolerance scaled by the array maximum would hide


@functools.lru_cache(maxsize=None)
def batch_pool():
    """the (segment, u) pairs the batch sizes draw from, with the model's answer for each: 12 segments x (the edges of u + 8 others)"""
    pc, times, orders = mixed_rows()
    rng = np.random.default_rng(7)
    us = np.concatenate([U_EDGES, rng.uniform(0, 1, 8)])
    seg = np.repeat(np.arange(12), len(us)).astype(np.int32)
    u = np.tile(us, 12)
    want, _ = M.state(pc, orders, seg, u)
    return seg, u, want


def batch_of(n):
    """n samples in scrambled segment order with repeats"""
    seg, u, want = batch_pool()
    pick = (np.arange(n, dtype=np.int64) * 7919 + 13) % len(seg)
    return seg[pick], u[pick], want[pick]


def test_state_batch_sizes_across_blocks_and_workspace_growth(T):
    """n = 0, one partial block, the block boundary (256 threads), and above the workspace floor of 4096 elements, where the three
    scratch buffers grow; then a small batch again in the grown buffers"""
    pc, times, orders = mixed_rows()
    t, keep = T._matrix(pc, times, orders)
    for n in (0, 1, 255, 256, 257, 4097, 1):
        seg, u, want = batch_of(n)
        assert n < 12 or len(np.unique(seg)) == 12
        out = np.full((n + 2, 9), SENTINEL)                            # a guard row on each side
        st = T._lib().pct_bezier_state_batch(C.byref(t), seg.ctypes.data, u.ctypes.data, n, out[1:].ctypes.data)
        assert st == 0, n
        assert same_bits(out[1:n + 1], want), n
        assert np.all(out[0] == SENTINEL) and np.all(out[n + 1] == SENTINEL), n
    assert same_bits(T.get_state_from_bezier(pc, times, orders, [], []), np.zeros((0, 9)))


def test_state_wide_rows_ignore_their_tail(T):
    pc, times, orders = mixed_rows()
    wide = np.full((12, 64), np.nan)
    for s, n in enumerate(orders):
        wide[s, :3 * (n + 1)] = pc[s, :3 * (n + 1)]
    seg, u, want = batch_of(600)
    narrow = T.get_state_from_bezier(pc, times, orders, seg, u)
    got = T.get_state_from_bezier(wide, times, orders, seg, u)         # row_stride = 64
    assert same_bits(got, narrow) and same_bits(got, want)


# ------------------------------------------------------------------------------------------------ pct_traj_wire_sample
def pack_wire(T, pc, times, orders):
    """the wire arrays packed here in numpy (control points of all segments concatenated, one array per axis)"""
    cx, cy, cz = [], [], []
    for s, n in enumerate(orders):
        m = int(n) + 1
        cx += pc[s, :m].tolist(); cy += pc[s, m:2 * m].tolist(); cz += pc[s, 2 * m:3 * m].tolist()
    return T.WireTraj(cx, cy, cz, times, orders)


@functools.lru_cache(maxsize=None)
def model_samples(name, samples):
    from pointcloudtraj_amd import traj
    got = M.wire_sample(pack_wire(traj, *TRAJ[name]), samples)
    for a in got:
        a.setflags(write=False)
    return got


def test_wire_packing_is_the_librarys(T):
    for name, (pc, times, orders) in TRAJ.items():
        w, mine = T.get_bezier_traj_wire(pc, times, orders), pack_wire(T, pc, times, orders)
        assert same_bits(w.coef_x, mine.coef_x) and same_bits(w.coef_y, mine.coef_y) and same_bits(w.coef_z, mine.coef_z)


@pytest.mark.parametrize("samples", [2, 3, 11, 257, 1001])
@pytest.mark.parametrize("name", list(TRAJ))
def test_wire_samples_and_steps_are_the_model_bit_for_bit(T, name, samples):
    w = pack_wire(T, *TRAJ[name])
    want_pos, want_step, _ = model_samples(name, samples)
    pos, step = T.wire_sample(w, samples)
    assert same_bits(pos, want_pos)
    assert same_bits(step, want_step)
    if name == "gap" and samples > 2:
        assert 1e-3 < want_step[samples] < 2e-3                        # the joint's step is the gap, not ~0
    # either output alone: the other one is not needed for it, and a NULL is not written through
    cw = w._c()
    total = w.num_segment * samples
    only_pos, only_step = np.full((total + 1, 3), SENTINEL), np.full(total + 1, SENTINEL)
    assert T._lib().pct_traj_wire_sample(C.byref(cw), samples, only_pos.ctypes.data, None) == 0
    assert T._lib().pct_traj_wire_sample(C.byref(cw), samples, None, only_step.ctypes.data) == 0
    assert same_bits(only_pos[:total], want_pos) and np.all(only_pos[total] == SENTINEL)
    assert same_bits(only_step[:total], want_step) and only_step[total] == SENTINEL


def test_wire_sample_refuses_one_sample_and_takes_an_empty_wire(E, T):
    w = pack_wire(T, *TRAJ["single"])
    with pytest.raises(E.EngineError) as ei:
        T.wire_sample(w, 1)
    assert ei.value.code == PCT_ERR_INVALID
    empty = T.WireTraj([], [], [], [], [])
    cw = empty._c()
    pos, step = np.full(12, SENTINEL), np.full(4, SENTINEL)
    for samples in (2, 1001):
        assert T._lib().pct_traj_wire_sample(C.byref(cw), samples, pos.ctypes.data, step.ctypes.data) == 0
    assert np.all(pos == SENTINEL) and np.all(step == SENTINEL)


# ------------------------------------------------------------------------------------------------ the walks
def fast_lens(step, L):
    """`len` after every subtraction: a - b is a + (-b) bit for bit and cumsum adds in sequence.  Used to bisect only; every pair
    it finds is confirmed with the model's plain loops before the device is asked."""
    return np.cumsum(np.concatenate([[L], -step]))[1:]


def fast_segm(step, nseg, L):
    neg = np.nonzero(fast_lens(step, L) < 0)[0]
    if not len(neg):
        return nseg - 1, 1
    g = int(neg[0])
    return g // M.SAMPLES, 1 if (g % M.SAMPLES) / 1000.0 > 0.5 else 0


def fast_used(step, L):
    if not L >= 0:
        return 0
    stop = np.nonzero(~(fast_lens(step, L) >= 0))[0]
    return int(stop[0]) + 1 if len(stop) else len(step)


@functools.lru_cache(maxsize=None)
def walk_lengths(name):
    """(segm_index lengths, nearest_voxels lengths): both members of every adjacent pair of doubles at which the model's answer
    changes -- the first half boundary (t > 0.5), the first joint, the last half boundary; three sample counts -- then the edges"""
    _, step, _ = model_samples(name, M.SAMPLES)
    nseg = len(TRAJ[name][1])
    acc = np.cumsum(step)
    total = float(acc[-1])
    first = 1 if name == "hover_then_move" else 0                      # no length ends inside a segment of no length
    brackets = [(first * 1001 + 498, first * 1001 + 503), ((nseg - 1) * 1001 + 498, (nseg - 1) * 1001 + 503)]
    if nseg - first > 1:
        brackets.append((first * 1001 + 998, (first + 1) * 1001 + 3))
    brackets = list(dict.fromkeys(brackets))                           # one segment: its first half boundary is its last
    seg_pairs = [M.adjacent_change(lambda L: fast_segm(step, nseg, L), float(acc[a]), float(acc[b])) for a, b in brackets]
    used_pairs = [M.adjacent_change(lambda L: fast_used(step, L), float(acc[g - 1]), float(acc[g + 1]))
                  for g in (first * 1001 + 3, len(step) // 2 + 77, len(step) - 3)]
    steps = step.tolist()
    for a, b in seg_pairs:
        assert M.segm_index(steps, nseg, a) != M.segm_index(steps, nseg, b)
    for a, b in used_pairs:
        assert M.points_used(steps, a) != M.points_used(steps, b)
    assert len(seg_pairs) + len(used_pairs) >= 4
    edges = [0.0, -0.0, -1.0, float("nan"), float("inf"), 10 * total]
    return [v for p in seg_pairs for v in p] + edges, [v for p in used_pairs for v in p] + [seg_pairs[0][0], seg_pairs[0][1]] + edges


@pytest.mark.parametrize("name", list(TRAJ))
def test_segm_index_at_the_doubles_where_the_answer_changes(T, name):
    w = pack_wire(T, *TRAJ[name])
    steps = model_samples(name, M.SAMPLES)[1].tolist()
    seen = set()
    for L in walk_lengths(name)[0]:
        want = M.segm_index(steps, w.num_segment, L)
        assert T.get_segm_index(w, L) == want, (name, L)
        seen.add(want)
    assert len(seen) >= (3 if w.num_segment > 1 else 2)
    if name == "hover_then_move":                                      # len is exactly 0.0 all through segment 0: `<`, not `<=`
        assert T.get_segm_index(w, 0.0) == (1, 0) and T.get_segm_index(w, -0.0) == (1, 0)


@pytest.mark.parametrize("name", list(TRAJ))
def test_nearest_voxels_at_the_doubles_where_the_count_changes(T, name):
    from pointcloudtraj_amd import voxel
    w = pack_wire(T, *TRAJ[name])
    pos, step, _ = model_samples(name, M.SAMPLES)
    steps = step.tolist()
    filler = np.float64([[55.5, -44.4, 33.3]])
    for res in (0.1, 0.25):
        vm = voxel.VoxelMap(res, 4096)
        lengths = walk_lengths(name)[1]
        for L in (lengths if res == 0.1 else lengths[:2] + lengths[-6:]):
            assert vm.add_point_cloud(filler) == 1 and len(vm) >= 1    # the map holds something else before the call
            used = C.c_int64(-1)
            cw = w._c()
            assert T._lib().pct_traj_nearest_voxels(C.byref(cw), float(L), vm._h, C.byref(used)) == 0
            want_used = M.points_used(steps, L)
            assert used.value == want_used, (name, res, L)
            model = VM.VoxelModel(res)
            _, _, _, ok = model.add(pos[:want_used])
            assert ok.all()
            assert len(vm) == len(model)                               # ... and was cleared: the filler's voxel is gone
            assert np.array_equal(vm.keys(), model.keys()), (name, res, L)
            assert same_bits(vm.get_voxel_cloud(np.float64), model.cloud_f64())
            assert np.array_equal(vm.get_voxel_cloud(np.float32).view(np.uint32), model.cloud_f32().view(np.uint32))
            assert not np.any(np.all(model.keys() == np.int32(VM.round_half_away(filler / res)), axis=1))
        vm.close()
    if name == "hover_then_move":
        assert M.points_used(steps, 0.0) == 1003                       # all of the hover, and two samples more


def test_walks_on_an_empty_wire(T):
    from pointcloudtraj_amd import voxel
    empty = T.WireTraj([], [], [], [], [])
    vm = voxel.VoxelMap(0.1, 4096)
    for L in (0.0, 1.0, float("nan"), float("inf"), -1.0):
        assert T.get_segm_index(empty, L) == (-1, 1)
        assert vm.add_point_cloud(np.float64([[1.0, 2.0, 3.0]])) == 1
        used = C.c_int64(-1)
        cw = empty._c()
        assert T._lib().pct_traj_nearest_voxels(C.byref(cw), L, vm._h, C.byref(used)) == 0
        assert used.value == 0 and len(vm) == 0
    vm.close()
