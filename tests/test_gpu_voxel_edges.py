"""GPU tests of the voxel map (voxel.hip, vox_key.hpp through include/pct_voxel.h) at its edges, against the model of
tests/helpers/voxel_exact_model.py, which tests/test_voxel_exact_model.py holds to the sequential oracle.

Bars: everything exact -- statuses, n_new, sizes, per-point flags and indices ==, keys np.array_equal, centres equal in their bits.
Every case goes through both pct_voxel_map_add (host records) and pct_voxel_map_add_dev (torch tensors; the per-point outputs are
device tensors framed by guard rows), by ctypes, because the Python wrapper raises on PCT_ERR_INVALID and drops the device outputs.

    ties             coordinates on and one double beside x.5 quotients at res 0.1, 0.25, 1/3: a true division, round half away
    key range        the last voxel inside [-2^20, 2^20) and the first outside on every axis, non-finite and huge coordinates, mixed
                     with valid points: the offenders are skipped (is_new 0, voxel_index -1), the rest added, PCT_ERR_INVALID
    tiles            n around the 1024-point rank tile, first occurrences only in the last tile, a repeat across a tile boundary
    probe chains     300 voxels that share the LAST home slot of the table, claimed concurrently, kept through a rehash
    windows          reads at (first, count), record strides, refused arguments"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import voxel_exact_model as VM  # noqa: E402

pytestmark = pytest.mark.gpu

PCT_OK, PCT_ERR_INVALID = 0, 2
GUARD = 8
NEW_SENTINEL, INDEX_SENTINEL = 0xAB, -77
LAYOUTS = [(np.float32, 12), (np.float32, 16), (np.float32, 20), (np.float64, 24), (np.float64, 32)]
LAYOUT_IDS = [f"{np.dtype(d).name}_stride{s}" for d, s in LAYOUTS]
FORMS = ("host", "dev")


@pytest.fixture(scope="module")
def E():
    import torch  # noqa: F401  (first: one HIP runtime per process)
    from pointcloudtraj_amd import engine
    engine.init(0)
    return engine


@pytest.fixture(scope="module")
def V(E):
    from pointcloudtraj_amd import voxel
    voxel._lib()
    return voxel


def records(pts, dtype, stride):
    """[n, stride / itemsize] records of dtype: x, y, z, then NaN in whatever the stride leaves over"""
    pts = np.asarray(pts)
    rec = np.full((len(pts), stride // np.dtype(dtype).itemsize), np.nan, dtype)
    rec[:, :3] = pts[:, :3]
    return rec


def add(V, vm, form, pts, dtype, stride):
    """one batch through ctypes -> (status, n_new, is_new uint8 [n], voxel_index int32 [n]); the guard rows are checked here"""
    rec = records(pts, dtype, stride)
    n = len(rec)
    f64 = int(np.dtype(dtype) == np.float64)
    n_new = C.c_int64(-5)
    L = V._lib()
    if form == "host":
        is_new, index = np.full(n + 2 * GUARD, NEW_SENTINEL, np.uint8), np.full(n + 2 * GUARD, INDEX_SENTINEL, np.int32)
        st = L.pct_voxel_map_add(vm._h, rec.ctypes.data, n, stride, f64, C.byref(n_new), is_new[GUARD:].ctypes.data, index[GUARD:].ctypes.data)
    else:
        import torch
        d_pts = torch.from_numpy(rec).cuda()
        assert d_pts.is_contiguous() and (n == 0 or d_pts.stride(0) * d_pts.element_size() == stride)
        d_new = torch.full((n + 2 * GUARD,), NEW_SENTINEL, dtype=torch.uint8, device="cuda")
        d_index = torch.full((n + 2 * GUARD,), INDEX_SENTINEL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        st = L.pct_voxel_map_add_dev(vm._h, d_pts.data_ptr(), n, stride, f64, C.byref(n_new), d_new.data_ptr() + GUARD,
                                     d_index.data_ptr() + 4 * GUARD)
        is_new, index = d_new.cpu().numpy(), d_index.cpu().numpy()
    for a, s in ((is_new, NEW_SENTINEL), (index, INDEX_SENTINEL)):
        assert np.all(a[:GUARD] == s) and np.all(a[GUARD + n:] == s), "a per-point output was written outside [0, n)"
    return st, n_new.value, is_new[GUARD:GUARD + n], index[GUARD:GUARD + n]


def add_and_compare(V, vm, model, form, pts, dtype, stride):
    """one batch into the map and into the model: status, n_new, flags and indices are the model's"""
    pts = np.asarray(pts, dtype)
    st, n_new, is_new, index = add(V, vm, form, pts, dtype, stride)
    want_new, want_is_new, want_index, ok = model.add(pts)
    assert st == (PCT_OK if ok.all() else PCT_ERR_INVALID)
    assert n_new == want_new
    assert np.array_equal(is_new, want_is_new)
    assert np.array_equal(index, want_index)
    assert np.all(index[~ok] == -1) and not np.any(is_new[~ok])                      # what a skipped point reports
    return index


def compare_store(vm, model):
    assert len(vm) == len(model)
    assert np.array_equal(vm.keys(), model.keys())
    assert np.array_equal(vm.get_voxel_cloud(np.float32).view(np.uint32), model.cloud_f32().view(np.uint32))
    assert np.array_equal(vm.get_voxel_cloud(np.float64).view(np.uint64), model.cloud_f64().view(np.uint64))


# ------------------------------------------------------------------------------------------------ ties and near-ties
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("res", [0.1, 0.25, 1.0 / 3.0], ids=["res0.1", "res0.25", "res1_3"])
@pytest.mark.parametrize("dtype,stride", LAYOUTS, ids=LAYOUT_IDS)
def test_ties_and_near_ties_divide_and_round_half_away(V, dtype, stride, res, form):
    pts = VM.tie_points(dtype)
    vm, model = V.VoxelMap(res), VM.VoxelModel(res)
    first = add_and_compare(V, vm, model, form, pts, dtype, stride)
    again = add_and_compare(V, vm, model, form, pts[::-1], dtype, stride)           # nothing new; the same ids, reversed
    assert np.array_equal(again, first[::-1])
    compare_store(vm, model)
    vm.close()


# ------------------------------------------------------------------------------------------------ the key range
@functools.lru_cache(maxsize=None)
def mixed_batch(res, dtype_name):
    """range and wild coordinates on each axis in turn, interleaved with valid points (one valid point after every offender and
    every edge point, some of them repeats)"""
    dtype = np.dtype(dtype_name).type
    edge = VM.on_each_axis(np.concatenate([VM.range_values(res, dtype), VM.wild_values(dtype)]), dtype)
    rng = np.random.default_rng(5)
    valid = (rng.integers(-40, 40, (len(edge), 3)) * res + rng.uniform(-0.3, 0.3, (len(edge), 3)) * res).astype(dtype)
    valid[1::3] = valid[0::3][: len(valid[1::3])]                                     # repeats among the valid ones
    out = np.empty((2 * len(edge), 3), dtype)
    out[0::2], out[1::2] = edge, valid
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("res", [0.1, 1.0])
@pytest.mark.parametrize("dtype,stride", LAYOUTS, ids=LAYOUT_IDS)
def test_key_range_edges_are_skipped_or_kept_exactly(V, dtype, stride, res, form):
    pts = mixed_batch(res, np.dtype(dtype).name)
    r, ok = VM.coords(pts, res)
    kept = set(r[ok].astype(np.int64).reshape(-1).tolist())
    assert VM.LIM - 1 in kept and -VM.LIM in kept                      # the last voxels inside, on the boundary's near side
    assert {VM.LIM, -VM.LIM - 1} <= set(r[~ok][np.abs(r[~ok]) < 2.0 ** 40].astype(np.int64).tolist())    # the first ones outside
    assert (~ok).sum() > 20 and ok.sum() > len(pts) // 2
    vm, model = V.VoxelMap(res), VM.VoxelModel(res)
    first = add_and_compare(V, vm, model, form, pts, dtype, stride)    # PCT_ERR_INVALID, the valid points added
    size = len(vm)
    assert size == len(model) > 0
    again = add_and_compare(V, vm, model, form, pts, dtype, stride)    # a second identical batch adds nothing
    assert len(vm) == size and np.array_equal(again, first)
    compare_store(vm, model)
    only_bad = pts[~ok]
    assert add(V, vm, form, only_bad, dtype, stride)[:2] == (PCT_ERR_INVALID, 0) and len(vm) == size
    assert add_and_compare(V, vm, model, form, pts[1::2][:5] + dtype(3.0), dtype, stride).min() >= 0    # the map goes on working: PCT_OK
    compare_store(vm, model)
    vm.close()


# ------------------------------------------------------------------------------------------------ rank tiles
def half_repeats(n, seed, res=0.1):
    """n points of which about half repeat an earlier one"""
    rng = np.random.default_rng(seed)
    pts = (rng.integers(-300, 300, (n, 3)) * res).astype(np.float32)
    for i in range(1, n):
        if rng.random() < 0.5:
            pts[i] = pts[rng.integers(0, i)]
    return pts


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", [1, 2, 1023, 1024, 1025, 3 * 1024 + 1])
def test_batch_sizes_around_the_rank_tile(V, n, form):
    pts = half_repeats(n, n)
    vm, model = V.VoxelMap(0.1), VM.VoxelModel(0.1)
    add_and_compare(V, vm, model, form, pts, np.float32, 12)
    assert n < 3 or len(model) < n                                     # there were repeats
    compare_store(vm, model)
    vm.close()


@pytest.mark.parametrize("form", FORMS)
def test_first_occurrences_only_in_the_last_tile(V, form):
    """two full tiles that only re-observe known voxels (tile totals 0, 0), then a tile with new ones"""
    known = half_repeats(500, 91)
    rng = np.random.default_rng(92)
    tail = (rng.integers(400, 700, (700, 3)) * 0.1).astype(np.float32)
    tail[1::2] = tail[0::2]
    batch = np.concatenate([known[rng.integers(0, 500, 2048)], tail])
    vm, model = V.VoxelMap(0.1), VM.VoxelModel(0.1)
    add_and_compare(V, vm, model, form, known, np.float32, 16)
    before = len(model)
    index = add_and_compare(V, vm, model, form, batch, np.float32, 16)
    assert index[:2048].max() < before <= index[2048:].min() and len(model) > before + 300
    compare_store(vm, model)
    vm.close()


@pytest.mark.parametrize("form", FORMS)
def test_first_occurrence_and_its_repeat_on_both_sides_of_a_tile_boundary(V, form):
    pts = half_repeats(1030, 93)
    pts[1023] = pts[1024] = np.float32([77.7, -77.7, 7.7])             # new at the last point of tile 0, repeated at the first of tile 1
    vm, model = V.VoxelMap(0.1), VM.VoxelModel(0.1)
    st, n_new, is_new, index = add(V, vm, form, pts, np.float32, 12)
    want_new, want_is_new, want_index, _ = model.add(pts)
    assert st == PCT_OK and n_new == want_new and np.array_equal(is_new, want_is_new) and np.array_equal(index, want_index)
    assert is_new[1023] == 1 and is_new[1024] == 0 and index[1023] == index[1024]
    compare_store(vm, model)
    vm.close()


# ------------------------------------------------------------------------------------------------ probe chains
@functools.lru_cache(maxsize=None)
def chain_voxels():
    k = VM.colliding_voxels(300, 16, 0xFFFF)
    k.setflags(write=False)
    return k


@pytest.mark.parametrize("form", FORMS)
def test_one_probe_chain_from_the_last_slot_through_a_rehash(V, form):
    """300 voxels whose home slot is the last one of any table up to 65 536 slots: their chain wraps to slot 0 and every claim
    walks it.  Each three times in one shuffled batch with 300 random voxels (many threads claim along the chain at once), the
    batch reversed, then 40 000 points from capacity_hint = 16 (the store grows, the table is rehashed beyond 65 536 slots where
    the 300 part), then the 300 again: the model's ids, flags and n_new after every step, and the 300 keep their ids."""
    res = 0.1
    keys = chain_voxels()
    rng = np.random.default_rng(17)
    chain = keys.astype(np.float64) * res
    assert np.array_equal(VM.coords(chain, res)[0].astype(np.int32), keys)        # the points do land in those voxels
    randoms = rng.integers(-150, 150, (300, 3)) * res
    batch = np.concatenate([chain, chain, chain, randoms])[rng.permutation(1200)]
    # pct_voxel_map_create floors the hint at 1024 voxels (a table of 2048 slots); the 1200-point batch makes it 4096 slots, so the
    # chain's home slot is 4095 and it wraps to slot 0
    vm, model = V.VoxelMap(res, capacity_hint=16), VM.VoxelModel(res)
    add_and_compare(V, vm, model, form, batch, np.float64, 24)
    ids = add_and_compare(V, vm, model, form, chain, np.float64, 24)
    assert len(np.unique(ids)) == 300
    add_and_compare(V, vm, model, form, batch[::-1], np.float64, 24)
    compare_store(vm, model)
    big = rng.uniform(-20, 20, (40000, 3))
    add_and_compare(V, vm, model, form, big, np.float64, 32)
    assert 2 * len(model) > 65536                                      # load factor <= 0.5: the table now has 131 072 slots
    assert np.array_equal(add_and_compare(V, vm, model, form, chain, np.float64, 24), ids)
    assert np.array_equal(add_and_compare(V, vm, model, form, chain[::-1].astype(np.float32), np.float32, 12), ids[::-1])
    compare_store(vm, model)
    vm.close()


# ------------------------------------------------------------------------------------------------ windows and refusals
def test_windows_equal_slices_of_the_full_read(V):
    L = V._lib()
    vm, model = V.VoxelMap(0.1), VM.VoxelModel(0.1)
    add_and_compare(V, vm, model, "host", VM.tie_points(np.float64), np.float64, 24)
    size = len(vm)
    assert size > 20
    keys, f32, f64 = model.keys(), model.cloud_f32(), model.cloud_f64()
    compare_store(vm, model)                                           # the full read is the model's
    for first, count in ((0, 0), (0, size), (5, 7), (size - 1, 1), (size, 0)):
        k = np.full((count + 1, 3), INDEX_SENTINEL, np.int32)
        a = np.full((count + 1, 3), -7.5, np.float32)
        b = np.full((count + 1, 3), -7.5)
        a4 = np.full((count + 1, 4), -7.5, np.float32)
        assert L.pct_voxel_map_get_keys(vm._h, first, count, k.ctypes.data) == PCT_OK
        assert L.pct_voxel_map_get_f32(vm._h, first, count, a.ctypes.data, 3) == PCT_OK
        assert L.pct_voxel_map_get_f64(vm._h, first, count, b.ctypes.data) == PCT_OK
        assert L.pct_voxel_map_get_f32(vm._h, first, count, a4.ctypes.data, 4) == PCT_OK
        assert np.array_equal(k[:count], keys[first:first + count]) and np.all(k[count] == INDEX_SENTINEL)
        assert np.array_equal(a[:count].view(np.uint32), f32[first:first + count].view(np.uint32)) and np.all(a[count] == -7.5)
        assert np.array_equal(b[:count].view(np.uint64), f64[first:first + count].view(np.uint64)) and np.all(b[count] == -7.5)
        assert np.array_equal(a4[:count, :3].view(np.uint32), f32[first:first + count].view(np.uint32))
        assert np.all(a4[:, 3] == -7.5) and np.all(a4[count] == -7.5)  # the fourth float of every record is untouched
    vm.close()


def test_refused_calls_change_nothing(V):
    import torch
    L = V._lib()
    vm, model = V.VoxelMap(0.1), VM.VoxelModel(0.1)
    add_and_compare(V, vm, model, "host", VM.tie_points(np.float32), np.float32, 12)
    size = len(vm)
    out = np.full((size + 4, 4), -7.5)
    refused = [
        lambda: L.pct_voxel_map_get_keys(vm._h, size, 1, out.ctypes.data),
        lambda: L.pct_voxel_map_get_f32(vm._h, size, 1, out.ctypes.data, 3),
        lambda: L.pct_voxel_map_get_f64(vm._h, size, 1, out.ctypes.data),
        lambda: L.pct_voxel_map_get_keys(vm._h, -1, 1, out.ctypes.data),
        lambda: L.pct_voxel_map_get_f32(vm._h, -1, 1, out.ctypes.data, 3),
        lambda: L.pct_voxel_map_get_f64(vm._h, -1, 1, out.ctypes.data),
        lambda: L.pct_voxel_map_get_f32(vm._h, 0, size, out.ctypes.data, 2),
        lambda: L.pct_voxel_map_get_keys(None, 0, 1, out.ctypes.data),
        lambda: L.pct_voxel_map_get_f32(None, 0, 1, out.ctypes.data, 3),
        lambda: L.pct_voxel_map_get_f64(None, 0, 1, out.ctypes.data),
        lambda: L.pct_voxel_map_clear(None),
        lambda: L.pct_voxel_map_size(None, C.byref(C.c_int64())),
    ]
    p32, p64 = np.ones((4, 8), np.float32), np.ones((4, 8), np.float64)
    d32, d64 = torch.from_numpy(p32).cuda(), torch.from_numpy(p64).cuda()
    torch.cuda.synchronize()
    for name, a32, a64 in (("pct_voxel_map_add", p32.ctypes.data, p64.ctypes.data), ("pct_voxel_map_add_dev", d32.data_ptr(), d64.data_ptr())):
        f = getattr(L, name)
        refused += [
            lambda f=f, a=a32: f(vm._h, a, 4, 8, 0, None, None, None),        # a stride that holds no three floats
            lambda f=f, a=a32: f(vm._h, a, 4, 14, 0, None, None, None),       # ... that is no multiple of a float
            lambda f=f, a=a64: f(vm._h, a, 4, 20, 1, None, None, None),       # ... that holds no three doubles
            lambda f=f, a=a32: f(vm._h, a, -1, 12, 0, None, None, None),
            lambda f=f, a=a32: f(vm._h, None, 4, 12, 0, None, None, None),
            lambda f=f, a=a32: f(None, a, 4, 12, 0, None, None, None),
        ]
    for k, call in enumerate(refused):
        assert call() == PCT_ERR_INVALID, k
        assert len(vm) == size, k
    assert np.all(out == -7.5)
    compare_store(vm, model)                                           # nothing was changed by any of them
    vm.clear()
    model.clear()
    assert len(vm) == 0
    index = add_and_compare(V, vm, model, "dev", VM.tie_points(np.float32), np.float32, 16)
    assert index[0] == 0 and index.max() == len(model) - 1             # ids start from 0 again
    compare_store(vm, model)
    vm.close()
