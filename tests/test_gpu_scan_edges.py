"""GPU tests of the block scan (csrc/scan.hpp) through every feature that ranks, offsets or compacts with it, at the sizes where the
shared code changes branch: a tile's last element (n = 1023 / 1024 / 1025; 2047 / 2048 / 2049 for the radius search's 2048-count
tiles) and the second round of the one-block carry loop (257 tiles).

References: numpy, and the models the neighbouring tests use (tests/helpers/ring_dedup_model.py, tests/helpers/depth_model.py,
numpy_voxels of tests/test_voxel.py, sq_dists of tests/test_gpu_knn.py).  Every comparison is exact: integers and bit patterns."""
import os
import re
import sys

import numpy as np
import pytest

from test_gpu_knn import sq_dists
from test_voxel import numpy_voxels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import depth_model as D  # noqa: E402
import ring_dedup_model as M  # noqa: E402

pytestmark = pytest.mark.gpu

TILE = 1024
SIZES = [1023, 1024, 1025, 256 * TILE + 1]            # the last one: 257 tiles, the carry loop's second round holds one tile


@pytest.fixture(scope="module")
def E():
    from pointcloudtraj_amd import engine
    engine.init(0)
    return engine


# ---- lidar crop (crop_count_kernel, scan_tile_sums_kernel, crop_scatter_kernel) ------------------------------------------------------

def crop_cloud(n):
    """every third point on the x axis within 1 m of the origin, the others on a parallel line 100 m away"""
    i = np.arange(n)
    pts = np.zeros((n, 3), np.float32)
    pts[:, 0] = (i % 1000) * np.float32(0.001)
    pts[:, 1] = np.where(i % 3 == 0, 0.0, 100.0)
    return pts


BALLS = {"all": ((0.0, 50.0, 0.0), 1000.0), "none": ((0.0, 0.0, 500.0), 1.0), "third": ((0.0, 0.0, 0.0), 2.0)}


@pytest.mark.parametrize("n", SIZES)
def test_crop_keeps_insertion_order_across_tile_edges(E, n):
    pts = crop_cloud(n)
    pts64 = pts.astype(np.float64)
    with E.Cloud(n) as c:
        c.set_input(pts)
        assert not c.has_grid
        for name, (centre, r) in BALLS.items():
            d2 = sq_dists(pts64, centre)
            want = np.flatnonzero(d2 <= np.float64(r) * np.float64(r))
            assert np.array_equal(want, {"all": np.arange(n), "none": np.arange(0), "third": np.arange(0, n, 3)}[name]), name
            idx, gd2, xyz = c.radius_crop(centre, r)
            assert np.array_equal(idx.astype(np.int64), want), f"n {n}, ball {name}: indices"
            assert np.array_equal(gd2, d2[want]), f"n {n}, ball {name}: squared distances"
            assert np.array_equal(xyz.view(np.uint32), pts[want].view(np.uint32)), f"n {n}, ball {name}: rows"


# ---- de-duplicating append (dd_rank_kernel, scan_tile_sums_kernel + DdPublish, dd_compact_kernel) ------------------------------------

DD_RES = 0.25


def dedup_frame(n):
    """odd positions repeat the point before them, except a tile's last position: kept points on both sides of every tile edge"""
    i = np.arange(n)
    fresh = (i % 2 == 0) | (i % TILE == TILE - 1)
    v = np.cumsum(fresh) - 1                              # the voxel of position i: a new one at every fresh position
    pts = np.stack([v % 80, (v // 80) % 80, v // 6400], axis=1).astype(np.float32) * np.float32(DD_RES)
    return pts, fresh


@pytest.mark.parametrize("n", SIZES)
def test_dedup_append_of_one_frame_into_an_empty_window(E, n):
    frame, fresh = dedup_frame(n)
    w = M.DedupWindow(n, DD_RES)
    want = w.append(frame)
    assert np.array_equal(want, fresh) and want[TILE - 2] and (n <= TILE or (want[TILE - 1] and want[TILE]))
    with E.Cloud(n) as c:
        c.ring_index(0.5, (20.0, 20.0, 12.0))
        c.ring_dedup(DD_RES)
        c.append(frame)
        last = c.ring_dedup_last()
        assert (last["offered"], last["kept"]) == (n, int(want.sum())), last
        assert np.array_equal(last["flags"], want)
        assert len(c) == w.count
        _, _, xyz = c.radius_crop((0.0, 0.0, 0.0), 1.0e4)     # the whole window, slot by slot
        assert np.array_equal(xyz.view(np.uint32), w.live().view(np.uint32))


# ---- depth append (depth_valid_kernel, dd_rank_kernel, scan_tile_sums_kernel + DdPublish, depth_unproject_kernel) --------------------

def test_depth_append_of_257_tiles(E):
    w, h = 513, 512
    assert -(-w * h // TILE) == 257
    p = np.arange(w * h)
    valid = (p % 2 == 0) | (p % TILE == TILE - 1)         # a checkerboard, plus a tile's last pixel: valid on both sides of every edge
    img = np.where(valid, 2.0 + (p % 977) * (8.0 / 1024.0), np.inf).astype(np.float32).reshape(h, w)
    view = E.depth_view((0.0, 0.0, 0.0), np.eye(3), w, h, fov_hor_deg=90.0)
    got_valid, frame = D.unproject(view, img)
    assert np.array_equal(got_valid, valid) and len(frame) == int(valid.sum())
    with E.Cloud(len(frame)) as c:
        c.ring_index()                                    # sized by the first data: the image itself
        offered, kept = c.append_depth(view, img)
        assert (offered, kept) == (len(frame), len(frame)) and len(c) == len(frame)
        _, _, xyz = c.radius_crop((0.0, 0.0, 0.0), 1.0e4)
        assert np.array_equal(xyz.view(np.uint32), frame.view(np.uint32))


# ---- voxel map (vox_rank_kernel, scan_tile_sums_kernel + VoxTotal, vox_commit_kernel) ------------------------------------------------

def test_voxel_batch_of_257_tiles(E):
    from pointcloudtraj_amd import voxel
    n, res = 256 * TILE + 1, 0.25
    i = np.arange(n)
    v = 3 * (i // 6) + i % 3                              # groups a b c a b c: every voxel twice, the firsts drift across the tile edges
    pts = np.stack([v % 64, (v // 64) % 64, v // 4096], axis=1).astype(np.float32) * np.float32(res)
    keys, want_index, want_new = numpy_voxels(pts, res)
    edges = np.arange(TILE, n, TILE)
    assert (want_new[edges - 1] & want_new[edges]).any() and (~want_new[edges - 1] & want_new[edges]).any()
    vm = voxel.VoxelMap(res)
    n_new, is_new, index = vm.add_points(pts)
    assert n_new == len(keys) == len(vm)
    assert np.array_equal(is_new, want_new) and np.array_equal(index, want_index)
    assert np.array_equal(vm.keys(), keys)                # ids in first-seen order
    assert np.array_equal(vm.get_voxel_cloud(np.float32), (keys * res).astype(np.float32))
    vm.close()


# ---- radius search with lists (rs_scan_tiles_kernel, scan_tile_sums_kernel<uint64_t>, rs_scan_final_kernel) --------------------------

RS_TILE = 2048
RS_SIZES = [2047, 2048, 2049, 256 * RS_TILE + 1]


@pytest.fixture(scope="module")
def rs_case():
    """64 points on a unit lattice; 256 * 2048 + 1 queries: most far away (empty rows), one in 61 and both sides of every tile edge on a
    lattice point with a small radius (1 entry), one in 4099 at the centre with a large one (all 64, many ties).  The reference of the
    largest batch, computed once and left unchanged; a smaller batch is its prefix."""
    a = np.arange(4, dtype=np.float32)
    pts = np.stack(np.meshgrid(a, a, a, indexing="ij"), axis=-1).reshape(-1, 3)
    Q = RS_SIZES[-1]
    i = np.arange(Q)
    q = np.empty((Q, 3), np.float32)
    q[:] = np.stack([100.0 + i % 7, np.full(Q, 50.0), np.full(Q, 50.0)], axis=1)
    r = np.full(Q, 0.5, np.float32)
    one = (i % 61 == 0) | (i % RS_TILE == 0) | (i % RS_TILE == RS_TILE - 1)
    q[one] = pts[i[one] % 64] + np.float32(0.125)
    r[one] = 0.25
    full = i % 4099 == 1
    q[full] = np.float32([1.5, 1.5, 1.5])
    r[full] = 100.0
    pts64 = pts.astype(np.float64)
    d2 = np.empty((Q, 64))
    for k in range(64):                                   # sq_dists per point: the contract's operation order, vectorised over the queries
        d2[:, k] = sq_dists(q.astype(np.float64), pts[k])
    hit = d2 <= (r.astype(np.float64) * r.astype(np.float64))[:, None]
    counts = hit.sum(axis=1)
    assert (counts == 0).mean() > 0.9 and (counts == 1).sum() > 8000 and (counts == 64).sum() == 128 and set(np.unique(counts)) == {0, 1, 64}
    assert counts[RS_TILE - 1] == counts[RS_TILE] == counts[Q - 1] == 1
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    rows, ids = np.nonzero(hit)                           # row-major: ascending index inside a row
    by_index = (ids.astype(np.uint32), d2[rows, ids])
    ids_d = ids.copy()
    for t in np.flatnonzero(counts > 1):                  # nearest first, equal d2 in ascending index
        s = slice(offsets[t], offsets[t + 1])
        ids_d[s] = ids[s][np.lexsort((ids[s], d2[t, ids[s]]))]
    by_dist = (ids_d.astype(np.uint32), d2[rows, ids_d])
    return dict(pts=pts, q=q, r=r, offsets=offsets, rows=[by_index, by_dist])


def rs_cloud(E, path, pts):
    c = E.Cloud(len(pts))
    if path == "ring":
        c.ring_index(1.0, (4.0, 4.0, 4.0))
        c.append(pts)
        assert c.has_ring_index
        return c, E.ALGO_AUTO
    c.set_input(pts)
    if path == "grid":
        c.build_grid()
        return c, E.ALGO_GRID
    return c, E.ALGO_STREAM


@pytest.mark.parametrize("order", [0, 1], ids=["by_index", "by_distance"])
@pytest.mark.parametrize("path", ["grid", "stream", "ring"])
def test_radius_search_offsets_across_tile_edges(E, rs_case, path, order):
    c, algo = rs_cloud(E, path, rs_case["pts"])
    want_idx, want_d2 = rs_case["rows"][order]
    for Q in RS_SIZES:
        offsets, idx, d2 = c.radius_search(rs_case["q"][:Q], rs_case["r"][:Q], order, algo)
        total = rs_case["offsets"][Q]
        assert offsets.dtype == np.int64 and np.array_equal(offsets, rs_case["offsets"][:Q + 1]), f"{path}, Q {Q}: offsets"
        assert np.array_equal(idx, want_idx[:total]), f"{path}, Q {Q}: indices"
        assert np.array_equal(d2, want_d2[:total]), f"{path}, Q {Q}: squared distances"
    c.close()


# ---- index build through the per-point-atomic path (scan_tiles_kernel, scan_tile_sums_kernel, scan_add_kernel) -----------------------

def test_index_build_with_more_than_256_tiles_of_cells(E):
    """65^3 = 274 625 cells of 0.5 m (269 tiles) under 3000 points: sort_into_cells takes the two-level LDS sort only from 4096
    points on, so this cloud goes through cell_histogram / scan_tiles / scan_tile_sums / scan_add / cell_scatter"""
    src = open(os.path.join(ROOT, "pointcloudtraj_amd", "csrc", "engine.hip")).read()
    m = re.search(r"\bn\s*>=\s*(\d+)\s*&&[^\n]*kGbMaxSlabCells", src)
    assert m, "sort_into_cells no longer selects its path this way: restate the condition here"
    rng = np.random.default_rng(77)
    n = 3000
    assert n < int(m.group(1))                            # the per-point-atomic path is taken
    pts = (rng.integers(0, 129, (n, 3)) * 0.25).astype(np.float32)     # multiples of 0.25 in [0, 32]: fp32 cell assignment is exact
    pts[0], pts[1] = (0.0, 0.0, 0.0), (32.0, 32.0, 32.0)
    with E.Cloud(n) as c:
        c.set_input(pts)
        c.build_grid(0.5)
        info = c.grid_info()
        assert info["dims"] == (65, 65, 65) and info["ncells"] == 65 ** 3 > 256 * TILE and info["cell_size"] == 0.5
        v = c.verify_grid()
        assert v == dict(bad_ids=0, duplicates=0, misplaced=0, decreasing=0, first=0, last=n), v
        cell_start, rec = c.debug_read_grid()
        cell = np.floor(pts.astype(np.float64) * 2.0).astype(np.int64)
        lin = cell[:, 0] + 65 * (cell[:, 1] + 65 * cell[:, 2])         # x fastest, then y, then z
        want = np.concatenate([[0], np.cumsum(np.bincount(lin, minlength=65 ** 3))])
        assert cell_start[-1] == n and np.array_equal(cell_start.astype(np.int64), want)
        ids = rec[:, 3].copy().view(np.uint32)
        assert np.array_equal(np.sort(ids), np.arange(n, dtype=np.uint32)) and np.array_equal(lin[ids], np.sort(lin))
