"""CPU checks of tests/helpers/voxel_exact_model.py, the model tests/test_gpu_voxel_edges.py holds voxel.hip to: against the
oracle's sequential restatement (oracle/voxel_port.c: C's round(), a true division) on in-range inputs -- the tables of ties and
near-ties, the last voxels inside the key range and ordinary clouds -- and its rounding and its hash against values worked by hand."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import voxel_exact_model as VM  # noqa: E402
from oracle import oracle as O  # noqa: E402
from pointcloudtraj_amd import synth  # noqa: E402

RES = (0.1, 0.25, 1.0 / 3.0)


def in_range_tables():
    rng = np.random.default_rng(12)
    out = {}
    for dt in (np.float32, np.float64):
        for res in RES:
            out[f"ties_{dt.__name__}_{res:.3g}"] = (VM.tie_points(dt), res)
        for res in (0.1, 1.0):
            v = VM.range_values(res, dt)
            r = VM.round_half_away(VM.quotient(v, res))
            out[f"range_{dt.__name__}_{res:.3g}"] = (VM.on_each_axis(v[(r >= -VM.LIM) & (r < VM.LIM)], dt), res)
    out["uniform_f32"] = (synth.uniform_points(31, 5000, -8, 8), 0.25)
    out["normal_f64"] = (rng.normal(0, 3, (5000, 3)), 0.2)
    out["negative_f32"] = (-synth.uniform_points(33, 3000, 0, 4), 0.05)
    return out


TABLES = in_range_tables()


def test_round_half_away_at_the_doubles_where_adding_a_half_goes_wrong():
    below_half = np.nextafter(0.5, 0.0)
    assert below_half == 0.49999999999999994 and np.float64(0.049999999999999996) / 0.1 == below_half
    assert np.floor(below_half + 0.5) == 1.0                          # what floor(v + 0.5) answers
    q = np.float64([below_half, -below_half, 0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 0.0, -0.0, 2.0 ** 52 + 1, -(2.0 ** 52 + 1), 2.0 ** 53, 4503599627370495.5])
    want = np.float64([0, -0, 1, -1, 2, -2, 3, -3, 0, -0, 2.0 ** 52 + 1, -(2.0 ** 52 + 1), 2.0 ** 53, 4503599627370496.0])
    assert np.array_equal(VM.round_half_away(q), want)
    r = VM.round_half_away(np.float64([np.nan, np.inf, -np.inf]))
    assert np.isnan(r[0]) and r[1] == np.inf and r[2] == -np.inf
    # a division is not a multiplication by the reciprocal: 0.15 / 0.1 is below the tie, 0.15 * 10 on it
    assert np.float64(0.15) / 0.1 == 1.4999999999999998 and np.float64(0.15) * (1.0 / 0.1) == 1.5
    assert VM.round_half_away(np.float64(0.15) / 0.1) == 1.0 and VM.round_half_away(np.float64(0.15) * (1.0 / 0.1)) == 2.0


def test_tie_table_holds_the_named_coordinates_and_separates_the_rounding_rules():
    v = VM.tie_values(np.float64)
    for x in (0.15, 0.25, 0.35, 0.45, 0.049999999999999996, np.nextafter(0.15, 1.0), np.nextafter(0.15, 0.0), -0.15, 2.0):
        assert x in v
    assert np.any((v == 0.0) & np.signbit(v))
    q = VM.quotient(v, 0.1)
    r = VM.round_half_away(q)
    assert np.any(r != np.rint(q))                                    # half-to-even differs on the table
    assert np.any(r != VM.round_half_away(v * (1.0 / 0.1)))           # so does the reciprocal
    assert np.any(r != np.where(q >= 0, np.floor(q + 0.5), np.ceil(q - 0.5)))    # and floor(q + 0.5)
    assert np.any(np.abs(q - np.trunc(q)) == 0.5)                     # exact ties are there
    v32 = VM.tie_values(np.float32)
    assert v32.dtype == np.float32 and np.float32(0.15) in v32


def test_hash_restates_the_finaliser():
    # murmur3's fmix64 of 1 (a published value of the finaliser) and the packing of the extreme keys
    assert int(VM.vox_hash(np.uint64([1]))[0]) == 0xb456bcfc34c2cb2c & 0xFFFFFFFF
    k = np.int64([[0, 0, 0], [-VM.LIM, -VM.LIM, -VM.LIM], [VM.LIM - 1, VM.LIM - 1, VM.LIM - 1], [1, -1, 2]])
    want = [(1 << 20) | (1 << 41) | (1 << 62), 0, (1 << 63) - 1, ((1 << 20) + 1) | (((1 << 20) - 1) << 21) | (((1 << 20) + 2) << 42)]
    assert VM.vox_pack(k).tolist() == want
    c = VM.colliding_voxels()
    assert c.shape == (300, 3) and len(np.unique(c, axis=0)) == 300
    assert np.all(VM.vox_hash(VM.vox_pack(c)) & np.uint32(0xFFFF) == 0xFFFF)
    for T in (1024, 4096, 65536):                                     # one home slot, the last, in every table up to 2^16 slots
        assert np.all(VM.vox_hash(VM.vox_pack(c)) & np.uint32(T - 1) == T - 1)


@pytest.mark.parametrize("name", list(TABLES))
def test_model_equals_the_sequential_oracle_on_in_range_input(name):
    O.build()
    pts, res = TABLES[name]
    om, mm = O.PortVoxelMap(res), VM.VoxelModel(res)
    for batch in (pts, pts[::-1], pts[: len(pts) // 3]):
        batch = np.ascontiguousarray(batch)
        n_new, is_new, index, ok = mm.add(batch)
        want_new, want_is_new, want_index = om.add(batch)
        assert ok.all()
        assert n_new == want_new and np.array_equal(is_new, want_is_new) and np.array_equal(index, want_index)
    assert len(mm) == len(om) and np.array_equal(mm.keys(), om.keys())
    assert np.array_equal(mm.cloud_f64().view(np.uint64), om.cloud_f64().view(np.uint64))
    assert np.array_equal(mm.cloud_f32().view(np.uint32), om.cloud_f32().view(np.uint32))


def test_model_skips_what_lies_outside_the_key_range():
    for dt in (np.float32, np.float64):
        for res in (0.1, 1.0):
            v = VM.range_values(res, dt)
            r, ok = VM.coords(VM.on_each_axis(v, dt), res)
            assert ok.any() and (~ok).any()
            assert np.array_equal(ok, np.all((r >= -VM.LIM) & (r <= VM.LIM - 1), axis=1))
        pts = VM.on_each_axis(VM.wild_values(dt), dt)
        m = VM.VoxelModel(0.1)
        n_new, is_new, index, ok = m.add(pts)
        assert n_new == 0 and not ok.any() and not is_new.any() and np.all(index == -1) and len(m) == 0
