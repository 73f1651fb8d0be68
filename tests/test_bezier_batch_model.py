"""CPU checks of tests/helpers/bezier_batch_model.py, the model tests/test_gpu_bezier_batch.py holds pct_bezier_check_batch* to: the
properties of the 54-candidate set that the GPU tests rely on -- colliding and free candidates, first hits on both sides of the small
caps, two free candidates whose minimum radius is attained by many samples (the lowest-index rule is observable), one candidate
without a sample, one nearest point per evaluated sample -- asserted as exact figures, so that a change of seed that loses one is
noticed."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import bezier_model as M  # noqa: E402
import bezier_batch_model as BM  # noqa: E402

ALL = list(range(54))


def test_candidate_set_shape():
    cands = BM.candidates()
    coef, T, od = M.scene()["traj"]
    assert len(cands) == 54 and len(BM.SHIFTS) == 49 and BM.SHIFTS[24] == (0.0, 0.0, 0.0)
    assert np.array_equal(cands[24][0], coef)                                   # the unshifted trajectory is among them
    c0, _, _, _ = cands[0]                                                      # i = j = -3: (-0.6, +0.6, -0.6) m on every control point
    for s in (0, 5, 12):
        m = int(od[s]) + 1
        for d, want in enumerate((-0.6, 0.6, -0.6)):
            assert np.allclose((c0[s, d * m:(d + 1) * m] - coef[s, d * m:(d + 1) * m]) * T[s], want, rtol=0, atol=1e-12)
        assert np.array_equal(c0[s, 3 * m:], coef[s, 3 * m:])                   # the padding stays
    assert [len(c[1]) for c in cands[49:]] == [1, 1, 6, 13, 13] and [int(c[2][0]) for c in cands[49:52]] == [12, 0, 3]
    assert [c[3] for c in cands[49:]] == [0.0, 0.0, 0.17, 5.05, float(T[0])]


def test_scene_properties():
    r = BM.model_batch(ALL)
    colliding = r["first_hit"] >= 0
    print("colliding", int(colliding.sum()), "total", int(r["offsets"][-1]), "first hits", sorted(r["first_hit"][colliding].tolist()))
    assert int(colliding.sum()) == 38 and int((~colliding).sum()) == 16
    assert int(r["offsets"][-1]) == 12885 and np.array_equal(np.diff(r["offsets"]), np.minimum(r["nsamples"], M.CAP_MAX))
    assert r["nsamples"][:49].tolist() == [255] * 49 and r["nsamples"][49:].tolist() == [20, 15, 115, 0, 240]
    assert int(r["first_hit"][colliding].min()) == 5 and int(r["first_hit"][colliding].max()) == 211
    # the empty candidate
    assert r["nsamples"][BM.EMPTY] == 0 and r["first_hit"][BM.EMPTY] == -1 and r["min_sample"][BM.EMPTY] == -1 and np.isposinf(r["min_radius"][BM.EMPTY])
    assert int((r["nsamples"] == 0).sum()) == 1
    # the two free candidates whose minimum is attained by many samples: the lowest of them is reported
    tied = {k: BM.ties_at_minimum(k) for k in ALL if not colliding[k] and BM.ties_at_minimum(k) > 1}
    assert tied == {49: 18, 50: 15}
    for k in tied:
        rad = BM.model_one(k)["radius"]
        assert r["min_sample"][k] == int(np.nonzero(rad == rad.min())[0][0]) and r["min_radius"][k] == rad.min()
        assert int(np.nonzero(rad == rad.min())[0][-1]) > r["min_sample"][k]
    # every other verdict against numpy
    for k in ALL:
        rad = BM.model_one(k)["radius"]
        if len(rad):
            assert r["min_radius"][k] == rad.min() and r["min_sample"][k] == int(np.argmin(rad))
            assert r["first_hit"][k] == BM.model_one(k)["first_hit"]


def test_small_caps_hide_later_hits():
    full, c64, c20 = BM.model_batch(ALL), BM.model_batch(ALL, cap=64), BM.model_batch(ALL, cap=20)
    assert np.array_equal(c20["nsamples"], full["nsamples"]) and np.array_equal(c64["nsamples"], full["nsamples"])      # unclipped
    assert int(c64["offsets"][-1]) == int(np.minimum(full["nsamples"], 64).sum()) and int(c20["offsets"][-1]) == int(np.minimum(full["nsamples"], 20).sum())
    for capped, cap in ((c64, 64), (c20, 20)):
        want = np.where((full["first_hit"] >= 0) & (full["first_hit"] < cap), full["first_hit"], -1)
        assert np.array_equal(capped["first_hit"], want)
    assert int((c20["first_hit"] >= 0).sum()) == 2 and int((c64["first_hit"] >= 0).sum()) == 11      # hits beyond the cap are not reported


def test_every_evaluated_sample_has_one_nearest_point():
    for k in ALL:
        M.assert_unique_nearest(BM.cloud(), BM.model_one(k))


def test_short_stop_times():
    two = BM.model_batch(ALL, stop_time=0.05)
    assert two["nsamples"].tolist() == [2] * 52 + [0, 2]
    ragged = BM.model_batch(ALL, stop_time=0.3)
    assert ragged["nsamples"].tolist() == [15] * 52 + [0, 15]                    # the segment-0-alone candidate ends with its segment
