"""Reference model of the batched Bezier check (pct_bezier_check_batch*) and the candidate set its tests share.

The model is a loop of bezier_model.model_check -- one trajectory at a time, exactly rounded Bernstein powers, exhaustive nearest
neighbour -- plus the two things the batch adds: the verdict fold (first radius < 0; the smallest radius, folded with `<` in ascending
sample order so that the lowest index wins a tie) and the offsets (prefix sums of the evaluated counts).

The candidate set: bezier_model.scene()'s `multi` cloud and `near` parameters, 54 candidates --
    0..48   the scene's trajectory with every control point translated by (0.2 i, -0.2 i, 0.2 j) m, i, j in -3..3 (i outer): the stored
            coefficients are control points divided by the segment time, so delta / T_s is added to those of segment s
    49      segment 12 alone (order 12)
    50      segment 0 alone (order 0)
    51      segments 3..8 with t_start = 0.17
    52      the whole trajectory with t_start = 5.05: no sample
    53      the whole trajectory with t_start = T[0]: on a boundary
Used by tests/test_bezier_batch_model.py (CPU) and tests/test_gpu_bezier_batch.py."""
import functools

import numpy as np

import bezier_model as M

STOP_TIME, DT = 100.0, 0.02
SHIFTS = [(0.2 * i, -0.2 * i, 0.2 * j) for i in range(-3, 4) for j in range(-3, 4)]
EMPTY, BOUNDARY = 52, 53


def shifted(coef, T, od, delta):
    """every control point of the trajectory translated by delta (metres)"""
    out = np.array(coef, np.float64)
    for s, n in enumerate(od):
        m = int(n) + 1
        for d in range(3):
            out[s, d * m:(d + 1) * m] += delta[d] / T[s]
    return out


@functools.lru_cache(maxsize=None)
def candidates():
    """list of (polycoef, seg_time, orders, t_start), read-only arrays"""
    coef, T, od = M.scene()["traj"]
    out = [(shifted(coef, T, od, d), T, od, 0.0) for d in SHIFTS]
    out.append((coef[12:13].copy(), T[12:13].copy(), od[12:13].copy(), 0.0))
    out.append((coef[0:1].copy(), T[0:1].copy(), od[0:1].copy(), 0.0))
    out.append((coef[3:9].copy(), T[3:9].copy(), od[3:9].copy(), 0.17))
    out.append((coef.copy(), T, od, 5.05))
    out.append((coef.copy(), T, od, float(T[0])))
    for c, t, o, _ in out:
        for a in (c, t, o):
            a.setflags(write=False)
    return out


def params():
    return M.scene()["params"]["near"]


def cloud():
    return M.scene()["clouds"]["multi"]


_one = {}


def model_one(k, stop_time=STOP_TIME, dt=DT, points=None, tag="multi"):
    """bezier_model.model_check of candidate k at cap 4096 (every smaller cap is a prefix of it), computed once per (k, stop_time, dt,
    cloud tag); `points` replaces the scene's cloud (give it a tag of its own)"""
    key = (k, float(stop_time), float(dt), tag)
    if key not in _one:
        c, t, o, ts = candidates()[k]
        _one[key] = M.model_check(cloud() if points is None else points, params(), c, t, o, ts, stop_time, dt, M.CAP_MAX)
    return _one[key]


def fold(radius):
    """(first_hit, min_sample, min_radius) of one row of radii"""
    first_hit, min_sample, min_radius = -1, -1, np.inf
    for k, r in enumerate(radius):
        r = float(r)
        if first_hit < 0 and r < 0.0:
            first_hit = k
        if min_sample < 0 or r < min_radius:
            min_sample, min_radius = k, r
    return first_hit, min_sample, min_radius


def model_batch(ks, cap=M.CAP_MAX, stop_time=STOP_TIME, dt=DT, points=None, tag="multi"):
    """The batch made of the candidates ks (indices into candidates(), repeats allowed).  Returns dict(nsamples, first_hit, min_sample,
    min_radius [B]; offsets [B + 1]; pos [total, 3], radius, d2 [total], idx [total] int64 with -1 = none)."""
    B = len(ks)
    ns, fh, ms = np.zeros(B, np.int64), np.zeros(B, np.int64), np.zeros(B, np.int64)
    mr = np.zeros(B, np.float64)
    offsets = np.zeros(B + 1, np.int64)
    rows = []
    folded = {}
    for b, k in enumerate(ks):
        one = model_one(k, stop_time, dt, points, tag)
        m = min(one["n"], int(cap), M.CAP_MAX)
        if k not in folded:
            folded[k] = fold(one["radius"][:m])
        ns[b] = one["n"]
        fh[b], ms[b], mr[b] = folded[k]
        offsets[b + 1] = offsets[b] + m
        rows.append((one, m))
    cat = lambda key, shape, dtype: (np.concatenate([o[key][:m] for o, m in rows]) if rows else np.zeros(shape, dtype))   # noqa: E731
    return dict(nsamples=ns, first_hit=fh, min_sample=ms, min_radius=mr, offsets=offsets, pos=cat("pos", (0, 3), np.float64).reshape(-1, 3),
                radius=cat("radius", 0, np.float64), d2=cat("d2", 0, np.float64), idx=cat("idx", 0, np.int64).astype(np.int64))


def ties_at_minimum(k, cap=M.CAP_MAX):
    """how many evaluated samples of candidate k attain its minimum radius"""
    one = model_one(k)
    r = one["radius"][:min(one["n"], cap)]
    return int((r == r.min()).sum()) if len(r) else 0
