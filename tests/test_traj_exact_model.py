"""CPU checks of tests/helpers/traj_exact_model.py, the model tests/test_gpu_traj_exact.py holds traj.hip to bit for bit.  The model
is held to two things it shares no code with:

(a) the oracle port (oracle/traj_port.c: glibc pow, compiled C): equal bit for bit on every sample where libm's pow returned the
    correctly rounded value for every power the sample takes.  The share of samples this leaves out is printed and capped at 5 %.
(b) the same sums evaluated entirely in rational arithmetic and rounded once: the model is within
    (2 * m + 4) * 2^-53 * sum_j |term_j| of it, m = the number of terms of the sum and |term_j| the magnitude of the exact term
    (derived at rational_bound below, not measured).  One departure, for the acceleration sums only: the inner subtraction of
    (c[j+2] - 2 c[j+1]) + c[j] rounds relative to itself, which under cancellation no multiple of |term_j| bounds, so one more
    2^-53 * sum_j |w_j (c[j+2] - 2 c[j+1])| is allowed there."""
import os
import sys
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import traj_exact_model as M  # noqa: E402
from oracle import oracle as O  # noqa: E402

TRAJ = M.trajectories()
LIBM_SHARE_CAP = 0.05


def wire_of(pc, times, orders):
    O.build()
    cx, cy, cz = O.traj_wire_from_matrix(pc, orders)
    return SimpleNamespace(coef_x=cx, coef_y=cy, coef_z=cz, time=np.asarray(times, np.float64), order=np.asarray(orders, np.uint32))


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------ (a) the oracle port
def test_recorded_libm_misses_are_exact_powers_of_the_grid():
    """LIBM_MISS_U are values i / 1000; the GPU test evaluates at them whatever this machine's libm does with them"""
    for u in M.LIBM_MISS_U:
        assert u in [i / 1000.0 for i in range(1001)]
    misses = M.scan_libm_misses()
    print(f"libm pow misses the correct rounding on {len(misses)} of {2 * 1001 * 13} powers x^k, x in {{i/1000, 1 - i/1000}}, k <= 12")
    assert len(misses) <= 0.01 * 2 * 1001 * 13


@pytest.mark.parametrize("name", list(TRAJ))
def test_state_equals_the_oracle_port_where_libm_is_correctly_rounded(name):
    O.build()
    pc, times, orders = TRAJ[name]
    grid = np.float64(sorted(set([i / 1000.0 for i in range(0, 1001, 4)] + list(M.LIBM_MISS_U) + [-0.25, 1.25, 1.0 / 3.0, 2.0 ** -30])))
    seg = np.repeat(np.arange(len(orders)), len(grid)).astype(np.int32)
    u = np.tile(grid, len(orders))
    got, ok = M.state(pc, orders, seg, u)
    want = O.traj_state(pc, orders, seg, u)
    left_out = 1.0 - ok.mean()
    print(f"{name}: libm flag leaves out {100 * left_out:.2f} % of {len(ok)} state samples")
    assert left_out <= LIBM_SHARE_CAP
    assert np.array_equal(bits(got[ok]), bits(want[ok]))
    assert np.allclose(got, want, rtol=1e-13, atol=1e-13 * np.abs(want).max())         # the others: a last-bit matter, nothing more


@pytest.mark.parametrize("name,samples", [("orders_1_to_12", 1001), ("orders_4_to_11", 101), ("single", 257), ("gap", 11), ("gap", 2),
                                          ("hover_then_move", 3)])
def test_wire_samples_equal_the_oracle_port_where_libm_is_correctly_rounded(name, samples):
    w = wire_of(*TRAJ[name])
    pos, step, ok = M.wire_sample(w, samples)
    opos, ostep = O.traj_wire_sample(w, samples)
    left_out = 1.0 - ok.mean()
    print(f"{name} x {samples}: libm flag leaves out {100 * left_out:.2f} % of {len(ok)} wire samples")
    assert left_out <= LIBM_SHARE_CAP
    assert np.array_equal(bits(pos[ok]), bits(opos[ok]))
    prev_ok = ok & np.concatenate([[True], ok[:-1]])                  # a step needs its predecessor's position too
    assert np.array_equal(bits(step[prev_ok]), bits(ostep[prev_ok]))
    assert step[0] == 0.0 and np.all(step >= 0)


def test_walks_equal_the_oracle_port_on_its_own_steps():
    """the two walks, fed the ORACLE's step lengths, answer as the oracle's own sequential loops do (their logic is independent of
    the evaluator): at round fractions, at the total, at both signs of zero, below zero and at infinity"""
    for name, tr in TRAJ.items():
        w = wire_of(*tr)
        ostep = O.traj_wire_sample(w, 1001)[1].tolist()
        total = float(np.sum(ostep))
        for L in (0.0, -0.0, -1.0, 1e-9, 0.05 * total, 0.31 * total, 0.5 * total, 0.77 * total, total, 10 * total, np.inf):
            assert M.segm_index(ostep, len(w.time), L) == O.traj_segm_index(w, L), (name, L)
            assert M.points_used(ostep, L) == O.traj_nearest_traj(w, 0.1, L)[1], (name, L)


def test_hover_trajectory_makes_the_strict_comparison_visible():
    """every step of the hover segment is exactly 0.0, so with twirl_len = 0 `len` is exactly 0 throughout it: `len < 0` first holds
    in segment 1 -- `len <= 0` would answer (0, 0) -- and `len >= 0` takes all of segment 0 and two samples more"""
    w = wire_of(*TRAJ["hover_then_move"])
    _, step, _ = M.wire_sample(w, 1001)
    assert np.all(step[:1002] == 0.0) and step[1002] > 0.0
    for zero in (0.0, -0.0):
        assert M.segm_index(step, 2, zero) == (1, 0)
        assert M.points_used(step, zero) == 1003


def test_adjacent_change_finds_neighbouring_doubles():
    step = M.wire_sample(wire_of(*TRAJ["single"]), 1001)[1].tolist()
    total = sum(step)
    a, b = M.adjacent_change(lambda L: M.segm_index(step, 1, L), 0.0, total)
    assert np.nextafter(a, np.inf) == b and M.segm_index(step, 1, a) == (0, 0) and M.segm_index(step, 1, b) == (0, 1)
    assert abs(a - sum(step[:501])) < 1e-12                           # the half boundary: t = 0.501 is the first t > 0.5


# ------------------------------------------------------------------------------------------------ (b) rational arithmetic
def rational_bound(m, mag, inner=0):
    """|model - round(exact sum)| <= (2 m + 4) * 2^-53 * sum_j |term_j|  [+ (1 + 2^-40) * 2^-53 * inner, acceleration only],
    m = number of terms, u = 2^-53, no underflow; |term_j| is the magnitude of the exact term, differences of control points included.

    Every float operation contributes one factor (1 + d), |d| <= u, to the terms it touches.  Per term, at the most:
        position       C * c (1), u^j and (1 - u)^(n - j) each rounded once (2), the two products by them (2)                     5
        velocity       c[j+1] - c[j] (1: fl(a - b) = (a - b)(1 + d), relative to the difference itself), (C * n) * dc (1; C * n is
                       an exact integer), powers and their products (4)                                                            6
        acceleration   the outer addition of (c[j+2] - 2 c[j+1]) + c[j] (1; 2 * c and (C * n) * (n - 1) are exact), the product
                       by it (1), powers and their products (4)                                                                    6
        wire sample    T * c (1), * C (1), powers and their products (4)                                                           6
    The sum adds m terms to 0.0: the first addition is exact, each of the m - 1 others puts one more factor on every term before
    it; rounding the exact sum once adds one u of |sum| <= sum |term|.  To first order that is (m - 1) + k + 1 = m + k units:
    m + 6 at worst, which is <= 2 m + 3 for m >= 3.  For m <= 2 every exponent is 0 or 1, so the powers are exact and a product
    by 1.0 is too, which leaves at most 4 roundings per term and m + 4 <= 2 m + 3 for m >= 1.  The second-order part of
    (1 + u)^(2 m + 3) - 1 is below (2 m + 3)^2 u^2 < u, which the one unit up to 2 m + 4 covers.

    THE ONE DEPARTURE from (2 m + 4) u sum |term_j|, for the acceleration sums alone: the INNER subtraction c[j+2] - 2 c[j+1]
    rounds relative to itself, not to the term -- fl(ddc) = ddc (1 + d2) + (c[j+2] - 2 c[j+1]) d1 (1 + d2) -- so under cancellation
    no multiple of u |term_j| bounds it.  Its share is carried apart: at most u * sum_j |w_j (c[j+2] - 2 c[j+1])| = u * inner,
    times the later factors of its term, (1 + u)^(2 m + 4) < 1 + 2^-40.  Nothing else is added to the bound as stated."""
    return (2 * m + 4) * Fraction(1, 2 ** 53) * mag + (1 + Fraction(1, 2 ** 40)) * Fraction(1, 2 ** 53) * inner


RATIONAL_U = (0.0, 1.0, 0.5, 1.0 / 3.0, 0.001, 0.999, 0.1, 0.77, -0.25, 1.25, M.LIBM_MISS_U[0], (2.0 ** 27 - 1) * 2.0 ** -27, 2.0 ** -30)


@pytest.mark.parametrize("name", list(TRAJ))
def test_state_is_within_the_derived_bound_of_rational_arithmetic(name):
    pc, times, orders = TRAJ[name]
    for s, n in enumerate(int(v) for v in orders):
        terms = (n + 1,) * 3 + (n,) * 3 + (n - 1,) * 3
        for u in RATIONAL_U:
            got, _ = M.state_one(pc[s], n, u)
            sums, mags, inner = M.state_rational(pc[s], n, u)
            assert not any(inner[:6])                                 # the carried share exists for the acceleration alone
            for k in range(9):
                assert abs(Fraction(got[k]) - Fraction(float(sums[k]))) <= rational_bound(terms[k], mags[k], inner[k]), (name, s, u, k)
                if terms[k] == 0:
                    assert got[k] == 0.0 and sums[k] == 0


@pytest.mark.parametrize("name", list(TRAJ))
def test_wire_samples_are_within_the_derived_bound_of_rational_arithmetic(name):
    w = wire_of(*TRAJ[name])
    samples = 11
    pos, _, _ = M.wire_sample(w, samples)
    for s in range(len(w.time)):
        for i in range(samples):
            sums, mags = M.wire_rational(w, s, i, samples)
            for d in range(3):
                got = pos[s * samples + i, d]
                assert abs(Fraction(float(got)) - Fraction(float(sums[d]))) <= rational_bound(int(w.order[s]) + 1, mags[d]), (name, s, i, d)
