"""De-duplicating appends on the rolling map as the interface states them (no GPU needed): the declared symbols, the Python methods,
the header's contract paragraph, and the reference model itself (tests/helpers/ring_dedup_model.py) holding the invariant."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import ring_dedup_model as M  # noqa: E402


def code_of(header):
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)


def test_engine_header_declares_both_symbols():
    code = code_of("pct_engine.h")
    assert re.search(r"int\s+pct_cloud_ring_dedup\s*\(\s*pct_cloud\s*\*\s*c\s*,\s*double\s+res\s*\)\s*;", code)
    m = re.search(r"int\s+pct_cloud_ring_dedup_last\s*\((.*?)\)\s*;", code, flags=re.S)
    assert m, "pct_cloud_ring_dedup_last is not declared"
    args = [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]
    assert args == ["pct_cloud *c", "int64_t *offered", "int64_t *kept", "uint8_t *flags", "int64_t cap", "uint64_t *total_offered",
                    "uint64_t *total_kept"]


def test_corridor_header_declares_its_symbol():
    assert re.search(r"int\s+pct_corridor_set_rolling_dedup\s*\(\s*pct_corridor\s*\*\s*c\s*,\s*double\s+res\s*\)\s*;", code_of("pct_corridor.h"))


def test_cxx_mirrors_have_the_setter():
    for h in ("pct_obstacle_map.hpp", "pct_corridor_finder.hpp"):
        assert re.search(r"void\s+setRollingDedup\s*\(\s*double\s+res\s*\)", open(os.path.join(ROOT, "include", h)).read()), h


def test_python_methods_exist():
    from pointcloudtraj_amd import corridor, engine
    assert callable(engine.Cloud.ring_dedup) and callable(engine.Cloud.ring_dedup_last)
    assert callable(corridor.SafeRegionRrtStar.setRollingDedup)


def test_contract_paragraph_names_the_invariant_and_the_host_wait():
    text = open(os.path.join(ROOT, "include", "pct_engine.h")).read()
    m = re.search(r"De-duplicating appends \(pct_cloud_ring_dedup\).*?\n \*\n", text, flags=re.S)
    assert m, "the contract paragraph is missing from the header comment"
    para = re.sub(r"\s*\n \*\s*", " ", m.group(0))
    assert "Invariant: after an append, the key of every keyed point of that frame is present in the window" in para
    assert "waits once on the host for the survivor count" in para
    assert "keyless" in para and "doomed" in para and "first occurrence wins" in para
    assert "no bound is promised" in para


@pytest.mark.parametrize("name,filed,zero_frames,largest", [("A", 6438, 15, 3866), ("B", 11774, 13, 5286)])
def test_model_holds_the_invariant(name, filed, zero_frames, largest):
    """0 sensed-but-missing keys after every frame of scenarios A and B; the figures the GPU test relies on"""
    frames = M.frames_of(name)
    w = M.DedupWindow(M.SCENARIOS[name]["cap"], M.RES)
    zero = 0
    for t, f in enumerate(frames):
        kept = w.append(f)
        zero += len(f) > 0 and not kept.any()
        assert not w.missing(f), f"scenario {name} frame {t}: keys of the frame are missing from the window"
    assert max(map(len, frames)) == largest <= w.cap
    assert (w.filed, zero) == (filed, zero_frames)
    if name == "B":
        assert w.filed > w.cap and any(len(f) == 0 for f in frames)         # the window wraps; the stream includes an empty frame


def test_model_keys_round_half_away_from_zero_and_keyless_points():
    import numpy as np
    keyed, k = M.keys_of(np.float32([[0.25, -0.25, 0.75], [np.nan, 0, 0], [0, np.inf, 0], [1e30, 0, 0], [0, 0, -1e30]]), 0.5)
    assert keyed.tolist() == [True, False, False, False, False]
    assert k[0].tolist() == [1, -1, 2]
    # a holder that the same append evicts does not suppress its replacement (the naive rule would drop it and lose the voxel)
    w = M.DedupWindow(4, 1.0)
    assert w.append(np.float32([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0]])).all()
    assert w.append(np.float32([[0, 0, 0], [3, 0, 0]])).tolist() == [True, False]      # slot 0 is doomed, slot 3 is not
    assert not w.missing(np.float32([[0, 0, 0], [3, 0, 0]]))
