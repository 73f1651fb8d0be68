"""CPU test: the launch-time choice of the dense NN batch kernel between 32-bit byte offsets from a scalar base and 64-bit addresses
(gridbuild.hpp narrow_offsets_fit, reached through pct_debug_narrow_offsets; no device is touched).  A byte offset wraps at 2^32, so the
narrow form serves at most 2^28 16-byte records (the cloud's points + its 16 spare ones) and sorted queries, and 2^30 4-byte run bounds."""
import pytest


@pytest.fixture(scope="module")
def narrow():
    from pointcloudtraj_amd import build, engine
    build.build_all()
    return engine.lib().pct_debug_narrow_offsets


def test_records_at_the_wrap(narrow):
    """n + kGridPad = 2^28 - 1 and 2^28 fit (the last record starts at byte 2^32 - 16), 2^28 + 1 does not"""
    cells, queries = 1000, 1 << 20
    assert narrow((1 << 28) - 1, cells, queries) == 1
    assert narrow(1 << 28, cells, queries) == 1
    assert narrow((1 << 28) + 1, cells, queries) == 0
    assert narrow(1 << 40, cells, queries) == 0


def test_run_bounds_and_batch_at_the_wrap(narrow):
    records = 10_000_016
    assert narrow(records, 1 << 30, 1) == 1 and narrow(records, (1 << 30) + 1, 1) == 0          # ncells + 1 entries of 4 bytes
    assert narrow(records, 1000, 1 << 28) == 1 and narrow(records, 1000, (1 << 28) + 1) == 0    # 16-byte sorted queries, 8-byte distances
    assert narrow(16, 2, 1) == 1                                                                 # a cloud without points


def test_negative_sizes_are_refused(narrow):
    assert narrow(-1, 1, 1) < 0 and narrow(1, -1, 1) < 0 and narrow(1, 1, -1) < 0
