"""The rolling-map search path as the interface states it (no GPU needed): the enum value, the Python constant and the header's
contract paragraphs."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pct_engine.h")


def strip_comments(text):
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def paragraph(text, start):
    m = re.search(re.escape(start) + r".*?\n \*\n", text, flags=re.S)
    assert m, f"the paragraph starting '{start}' is missing from the header comment"
    return re.sub(r"\s*\n \*\s*", " ", m.group(0))


def test_header_enum_has_algo_ring():
    code = strip_comments(open(HEADER).read())
    m = re.search(r"enum\s+pct_algo\s*\{(.*?)\}", code, flags=re.S)
    assert m, "enum pct_algo is missing"
    values = dict(re.findall(r"(PCT_ALGO_\w+)\s*=\s*(\d+)", m.group(1)))
    assert values == {"PCT_ALGO_AUTO": "0", "PCT_ALGO_STREAM": "1", "PCT_ALGO_GRID": "2", "PCT_ALGO_STREAM_EXACT": "3", "PCT_ALGO_RING": "4"}


def test_python_constant():
    from pointcloudtraj_amd import engine
    assert engine.ALGO_RING == 4
    assert (engine.ALGO_AUTO, engine.ALGO_STREAM, engine.ALGO_GRID, engine.ALGO_STREAM_EXACT) == (0, 1, 2, 3)


def test_header_names_the_ring_path_in_the_knn_and_radius_search_paragraphs():
    text = open(HEADER).read()
    for start in ("k nearest neighbours (pct_knn_batch*", "Radius search with lists (pct_radius_search_batch*"):
        para = paragraph(text, start)
        assert "PCT_ALGO_RING" in para and "rolling-map index" in para, start
    # the exhaustive answer is still what PCT_ALGO_STREAM and a small host-mapped cloud give
    assert "NOT index-accelerated" in paragraph(text, "Radius search with lists (pct_radius_search_batch*")
    # the device forms cannot refile a table that lost points
    assert re.search(r"device forms? .{0,200}cannot repair", re.sub(r"\s*\n \*\s*", " ", text))
