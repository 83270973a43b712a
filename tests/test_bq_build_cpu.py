"""The BQ build-time scoring without a GPU: the C ABI of include/jvector_bq_build.h is exactly its three entry points, exported by the
library and mirrored by bq_build.BQ_BUILD_SIGNATURES; the three other headers keep their symbol sets; and the CPU mock of the product library still binds."""
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["jv_hip_bq_graph_search_nodes", "jv_hip_bq_retain_diverse", "jv_hip_bq_retain_diverse_max_candidates"]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    import jvector_amd
    raw = None
    if os.path.exists(jvector_amd.LIB_PATH):
        raw = ctypes.CDLL(jvector_amd.LIB_PATH)
    if raw is None or not all(hasattr(raw, n) for n in NAMES):
        g.build()
    return jvector_amd.load()


def header_text(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def header_symbols(name):
    return re.findall(r"JV_API\s+[\w\s\*]+?\b(\w+)\s*\(", header_text(name))


def test_header_symbols_are_exported_and_mirrored(lib):
    from jvector_amd import bq_build
    names = header_symbols("jvector_bq_build.h")
    assert sorted(names) == NAMES
    assert set(names) == set(bq_build.BQ_BUILD_SIGNATURES)
    raw = ctypes.CDLL(os.path.join(ROOT, "jvector_amd", "libjvector_hip.so"))
    assert [n for n in names if not hasattr(raw, n)] == []
    assert bq_build.lib() is lib
    for n in names:
        assert getattr(lib, n).argtypes == bq_build.BQ_BUILD_SIGNATURES[n][1], n


def test_argument_counts_match_the_header():
    from jvector_amd import bq_build
    text = header_text("jvector_bq_build.h")
    for name, (_, args) in bq_build.BQ_BUILD_SIGNATURES.items():
        decl = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S).group(1)
        assert len(decl.split(",")) == len(args), name


def test_the_other_headers_are_as_they_were():
    from jvector_amd import bq, bq_graph
    assert len(header_symbols("jvector_bq.h")) == 14 and set(header_symbols("jvector_bq.h")) == set(bq.BQ_SIGNATURES)
    assert sorted(header_symbols("jvector_bq_graph.h")) == ["jv_hip_bq_graph_max_rerank_k", "jv_hip_bq_graph_search"]
    assert set(header_symbols("jvector_bq_graph.h")) == set(bq_graph.BQ_GRAPH_SIGNATURES)
    for h in ("jvector_hip.h", "jvector_formats.h"):
        assert "jv_hip_bq_" not in open(os.path.join(ROOT, "include", h)).read(), h
    for h in ("jvector_bq.h", "jvector_bq_graph.h"):
        text = open(os.path.join(ROOT, "include", h)).read()
        assert "retain_diverse" not in text and "search_nodes" not in text, h
    assert '#include "jvector_bq_graph.h"' in open(os.path.join(ROOT, "include", "jvector_bq_build.h")).read()


def test_package_exports_the_scorer():
    import jvector_amd as J
    from jvector_amd import bq_build
    assert J.BQBuildScorer is bq_build.BQBuildScorer
    for m in ("search_nodes", "retain_diverse", "max_candidates"):
        assert callable(getattr(J.BQBuildScorer, m))


def test_integration_doc_lists_the_entry_points():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert [n for n in NAMES if n not in doc] == []


def test_mock_library_still_binds():
    sys.path.insert(0, os.path.join(ROOT, "tests", "mock"))
    try:
        import mockbind
        with mockbind.mock_jvector() as J:
            assert J.device_count() >= 1
    finally:
        sys.path.remove(os.path.join(ROOT, "tests", "mock"))
