"""The BQ graph search without a GPU: the C ABI of include/jvector_bq_graph.h is exported and mirrored by
bq_graph.BQ_GRAPH_SIGNATURES, the headers it must leave alone are as they were, and the CPU mock of the product library (which
compiles graph_search.cpp with the new graph accessor, and not bq_graph.cpp) still binds."""
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    import jvector_amd
    if not os.path.exists(jvector_amd.LIB_PATH):
        g.build()
    return jvector_amd.load()


def header_symbols(name):
    text = open(os.path.join(ROOT, "include", name)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.findall(r"JV_API\s+[\w\s\*]+?\b(\w+)\s*\(", text)


def test_header_symbols_are_exported_and_mirrored(lib):
    from jvector_amd import bq_graph
    names = header_symbols("jvector_bq_graph.h")
    assert sorted(names) == ["jv_hip_bq_graph_max_rerank_k", "jv_hip_bq_graph_search"]
    assert set(names) == set(bq_graph.BQ_GRAPH_SIGNATURES)
    raw = ctypes.CDLL(os.path.join(ROOT, "jvector_amd", "libjvector_hip.so"))
    assert [n for n in names if not hasattr(raw, n)] == []
    assert bq_graph.lib() is lib and lib.jv_hip_bq_graph_search.argtypes == bq_graph.BQ_GRAPH_SIGNATURES["jv_hip_bq_graph_search"][1]


def test_argument_counts_match_the_header():
    from jvector_amd import bq_graph
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jvector_bq_graph.h")).read(), flags=re.S)
    for name, (_, args) in bq_graph.BQ_GRAPH_SIGNATURES.items():
        decl = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S).group(1)
        assert len(decl.split(",")) == len(args), name


def test_the_other_headers_are_as_they_were():
    from jvector_amd import bq
    assert len(header_symbols("jvector_bq.h")) == 14 and set(header_symbols("jvector_bq.h")) == set(bq.BQ_SIGNATURES)
    assert "jv_hip_bq_graph" not in open(os.path.join(ROOT, "include", "jvector_bq.h")).read()
    for h in ("jvector_hip.h", "jvector_formats.h"):
        assert "jv_hip_bq_" not in open(os.path.join(ROOT, "include", h)).read(), h
    assert '#include "jvector_bq.h"' in open(os.path.join(ROOT, "include", "jvector_bq_graph.h")).read()


def test_package_exports_the_searcher():
    import jvector_amd as J
    from jvector_amd import bq_graph
    assert J.BQGraphSearcher is bq_graph.BQGraphSearcher


def test_mock_library_still_binds():
    sys.path.insert(0, os.path.join(ROOT, "tests", "mock"))
    try:
        import mockbind
        with mockbind.mock_jvector() as J:
            assert J.device_count() >= 1
    finally:
        sys.path.remove(os.path.join(ROOT, "tests", "mock"))
