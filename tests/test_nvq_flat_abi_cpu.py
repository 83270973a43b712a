"""CPU-only boundary check of include/jvector_nvq_flat.h: libjvector_hip.so exports every JV_API symbol the header declares, and the
Python signature table (jvector_amd/nvq_flat.py) names the same set."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "jvector_nvq_flat.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.findall(r"JV_API\s+[\w\s\*]+?\b(\w+)\s*\(", text)


def test_header_library_and_signature_table_agree():
    import __graft_entry__ as g
    import jvector_amd
    from jvector_amd import nvq_flat
    if not os.path.exists(jvector_amd.LIB_PATH):
        g.build()
    names = declared_symbols()
    assert names == ["jv_hip_nvq_search_flat"]
    raw = ctypes.CDLL(jvector_amd.LIB_PATH)
    assert [n for n in names if not hasattr(raw, n)] == []
    assert set(names) == set(nvq_flat.NVQ_FLAT_SIGNATURES)
    assert hasattr(jvector_amd.NVQVectors, "search_flat")
