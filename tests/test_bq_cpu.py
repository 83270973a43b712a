"""Binary quantization without a GPU: the C ABI of include/jvector_bq.h is exported and mirrored by bq.BQ_SIGNATURES, the byte
parser (jv_hip_bq_describe, host only) reads blocks written here from the reference's layout (BinaryQuantization.write +
BQVectors.write, big-endian) and rejects the bad ones, and the CPU mock of the product library still binds."""
import ctypes
import os
import re
import struct
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    import jvector_amd
    if not os.path.exists(jvector_amd.LIB_PATH):
        g.build()
    return jvector_amd.load()


def bq_header_symbols():
    text = open(os.path.join(ROOT, "include", "jvector_bq.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.findall(r"JV_API\s+[\w\s\*]+?\b(\w+)\s*\(", text)


def java_block(D, words, count=None, length=None):
    """BinaryQuantization.write (int D, D zero floats) + BQVectors.write (int count, [int compressedLength, longs])"""
    words = np.asarray(words, np.uint64).reshape(-1, (D + 63) // 64) if words is not None else None
    n = len(words) if count is None else count
    out = struct.pack(">i", D) + b"\0" * (4 * D) + struct.pack(">i", n)
    if n > 0:
        out += struct.pack(">i", words.shape[1] if length is None else length)
        out += words.astype(">u8").tobytes()
    return out


def test_header_symbols_are_exported_and_mirrored(lib):
    from jvector_amd import bq
    names = bq_header_symbols()
    assert len(names) == 14
    assert set(names) == set(bq.BQ_SIGNATURES), set(names) ^ set(bq.BQ_SIGNATURES)
    raw = ctypes.CDLL(os.path.join(ROOT, "jvector_amd", "libjvector_hip.so"))
    assert [n for n in names if not hasattr(raw, n)] == []


def test_bq_symbols_stay_out_of_the_core_headers():
    for h in ("jvector_hip.h", "jvector_formats.h"):
        assert "jv_hip_bq_" not in open(os.path.join(ROOT, "include", h)).read(), h


@pytest.mark.parametrize("D", [1, 64, 65, 768])
def test_describe_reads_the_java_layout(lib, D):
    from jvector_amd import bq
    W = (D + 63) // 64
    rng = np.random.default_rng(D)
    words = rng.integers(0, 2**63, size=(5, W), dtype=np.uint64)
    blob = java_block(D, words) + b"trailing bytes of the next block"
    info = bq.describe(blob)
    assert info == {"dimension": D, "count": 5, "words": W, "data_offset": 4 + 4 * D + 8, "block_len": 4 + 4 * D + 8 + 40 * W}
    # count 0: no compressedLength field
    empty = java_block(D, None, count=0)
    assert len(empty) == 4 + 4 * D + 4
    assert bq.describe(empty + b"\x7f\x7f\x7f\x7f") == {"dimension": D, "count": 0, "words": 0, "data_offset": 4 + 4 * D + 4,
                                                      "block_len": 4 + 4 * D + 4}


def test_describe_rejects_bad_blocks(lib):
    from jvector_amd import bq
    from jvector_amd._lib import UnsupportedError
    D = 65
    good = java_block(D, np.arange(6, dtype=np.uint64))
    for cut in (0, 3, 4 + 4 * D, 4 + 4 * D + 4, 4 + 4 * D + 7, len(good) - 1):
        with pytest.raises(ValueError, match="truncated"):
            bq.describe(good[:cut])
    with pytest.raises(ValueError, match="count"):
        bq.describe(java_block(D, None, count=-1))
    with pytest.raises(ValueError, match="dimension"):
        bq.describe(java_block(D, np.zeros((1, 2), np.uint64), length=-2))
    with pytest.raises(ValueError, match="dimension"):
        bq.describe(struct.pack(">i", 0) + struct.pack(">i", 0))
    # a compressedLength the reference would accept but the device layout cannot hold
    with pytest.raises(UnsupportedError, match="compressed length 3"):
        bq.describe(java_block(D, np.zeros((2, 3), np.uint64).reshape(-1), count=2, length=3)[:4 + 4 * D + 8] + b"\0" * 48)


def test_mock_library_still_binds():
    sys.path.insert(0, os.path.join(ROOT, "tests", "mock"))
    try:
        import mockbind
        with mockbind.mock_jvector() as J:
            assert J.device_count() >= 1
    finally:
        sys.path.remove(os.path.join(ROOT, "tests", "mock"))
