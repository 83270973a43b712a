"""The top-k edge cases of tests/test_zz_topk_paths_gpu.py, a reduced set, on the mock device.  The mock's launch_topk
(tests/mock/mock_kernels.cpp) is a host restatement of the NodeQueue order that shares nothing with k_topk.hip, so these runs say
nothing about the kernels; they prove that the case builders and the oracle agree with that second restatement (a wrong expectation
would fail here first), exercise jv_hip_topk's host side (sizes, staging of strided rows, the error path), and keep the builders
from rotting on machines without a GPU.  JVECTOR_HIP_TOPK_RADIX means nothing to the mock: check()'s second run repeats the first."""
import ctypes as C
import os
import platform
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "mock"))

pytestmark = pytest.mark.skipif(platform.machine() != "x86_64", reason="the lane emulator's context switch is x86-64 assembly")


@pytest.fixture(scope="module")
def J():
    import build_mock
    import jvector_amd
    import jvector_amd._lib as L
    lib = C.CDLL(build_mock.build())
    for table in (L.SIGNATURES, L.COMPAT_SIGNATURES, L.FORMAT_SIGNATURES):
        for name, (res, args) in table.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    saved, L._lib = L._lib, lib
    saved_threads = os.environ.get("JVECTOR_HIP_HOST_THREADS")
    os.environ["JVECTOR_HIP_HOST_THREADS"] = "1"
    try:
        assert b"mock" in lib.jv_hip_active_arch(0)
        yield jvector_amd
    finally:
        L._lib = saved
        if saved_threads is None:
            os.environ.pop("JVECTOR_HIP_HOST_THREADS", None)
        else:
            os.environ["JVECTOR_HIP_HOST_THREADS"] = saved_threads


@pytest.fixture()
def ctx(J):
    c = J.HipContext(0)
    yield c
    c.close()


def test_special_values_and_digit_boundaries_on_the_mock(J, ctx, monkeypatch):
    import test_zz_topk_paths_gpu as T
    T.test_special_values(ctx, monkeypatch, 100, False)                     # a
    T.test_special_values(ctx, monkeypatch, 300, True)
    T.test_special_values(ctx, monkeypatch, 9000, True)
    for spread_bits in (21, 10):                                            # b
        T.test_digit_boundary_in_the_score(ctx, monkeypatch, spread_bits)
    for shift, n in ((21, 1024), (10, 3000), (0, 3000)):
        T.test_digit_boundary_in_the_id(ctx, monkeypatch, shift, n)
    T.test_kth_and_next_differ_in_the_lowest_id_bit(ctx, monkeypatch, 0x12345400)
    T.test_kth_and_next_differ_in_the_lowest_id_bit(ctx, monkeypatch, T.INT_MAX - 2999)


def test_sizes_ids_strides_and_rows_on_the_mock(J, ctx, monkeypatch):
    import test_zz_topk_paths_gpu as T
    for n in (1, 2, 65, 129, 4097, 8193):                                   # c
        T.test_size_boundaries(ctx, monkeypatch, n)
    T.test_largest_k(ctx, monkeypatch, 8193, 8192)
    T.test_largest_k(ctx, monkeypatch, 20000, 3)
    T.test_k_above_the_maximum_is_refused(ctx, monkeypatch)
    T.test_ids_with_holes(ctx, monkeypatch, 300, (10, 64))                  # d
    T.test_ids_with_holes(ctx, monkeypatch, 9000, (100,))
    T.test_fewer_valid_entries_than_k(ctx, monkeypatch, 300, 5, 10)
    T.test_fewer_valid_entries_than_k(ctx, monkeypatch, 9000, 40, 100)
    T.test_extreme_ids_with_tied_scores(ctx, monkeypatch, 110, 110)
    T.test_extreme_ids_with_tied_scores(ctx, monkeypatch, 9000, 100)
    T.test_stride_and_id_base(ctx, monkeypatch, 110, (10, 100))             # e
    T.test_stride_and_id_base(ctx, monkeypatch, 9000, (100,))
    T.test_stride_below_n_is_an_error(ctx)
    for Q, n, k in ((5, 110, 10), (1027, 110, 10), (9, 8193, 10), (7, 5000, 100)):   # f
        T.test_row_counts(ctx, monkeypatch, Q, n, k)
