"""ubr_table_kernel (k_ubr_table.hip) over shapes and inputs beyond the headline's: its bytes == gs_host.h gs_ubr_build_ref
(through the lane emulator's gs_emu_ubr_table_vsf) for every similarity, M in {16, 64, 96, 128, 192, 256}, ragged blocks of the
8-queries-per-block kernel, and queries whose tables are unusable (zero, NaN, +-inf, finite inputs whose entries overflow to inf).
M > 256 is refused with JV_ERR_UNSUPPORTED."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import jvector_amd as J
from jvector_amd import VectorSimilarityFunction as VSF
from test_zz_ubr_gpu import emu_lib


@pytest.fixture(scope="module")
def ctx():
    c = J.HipContext(0)
    yield c
    c.close()


def _queries(rng, Q, D):
    q = rng.standard_normal((Q, D)).astype(np.float32)
    special = {}
    if Q >= 4:
        q[1] = 0.0                   # every entry 0: the scale floor
        q[2, 5] = np.nan
        q[3, 9] = np.inf
        special.update({2: "nan", 3: "inf"})
    if Q >= 5:
        q[4, :8] = 3.0e38            # subspace 0, code 0 (all ones): 8 x 3e38 overflows to inf from finite inputs
        special[4] = "overflow"
    if Q >= 21:
        q[7, 17] = -np.inf
        q[11] = 1e-20
        q[13] *= 1e18
        special[7] = "-inf"
    return q, special


@pytest.mark.parametrize("M", [16, 64, 96, 128, 192, 256])
def test_bound_tables_shapes(ctx, M):
    D = 8 * M
    rng = np.random.default_rng(1000 + M)
    cb = (rng.standard_normal(256 * D) * 0.3).astype(np.float32)
    cb[:8] = 1.0
    centroid = (rng.standard_normal(D) * 0.05).astype(np.float32)
    pq = J.ProductQuantization.from_codebooks(ctx, D, M, cb, centroid)
    L = emu_lib()
    for Q in (1, 3, 4, 5, 21, 4099):
        q, special = _queries(rng, Q, D)
        cq = (q - centroid).astype(np.float32)
        # the emulator's reference for a sample of the queries (every one of the small batches)
        check = range(Q) if Q <= 64 else sorted(set(range(16)) | set(range(Q - 8, Q)) | set(rng.integers(0, Q, 24).tolist()))
        for vsf in (VSF.EUCLIDEAN, VSF.DOT_PRODUCT, VSF.COSINE):
            luts = J.QueryTables(ctx, pq, Q).build(q, vsf, J.DecoderKind.FUSED)
            tab, meta = luts.bound_tables()
            luts.close()
            for i in check:
                wt = np.empty(M * 64, np.uint32)
                wm = np.empty(4, np.float32)
                L.gs_emu_ubr_table_vsf(cb.ctypes.data_as(C.c_void_p), np.ascontiguousarray(cq[i]).ctypes.data_as(C.c_void_p), M,
                                       wt.ctypes.data_as(C.c_void_p), wm.ctypes.data_as(C.c_void_p), 0 if vsf == VSF.EUCLIDEAN else 1)
                assert np.array_equal(tab[i], wt), (M, Q, vsf, i, np.argwhere(tab[i] != wt)[:4])
                if i in special:
                    # no usable table: all zero, flagged; (the restatement's extremes treat NaN differently, so base / scale are not compared)
                    assert meta[i, 2] == 0.0 and wm[2] == 0.0 and not tab[i].any(), (M, Q, vsf, i, special[i])
                else:
                    assert np.array_equal(meta[i].view(np.uint32), wm.view(np.uint32)), (M, Q, vsf, i, meta[i], wm)


def test_bound_tables_refuse_m_above_256(ctx):
    M = 264
    D = 8 * M
    rng = np.random.default_rng(7)
    pq = J.ProductQuantization.from_codebooks(ctx, D, M, (rng.standard_normal(256 * D) * 0.3).astype(np.float32))
    luts = J.QueryTables(ctx, pq, 3).build(rng.standard_normal((3, D)).astype(np.float32), VSF.COSINE, J.DecoderKind.FUSED)
    with pytest.raises(J.UnsupportedError, match="at most 256"):
        luts.bound_tables()
    luts.close()
