"""Every instantiation of the PQ encode kernels (k_pq.hip) at the edges of closestCentroidIndex (ProductQuantization.java:507-520:
strict `<`, the first minimum wins, NaN never wins, `best` stays 0 when nothing beats Float.MAX_VALUE), bit-exact against the oracle
on the inputs of tests/pq_edge_cases.py (which tests/test_pq_edge_cases_cpu.py shows to tie, overflow and underflow as claimed).

The parameter ids name the kernel launch_pq_encode picks:
    uniform size 2, 4, 6, 8, 12, 16   pq_encode_sgpr_kernel<S>; with JVECTOR_HIP_ENCODE_LDS=1 (read at each launch) pq_encode_kernel<S>
    uniform size 1, 3                 pq_encode_kernel<S> either way
    uniform size 5, D = 10 over M = 3 pq_encode_generic_kernel

Subnormal sums (the `subnormal` case: every winning distance a non-zero f32 below 2^-126) on gfx950: all three kernels keep them — the
packed v_pk_mul_f32 / v_pk_add_f32 chains, the fminf reduction of the blocks of eight and the `==` of the recomputation neither flush
nor reorder them; the codes equal the oracle's at every size.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import jvector_amd as J
import pq_edge_cases as E
from oracle import oracle as O

SGPR_SIZES = (2, 4, 6, 8, 12, 16)


def kernel(S, lds):
    if S == 5:
        return "pq_encode_generic_kernel"
    return f"pq_encode_sgpr_kernel<{S}>" if S in SGPR_SIZES and not lds else f"pq_encode_kernel<{S}>"


MODES = [pytest.param(S, lds, id=f"{kernel(S, lds)}-{'lds' if lds else 'default'}") for S in E.SIZES for lds in (False, True)]


@pytest.fixture(scope="module")
def ctx():
    c = J.HipContext(0)
    yield c
    c.close()


@pytest.fixture
def mode(monkeypatch):
    def set_mode(lds):
        if lds:
            monkeypatch.setenv("JVECTOR_HIP_ENCODE_LDS", "1")
        else:
            monkeypatch.delenv("JVECTOR_HIP_ENCODE_LDS", raising=False)
    return set_mode


@functools.lru_cache(maxsize=None)
def reference(name, S, *args):
    """(case, oracle codes), computed once and shared by both modes"""
    case = getattr(E, name)(S, *args)
    D, M, cb, cen, v = case
    for a in (cb, cen, v):
        if a is not None:
            a.setflags(write=False)
    return case, O.OraclePQ(D, M, cb, cen).encode_all(v)


def check(ctx, case, want):
    D, M, cb, cen, v = case
    assert len(v) <= 1000
    pq = J.ProductQuantization.from_codebooks(ctx, D, M, cb, cen)
    got = pq.encode_all(v)
    pq.close()
    assert got.dtype == np.uint8 and got.shape == want.shape
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{len(bad)} codes differ, first (vector, subspace) {bad[0]}: got {got[tuple(bad[0])]} want {want[tuple(bad[0])]}"
    return got


@pytest.mark.parametrize("S,lds", MODES)
@pytest.mark.parametrize("n", E.RANDOM_COUNTS)
def test_random_counts(ctx, mode, S, lds, n):
    mode(lds)
    check(ctx, *reference("random", S, n))


@pytest.mark.parametrize("S,lds", MODES)
@pytest.mark.parametrize("name", ["ties", "nonfinite", "overflow", "survivor", "subnormal"])
def test_edge_case(ctx, mode, S, lds, name):
    mode(lds)
    case, want = reference(name, S)
    got = check(ctx, case, want)
    if name == "overflow":
        assert (got == 0).all()
    if name == "survivor":
        assert (got == E.SURVIVOR).all()


@pytest.mark.parametrize("S,lds", MODES)
@pytest.mark.parametrize("centroid", [True, False], ids=["centroid", "nocentroid"])
def test_host_and_device_input(ctx, mode, S, lds, centroid):
    """the host path (staged copy), encode_all on a device tensor, PQVectors.encode_and_build on device-resident rows"""
    import torch
    mode(lds)
    case, want = reference("random", S, 600, centroid)
    D, M, cb, cen, v = case
    assert (cen is not None) == centroid
    check(ctx, case, want)
    pq = J.ProductQuantization.from_codebooks(ctx, D, M, cb, cen)
    tv = torch.from_numpy(v.copy()).cuda()
    cv = J.PQVectors.encode_and_build(ctx, pq, J.VectorSet(ctx, tv))
    ctx.sync()
    assert np.array_equal(cv.get(0, len(v)), want)
    tcodes = pq.encode_all(tv)
    ctx.sync()
    assert tcodes.is_cuda and tcodes.dtype == torch.uint8 and np.array_equal(tcodes.cpu().numpy(), want)


@pytest.mark.parametrize("lds", [False, True], ids=["default", "lds"])
@pytest.mark.parametrize("k", [16, 255])
@pytest.mark.parametrize("S", [2, 4, 6, 16])
def test_fewer_than_256_clusters(ctx, mode, S, k, lds):
    """the device rows k..255 are copies of centroid 0: they tie with it on every vector whose sub-vector IS centroid 0, in every
    block of eight after the first, and must never be chosen"""
    mode(lds)
    D, M, cb, _, v = E.small_k(S, k)
    want = O.OraclePQ(D, M, cb, None, k=k).encode_all(v)
    assert (want[:, 0] == 0).all()
    pq = J.ProductQuantization.from_codebooks(ctx, D, M, cb, None, cluster_count=k)
    got = pq.encode_all(v)
    assert got.dtype == np.uint8 and np.array_equal(got, want) and int(got.max()) < k


@pytest.mark.parametrize("lds", [False, True], ids=["default", "lds"])
@pytest.mark.parametrize("name", ["ties", "nonfinite"])
def test_non_uniform_split(ctx, mode, name, lds):
    """D = 10 over M = 3: sizes 4, 3, 3 through pq_encode_generic_kernel, whatever the mode"""
    mode(lds)
    D, M, cb, cen, v = getattr(E, name)(None, sizes=(4, 3, 3))
    assert (D, M) == (10, 3) and list(O.subvector_sizes_offsets(D, M)[0]) == [4, 3, 3]
    check(ctx, (D, M, cb, cen, v), O.OraclePQ(D, M, cb, cen).encode_all(v))
