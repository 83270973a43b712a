"""The reference of tests/test_zz_flat_filter_gpu.py, checked without a GPU.  tests/flat_filter_ref.py restates the bound of the
flat search's two-stage filter (k_adc_bq.hip) in float64 and derives the pairs the bound scan MUST reject; the same module holds a
plain f32 numpy transcription of adc_bq_table_kernel and of adc_bq_kernel's reject tests.  Here the two meet, on the inputs the
GPU test uses at a few thousand rows:
  * the transcription drops no row whose exact score (the oracle's) reaches the threshold;
  * the transcription rejects every must-reject pair, and no must-reject pair is a passer;
  * must-reject is not vacuous: over the thresholds ranked 2 ... median it covers at least half of the pairs below the threshold.
The transcription shares its arithmetic with the kernel's SOURCE, not with the float64 restatement, so a wrong margin in the
restatement fails here first.  One more test: the mock device mocks neither filter kernel, and jv_hip_adc_filter says so."""
import os
import platform
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "mock"))

import flat_filter_ref as R   # noqa: E402
from oracle import oracle as O   # noqa: E402

VSFS = (R.EUCLIDEAN, R.DOT, R.COSINE)


def run_reference(vecs, queries, cb, centroid, D, M, vsf, check_coverage):
    """all three assertions for one input; returns (must-reject pairs, pairs below the threshold) over STRENGTH_KINDS"""
    opq = O.OraclePQ(D, M, cb, centroid)
    codes = R.duplicate_rows(opq.encode_all(vecs))
    covered = below = 0
    for q in range(queries.shape[0]):
        lut, amag, bm = opq.decoder(queries[q], vsf)
        scores = opq.adc_scores(queries[q], vsf, codes)
        norms = R.row_norms_f32(amag, codes) if vsf == R.COSINE else None
        ref = R.BoundRef(lut, codes)
        tab, base, S, ok = R.table_f32(vsf, lut, M)
        assert not (ref.usable and not ok) and not (ref.unusable and ok), (vsf, q)
        for kind in R.kinds_for(vsf):
            tau = R.threshold(scores, kind)
            P = R.passers(scores, tau)
            keep = R.survivors_f32(vsf, tab, base, S, ok, codes, tau, norms, bm)
            mr = ref.must_reject(vsf, tau, norms, bm)
            assert not (P & ~keep).any(), ("a passer dropped", vsf, q, kind)
            assert not (mr & keep).any(), ("a must-reject pair kept", vsf, q, kind, int((mr & keep).sum()))
            assert not (mr & P).any(), ("must-reject claims a passer", vsf, q, kind)
            if kind in R.STRENGTH_KINDS:
                covered += int(mr.sum())
                below += int((~P).sum())
    if check_coverage:
        assert covered * 2 >= below, (vsf, covered, below)
    return covered, below


@pytest.mark.parametrize("vsf", VSFS)
@pytest.mark.parametrize("kind,centroid", [("clustered", False), ("clustered", True), ("grid", False), ("grid", True)])
def test_reference_is_consistent_and_bites_pq16(kind, centroid, vsf):
    D, M, N, Q = 128, 16, 6000, 6
    vecs, queries, cb, c = R.problem(kind, 16, N, D, M, Q, centroid)
    cov, below = run_reference(vecs, queries, cb, c, D, M, vsf, True)
    print(f"coverage {kind} centroid={centroid} vsf={vsf} M={M}: {cov / below:.3f}")


@pytest.mark.parametrize("vsf", VSFS)
@pytest.mark.parametrize("kind,M,N", [("clustered", 32, 4000), ("clustered", 96, 3000), ("grid", 96, 3000), ("grid", 192, 2500)])
def test_reference_is_consistent_and_bites_wide_pq(kind, M, N, vsf):
    D, Q = 8 * M, 3
    vecs, queries, cb, c = R.problem(kind, M, N, D, M, Q, False)
    cov, below = run_reference(vecs, queries, cb, c, D, M, vsf, True)
    print(f"coverage {kind} vsf={vsf} M={M}: {cov / below:.3f}")


@pytest.mark.parametrize("vsf", VSFS)
def test_queries_without_a_usable_bound_are_classified(vsf):
    """the GPU test's four ways to lose the bound: what the reference says about each, and that the transcription agrees"""
    D, M, N, Q = 128, 16, 3000, 4
    vecs, queries, cb, c = R.problem("clustered", 5, N, D, M, Q)
    queries = R.no_bound_queries(queries)
    opq = O.OraclePQ(D, M, cb, c)
    codes = opq.encode_all(vecs)
    usable = []
    for q in range(Q):
        lut, _, _ = opq.decoder(queries[q], vsf)
        ref = R.BoundRef(lut, codes)
        _, _, _, ok = R.table_f32(vsf, lut, M)
        assert not (ref.usable and not ok) and not (ref.unusable and ok), (vsf, q)
        usable.append(ok)
    assert not usable[1], "a NaN component switches the bound off for every similarity function"
    if vsf == R.EUCLIDEAN:
        assert not usable[2], "a query scaled by 1e18: squared distances of 1e36 that differ by 1e18"
    run_reference(vecs, queries, cb, c, D, M, vsf, False)
    vecs, queries, cb, c = R.far_cluster_problem(6, N, D, M, Q)
    opq = O.OraclePQ(D, M, cb, c)
    codes = opq.encode_all(vecs)
    for q in range(Q):
        lut, _, _ = opq.decoder(queries[q], vsf)
        if vsf != R.EUCLIDEAN:
            assert R.BoundRef(lut, codes).unusable and not R.table_f32(vsf, lut, M)[3], (vsf, q)
    run_reference(vecs, queries, cb, c, D, M, vsf, False)


@pytest.mark.parametrize("vsf", (R.EUCLIDEAN, R.DOT))
def test_tables_near_the_usable_gate(vsf):
    """synthetic tables pushed towards `S * 1e6 >= max |entry|` by an offset: on either side of the gate the transcription drops no
    passer and rejects what the reference says it must, and beyond the gate the reference claims nothing"""
    rng = np.random.default_rng(9)
    M, N = 16, 4000
    codes = rng.integers(0, 256, (N, M)).astype(np.uint8)
    t0 = (rng.standard_normal((M, 256)) ** 2).astype(np.float32)
    S0 = float((t0.max(axis=1) - t0.min(axis=1)).max()) / 127.0
    for ratio in (100.0, 2.0, 1.01, 1.0, 0.99, 0.5):
        off = np.float32(S0 * 1e6 / ratio)
        lut = (t0 + (off if vsf == R.EUCLIDEAN else -off)).astype(np.float32)
        raw = np.zeros(N, np.float32)
        for m in range(M):
            raw = (raw + lut[m, codes[:, m]]).astype(np.float32)
        with np.errstate(all="ignore"):
            scores = (np.float32(1) / (np.float32(1) + raw)) if vsf == R.EUCLIDEAN else ((np.float32(1) + raw) / np.float32(2))
        scores = scores.astype(np.float32)
        ref = R.BoundRef(lut.reshape(-1), codes)
        tab, base, S, ok = R.table_f32(vsf, lut.reshape(-1), M)
        assert not (ref.usable and not ok) and not (ref.unusable and ok), ratio
        for kind in R.kinds_for(vsf):
            tau = R.threshold(scores, kind)
            P = R.passers(scores, tau)
            keep = R.survivors_f32(vsf, tab, base, S, ok, codes, tau)
            mr = ref.must_reject(vsf, tau)
            assert not (P & ~keep).any(), ("a passer dropped", ratio, kind)
            assert not (mr & keep).any() and not (mr & P).any(), (ratio, kind)
            if not ok:
                assert keep.all() and not mr.any(), (ratio, kind)


@pytest.mark.skipif(platform.machine() != "x86_64", reason="the lane emulator's context switch is x86-64 assembly")
def test_mock_device_refuses_the_filter_accessor():
    """adc_mq_supported / adc_bq_supported are false on the mock device: the accessor must say JV_ERR_UNSUPPORTED, not run anything"""
    from mockbind import mock_jvector
    with mock_jvector() as J:
        ctx = J.HipContext(0)
        try:
            rng = np.random.default_rng(0)
            D, M, N, Q = 128, 16, 64, 3
            pq = J.ProductQuantization.from_codebooks(ctx, D, M, rng.standard_normal(256 * D).astype(np.float32))
            cv = J.PQVectors(ctx, pq, rng.integers(0, 256, (N, M)).astype(np.uint8))
            sf = cv.precomputed_score_function_for(rng.standard_normal((Q, D)).astype(np.float32), J.VectorSimilarityFunction.DOT_PRODUCT)
            for stages in (1, 2):
                with pytest.raises(J.UnsupportedError, match="adc_filter"):
                    sf.threshold_filter(0, N, np.zeros(Q, np.float32), stages, 16)
            with pytest.raises(ValueError):
                sf.threshold_filter(0, N + 1, np.zeros(Q, np.float32), 1, 16)
            with pytest.raises(ValueError):
                sf.threshold_filter(0, N, np.zeros(Q, np.float32), 3, 16)
        finally:
            ctx.close()
