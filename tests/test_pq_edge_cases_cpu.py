"""The inputs of tests/pq_edge_cases.py do what they claim — conditions on the ORACLE's answers, so that the GPU comparison in
tests/test_zz_pq_encode_edges_gpu.py cannot pass vacuously: the planted ties really tie (and the first minimum wins), NaN rows never
win, overflow leaves code 0, the survivor survives, the subnormal sums are subnormal and decide the code."""
import numpy as np
import pytest

import pq_edge_cases as E
from oracle import oracle as O

FLT_MIN = np.float32(2.0 ** -126)
SPLITS = [(S, None) for S in E.SIZES] + [(None, (4, 3, 3))]     # the uniform sizes, and D = 10 over M = 3
IDS = [f"S{S}" if sz is None else "D10M3" for S, sz in SPLITS]


def oracle_codes(case):
    D, M, cb, cen, v = case
    sizes = None if D % M == 0 else O.subvector_sizes_offsets(D, M)[0]
    opq = O.OraclePQ(D, M, cb, cen, sizes=sizes)
    return opq, opq.encode_all(v)


def subspaces(case):
    """-> per subspace (rows[256, s], centred sub-vectors[n, s] in f32)"""
    D, M, cb, cen, v = case
    sizes, _ = O.subvector_sizes_offsets(D, M)
    with np.errstate(invalid="ignore", over="ignore"):
        x = v if cen is None else (v - cen).astype(np.float32)
    out, at = [], 0
    for m, sub in enumerate(E.split(x, sizes)):
        out.append((cb[at: at + E.K * sizes[m]].reshape(E.K, sizes[m]), sub))
        at += E.K * sizes[m]
    return out


def test_split_matches_reference_sizes():
    assert list(O.subvector_sizes_offsets(10, 3)[0]) == [4, 3, 3]
    for S in E.SIZES:
        assert list(O.subvector_sizes_offsets(3 * S, 3)[0]) == [S] * 3


@pytest.mark.parametrize("S,sizes", SPLITS, ids=IDS)
def test_ties_tie_and_the_first_minimum_wins(S, sizes):
    case = E.ties(S, sizes=sizes)
    D, M, cb, cen, v = case
    assert np.abs(cb).max() <= 4 and np.array_equal(cb, np.round(cb)) and np.array_equal(v, np.round(v))
    opq, codes = oracle_codes(case)
    for m, (rows, sub) in enumerate(subspaces(case)):
        assert np.abs(sub).max() <= 4
        d = ((sub[:, None, :].astype(np.float64) - rows[None].astype(np.float64)) ** 2).sum(axis=2)   # exact: small integers
        dmin = d.min(axis=1)
        assert np.array_equal(codes[:, m], d.argmin(axis=1))                    # argmin: the FIRST minimum
        assert ((d == dmin[:, None]).sum(axis=1) >= 2).sum() >= len(E.TIE_PAIRS)
        for a, b in E.TIE_PAIRS:
            hit = (d[:, a] == dmin) & (d[:, b] == dmin)
            assert (hit & (dmin == 0)).any(), (m, a, b)                         # a vector ON the duplicated row
            assert (codes[hit & (dmin == 0), m] == a).all(), (m, a, b)          # (its value is at a and b only)
            assert (codes[hit, m] <= a).all(), (m, a, b)                        # (further off, an earlier row may tie too)
        halves = E.HALF_PAIRS if rows.shape[1] > 1 else E.HALF_PAIRS[:1]
        for a, b in halves:
            assert not np.array_equal(rows[a], rows[b])
            hit = (d[:, a] == dmin) & (d[:, b] == dmin) & (dmin == 1)
            assert hit.any(), (m, a, b)
            if rows.shape[1] > 1:
                assert ((d[hit] == 1).sum(axis=1) == 2).all()                   # those two rows and no other
                assert (codes[hit, m] == a).all()


@pytest.mark.parametrize("S,sizes", SPLITS, ids=IDS)
def test_nonfinite_rows_never_win(S, sizes):
    case = E.nonfinite(S, sizes=sizes)
    D, M, cb, cen, v = case
    opq, codes = oracle_codes(case)
    bad = E.nonfinite_bad_subspace(M)
    assert len(bad) == len(v)
    for m, (rows, sub) in enumerate(subspaces(case)):
        nan_rows = np.flatnonzero(np.isnan(rows).any(axis=1))
        assert set(E.NAN_ROWS) == set(nan_rows.tolist()) and np.isinf(rows[E.INF_ROW]).any()
        d = E.f32_distances(sub, rows)
        assert np.isnan(d[:, list(E.NAN_BLOCK)]).all()                          # a block of eight with no sum to offer
        fine = bad != m
        assert np.isfinite(sub[fine]).all() and not np.isfinite(d[~fine]).any() and (~fine).sum() == 3 * E.N_EACH
        assert not np.isin(codes[fine, m], nan_rows).any() and (codes[fine, m] != E.INF_ROW).all()
        assert (codes[~fine, m] == 0).all()                                     # NaN, Inf, all-overflow: `best` stays 0
        assert len(np.unique(codes[fine, m])) > 100
        for w, rows_at in E.nonfinite_winner_rows():
            assert (codes[rows_at, m] == w).all(), (m, w)
    for w in E.WINNERS:                                                         # a NaN row on either side, in the winner's block
        assert w - 1 in E.NAN_ROWS and w + 1 in E.NAN_ROWS and (w - 1) // 8 == (w + 1) // 8


@pytest.mark.parametrize("S,sizes", SPLITS, ids=IDS)
def test_overflow_and_survivor(S, sizes):
    case = E.overflow(S, sizes=sizes)
    for rows, sub in subspaces(case):
        assert np.isposinf(E.f32_distances(sub, rows)).all()
    assert (oracle_codes(case)[1] == 0).all()
    case = E.survivor(S, sizes=sizes)
    for rows, sub in subspaces(case):
        d = E.f32_distances(sub, rows)
        assert np.isposinf(np.delete(d, E.SURVIVOR, axis=1)).all() and np.isfinite(d[:, E.SURVIVOR]).all()
    assert (oracle_codes(case)[1] == E.SURVIVOR).all()


@pytest.mark.parametrize("S", E.SIZES)
def test_subnormal_sums_decide_the_code(S):
    case = E.subnormal(S)
    opq, codes = oracle_codes(case)
    for m, (rows, sub) in enumerate(subspaces(case)):
        d = E.f32_distances(sub, rows)
        assert np.array_equal(codes[:, m], d.argmin(axis=1))                    # the f32 chain above is the oracle's
        win = d[np.arange(len(d)), codes[:, m]]
        share = ((win > 0) & (win < FLT_MIN)).mean()
        distinct, zeros = len(np.unique(codes[:, m])), (codes[:, m] == 0).mean()
        print(f"S={S} m={m}: subnormal winners {share:.3f}, distinct codes {distinct}, code 0 {zeros:.3f}")
        assert share >= 0.9 and distinct >= 100 and zeros < 0.05


@pytest.mark.parametrize("S", [2, 4, 6, 16])
@pytest.mark.parametrize("k", [16, 255])
def test_small_k_vectors_sit_on_centroid_0(S, k):
    D, M, cb, cen, v = E.small_k(S, k)
    opq = O.OraclePQ(D, M, cb, None, k=k)
    codes = opq.encode_all(v)
    assert (codes[:, 0] == 0).all() and int(codes.max()) < k and len(np.unique(codes[:, 1])) > 1
    assert np.array_equal(np.stack([opq.decode(c) for c in codes]), v)


@pytest.mark.parametrize("n", E.RANDOM_COUNTS)
def test_random_shapes(n):
    D, M, cb, cen, v = E.random(4, n)
    assert (D, M) == (12, 3) and v.shape == (n, 12) and cb.shape == (256 * 12,) and cen.shape == (12,)
    assert E.random(4, n, centroid=False)[3] is None
