"""launch_topk (k_topk.hip) at the edges of each of its three algorithms, against the oracle's NodeQueue order.

Which kernel a shape reaches (launch_topk's own conditions; nothing in the product is added to observe it):

  register    n <= 4096 and k <= 64: topk_small_kernel<NPL>, NPL = 2, 4, 8, 16, 32, 64 at n <= 128, 256, 512, 1024, 2048, 4096;
              one wavefront per row, four rows per block
  sort-all    otherwise n <= 8192: topk_sortall_kernel, bitonic sort of next_pow2(n) keys in LDS (64 KB at 8192)
  radix       n > 8192, or JVECTOR_HIP_TOPK_RADIX set (read on every launch): topk_hist_kernel / topk_select_kernel over six digits
              of 11/11/10 | 11/11/10 bits, topk_collect_kernel, topk_sort_kernel over next_pow2(k) keys (64 KB at k = 8192)

So below: n in {1 ... 4096} with k <= 64 is the register kernel; the same n with k >= 65, and n in {4097 ... 8192} with any k, is
sort-all; n in {8193, 9000, 20000} is the radix select.  check() runs every shape of n <= 8192 a second time with
JVECTOR_HIP_TOPK_RADIX set, which sends it through the radix select whatever n and k are, and wants the oracle's answer from both.

Scores are compared as bit patterns: NaN (the kernels hand back Float.floatToIntBits' canonical 0x7FC00000, which sorts above
+inf) and the two zeros are distinct keys of the order and equal or unequal in the wrong way under a float comparison.

The functions take `ctx` (and `monkeypatch`) so that tests/test_topk_cases_cpu.py re-runs a reduced set on the mock device."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import jvector_amd as J
from oracle import oracle as O

NEG_INF_BITS = 0xFF800000
INT_MAX = 2147483647
RADIX_ENV = "JVECTOR_HIP_TOPK_RADIX"
SORTALL_MAX_N = 8192                       # rows above it take the radix select by themselves
GAP = 37                                   # stride - n of the strided cases


@pytest.fixture(scope="module")
def ctx():
    c = J.HipContext(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------
# the one helper
# ------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _run(ctx, scores, k, ids, id_base, stride):
    """(ids, scores) of one launch.  Through jvector_amd.topk, or — stride / id_base given — through the C entry on rows of `stride`
    cells whose gap cells hold +inf and ids that look valid: a read past n then wins the row."""
    if stride is None and id_base == 0:
        return J.topk(ctx, scores, k, ids=ids)
    Q, n = scores.shape
    stride = n if stride is None else stride
    sc = np.full((Q, stride), np.inf, np.float32)
    sc[:, :n] = scores
    idp = None
    if ids is not None:
        idp = np.tile(1_500_000_000 + np.arange(stride, dtype=np.int32), (Q, 1))
        idp[:, :n] = ids
    oi = np.full((Q, k), -7, np.int32)
    osc = np.full((Q, k), 1234.5, np.float32)
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731
    rc = ctx._lib.jv_hip_topk(ctx._h, p(sc), p(idp), Q, n, stride, int(id_base), int(k), p(oi), p(osc))
    assert rc == 0, J._lib.last_error()
    return oi, osc


def _compare(got, want, k, tag):
    gi, gs = np.asarray(got[0]), _bits(got[1])
    assert gi.shape == gs.shape == (len(want), k), tag
    for q, (wi, ws) in enumerate(want):
        cnt = len(wi)
        assert np.array_equal(gi[q, :cnt], wi), (tag, q, "ids")
        assert np.array_equal(gs[q, :cnt], _bits(ws)), (tag, q, "score bits")
        assert np.all(gi[q, cnt:] == -1) and np.all(gs[q, cnt:] == NEG_INF_BITS), (tag, q, "tail")


def check(ctx, scores, k, ids=None, id_base=0, stride=None, monkeypatch=None):
    """every row of the device's top-k equals oracle.topk's: ids, score bit patterns, and a (-1, -inf) tail past the oracle's count.
    Rows of n <= 8192 run twice, as dispatched and with the radix select forced."""
    scores = np.ascontiguousarray(scores, np.float32)
    Q, n = scores.shape
    want = []
    for q in range(Q):
        if ids is None:
            want.append(O.topk((id_base + np.arange(n, dtype=np.int64)).astype(np.int32), scores[q], k))
        else:
            valid = ids[q] >= 0
            want.append(O.topk(ids[q][valid], scores[q][valid], k))
    tag = (Q, n, k, id_base, stride)
    got = _run(ctx, scores, k, ids, id_base, stride)
    _compare(got, want, k, tag + ("dispatched",))
    if n > SORTALL_MAX_N:
        return
    assert monkeypatch is not None, "rows of n <= 8192 need monkeypatch to force the radix select"
    monkeypatch.setenv(RADIX_ENV, "1")
    try:
        forced = _run(ctx, scores, k, ids, id_base, stride)
    finally:
        monkeypatch.delenv(RADIX_ENV)
    _compare(forced, want, k, tag + ("radix forced",))
    assert np.array_equal(np.asarray(got[0]), np.asarray(forced[0])) and np.array_equal(_bits(got[1]), _bits(forced[1])), tag


# ------------------------------------------------------------------------------------------------
# a. special values
# ------------------------------------------------------------------------------------------------
SPECIAL_BITS = np.array([
    0x7FC00000, 0xFFC00000, 0x7FC00001, 0xFFC00001, 0x7FFFFFFF, 0xFFFFFFFF,      # quiet NaNs, both signs, payloads
    0x7F800001, 0xFF800001, 0x7FBFFFFF, 0xFFA00000,                              # signalling NaNs
    0x7F800000, 0xFF800000,                                                      # +-inf
    0x00000000, 0x80000000,                                                      # +0.0, -0.0
    0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF,                              # +-1e-45, the largest denormals
    0x00800000, 0x80800000,                                                      # +-FLT_MIN
    0x7F7FFFFF, 0xFF7FFFFF,                                                      # +-FLT_MAX
], np.uint32)


def special_row(rng, n):
    """n score bit patterns: every special value, each again as a run of duplicates, normal values in between, shuffled"""
    normal = rng.standard_normal(n).astype(np.float32)
    normal[::3] = np.round(normal[::3] * 2) / 2                     # duplicates among the normal values too
    row = normal.view(np.uint32).copy()
    filler = np.concatenate([SPECIAL_BITS, np.repeat(SPECIAL_BITS, 2)])[: max(1, (2 * n) // 3)]
    row[: len(filler)] = filler
    return row[rng.permutation(n)]


@pytest.mark.parametrize("explicit_ids", [False, True])
@pytest.mark.parametrize("n", [100, 300, 5000, 9000])
def test_special_values(ctx, monkeypatch, n, explicit_ids):
    """NaN of every kind, +-inf, the zeros, denormals, +-FLT_MAX and duplicates in one row: register kernel (n = 100, 300 at
    k <= 64), sort-all (k = 65, n = 5000) and radix (n = 9000, and every shape forced)"""
    rng = np.random.default_rng(1000 + n)
    scores = np.stack([special_row(rng, n), special_row(rng, n)]).view(np.float32)
    assert np.isnan(scores).sum() >= 20 and (_bits(scores) == 0x80000000).any()
    ids = None
    if explicit_ids:
        ids = np.stack([rng.permutation(3 * n)[:n] for _ in range(2)]).astype(np.int32)
    # what the issue measured on the oracle: the canonical NaN first, and 1e-45 > 0.0 > -0.0 > -1e-45
    wi, ws = O.topk(None, scores[0], n)
    assert _bits(ws)[0] == 0x7FC00000
    order = [int(np.flatnonzero(_bits(ws) == b)[0]) for b in (0x00000001, 0x00000000, 0x80000000, 0x80000001)]
    assert order == sorted(order)
    for k in (10, 64, 65):
        if k <= n:
            check(ctx, scores, k, ids=ids, monkeypatch=monkeypatch)


# ------------------------------------------------------------------------------------------------
# b. the digit at which the radix select stops
# ------------------------------------------------------------------------------------------------
DIGIT_KS = (1, 17, 1000, 2999)


def prefix_scores(rng, n, spread_bits):
    """three rows of float32 built from 0x3F000000 + j, j < 2^spread_bits: random j; j in four places of the highest digit that
    varies (bits 10 and up of j when there are any, else four values in all), so that every k lies strictly inside a bin there;
    and j as evenly spread as n allows (all distinct if 2^spread_bits >= n)"""
    top = 1 << spread_bits
    j0 = rng.integers(0, top, n)
    pick = rng.integers(0, 4, n)
    if spread_bits > 10:
        j1 = (rng.choice(top >> 10, 4, replace=False)[pick] << 10) | rng.integers(0, 1024, n)
    else:
        j1 = rng.choice(top, 4, replace=False)[pick]
    j2 = rng.permutation(top)[:n] if top >= n else rng.permutation(n) % top
    return (np.uint32(0x3F000000) + np.stack([j0, j1, j2]).astype(np.uint32)).view(np.float32)


@pytest.mark.parametrize("spread_bits", [21, 10])
def test_digit_boundary_in_the_score(ctx, monkeypatch, spread_bits):
    """n = 3000 (sort-all; radix when forced).  Scores share their top 11 bits (spread 21: the select has to go into the 2nd and 3rd
    score digit) or their top 22 bits (spread 10: only the 3rd score digit differs, and every value repeats, so the id digits
    run too)"""
    rng = np.random.default_rng(spread_bits)
    n = 3000
    scores = prefix_scores(rng, n, spread_bits)
    top = _bits(scores) >> (32 - (11 if spread_bits == 21 else 22))
    assert (top == top[0, 0]).all()
    ids = np.stack([rng.permutation(n) for _ in range(3)]).astype(np.int32)
    for k in DIGIT_KS:
        check(ctx, scores, k, monkeypatch=monkeypatch)
        check(ctx, scores, k, ids=ids, monkeypatch=monkeypatch)


@pytest.mark.parametrize("shift,n", [(21, 1024), (10, 3000), (0, 3000)])
def test_digit_boundary_in_the_id(ctx, monkeypatch, shift, n):
    """all scores identical, ids i << shift shuffled within the row: they differ only in the 1st (shift 21, at most 1024 ids below
    2^31), the 1st and 2nd (shift 10) or the 2nd and 3rd (shift 0) id digit.  i << 10: the 1st id digit's top bin holds 2048 keys,
    the next 952; i: the 2nd id digit's bins hold 1024, 1024 and 952 — no k below falls on a bin's edge at those digits"""
    rng = np.random.default_rng(shift)
    Q = 3
    scores = np.full((Q, n), 0.75, np.float32)
    scores[2] = -0.0
    ids = np.stack([(rng.permutation(n).astype(np.int64) << shift) for _ in range(Q)])
    assert ids.max() <= INT_MAX
    ids = ids.astype(np.int32)
    for k in DIGIT_KS + ((1023,) if n == 1024 else ()):
        check(ctx, scores, k, ids=ids, monkeypatch=monkeypatch)


@pytest.mark.parametrize("base", [0, 0x12345400, INT_MAX - 2999])
def test_kth_and_next_differ_in_the_lowest_id_bit(ctx, monkeypatch, base):
    """identical scores, ids base + i: the k-th key ends in ...0 and the (k+1)-th in ...1 for odd k, so the threshold is the k-th
    key itself and all six digits run"""
    rng = np.random.default_rng(5)
    n = 3000
    scores = np.full((2, n), 0.5, np.float32)
    scores[1, rng.permutation(n)[:40]] = 1.0                      # 40 above: the tie starts at place 41
    ids = (base + np.stack([rng.permutation(n) for _ in range(2)])).astype(np.int32)
    assert base % 2 == 0
    for k in (1, 17, 41, 57, 1001, 2999):
        check(ctx, scores, k, ids=ids, monkeypatch=monkeypatch)
    check(ctx, scores, 17, id_base=base, monkeypatch=monkeypatch)


# ------------------------------------------------------------------------------------------------
# c. size boundaries
# ------------------------------------------------------------------------------------------------
def five_rows(rng, n):
    scores = rng.standard_normal((5, n)).astype(np.float32)
    scores[1] = np.round(scores[1] * 4) / 4            # heavy ties
    scores[2] = np.round(scores[2] * 4) / 4
    scores[3] = 0.5                                    # all equal: ids decide
    scores[4, ::7] = scores[4, 0]
    return scores


def boundary_ks(n):
    return sorted({k for k in (1, 2, 63, 64, 65, n - 1, n, n + 1) if 1 <= k <= 8192})


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 128, 129, 4096, 4097, 8191, 8192, 8193])
def test_size_boundaries(ctx, monkeypatch, n):
    """k <= 64: register kernel up to n = 4096 (NPL 2 up to 128, 4 at 129, 64 at 4096), sort-all from 4097; k >= 65: sort-all up to
    8192 (npad 2 at n = 1; 8192 = 64 KB at 4097 ...  8192); n = 8193: radix.  k = n - 1, n, n + 1: the last valid place, a full
    row, and a tail"""
    rng = np.random.default_rng(n)
    scores = five_rows(rng, n)
    for k in boundary_ks(n):
        check(ctx, scores, k, monkeypatch=monkeypatch)


@pytest.mark.parametrize("n,k", [(8192, 8192), (8193, 8192), (20000, 8192), (20000, 4097), (20000, 3)])
def test_largest_k(ctx, monkeypatch, n, k):
    """k = kMaxK: the 64 KB sort of sort-all (n = 8192) and of the radix select's last step (n = 8193, 20 000); 4097: kpad 8192
    more than half empty; 3: kpad 4"""
    check(ctx, five_rows(np.random.default_rng(n + k), n), k, monkeypatch=monkeypatch)


def test_k_above_the_maximum_is_refused(ctx, monkeypatch):
    for n in (100, 20000):
        with pytest.raises(J.UnsupportedError, match="8193"):
            J.topk(ctx, np.zeros((2, n), np.float32), 8193)
    monkeypatch.setenv(RADIX_ENV, "1")
    try:
        with pytest.raises(J.UnsupportedError, match="8193"):
            J.topk(ctx, np.zeros((2, 100), np.float32), 8193)
    finally:
        monkeypatch.delenv(RADIX_ENV)


# ------------------------------------------------------------------------------------------------
# d. ids
# ------------------------------------------------------------------------------------------------
def tied_scores(rng, Q, n):
    return (np.round(rng.standard_normal((Q, n)) * 4) / 4).astype(np.float32)


@pytest.mark.parametrize("n,ks", [(300, (10, 64)), (5000, (10, 100)), (9000, (10, 100))])
def test_ids_with_holes(ctx, monkeypatch, n, ks):
    """-1 scattered through the row (register, sort-all, radix), one row entirely -1 and one with a single valid entry"""
    rng = np.random.default_rng(n)
    Q = 4
    scores = tied_scores(rng, Q, n)
    ids = np.stack([rng.permutation(1_000_000)[:n] for _ in range(Q)]).astype(np.int32)
    ids[0, rng.random(n) < 0.3] = -1
    ids[1, rng.random(n) < 0.9] = -1
    ids[2] = -1
    ids[3] = -1
    ids[3, n // 2] = 77
    scores[2, ::2] = np.inf                                   # a score next to a -1 id is never looked at
    for k in ks:
        check(ctx, scores, k, ids=ids, monkeypatch=monkeypatch)


@pytest.mark.parametrize("n,valid,k", [(300, 5, 10), (300, 63, 64), (5000, 70, 100), (5000, 10, 10), (9000, 40, 100), (9000, 99, 100)])
def test_fewer_valid_entries_than_k(ctx, monkeypatch, n, valid, k):
    """the radix select's pass-0 exit (total <= k) and the empty-key tails of the other two kernels; valid == k: a full answer
    that needs every valid entry"""
    rng = np.random.default_rng(n + valid)
    Q = 3
    scores = tied_scores(rng, Q, n)
    ids = np.full((Q, n), -1, np.int32)
    for q in range(Q):
        at = rng.permutation(n)[:valid]
        ids[q, at] = rng.permutation(1_000_000)[:valid]
    ids[2, np.flatnonzero(ids[2] >= 0)[0]] = -1               # one fewer in the last row
    check(ctx, scores, k, ids=ids, monkeypatch=monkeypatch)


@pytest.mark.parametrize("n,k", [(110, 10), (110, 110), (5000, 100), (9000, 100)])
def test_extreme_ids_with_tied_scores(ctx, monkeypatch, n, k):
    """id 0 (low key word 0xFFFFFFFF) and 2147483647 (low key word 0x80000000) among tied scores, and a row of one score"""
    rng = np.random.default_rng(n)
    Q = 3
    scores = np.round(rng.standard_normal((Q, n))).astype(np.float32)
    scores[2] = 3.0
    ids = np.stack([rng.permutation(np.unique(rng.integers(2, INT_MAX - 1, 2 * n))[:n]) for _ in range(Q)]).astype(np.int32)
    for q in range(Q):
        a, b, c, d = rng.permutation(n)[:4]
        ids[q, a], ids[q, b], ids[q, c], ids[q, d] = 0, INT_MAX, 1, INT_MAX - 1
        scores[q, b] = scores[q, a]                            # 0 and INT_MAX tie with each other
        scores[q, d] = scores[q, c] = scores[q].max()
    check(ctx, scores, k, ids=ids, monkeypatch=monkeypatch)


# ------------------------------------------------------------------------------------------------
# e. stride and id_base through the C entry
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,ks", [(110, (10, 100)), (5000, (100,)), (9000, (100,))])
def test_stride_and_id_base(ctx, monkeypatch, n, ks):
    """rows of n + 37 cells (register and sort-all at n = 110, sort-all at 5000, radix at 9000) with explicit ids, and
    ids = NULL with id_base 1000 and 2147483647 - n (the last id is then 2147483646)"""
    rng = np.random.default_rng(n)
    Q = 3
    scores = tied_scores(rng, Q, n)
    ids = np.stack([rng.permutation(1_000_000)[:n] for _ in range(Q)]).astype(np.int32)
    ids[1, ::9] = -1
    for k in ks:
        check(ctx, scores, k, ids=ids, stride=n + GAP, monkeypatch=monkeypatch)
        check(ctx, scores, k, stride=n + GAP, monkeypatch=monkeypatch)
        for id_base in (1000, INT_MAX - n):
            check(ctx, scores, k, id_base=id_base, monkeypatch=monkeypatch)
            check(ctx, scores, k, id_base=id_base, stride=n + GAP, monkeypatch=monkeypatch)


def test_stride_below_n_is_an_error(ctx):
    scores = np.zeros((2, 100), np.float32)
    oi, osc = np.zeros((2, 5), np.int32), np.zeros((2, 5), np.float32)
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    assert ctx._lib.jv_hip_topk(ctx._h, p(scores), None, 2, 100, 99, 0, 5, p(oi), p(osc)) == J._lib.JV_ERR_INVALID
    assert "bad sizes" in J._lib.last_error()
    assert ctx._lib.jv_hip_topk(ctx._h, p(scores), None, 2, 100, 100, 0, 5, p(oi), p(osc)) == 0


# ------------------------------------------------------------------------------------------------
# f. row counts
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q,n,k", [(1, 110, 10), (5, 110, 10), (1027, 110, 10), (9, 8193, 10), (33, 8193, 10), (7, 5000, 100)])
def test_row_counts(ctx, monkeypatch, Q, n, k):
    """register kernel with a last block of 1, 1 and 3 rows (Q = 1, 5, 1027); radix with Q > 8, where each row gets an eighth of
    the blocks; sort-all with one block per row.  Every row is drawn on its own and tied within itself, so a mixed-up row shows"""
    rng = np.random.default_rng(Q + n)
    scores = tied_scores(rng, Q, n)
    scores += np.arange(Q, dtype=np.float32)[:, None] * np.float32(0.25)
    check(ctx, scores, k, monkeypatch=monkeypatch)
    ids = np.stack([rng.permutation(4 * n)[:n] for _ in range(min(Q, 40))]).astype(np.int32)
    check(ctx, scores[: len(ids)], k, ids=ids, monkeypatch=monkeypatch)
