"""Inputs for the PQ encode kernels at their edges (k_pq.hip: pq_encode_sgpr_kernel, pq_encode_kernel, pq_encode_generic_kernel),
shared by tests/test_pq_edge_cases_cpu.py (the inputs do what they claim, oracle only) and tests/test_zz_pq_encode_edges_gpu.py
(kernel == oracle on them).  TEST HELPER, not a test module; numpy only.

Every generator returns (D, M, codebooks, centroid, vectors) for a sub-vector size S with M = 3 and D = 3 S — so that blockIdx.y,
offsets[m] and the per-subspace codebook offset all matter — or, with `sizes=`, for any split (the non-uniform D = 10, M = 3 is
sizes (4, 3, 3)).  `codebooks` is the concatenation over m of 256 * size_m floats, centroid-major; every subspace has rows of its own.

  random     Gaussian everything; n chooses the block shape (1, 255, 256, 257, 600)
  ties       small integers: every distance is exact.  Duplicate rows at TIE_PAIRS, rows 2 apart in one coordinate at HALF_PAIRS;
             vectors equal to a duplicated row (distance 0 at both) or half way between a HALF pair (distance 1 at both)
  nonfinite  NaN rows (a whole block of eight, row 0, the neighbours of planted winners), a +Inf row, NaN / Inf / 1e20 vectors
  overflow   every row -1e20, vectors 1e20 and Gaussian: every sum is +Inf, nothing beats Float.MAX_VALUE, the code stays 0
  survivor   every row -1e20 except SURVIVOR: the code is SURVIVOR
  subnormal  Gaussian scaled by 2^-e: the winning sums are non-zero f32 subnormals
"""
import numpy as np

f32 = np.float32
K = 256
M = 3

SIZES = (1, 2, 3, 4, 5, 6, 8, 12, 16)
RANDOM_COUNTS = (1, 255, 256, 257, 600)   # one thread, a block minus one, a block, a tail of one, blocks and a tail

# duplicate rows: the halves of a packed pair, both sides of a boundary between blocks of eight (twice), far apart (twice)
TIE_PAIRS = ((2, 3), (7, 8), (15, 16), (0, 255), (5, 250))
# distinct rows at the same non-zero distance: a packed pair, a block boundary, far apart, another block boundary
HALF_PAIRS = ((20, 21), (39, 40), (1, 254), (63, 64))

NAN_BLOCK = tuple(range(8, 16))
WINNERS = (100, 45)                       # planted winners: the x half of pair 50, the y half of pair 22
NAN_ROWS = NAN_BLOCK + (0, 99, 101, 44, 46)
INF_ROW = 200
SURVIVOR = 201
# rows of nonfinite()'s vectors, in order: N_PLAIN Gaussian, then per winner N_EACH vectors at that winner, then per subspace
# N_EACH with a NaN in that subspace only, N_EACH with an Inf component in one subspace, N_EACH of 1e20 in one subspace
N_PLAIN, N_EACH = 300, 6


def _sizes(S, sizes):
    return [int(S)] * M if sizes is None else [int(s) for s in sizes]


def _pack(rows):
    return np.concatenate([r.reshape(-1) for r in rows]).astype(f32)


def split(vectors, sizes):
    offs = np.concatenate([[0], np.cumsum(sizes)])
    return [vectors[:, offs[m]: offs[m + 1]] for m in range(len(sizes))]


def random(S, n, centroid=True, seed=0, sizes=None):
    sizes = _sizes(S, sizes)
    D = sum(sizes)
    rng = np.random.default_rng(1000 * D + n + seed)
    cb = _pack([rng.standard_normal((K, s)) for s in sizes])
    cen = (0.1 * rng.standard_normal(D)).astype(f32) if centroid else None
    return D, len(sizes), cb, cen, rng.standard_normal((n, D)).astype(f32)


# ---------------------------------------------------------------------------------------------------------------------
# ties
# ---------------------------------------------------------------------------------------------------------------------
def _lattice(rng, s):
    return rng.integers(-4, 5, s)


def _tie_subspace(rng, s):
    """-> (rows[256, s], specials): integer rows in [-4, 4].  Row values at TIE_PAIRS occur at those two indices only; a HALF pair is
    (L, L + 2 e_j) with the midpoint — and every lattice point next to it but the two ends — absent from the codebook, so the
    midpoint's minimum distance is exactly 1, at exactly those two rows.  One coordinate has 9 values: there one HALF pair, and all
    the other rows share the one value left."""
    halves = HALF_PAIRS if s > 1 else HALF_PAIRS[:1]
    near = lambda p, q: int(np.abs(p - q).sum()) <= 1   # lattice points: squared distance <= 1
    while True:                                          # (s = 1 can paint itself into a corner: draw again)
        mids, ends, planted = [], [], []
        ok = True
        for _ in halves:
            for _try in range(1000):
                j = int(rng.integers(0, s))
                lo = _lattice(rng, s)
                lo[j] = rng.integers(-4, 3)
                hi, mid = lo.copy(), lo.copy()
                hi[j] += 2
                mid[j] += 1
                if any(near(e, mid) for e in ends) or any(near(lo, m) or near(hi, m) for m in mids):
                    continue
                if any(np.array_equal(e, x) for e in ends for x in (lo, hi)):
                    continue
                mids.append(mid), ends.extend([lo, hi])
                break
            else:
                ok = False
        for _ in TIE_PAIRS:
            for _try in range(1000):
                p = _lattice(rng, s)
                if any(near(p, m) for m in mids) or any(np.array_equal(p, x) for x in ends + planted):
                    continue
                planted.append(p)
                break
            else:
                ok = False
        if not ok:
            continue
        rows = np.empty((K, s), np.int64)
        fill_ok = True
        for i in range(K):
            for _try in range(1000):
                p = _lattice(rng, s)
                if any(near(p, m) for m in mids) or any(np.array_equal(p, x) for x in ends + planted):
                    continue
                rows[i] = p
                break
            else:
                fill_ok = False
        if not fill_ok:
            continue
        for (a, b), p in zip(TIE_PAIRS, planted):
            rows[a] = rows[b] = p
        for t, (a, b) in enumerate(halves):
            rows[a], rows[b] = (ends[2 * t], ends[2 * t + 1]) if t % 2 == 0 else (ends[2 * t + 1], ends[2 * t])
        return rows, planted + mids


def ties(S, seed=0, n=240, sizes=None):
    sizes = _sizes(S, sizes)
    D = sum(sizes)
    rng = np.random.default_rng(77 * D + seed)
    subs = [_tie_subspace(rng, s) for s in sizes]
    cen = rng.integers(-1, 2, D).astype(f32)
    v = np.empty((n, D), f32)
    off = 0
    for s, (rows, specials) in zip(sizes, subs):
        ns = len(specials)
        for i in range(n):
            if i < 2 * ns:
                sub = specials[i % ns]                    # every special in every subspace, whatever the draws below give
            else:
                c = int(rng.integers(0, ns + 3))
                sub = specials[c] if c < ns else _lattice(rng, s)
            v[i, off: off + s] = sub
        off += s
    return D, len(sizes), _pack([rows for rows, _ in subs]), cen, (v + cen).astype(f32)   # small integers: the sum is exact


# ---------------------------------------------------------------------------------------------------------------------
# NaN, Inf, overflow
# ---------------------------------------------------------------------------------------------------------------------
def nonfinite(S, seed=0, sizes=None):
    sizes = _sizes(S, sizes)
    D, Ms = sum(sizes), len(sizes)
    rng = np.random.default_rng(55 * D + seed)
    rows = [rng.standard_normal((K, s)).astype(f32) for s in sizes]
    clean = [r.copy() for r in rows]
    for m, r in enumerate(rows):
        for t, i in enumerate(NAN_ROWS):
            if (t + m) % 2:
                r[i, :] = np.nan                           # the whole row
            else:
                r[i, (t + m) % r.shape[1]] = np.nan        # one component
        r[INF_ROW, m % r.shape[1]] = np.inf
    cen = (0.1 * rng.standard_normal(D)).astype(f32)
    n = N_PLAIN + N_EACH * (len(WINNERS) + 3 * Ms)
    v = rng.standard_normal((n, D)).astype(f32)
    offs = np.concatenate([[0], np.cumsum(sizes)])
    at = N_PLAIN
    for w in WINNERS:                                      # sub-vector m == row w of codebook m (up to the centring's rounding)
        for m in range(Ms):
            v[at: at + N_EACH, offs[m]: offs[m + 1]] = clean[m][w] + cen[offs[m]: offs[m + 1]]
        at += N_EACH
    for bad in (np.nan, np.inf, 1e20):
        for m in range(Ms):
            for i in range(N_EACH):
                if bad == 1e20:
                    v[at + i, offs[m]: offs[m + 1]] = 1e20   # (1e20 - c)^2 > Float.MAX_VALUE in every coordinate
                else:
                    v[at + i, offs[m] + i % sizes[m]] = bad
            at += N_EACH
    assert at == n
    return D, Ms, _pack(rows), cen, v


def nonfinite_bad_subspace(Ms=M):
    """-> bad[n] : the subspace of row i of nonfinite()'s vectors that holds NaN / Inf / 1e20, or -1"""
    bad = np.full(N_PLAIN + N_EACH * (len(WINNERS) + 3 * Ms), -1)
    at = N_PLAIN + N_EACH * len(WINNERS)
    for _ in range(3):
        for m in range(Ms):
            bad[at: at + N_EACH] = m
            at += N_EACH
    return bad


def nonfinite_winner_rows():
    """-> [(winner, slice of nonfinite()'s vectors planted at it)]"""
    return [(w, slice(N_PLAIN + t * N_EACH, N_PLAIN + (t + 1) * N_EACH)) for t, w in enumerate(WINNERS)]


def overflow(S, seed=0, sizes=None):
    sizes = _sizes(S, sizes)
    D = sum(sizes)
    rng = np.random.default_rng(66 * D + seed)
    cb = np.full(K * D, -1e20, f32)
    v = rng.standard_normal((40, D)).astype(f32)
    v[:20] = 1e20
    return D, len(sizes), cb, (0.1 * rng.standard_normal(D)).astype(f32), v


def survivor(S, seed=0, sizes=None):
    sizes = _sizes(S, sizes)
    D = sum(sizes)
    rng = np.random.default_rng(88 * D + seed)
    rows = [np.full((K, s), -1e20, f32) for s in sizes]
    for r in rows:
        r[SURVIVOR] = rng.standard_normal(r.shape[1])
    return D, len(sizes), _pack(rows), (0.1 * rng.standard_normal(D)).astype(f32), rng.standard_normal((40, D)).astype(f32)


# ---------------------------------------------------------------------------------------------------------------------
# subnormal sums
# ---------------------------------------------------------------------------------------------------------------------
def subnormal_exponent(s):
    """Gaussian * 2^-e.  A squared difference d^2 2^-2e is a non-zero f32 subnormal for 2^-149 <= d^2 2^-2e < 2^-126.  The distance
    that decides the code is the one to the NEAREST of 256 Gaussian rows, d^2 ~ 2^-16 in one dimension, 2^-6 in two, 2^-3 in three
    and 1..2^5 from four on — so the exponent follows the size"""
    return {1: 60, 2: 66, 3: 68}.get(int(s), 72)


def subnormal(S, seed=0, n=1000, sizes=None):
    sizes = _sizes(S, sizes)
    D = sum(sizes)
    rng = np.random.default_rng(99 * D + seed)
    scale = f32(2.0) ** f32(-subnormal_exponent(min(sizes)))
    cb = _pack([rng.standard_normal((K, s)) for s in sizes]) * scale
    cen = (0.1 * rng.standard_normal(D)).astype(f32) * scale
    return D, len(sizes), cb, cen, rng.standard_normal((n, D)).astype(f32) * scale


# ---------------------------------------------------------------------------------------------------------------------
# fewer than 256 clusters
# ---------------------------------------------------------------------------------------------------------------------
def small_k(S, k, seed=0, n=200):
    """-> (D, M, codebooks[k rows per subspace], None, vectors): integer rows, all distinct within a subspace; the vectors are decoded
    code words whose sub-vector 0 is centroid 0 — at distance 0 from centroid 0 AND from each of its 256 - k padded copies on the
    device, which must never be chosen"""
    sizes = [int(S)] * M
    D = sum(sizes)
    rng = np.random.default_rng(11 * D + k + seed)
    rows = []
    for s in sizes:
        r = np.empty((k, s), np.int64)
        r[:, 0] = rng.permutation(k) - k // 2             # distinct rows
        r[:, 1:] = rng.integers(-4, 5, (k, s - 1))
        rows.append(r)
    codes = rng.integers(0, k, (n, M))
    codes[:, 0] = 0
    codes[: n // 4, :] = 0
    v = np.concatenate([rows[m][codes[:, m]] for m in range(M)], axis=1).astype(f32)
    return D, M, _pack(rows), None, v


def f32_distances(sub, rows):
    """squareL2Distance of every sub-vector to every row in f32, the coordinates added in ascending order like the reference's
    scalar loop: -> [n, 256] float32"""
    acc = np.zeros((sub.shape[0], rows.shape[0]), f32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for j in range(sub.shape[1]):
            d = (sub[:, j: j + 1] - rows[None, :, j]).astype(f32)
            acc = (acc + (d * d).astype(f32)).astype(f32)
    return acc
