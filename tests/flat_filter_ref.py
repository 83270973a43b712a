"""References for the flat search's threshold filters (k_adc_mq.hip's FILTER epilogue, k_adc_bq.hip), shared by
tests/test_zz_flat_filter_gpu.py and tests/test_flat_filter_reference_cpu.py.  TEST HELPER, not a test module.

Three things live here:
  * the inputs of both test modules (problem, far_cluster_problem, thresholds);
  * BoundRef: the bound of k_adc_bq.hip restated in float64 from a query's float table, and `must_reject`: the pairs the bound
    scan has to drop whatever way its f32 roundings fall — the loosest bound the code allows still misses the cut;
  * a plain f32 numpy transcription of adc_bq_table_kernel and of adc_bq_kernel's reject tests (table_f32, survivors_f32), which
    the CPU test runs against the float64 restatement.

Margins of must_reject, derived from the code (k_adc_bq.hip), not measured:
  * the kernel's bucket of an entry is within one of b* = clip(floor((e - lo) / S), 0, 127): the truncated f32 quotient is within
    one of the real one and the +-2 corrections only undo f32 rounding of the edge test.  Over M subspaces: isum within M of isum*;
  * dot product / cosine bound the entry by the bucket's UPPER edge: M more buckets;
  * the integer threshold ceil(tf) + 1 / floor(tf) - 1 keeps up to 2 buckets beyond the real quotient, and one more bucket pays for
    the f32 rounding of tf, of the cut (1 / tau - 1 and 2 tau - 1 cancel near tau = 1: an absolute 2^-24) and of the base — each
    below 2^-22 of |cut| + 1 + |sum lo|, which `_conditioned` keeps under 1/4 of a bucket: 3 buckets;
  * the kernel's base carries one slack = 4e-5 sum_abs; the second slack covers the f32 sums of lo, of sum_abs and the bound itself;
  * cosine: twice the kernel's 8e-6 (|cc| + 1) covers the few-ulp rsq and the f32 product against float64 sqrt;
  * the kernel applies no bound when |tf| >= 1e9 (a degenerate scale, e.g. a constant table): nor does the reference (|tf| < 5e8).
"""
import numpy as np

from oracle import oracle as O

EUCLIDEAN, DOT, COSINE = 0, 1, 2
f32 = np.float32


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def problem(kind, seed, N, D, M, Q, centroid=False):
    """(vecs[N, D], queries[Q, D], codebooks, centroid | None): `clustered` unit vectors as in test_zz_flat_bq_gpu.problem, or a
    small-integer `grid` as in test_filtered_search_matches_oracle (massive score ties); codebooks sampled from the (centred) rows"""
    rng = np.random.default_rng(seed)
    if kind == "clustered":
        centers = rng.standard_normal((200, D)).astype(f32)
        vecs = (centers[rng.integers(0, 200, N)] + 0.35 * rng.standard_normal((N, D)).astype(f32)).astype(f32)
        vecs /= np.linalg.norm(vecs, axis=1, keepdims=True)
        queries = (vecs[rng.integers(0, N, Q)] + 0.05 * rng.standard_normal((Q, D))).astype(f32)
    else:
        vecs = np.round(rng.standard_normal((N, D)) * 2).astype(f32)
        vecs[vecs == 0] = 1.0
        queries = vecs[rng.integers(0, N, Q)].copy()
    c = vecs.mean(axis=0).astype(f32) if centroid else None
    src = vecs - c if centroid else vecs
    sizes, offs = O.subvector_sizes_offsets(D, M)
    pick = rng.choice(N, 256, replace=False)
    cb = np.concatenate([src[pick, offs[m]: offs[m] + sizes[m]].reshape(-1) for m in range(M)]).astype(f32)
    return vecs, queries, cb, c


def far_cluster_problem(seed, N, D, M, Q):
    """a tight cluster far from the origin: dot-product tables of about 8e8 that differ by a few thousand — the bound's scale is
    too coarse for its 4e-5 slack to mean anything and the table kernel switches it off (S * 1e6 < max |entry|)"""
    rng = np.random.default_rng(seed)
    vecs = (1e4 + 0.01 * rng.standard_normal((N, D))).astype(f32)
    queries = vecs[rng.integers(0, N, Q)].copy()
    sizes, offs = O.subvector_sizes_offsets(D, M)
    pick = rng.choice(N, 256, replace=False)
    cb = np.concatenate([vecs[pick, offs[m]: offs[m] + sizes[m]].reshape(-1) for m in range(M)]).astype(f32)
    return vecs, queries, cb, None


def no_bound_queries(queries):
    """the first three queries replaced by ones whose tables give the bound scan nothing to work with: a zero query (constant
    dot-product tables), a NaN component, a query scaled by 1e18 (squared distances of 1e36 whose differences drown)"""
    queries = queries.copy()
    queries[0] = 0.0
    queries[1, 7] = np.nan
    queries[2] *= f32(1e18)
    return queries


def duplicate_rows(codes, at=0):
    """two hundred equal rows: they tie exactly at every threshold they reach"""
    codes = codes.copy()
    codes[at: at + 200] = codes[at]
    return codes


KINDS = ("best", "rank2", "rank20", "rank20_up", "rank20_down", "rank500", "median", "last", "-inf", "+inf", "2.0", "nan")
KINDS_L2 = ("0.0", "1e-7")          # the two sides of euclidean's `tq > 1e-6` gate
STRENGTH_KINDS = ("rank2", "rank20", "rank20_up", "rank20_down", "rank500", "median")   # "ranked 2 ... median"


def kinds_for(vsf):
    return KINDS + (KINDS_L2 if int(vsf) == EUCLIDEAN else ())


def threshold(scores, kind):
    """one threshold of a query, taken from its exact scores"""
    fixed = {"-inf": -np.inf, "+inf": np.inf, "2.0": 2.0, "nan": np.nan, "0.0": 0.0, "1e-7": 1e-7}
    if kind in fixed:
        return f32(fixed[kind])
    s = np.sort(scores[scores == scores])[::-1]
    if s.size == 0:
        return f32(0.5)
    if kind == "median":
        return s[s.size // 2]
    if kind == "last":
        return s[-1]
    rank = {"best": 1, "rank2": 2, "rank20": 20, "rank20_up": 20, "rank20_down": 20, "rank500": 500}[kind]
    t = s[min(rank, s.size) - 1]
    if kind == "rank20_up":
        t = np.nextafter(t, f32(np.inf))
    if kind == "rank20_down":
        t = np.nextafter(t, f32(-np.inf))
    return f32(t)


def thresholds(scores, kind):
    """tau[Q] of one kind from scores[Q, N]"""
    return np.array([threshold(scores[q], kind) for q in range(scores.shape[0])], f32)


def passers(scores, tau):
    """bool[N]: score >= tau as the kernels compare it (false for a NaN on either side)"""
    with np.errstate(invalid="ignore"):
        return scores >= f32(tau)


def row_norms_f32(self_mag, codes):
    """the per-row decoded magnitude the cosine kernels stream: sum over m of self_mag[m, code[m]], f32, ascending m (k_adc.hip)"""
    M = codes.shape[1]
    t = np.asarray(self_mag, f32).reshape(M, 256)
    acc = np.zeros(codes.shape[0], f32)
    for m in range(M):
        acc = (acc + t[m, codes[:, m]]).astype(f32)
    return acc


# ---------------------------------------------------------------------------------------------------------------------
# the bound restated in float64
# ---------------------------------------------------------------------------------------------------------------------
class BoundRef:
    """the bound of one query's float table lut[M * 256] over codes[N, M], float64"""

    def __init__(self, lut, codes):
        self.N, M = codes.shape
        self.M = M
        t = np.asarray(lut, f32).reshape(M, 256).astype(np.float64)
        self.finite = bool(np.isfinite(t).all())
        if not self.finite:
            self.usable = False
            self.unusable = True
            return
        lo, hi = t.min(axis=1), t.max(axis=1)
        S = max(float((hi - lo).max()) / 127.0, 1e-30)
        a = np.maximum(np.abs(lo), np.abs(hi))
        self.lo, self.S = lo, S
        self.sum_lo = float(lo.sum())
        self.sum_abs = float((a + 128.0 * S).sum())
        self.slack = 4e-5 * self.sum_abs
        max_abs = float(a.max())
        # the table kernel's gate `S * 1e6f >= max_abs` (f32) and its finite f32 sum_abs: a factor 1.001 away on either side,
        # the reference knows which way the f32 test goes
        self.usable = S * 1e6 >= max_abs * 1.001 and self.sum_abs < 3e38
        self.unusable = S * 1e6 < max_abs * 0.999 or self.sum_abs > 3.5e38
        b = np.clip(np.floor((t - lo[:, None]) / S), 0, 127)
        self.isum = b[np.arange(M)[None, :], codes].sum(axis=1)          # isum*[N]

    def must_reject(self, vsf, tau, norms=None, bmag=None):
        """bool[N]: the rows the bound scan has to drop for threshold tau (all false where the reference does not know the
        bound to be in force)"""
        none = np.zeros(self.N, bool)
        tau = float(f32(tau))
        if not self.usable or tau != tau:
            return none
        S, M = self.S, self.M
        with np.errstate(all="ignore"):
            if vsf == EUCLIDEAN:
                if not tau > 1.001e-6:
                    return none
                cut = (1.0 / tau - 1.0) * 1.000002 + 4e-6
                tf = (cut - self.sum_lo) / S
                if not (self._conditioned(cut) and abs(tf) < 5e8):
                    return none
                return self.sum_lo - 2 * self.slack + S * (self.isum - M - 3) > cut
            x = 2.0 * tau - 1.0
            ub = self.sum_lo + 2 * self.slack + S * (self.isum + 2 * M + 3)
            if vsf == DOT:
                cut = x - 4e-6 * (abs(x) + 1.0)
                tf = (cut - self.sum_lo) / S - M
                if not (cut == cut and self._conditioned(cut) and abs(tf) < 5e8):
                    return none
                return ub < cut
            if not np.isfinite(x):
                return none
            prod = (np.asarray(norms, f32) * f32(bmag)).astype(f32).astype(np.float64)
            ok = (prod > 1.001e-30) & (prod < 0.999e30)
            cc = ub / np.sqrt(np.where(ok, prod, 1.0))
            return ok & (cc < x - 1.6e-5 * (np.abs(cc) + 1.0))

    def _conditioned(self, cut):
        """the f32 roundings of the cut, the base and their quotient stay below a quarter of a bucket"""
        return np.isfinite(cut) and (abs(cut) + 1.0 + abs(self.sum_lo) + self.slack) * 2.0 ** -22 <= 0.25 * self.S


# ---------------------------------------------------------------------------------------------------------------------
# k_adc_bq.hip in f32 numpy: adc_bq_table_kernel, and the reject tests of adc_bq_kernel
# ---------------------------------------------------------------------------------------------------------------------
def table_f32(vsf, lut, M):
    """-> (buckets uint8[M, 256], base f32, S f32, usable bool) as adc_bq_table_kernel writes them"""
    t = np.asarray(lut, f32).reshape(M, 256)
    with np.errstate(all="ignore"):
        bad = bool((~((t - t) == 0)).any())
        lo, hi = t.min(axis=1), t.max(axis=1)
        if bad:     # (min / max of a table with NaNs: the kernel's result is not specified and not used — the bound is off)
            return np.zeros((M, 256), np.uint8), f32(0), f32(1e-30), False
        rng = f32(0)
        for m in range(M):
            r = f32(hi[m] - lo[m])
            if r > rng:
                rng = r
        S = f32(rng / f32(127))
        if not S > f32(1e-30):
            S = f32(1e-30)
        sum_lo, sum_abs, max_abs = f32(0), f32(0), f32(0)
        for m in range(M):
            sum_lo = f32(sum_lo + lo[m])
            a = f32(max(abs(lo[m]), abs(hi[m])))
            sum_abs = f32(sum_abs + f32(a + f32(f32(128) * S)))
            if a > max_abs:
                max_abs = a
        ok = bool((sum_abs - sum_abs == 0) and f32(S * f32(1e6)) >= max_abs)
        slack = f32(f32(4e-5) * sum_abs)
        base = f32(sum_lo - slack) if vsf == EUCLIDEAN else f32(sum_lo + slack)
        inv = f32(f32(1) / S)
        l = lo[:, None]
        b = np.clip(((t - l).astype(f32) * inv).astype(f32), -1.0, 1e9).astype(np.int64)   # (int) of a non-negative float
        b = np.clip(b, 0, 127)
        edge = lambda k: (l + (S * k.astype(f32)).astype(f32)).astype(f32)   # noqa: E731
        if vsf == EUCLIDEAN:      # lower edge l + S b <= e
            for _ in range(2):
                b = np.where((b > 0) & (edge(b) > t), b - 1, b)
            b = np.where(edge(b) > t, 0, b)
        else:                     # upper edge l + S (b + 1) >= e
            for _ in range(2):
                b = np.where((b < 127) & (edge(b + 1) < t), b + 1, b)
            b = np.where(edge(b + 1) < t, 127, b)
    return b.astype(np.uint8), base, S, ok


def survivors_f32(vsf, tab, base, S, usable, codes, tau, norms=None, bmag=None):
    """bool[N]: the rows adc_bq_kernel keeps for threshold tau"""
    N, M = codes.shape
    keep = np.ones(N, bool)
    tq = f32(tau)
    with np.errstate(all="ignore"):
        on = usable and tq == tq
        if vsf == EUCLIDEAN:
            cut = f32(f32(f32(f32(1) / tq) - f32(1)) * f32(1.000002)) + f32(4e-6)
            cut = f32(cut)
            on = on and tq > f32(1e-6)
        elif vsf == DOT:
            x = f32(f32(2) * tq - f32(1))
            cut = f32(x - f32(f32(4e-6) * f32(abs(x) + f32(1))))
        else:
            cut = f32(f32(2) * tq - f32(1))
        if not on:
            return keep
        isum = tab.astype(np.int64)[np.arange(M)[None, :], codes].sum(axis=1)
        assert isum.max() <= 0xFFFF            # the kernel's 16-bit lanes
        if vsf != COSINE:
            tf = f32(f32(f32(cut - base) / S) - (f32(M) if vsf == DOT else f32(0)))
            if not (tf == tf and abs(tf) < f32(1e9)):
                return keep
            if vsf == EUCLIDEAN:
                return ~(isum >= int(np.ceil(tf)) + 1)
            return ~(isum <= int(np.floor(tf)) - 1)
        ub = (base + (S * (isum.astype(f32) + f32(M)).astype(f32)).astype(f32)).astype(f32)
        prod = (np.asarray(norms, f32) * f32(bmag)).astype(f32)
        rsq = (1.0 / np.sqrt(prod.astype(np.float64))).astype(f32)      # v_rsq_f32 is within an ulp of this
        cc = (ub * rsq).astype(f32)
        rhs = (cut - (f32(8e-6) * (np.abs(cc) + f32(1)).astype(f32)).astype(f32)).astype(f32)
        reject = (prod > f32(1e-30)) & (prod < f32(1e30)) & (cc < rhs)
    return ~reject
