"""The flat search's threshold filters at the threshold itself.  jv_hip_search_flat rests on one promise of both filters — the
single-stage exact one (adc_mq_kernel<..., FILTER>, k_adc_mq.hip) and the two-stage one (adc_bq_table_kernel, adc_bq_kernel, the
exact gather and adc_bq_count_kernel, k_adc_bq.hip): a query's candidate list holds EVERY row whose exact ADC score is >= the
query's threshold, with exact scores.  Through the search only the best k1 of about 3 k1 candidates are ever compared, so a filter
that loses rows just above the threshold goes unseen.  Here the filters run through jv_hip_adc_filter with thresholds taken from
the oracle's exact scores — the best score, ranks 2 / 20 / 500, the median, the last, the neighbours of the rank-20 score, +-inf,
2.0, NaN, euclidean's 1e-6 gate — over rows that tie two hundred at a time, and are checked against the oracle:

  stages 1   the ids are exactly {first + i : score >= tau}, no duplicates, scores bit-equal, the count the set's size;
  stages 2   soundness: the ids contain that set, are distinct and in range, scores bit-equal, the second count = #{score >= tau},
             slots behind the count untouched;
             strength: no pair that the bound MUST reject (tests/flat_filter_ref.py: the bound restated in float64, with the
             loosest margins the code allows) is among the survivors — and must-reject covers at least half of the pairs below
             the thresholds ranked 2 ... median, so the condition bites;
  queries without a usable bound keep every row.

Shapes: the smallest that reach each branch of the launchers on a 256-CU device — SLCH 1 / 2, two LDS slices per pass, R = 4 / 8,
the XCD tile order with a T % 8 tail and the plain order, more than 32 query groups, first != 0, LDS staging overflow, the exact
filter's staged / unstaged forms, lists that outgrow cap.  Each case prints the must-reject coverage and the survivor excess
(survivors / passers) it saw; they are recorded, not asserted."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import jvector_amd as J
from jvector_amd import VectorSimilarityFunction as VSF
from oracle import oracle as O

import flat_filter_ref as R

ALL = None   # every threshold kind of the similarity function


@pytest.fixture(scope="module")
def ctx():
    c = J.HipContext(0)
    yield c
    c.close()


class Case:
    """one input on the device: quantizer, duplicated code rows, the oracle's twin"""

    def __init__(self, ctx, kind, seed, N, M, Q, centroid=False, dup_at=0, queries=None):
        D = 8 * M
        gen = R.far_cluster_problem(seed, N, D, M, Q) if kind == "far" else R.problem(kind, seed, N, D, M, Q, centroid)
        vecs, self.queries, cb, c = gen
        if queries is not None:
            self.queries = queries(self.queries)
        self.pq = J.ProductQuantization.from_codebooks(ctx, D, M, cb, c)
        self.opq = O.OraclePQ(D, M, cb, c)
        vs = J.VectorSet(ctx, vecs)
        cv = J.PQVectors.encode_and_build(ctx, self.pq, vs)
        self.codes = R.duplicate_rows(cv.get(0, N), dup_at)
        cv.close()
        vs.close()
        self.cv = J.PQVectors(ctx, self.pq, self.codes)
        self.N, self.M, self.Q = N, M, Q


@pytest.fixture(scope="module")
def case(ctx):
    @functools.lru_cache(maxsize=2)      # (the three similarity functions of a shape run back to back)
    def get(*a, **kw):
        return Case(ctx, *a, **kw)
    return get


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_scores(got, want):
    return np.array_equal(bits(got), bits(want)) or np.array_equal(got, want, equal_nan=True)


class Stats:
    def __init__(self):
        self.covered = self.below = self.survivors = self.passers = 0


def run(c, vsf, first, count, kinds=ALL, cap=None, stages=(1, 2), sample=None, coverage=False, label="", mixed=None):
    """run the filters over rows [first, first + count) for every threshold kind and check the sampled queries against the oracle.
    Returns {(stages, kind): [sorted written ids of each sampled query]}.  mixed: (kinds, filler) — ONE call whose sampled queries
    cycle through the kinds while every other query gets the filler threshold."""
    Q = c.Q
    cap = count if cap is None else cap
    sample = list(range(Q)) if sample is None else list(sample)
    rows = c.codes[first: first + count]
    sf = c.cv.precomputed_score_function_for(c.queries, vsf)
    scores = np.stack([c.opq.adc_scores(c.queries[q], int(vsf), rows) for q in sample])
    norms = R.row_norms_f32(c.pq.self_magnitudes(), rows) if vsf == VSF.COSINE else None
    refs = {}
    if 2 in stages:
        for q in sample:
            lut, bm = sf.luts.table(q)
            refs[q] = (R.BoundRef(lut, rows), bm)
    st, out = Stats(), {}
    plan = []
    if mixed is not None:
        mk, filler = mixed
        tau = np.full(Q, filler, np.float32)
        for j, q in enumerate(sample):
            tau[q] = R.threshold(scores[j], mk[j % len(mk)])
        plan.append(("+".join(mk), tau, True))
    else:
        for kind in (R.kinds_for(vsf) if kinds is ALL else kinds):
            ts = R.thresholds(scores, kind)
            tau = ts[np.arange(Q) % len(sample)]          # the other queries borrow a sampled query's threshold
            tau[sample] = ts
            plan.append((kind, tau, kind in R.STRENGTH_KINDS))
    for kind, tau, strength in plan:
        for stage in stages:
            ids, sc, counts = sf.threshold_filter(first, count, tau, stage, cap)
            written = []
            for j, q in enumerate(sample):
                what = (label, vsf.name, "stages", stage, kind, "query", q, "tau", float(tau[q]))
                P = R.passers(scores[j], tau[q])
                want = (np.flatnonzero(P) + first).astype(np.int32)
                n = int(counts[0, q])
                w = min(n, cap)
                got = ids[q, :w]
                assert (got >= first).all() and (got < first + count).all(), what
                assert np.unique(got).size == w, ("duplicate ids",) + what
                assert same_scores(sc[q, :w], scores[j][got - first]), ("scores differ from the oracle",) + what
                assert (ids[q, w:] == -1).all() and (sc[q, w:] == -np.inf).all(), ("slots behind the count were written",) + what
                if stage == 1:
                    assert n == want.size, ("count", n, want.size) + what
                    if tau[q] != tau[q]:
                        assert n == 0, what
                    if n <= cap:
                        assert np.array_equal(np.sort(got), want), ("not the passing set",) + what
                    else:
                        assert np.isin(got, want).all(), ("a written id does not pass",) + what
                else:
                    ref, bm = refs[q]
                    if n <= cap:
                        assert np.isin(want, got).all(), ("a passer was dropped", int((~np.isin(want, got)).sum())) + what
                        assert int(counts[1, q]) == want.size, ("second count", int(counts[1, q]), want.size) + what
                    else:
                        assert int(counts[1, q]) == int(R.passers(sc[q, :w], tau[q]).sum()), ("second count",) + what
                    if ref.unusable:
                        assert n == count, ("no usable bound, yet rows were dropped", n, count) + what
                    mr = ref.must_reject(int(vsf), tau[q], norms, bm)
                    assert not mr[got - first].any(), ("a must-reject pair survived", int(mr[got - first].sum())) + what
                    if strength:
                        st.covered += int(mr.sum())
                        st.below += int((~P).sum())
                        st.survivors += n
                        st.passers += int(want.size)
                written.append(np.sort(got))
            out[(stage, kind)] = written
    if 2 in stages and st.below:
        print(f"[flat filter] {label} {vsf.name}: must-reject coverage {st.covered / st.below:.3f}, "
              f"survivors / passers {st.survivors / max(st.passers, 1):.2f} ({st.survivors} / {st.passers})")
        if coverage:
            assert 2 * st.covered >= st.below, ("the must-reject condition does not bite", label, vsf.name, st.covered, st.below)
    return out


@pytest.mark.parametrize("vsf", list(VSF))
@pytest.mark.parametrize("kind,centroid", [("clustered", False), ("clustered", True), ("grid", False), ("grid", True)])
def test_every_threshold_pq16(case, kind, centroid, vsf):
    """SLCH = 1, a ragged last tile, Q % 16 and Q % 4 != 0"""
    c = case(kind, 16, 9000, 16, 37, centroid)
    run(c, vsf, 0, 9000, coverage=True, label=f"M16 Q37 N9000 {kind}{' centroid' if centroid else ''}")


@pytest.mark.parametrize("vsf", list(VSF))
@pytest.mark.parametrize("kind,M,N,Q", [("clustered", 32, 9000, 20), ("clustered", 96, 9000, 20), ("grid", 96, 9000, 20), ("grid", 192, 5000, 5)])
def test_every_threshold_wide_pq(case, kind, M, N, Q, vsf):
    """SLCH = 2 (M 32, 96); M 192: two LDS slices per pass, 16-bit bucket sums near their top"""
    c = case(kind, M, N, M, Q)
    run(c, vsf, 0, N, sample=range(0, Q, 2) if M == 96 else None, coverage=True, label=f"M{M} Q{Q} N{N} {kind}")


@pytest.mark.parametrize("vsf", list(VSF))
def test_range_that_does_not_start_at_row_zero(case, vsf):
    c = case("clustered", 3, 13000, 16, 17, dup_at=5000)
    run(c, vsf, 4099, 8200, label="M16 Q17 rows 4099+8200")


@pytest.mark.parametrize("vsf", list(VSF))
def test_xcd_tile_order_with_a_tail_equals_the_plain_order(case, vsf, monkeypatch):
    """T = 11 tiles of 4096 rows: eight in the XCD order, a tail of three in the plain one"""
    c = case("clustered", 4, 10 * 4096 + 5, 16, 33)
    kinds = ("rank2", "rank20", "rank20_down", "rank500", "median", "-inf")
    a = run(c, vsf, 0, c.N, kinds=kinds, stages=(2,), label="M16 Q33 T11 xcd order")
    monkeypatch.setenv("JVECTOR_HIP_ADC_BQ_PLAIN_ORDER", "1")
    b = run(c, vsf, 0, c.N, kinds=kinds, stages=(2,), label="M16 Q33 T11 plain order")
    for key in a:
        assert all(np.array_equal(x, y) for x, y in zip(a[key], b[key])), (vsf, key)


def spread(Q, n=24):
    """sampled queries: the first and the last group of sixteen whole or in part, the rest spread out"""
    return sorted(set([0, 1, 5, 15, 16, Q - 17, Q - 16, Q - 2, Q - 1] + list(range(37, Q - 17, max(1, Q // (n - 9))))))[:n + 4]


@pytest.mark.parametrize("vsf", list(VSF))
def test_eight_rows_per_lane_and_many_query_groups(case, vsf):
    """Q = 1024 over seven tiles of 8192 rows + 5: R = 8, 64 bound-scan groups (plain order), 256 exact-filter groups"""
    c = case("clustered", 7, 7 * 8192 + 5, 16, 1024)
    run(c, vsf, 0, c.N, kinds=("best", "rank20", "rank20_up", "rank500", "nan"), cap=16384, sample=spread(1024), label="M16 Q1024 R8")


@pytest.mark.parametrize("vsf", list(VSF))
def test_eight_rows_per_lane_in_the_xcd_order(case, vsf):
    """Q = 512 over sixteen tiles of 8192 rows + 5: R = 8 with the XCD order on (32 groups) and a tail tile"""
    c = case("clustered", 8, 16 * 8192 + 5, 16, 512)
    run(c, vsf, 0, c.N, kinds=("rank2", "rank20", "rank500"), cap=16384, sample=spread(512), label="M16 Q512 R8 xcd order")


@pytest.mark.parametrize("vsf", list(VSF))
def test_staging_overflow_four_rows_per_lane(case, vsf):
    """a workgroup's 4096 rows against its LDS staging area of 1024 (bound scan) / 2048 (exact filter) entries per query"""
    c = case("clustered", 16, 9000, 16, 37, False)
    run(c, vsf, 0, 9000, kinds=("median", "-inf"), label="M16 staging overflow R4")


@pytest.mark.parametrize("vsf", list(VSF))
def test_staging_overflow_eight_rows_per_lane(case, vsf):
    """M 32 (SLCH 2: 2048 / 4096 entries) at the R = 8 shape, 8192 rows per workgroup; the sampled queries take the median and
    -inf, the others a threshold nothing reaches, and the lists hold every row"""
    c = case("clustered", 9, 7 * 8192 + 5, 32, 1024)
    run(c, vsf, 0, c.N, sample=spread(1024, 12), mixed=(("median", "-inf"), 2.0), label="M32 Q1024 staging overflow R8")


@pytest.mark.parametrize("vsf", list(VSF))
def test_exact_filter_staged_and_unstaged(case, vsf, monkeypatch):
    """cap 64 over 9000 rows: fewer than 16 expected survivors per workgroup, no staging; cap = count: staged; and staging off"""
    c = case("clustered", 10, 9000, 16, 8)
    kinds = ("best", "rank2", "rank20", "rank20_up", "rank20_down", "rank500", "median", "nan")
    a = run(c, vsf, 0, 9000, kinds=kinds, cap=64, stages=(1,), label="cap 64")
    b = run(c, vsf, 0, 9000, kinds=kinds, stages=(1,), label="cap = count")
    monkeypatch.setenv("JVECTOR_HIP_ADC_NO_STAGING", "1")
    d = run(c, vsf, 0, 9000, kinds=kinds, stages=(1,), label="staging off")
    for key in b:
        assert all(np.array_equal(x, y) for x, y in zip(b[key], d[key])), (vsf, key)
    for key in (k for k in a if k[1] in ("best", "rank2")):      # (short enough for cap 64 unless they tie with the duplicates)
        assert all(np.array_equal(x, y) for x, y in zip(a[key], b[key]) if y.size <= 64), (vsf, key)


@pytest.mark.parametrize("vsf", list(VSF))
def test_list_outgrows_cap(case, vsf):
    """cap 128, tau = the median: the count is the true total, the 128 written are distinct members of the passing set (stages 2:
    distinct rows of the range with exact scores, none of them a must-reject pair)"""
    c = case("clustered", 10, 9000, 16, 8)
    out = run(c, vsf, 0, 9000, kinds=("median",), cap=128, label="cap 128")
    assert all(x.size == 128 for key in out for x in out[key])


@pytest.mark.parametrize("vsf", list(VSF))
def test_queries_without_a_usable_bound_keep_every_row(case, vsf):
    """a zero query, a NaN component, a query scaled by 1e18; and a tight cluster far from the origin.  Where the table kernel has
    to switch the bound off (the reference says where: a NaN table for every function, the scaled query for euclidean, the far
    cluster for dot product and cosine) stages 2 keeps every row; everywhere nothing is lost."""
    kinds = ("best", "rank20", "median", "last", "+inf", "nan")
    c = case("clustered", 5, 9000, 16, 37, queries=R.no_bound_queries)
    run(c, vsf, 0, 9000, kinds=kinds, sample=range(8), label="no-bound queries")
    c = case("far", 6, 9000, 16, 37)
    run(c, vsf, 0, 9000, kinds=kinds, sample=range(4), label="far cluster")
