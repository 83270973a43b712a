"""The flat PQ search under an accept filter on the MI355X (jv_hip_search_flat_filtered) against its two baselines, alternated point by
point in one run: the unfiltered jv_hip_search_flat (what a caller pays who ignores the filter and post-filters), and the four-call
composition a caller had to write before this call existed — jv_hip_adc_scores over a Q x B ordinal matrix, jv_hip_topk,
jv_hip_exact_scores, jv_hip_topk — with the ordinal matrix already built and resident on the device (the host work of building it
from the bitmap is NOT in its time: the comparison leans toward the baseline).  Selectivities 0.1 %, 1 %, 10 %, 100 %, one shared mask
and one mask per query.  Seeded synthetic data (benchlib.Mixture, unit vectors).  Every shape is warmed up first; a point is timed for
several hundred milliseconds with a device synchronise inside the clock.  One JSON object per point on stdout, then a summary line.

Algorithmic bytes of the list kernel at a point: n_acc (M + 4) per group of four queries (code row + list entry) plus 4 Q n_acc of
scores.  Their share of the HBM peak needs the kernel's own time: run the script under `rocprofv3 --kernel-trace --stats` with
--only filtered and read adc_mq_list_kernel (shared masks) / adc_kernel (per-query masks) from the stats.
usage: python scripts/flat_filtered_bench.py [N=1048576] [D=128] [M=16] [--q 256] [--ms 300] [--only filtered] [--no-compose-above B]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import benchlib
import jvector_amd as J
from jvector_amd import VectorSimilarityFunction as VSF


def flag(name, dflt):
    return type(dflt)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else dflt


pos = []
skip = False
for a in sys.argv[1:]:
    if skip:
        skip = False
    elif a.startswith("--"):
        skip = True
    else:
        pos.append(a)
N = int(pos[0]) if len(pos) > 0 else 1 << 20
D = int(pos[1]) if len(pos) > 1 else 128
M = int(pos[2]) if len(pos) > 2 else 16
Q, MS, ONLY = flag("--q", 256), flag("--ms", 300), flag("--only", "")
COMPOSE_MAX_B = flag("--no-compose-above", 1 << 21)     # the composition's Q x B ordinal and score matrices: 8 Q B bytes
K, RK = 10, 100
HBM_PEAK = 8.0e12                                        # bytes / s, the MI355X's stated HBM3E peak
SELECTIVITIES = (0.001, 0.01, 0.1, 1.0)

dev = torch.device("cuda:0")
ctx = J.HipContext(0)
mix = benchlib.Mixture(D, 1, dev)
base = mix.sample(N, 2)
queries = mix.sample(Q, 3)
vs = J.VectorSet(ctx, base)
pq = J.ProductQuantization.from_codebooks(ctx, D, M, benchlib.train_codebooks(base, M, 5))
cv = J.PQVectors.encode_and_build(ctx, pq, vs)
fs = J.FlatSearcher(ctx, pq, cv, vs, max_queries=Q)
luts = J.QueryTables(ctx, pq, Q)
vsf = VSF.DOT_PRODUCT


def timed(fn):
    """seconds per call: warm-up, then whole calls until MS milliseconds have passed, the device synchronised inside the clock"""
    fn()
    ctx.sync()
    torch.cuda.synchronize()
    reps, t0 = 0, time.perf_counter()
    while True:
        fn()
        ctx.sync()
        torch.cuda.synchronize()
        reps += 1
        dt = time.perf_counter() - t0
        if dt * 1e3 >= MS:
            return dt / reps, reps


def compose(ords):
    sf = cv.precomputed_score_function_for(queries, vsf, luts)
    sc = sf.similarity_to(ords)
    ids1, _ = J.topk(ctx, sc, RK, ids=ords)
    ex = vs.scores(queries, vsf, ids1)
    return J.topk(ctx, ex, K, ids=ids1)


gen = torch.Generator(device=dev).manual_seed(7)
SHIFTS = torch.arange(64, device=dev, dtype=torch.int64)


def device_mask(sel):
    """(bool [N] on the device, its packed words as int64 [ceil(N / 64)]): bit n of word n // 64 <-> row n"""
    m = torch.rand(N, generator=gen, device=dev) < sel if sel < 1.0 else torch.ones(N, dtype=torch.bool, device=dev)
    padded = torch.zeros((N + 63) // 64 * 64, dtype=torch.int64, device=dev)
    padded[:N] = m
    return m, (padded.view(-1, 64) << SHIFTS).sum(dim=1)


points = []
for per_query in (False, True):
    for sel in SELECTIVITIES:
        rows = [device_mask(sel) for _ in range(Q if per_query else 1)]
        lists = [torch.nonzero(m).flatten().to(torch.int32) for m, _ in rows]
        counts = np.array([len(l) for l in lists] * (1 if per_query else Q))
        words = torch.stack([w for _, w in rows]).contiguous() if per_query else rows[0][1]
        del rows
        n_acc = float(counts.mean())
        B = int(counts.max())
        pt = {"n": N, "dim": D, "M": M, "Q": Q, "topK": K, "rerankK": RK, "masks": "per-query" if per_query else "shared", "selectivity": sel,
              "accepted_mean": n_acc}
        t, reps = timed(lambda: fs.search_filtered(queries, vsf, K, RK, words))
        pt["filtered_ms"], pt["filtered_reps"] = t * 1e3, reps
        groups = (Q + 3) // 4
        pt["list_kernel_algorithmic_bytes"] = (groups * n_acc * (M + 4) + 4.0 * Q * n_acc) if not per_query else (Q * n_acc * (M + 4) + 4.0 * Q * n_acc)
        pt["algorithmic_bytes_over_call_time_share_of_hbm_peak"] = pt["list_kernel_algorithmic_bytes"] / t / HBM_PEAK
        if ONLY != "filtered":
            t, reps = timed(lambda: fs.search(queries, vsf, K, RK))
            pt["unfiltered_ms"], pt["unfiltered_reps"] = t * 1e3, reps
            if B <= COMPOSE_MAX_B and B > 0:
                d_ords = torch.full((Q, B), -1, dtype=torch.int32, device=dev)
                for q in range(Q):
                    l = lists[q if per_query else 0]
                    d_ords[q, :len(l)] = l
                got, want = compose(d_ords), fs.search_filtered(queries, vsf, K, RK, words)
                pt["composition_equals_filtered"] = bool(torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]))
                t, reps = timed(lambda: compose(d_ords))
                pt["composition_ms"], pt["composition_reps"] = t * 1e3, reps
                del d_ords
            else:
                pt["composition_ms"] = None
                pt["composition_skipped"] = "Q x B ordinal and score matrices above --no-compose-above"
        del words, lists
        print(json.dumps(pt), flush=True)
        points.append(pt)

if ONLY != "filtered":
    sh = [p for p in points if p["masks"] == "shared" and p["selectivity"] <= 0.1]
    print(json.dumps({"summary": "shared mask, selectivity <= 10 %: filtered beats both baselines",
                      "holds": all(p["filtered_ms"] < p["unfiltered_ms"] and (p["composition_ms"] is None or p["filtered_ms"] < p["composition_ms"]) for p in sh),
                      "stats": {k: ctx.stat(k) for k in ("flat_acc_calls", "flat_acc_queries", "flat_acc_rows", "flat_acc_chunks", "flat_acc_generic")}}))
