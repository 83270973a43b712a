"""Binary quantization on the MI355X: encode rate, the flat scan's (query, row) pair rate against its derived VALU-issue ceiling,
flat-search QPS and recall@10 at several rerankK, and jv_hip_search_flat (PQ-96) at the same N for context.  Seeded synthetic
data (benchlib.Mixture, unit vectors), exact ground truth from jv_hip_exact_scan_dense (+ the bit-exact rescoring of its
candidates).  Times: wall clock around synchronised calls and the engine's HIP events (HipContext.profile: region "adc" = the
scan kernels of jv_hip_bq_search_flat).  Kernel names for a separate `rocprofv3 --kernel-trace --stats` run: bq_encode_kernel,
bq_scan_kernel<QT, 0> (histogram pass), bq_scan_kernel<QT, 1> (emit pass), bq_threshold_kernel, bq_tie_prefix_kernel,
bq_scan_kernel<QT, 2> (ranked ties; returns at once unless ties overflow).  One JSON object on stdout.
usage: python scripts/bq_bench.py [N=10000000] [D=768] [--quick] [--no-pq]"""
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import benchlib
import jvector_amd as J
from jvector_amd import VectorSimilarityFunction as VSF

args = [a for a in sys.argv[1:] if not a.startswith("--")]
N = int(args[0]) if len(args) > 0 else 10_000_000
D = int(args[1]) if len(args) > 1 else 768
QUICK, NO_PQ = "--quick" in sys.argv, "--no-pq" in sys.argv
Q_SCAN = (1, 256, 4096) if not QUICK else (1, 256)
Q_GT = 1000 if not QUICK else 100
RERANKS = (0, 10, 100, 1000)
K = 10

# derived ceiling: xor + bcnt per 32-bit half of a word = 2 x ceil(D / 32) VALU lane-ops per (query, row) pair;
# issue rate 256 CUs x 4 SIMDs x 32 lanes / clk (a wave64 VALU instruction over 2 cycles) x 2.4 GHz
LANE_OPS_PER_PAIR = 2 * math.ceil(D / 32)
ISSUE = 256 * 4 * 32 * 2.4e9
CEIL_PAIRS = ISSUE / LANE_OPS_PER_PAIR

dev = torch.device("cuda:0")
ctx = J.HipContext(0)
mix = benchlib.Mixture(D, 1, dev)
base = mix.sample(N, 2)
queries = mix.sample(max(max(Q_SCAN), Q_GT), 3)
vs = J.VectorSet(ctx, base)
out = {"n": N, "dim": D, "words_per_row": (D + 63) // 64, "labels": "measured unless the key says derived",
       "scan_ceiling_derived": {"lane_ops_per_pair": LANE_OPS_PER_PAIR, "issue_lane_ops_per_s": ISSUE, "pairs_per_s": CEIL_PAIRS}}


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        r = fn()
    ctx.sync()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps, r


bq = J.BinaryQuantization(ctx, D)
enc_s, bv = timed(lambda: bq.encode_all(vs), 3)
out["encode_rows_per_s"] = N / enc_s
out["encode_ms"] = enc_s * 1e3

searcher = J.BQFlatSearcher(ctx, bv, vs)
scan = {}
for Q in Q_SCAN:
    qs = queries[:Q].contiguous()
    reps = 5 if Q < 4096 else 2
    wall, _ = timed(lambda: searcher.search(qs, VSF.DOT_PRODUCT, K, 0), 1)
    ctx.profile(True)
    wall, _ = timed(lambda: searcher.search(qs, VSF.DOT_PRODUCT, K, 0), reps)
    adc_ms, adc_n = ctx.profile_read("adc")
    ctx.profile(False)
    sel_ms = adc_ms / max(1, adc_n)   # one region per call: histogram pass + thresholds + emit pass + tie kernels
    pairs = 2.0 * Q * N               # two full passes over the rows
    rate = pairs / (sel_ms * 1e-3)
    scan[str(Q)] = {"qps": Q / wall, "call_ms": wall * 1e3, "select_ms": sel_ms, "scan_pairs_per_s": rate,
                    "share_of_derived_ceiling": rate / CEIL_PAIRS}
out["scan"] = scan

# recall@10 against exact ground truth (dot product over unit vectors)
qg = queries[:Q_GT].contiguous()
t0 = time.perf_counter()
gt = benchlib.ground_truth(J, ctx, vs, qg, VSF.DOT_PRODUCT, K, dense=True, q_group=1024).cpu().numpy()
out["ground_truth_s"] = time.perf_counter() - t0
rec = {}
for rk in RERANKS:
    wall, (ids, _) = timed(lambda: searcher.search(qg, VSF.DOT_PRODUCT, K, rk), 2)
    ids = ids.cpu().numpy() if hasattr(ids, "cpu") else ids
    rec[str(rk)] = {"recall_at_10": benchlib.recall_at_k(ids, gt), "qps": Q_GT / wall}
out["search"] = {"queries": Q_GT, "by_rerank_k": rec}

if not NO_PQ:
    M = 96
    cb = benchlib.train_codebooks(base, M, 5)
    pq = J.ProductQuantization.from_codebooks(ctx, D, M, cb)
    cv = J.PQVectors.encode_and_build(ctx, pq, vs)
    fs = J.FlatSearcher(ctx, pq, cv, vs, max_queries=Q_GT)
    pqr = {}
    for rk in (100, 1000):
        wall, (ids, _) = timed(lambda: fs.search(qg, VSF.DOT_PRODUCT, K, rk), 2)
        ids = ids.cpu().numpy() if hasattr(ids, "cpu") else ids
        pqr[str(rk)] = {"recall_at_10": benchlib.recall_at_k(ids, gt), "qps": Q_GT / wall}
    out["pq96_search_flat"] = {"queries": Q_GT, "by_rerank_k": pqr}

print(json.dumps(out))
