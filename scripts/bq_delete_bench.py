"""Deleting from a BQ graph next to the only alternative there was, building the survivors' graph again, on the MI355X: N rows are built
with BQGraphBuilder, a seeded 10 % and 30 % are marked, and remove_deleted is timed with the engine's own clock (the growth of seconds3[2]
of jv_hip_bq_builder_stats, which remove_deleted adds its time to); beside it the engine's seconds of a fresh BQGraphBuilder build of
the survivors with the same parameters and batch size, and recall@10 of BQGraphSearcher (exact rerank, rerankK 200) on both graphs
against exact ground truth over the survivors.  Report only, no bar.  One JSON object on stdout.
usage: python scripts/bq_delete_bench.py [N=200000] [D=768]"""
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

N = int(sys.argv[1]) if len(sys.argv) > 1 else 200_000
D = int(sys.argv[2]) if len(sys.argv) > 2 else 768
K, DEGREE, BEAM, ALPHA, OVERFLOW, BATCH, Q, RERANK = 10, 32, 100, 1.2, 1.25, 4096, 1000, 200
T0 = time.perf_counter()


def log(msg):
    print(f"[bq_delete_bench +{time.perf_counter() - T0:.0f}s] {msg}", file=sys.stderr, flush=True)


def build(ctx, bq, n):
    gb = J.BQGraphBuilder(ctx, bq, DEGREE, BEAM, ALPHA, OVERFLOW)
    gb.seed(0)
    lo = 1
    while lo < n:
        hi = min(n, lo + min(BATCH, lo))
        gb.insert_batch(np.arange(lo, hi, dtype=np.int32))
        lo = hi
    return gb


def seconds(gb):
    st = gb.stats()
    return st["search_s"] + st["prune_s"] + st["backlink_s"]


def recall(ctx, gb, bq, vs, n, queries, truth, ids_map=None):
    rows = gb.finish(np.empty((n, DEGREE), np.int32))
    g = J.GraphIndex(ctx, n, [(None, rows)], gb.entry, 0)
    ids, _ = J.BQGraphSearcher(ctx, g, bq, vs).search(queries, VSF.DOT_PRODUCT, K, RERANK)
    g.close()
    ids = ids if ids_map is None else np.where(ids >= 0, ids_map[np.maximum(ids, 0)], -1)
    return float(np.mean([len(set(ids[i].tolist()) & set(truth[i].tolist())) / K for i in range(len(ids))]))


dev = torch.device("cuda:0")
ctx = J.HipContext(0)
mix = benchlib.Mixture(D, 1, dev)
base = mix.sample(N, 2).cpu().numpy()
queries = mix.sample(Q, 3).cpu().numpy()
out = {"n": N, "dim": D, "degree": DEGREE, "beam": BEAM, "alpha": ALPHA, "overflow": OVERFLOW, "batch": BATCH, "cases": []}
for frac in (0.10, 0.30):
    rng = np.random.default_rng(int(100 * frac))
    gone = np.sort(rng.choice(N, int(N * frac), replace=False)).astype(np.int32)
    keep = np.setdiff1d(np.arange(N), gone)
    truth = keep[np.argsort(-(queries @ base[keep].T), axis=1, kind="stable")[:, :K]]
    vs = J.VectorSet(ctx, base)
    bq = J.BinaryQuantization(ctx, D).encode_all(vs)
    gb = build(ctx, bq, N)
    built_s = seconds(gb)
    gb.mark_deleted(gone)
    before = gb.stats()["backlink_s"]
    counts = gb.remove_deleted(0)
    remove_s = gb.stats()["backlink_s"] - before
    case = {"marked": len(gone), "build_all_s": built_s, "remove_deleted_s": remove_s, "counts": counts,
            "recall_repaired": recall(ctx, gb, bq, vs, N, queries, truth)}
    gb.close()
    vk = J.VectorSet(ctx, base[keep])
    bk = J.BinaryQuantization(ctx, D).encode_all(vk)
    gk = build(ctx, bk, len(keep))
    case["rebuild_survivors_s"] = seconds(gk)
    case["recall_rebuilt"] = recall(ctx, gk, bk, vk, len(keep), queries, truth, keep)
    gk.close()
    log(json.dumps(case))
    out["cases"].append(case)
print(json.dumps(out))
