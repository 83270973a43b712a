"""A layered graph built from binary-quantized rows alone (jv_hip_bq_build_layered) next to the PQ build of the same rows
(jv_hip_build_layered, PQ with D / 8 sub-vectors) on the MI355X: the engine's own seconds4 = {search, prune, backlink, total} for both
builds, then both graphs searched with BQGraphSearcher + exact rerank: recall@10 and mean visited at rerankK 100 and 1000.  The data are
seeded benchlib.Mixture unit vectors; exact ground truth from jv_hip_exact_scan_dense.  One JSON object on stdout.
usage: python scripts/bq_builder_bench.py [N=1000000] [D=768] [--improve=P]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import benchlib
import jvector_amd as J
from jvector_amd import VectorSimilarityFunction as VSF
from jvector_amd.builder import build_hierarchical

args = [a for a in sys.argv[1:] if not a.startswith("--")]
N = int(args[0]) if len(args) > 0 else 1_000_000
D = int(args[1]) if len(args) > 1 else 768
IMPROVE = next((int(a.split("=")[1]) for a in sys.argv[1:] if a.startswith("--improve=")), 0)
K, DEGREE, BEAM, ALPHA, OVERFLOW, SEED, Q_GT = 10, 32, 100, 1.2, 1.25, 11, 1000
RERANKS = (100, 1000)
M = D // 8

T0 = time.perf_counter()


def log(msg):
    print(f"[bq_builder_bench +{time.perf_counter() - T0:.0f}s] {msg}", file=sys.stderr, flush=True)


def host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


dev = torch.device("cuda:0")
ctx = J.HipContext(0)
mix = benchlib.Mixture(D, 1, dev)
base = mix.sample(N, 2)
queries = mix.sample(Q_GT, 3).contiguous()
vs = J.VectorSet(ctx, base)
bv = J.BinaryQuantization(ctx, D).encode_all(vs)
out = {"n": N, "dim": D, "degree": DEGREE, "beam": BEAM, "alpha": ALPHA, "overflow": OVERFLOW, "improve_passes": IMPROVE, "pq_subvectors": M}

g_bq = J.build_bq_layered(ctx, bv, DEGREE, BEAM, ALPHA, OVERFLOW, improve=IMPROVE, seed=SEED)
st = g_bq.build_stats
out["bq_build"] = {"seconds4": [st["search_s"], st["prune_s"], st["backlink_s"], st["total_s"]], "levels": st["levels"], "reprunes": st["reprunes"],
                   "visited": st["visited"], "expanded": st["expanded"]}
log("BQ build: " + json.dumps(out["bq_build"]))

cb = benchlib.train_codebooks(base, M, 5)
pq = J.ProductQuantization.from_codebooks(ctx, D, M, cb)
cv = J.PQVectors.encode_and_build(ctx, pq, vs)
levels, entry, entry_level, _nb0, ps = build_hierarchical(ctx, pq, cv, base, VSF.DOT_PRODUCT, max_degree=DEGREE, beam_width=BEAM, alpha=ALPHA,
                                                          seed=SEED, overflow=OVERFLOW, improve=IMPROVE, vector_set=vs)
out["pq_build"] = {"seconds4": [ps["search_s"], ps["prune_s"], ps["backlink_s"], ps["total_s"]], "levels": ps["levels"], "reprunes": ps["reprunes"],
                   "visited": ps["visited"], "expanded": ps["expanded"]}
log("PQ build: " + json.dumps(out["pq_build"]))
g_pq = J.GraphIndex(ctx, N, levels, entry, entry_level)

gt = benchlib.ground_truth(J, ctx, vs, queries, VSF.DOT_PRODUCT, K, dense=True, q_group=1024).cpu().numpy()
for name, graph in (("bq_graph", g_bq), ("pq_graph", g_pq)):
    searcher = J.BQGraphSearcher(ctx, graph, bv, vs)
    res = {}
    for rk in RERANKS:
        ids, _, stats = searcher.search(queries, VSF.DOT_PRODUCT, K, rk, return_stats=True)
        res[str(rk)] = {"recall_at_10": benchlib.recall_at_k(host(ids), gt), "mean_visited": float(stats[:, 0].mean())}
    out[name + "_searched_with_bq"] = res
    log(name + ": " + json.dumps(res))
print(json.dumps(out))
