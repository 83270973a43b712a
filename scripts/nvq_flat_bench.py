"""The NVQ flat search on the MI355X (jv_hip_nvq_search_flat, topK 10, candK 40) against the recipe it replaces — NVQVectors.scores
over all ordinals in row chunks, a top-k per chunk and a merge — on the same inputs: median wall time per call after a warm-up, the
peak device memory of each side over the resident data, and whether the ids agree.  For context, jv_hip_search_exact on the float rows
the NVQ rows were encoded from.  Prints one JSON object.

usage: python scripts/nvq_flat_bench.py [--n 1048576] [--d 768] [--s 2] [--q 2048] [--reps 3] [--vsf 1] [--learn 0] [--chunk 65536]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch

import jvector_amd as J


def used_bytes():
    free, total = torch.cuda.mem_get_info()
    return total - free


def timed(fn, ctx, reps):
    fn()   # warm-up: scratch buffers grow here
    ctx.sync()
    times, peak = [], used_bytes()
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        ctx.sync()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
        peak = max(peak, used_bytes())
    return out, statistics.median(times), min(times), peak


def recipe(ctx, nv, queries, vsf, k, chunk):
    """the parent commit's only way to a top-k over NVQ rows: NVQScorer's score of every (query, row), a Q x chunk matrix at a time"""
    Q, N = queries.shape[0], nv.count()
    ids, scores = [], []
    for s in range(0, N, chunk):
        c = min(chunk, N - s)
        ords = torch.arange(s, s + c, dtype=torch.int32, device="cuda").expand(Q, c).contiguous()
        i, sc = J.topk(ctx, nv.scores(queries, vsf, ords), min(k, c), id_base=s)
        ids.append(i)
        scores.append(sc)
    if len(ids) == 1:
        return ids[0], scores[0]
    return J.topk(ctx, torch.cat(scores, 1).contiguous(), k, ids=torch.cat(ids, 1).contiguous())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--s", type=int, default=2)
    ap.add_argument("--q", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--vsf", type=int, default=1)
    ap.add_argument("--learn", type=int, default=0, help="1: the growth-rate search of the encoder (slower to encode, same cost to score)")
    ap.add_argument("--chunk", type=int, default=65536, help="rows per chunk of the recipe")
    a = ap.parse_args()
    vsf, k = J.VectorSimilarityFunction(a.vsf), 10
    g = torch.Generator(device="cuda").manual_seed(1)
    vecs = torch.randn(a.n, a.d, device="cuda", generator=g)
    vecs /= vecs.norm(dim=1, keepdim=True)
    queries = torch.randn(a.q, a.d, device="cuda", generator=g)
    ctx = J.HipContext(0)
    vs = J.VectorSet(ctx, vecs)
    nv = J.NVQuantization.compute(ctx, vs, a.s).set_learn(bool(a.learn)).encode_all(vs)
    res = {"n": a.n, "d": a.d, "s": a.s, "q": a.q, "vsf": vsf.name, "top_k": k, "cand_k": 4 * k, "reps": a.reps, "learn": a.learn}

    base = used_bytes()
    (ids, _), med, best, peak = timed(lambda: vs.search_exact(queries, vsf, k, 4 * k), ctx, a.reps)
    res["search_exact_float_rows"] = {"median_ms": med, "min_ms": best, "peak_bytes_over_data": peak - base}

    stats = ("nvq_flat_fused_calls", "nvq_flat_fallbacks", "nvq_flat_listed")
    before = [ctx.stat(s) for s in stats]
    base = used_bytes()
    (ids, _), med, best, peak = timed(lambda: nv.search_flat(queries, vsf, k, 4 * k), ctx, a.reps)
    res["nvq_search_flat"] = {"median_ms": med, "min_ms": best, "peak_bytes_over_data": peak - base,
                              **{s: (ctx.stat(s) - b) // (a.reps + 1) for s, b in zip(stats, before)}}

    base = used_bytes()
    (gt, _), med, best, peak = timed(lambda: recipe(ctx, nv, queries, vsf, k, a.chunk), ctx, a.reps)
    res["recipe"] = {"median_ms": med, "min_ms": best, "peak_bytes_over_data": peak - base, "chunk": a.chunk}
    res["same_ids"] = bool(torch.equal(gt.cpu().to(torch.int32), ids.cpu().to(torch.int32)))
    res["time_ratio"] = res["nvq_search_flat"]["median_ms"] / res["recipe"]["median_ms"]
    print(json.dumps(res))
    assert res["same_ids"], "the call and the recipe disagree"


if __name__ == "__main__":
    main()
