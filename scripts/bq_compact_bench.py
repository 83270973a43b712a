"""Compacting a BQ builder on the MI355X: N rows are built with BQGraphBuilder, a seeded fifth is marked and removed, and
BQGraphBuilder.compact moves the survivors into a new builder.  Timed with a host clock around the call, which ends in a device
synchronise: the whole entry point — the scratch and the new builder's allocations, the rank, the two gathers, the blank tail, and the
copies of the two maps to the host — REPEAT times into a fresh destination each, after one warm-up.  Beside the times: the bytes the
compaction must move (live x R x 8 adjacency and scores + live x 4 diverseBefore + live x W x 8 BQ rows, read and as much written,
plus the maps: n / 8 present bits read, n x 4 + live x 4 written) and those bytes over the best time as a fraction of the HBM peak
(8 TB/s).  Report only, no bar.  One JSON object on stdout.
usage: python scripts/bq_compact_bench.py [N=200000] [D=768] [BEAM=100]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import benchlib
import jvector_amd as J

N = int(sys.argv[1]) if len(sys.argv) > 1 else 200_000
D = int(sys.argv[2]) if len(sys.argv) > 2 else 768
BEAM = int(sys.argv[3]) if len(sys.argv) > 3 else 100
DEGREE, ALPHA, OVERFLOW, BATCH, REPEAT, HBM_PEAK = 32, 1.2, 1.25, 4096, 5, 8.0e12
T0 = time.perf_counter()


def log(msg):
    print(f"[bq_compact_bench +{time.perf_counter() - T0:.0f}s] {msg}", file=sys.stderr, flush=True)


def build(ctx, bq, n):
    gb = J.BQGraphBuilder(ctx, bq, DEGREE, BEAM, ALPHA, OVERFLOW)
    gb.seed(0)
    lo = 1
    while lo < n:
        hi = min(n, lo + min(BATCH, lo))
        gb.insert_batch(np.arange(lo, hi, dtype=np.int32))
        lo = hi
    return gb


dev = torch.device("cuda:0")
ctx = J.HipContext(0)
mix = benchlib.Mixture(D, 1, dev)
base = mix.sample(N, 2).cpu().numpy()
vs = J.VectorSet(ctx, base)
bq = J.BinaryQuantization(ctx, D).encode_all(vs)
gb = build(ctx, bq, N)
st = gb.stats()
log(f"built {N} x {D} in {st['search_s'] + st['prune_s'] + st['backlink_s']:.1f}s")
gone = np.sort(np.random.default_rng(20).choice(N, N // 5, replace=False)).astype(np.int32)
gb.mark_deleted(gone)
counts = gb.remove_deleted(0)
live, R, W = gb.stats()["inserted"], gb.row_width(), bq.words
log(f"removed {counts['removed']}, {live} live")

rows_bytes = live * R * 8 + live * 4 + live * W * 8
map_bytes = N // 8 + N * 4 + live * 4
moved = 2 * rows_bytes + map_bytes
times, renumber = [], []
for rep in range(REPEAT + 1):
    dst = J.BQVectors(ctx, D, count=live)
    torch.cuda.synchronize()
    t = time.perf_counter()
    new, o2n, n2o = gb.compact(dst)
    dt = time.perf_counter() - t
    if rep == 0:   # checked once, outside the timed calls: the maps are the sequential renumbering
        present = np.ones(N, bool)
        present[gone] = False
        assert np.array_equal(n2o, np.flatnonzero(present)) and new.stats()["inserted"] == live
    else:
        times.append(dt)
    new.close()
    dst.close()
    t = time.perf_counter()
    gb.renumbering()
    if rep > 0:
        renumber.append(time.perf_counter() - t)
best = min(times)
out = {"n": N, "dim": D, "degree": DEGREE, "beam": BEAM, "row_width": R, "words": W, "removed": int(counts["removed"]), "live": int(live),
       "compact_s": times, "compact_best_s": best, "compact_median_s": float(np.median(times)), "renumbering_best_s": min(renumber),
       "bytes_rows_each_way": int(rows_bytes), "bytes_maps": int(map_bytes), "bytes_moved": int(moved),
       "bytes_per_s_best": moved / best, "fraction_of_hbm_peak": moved / best / HBM_PEAK}
print(json.dumps(out))
