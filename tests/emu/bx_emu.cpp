// bx_emu.cpp — compiles the BQ builder's deletion bodies (jvector_amd/csrc/bx_body.h: the affected list, and the gather / score / sort /
// merge of one affected node) for the lane emulator.  TEST HARNESS: g++ -O2 -ffp-contract=off, never linked into the product.  The
// wave API is bg_emu.cpp's, taken in unchanged.
#include "bg_emu.cpp"

#include "../../jvector_amd/csrc/bx_body.h"

namespace {
struct BxLaunch {
    const jv::BxParams *p;
    int step, wt;
    int64_t index;
    char *lds;
};
void bx_lane_main(void *arg)
{
    const BxLaunch &L = *(const BxLaunch *)arg;
    if (L.step == 0) return jv::bx_affected_word(*L.p, L.index);
    if (L.step == 1) return jv::bx_compact(*L.p);
    switch (L.wt) {   // widths k_bq_delete.hip compiles, and the generic form
    case 0: jv::bx_node<0>(*L.p, (int)L.index, L.lds); break;
    case 1: jv::bx_node<1>(*L.p, (int)L.index, L.lds); break;
    case 2: jv::bx_node<2>(*L.p, (int)L.index, L.lds); break;
    case 12: jv::bx_node<12>(*L.p, (int)L.index, L.lds); break;
    default: abort();
    }
}
}  // namespace

// the two launches of launch_bq_delete_affected: tasks_out [n] (garbage behind the count), count_out [1].  Returns 0, -1 on bad arguments.
extern "C" int bx_emu_affected(const int32_t *nbrs, int64_t n, int R, const uint64_t *present, const uint64_t *marked, int32_t *tasks_out,
                               uint32_t *count_out)
{
    if (n < 1 || R < 1 || R > 64) return -1;
    std::vector<uint64_t> aff((size_t)((n + 63) / 64), 0x5a5a5a5a5a5a5a5aull);   // garbage: every word must be written before it is read
    jv::BxParams p{};
    p.n = n; p.R = R; p.nbrs = nbrs; p.present = present; p.marked = marked; p.affected = aff.data(); p.tasks = tasks_out; p.task_count = count_out;
    for (int64_t w = 0; w < (n + 63) / 64; ++w) {
        BxLaunch L{&p, 0, 0, w, nullptr};
        emu::run_wave(bx_lane_main, &L);
    }
    BxLaunch L{&p, 1, 0, 0, nullptr};
    emu::run_wave(bx_lane_main, &L);
    return 0;
}

// launch_bq_delete_merge, one emulated wave per task.  wt: the compiled row width to run (must equal W) or 0 for the generic form.
// given (nullable): [P][G] explicit candidates with given_n [P].  list (nullable: count only) / lsc [P][L]; ln / cn [P].
// Returns 0, -1 on bad arguments, -3 if a task wrote past its LDS block.
extern "C" int bx_emu_merge(const uint64_t *rows_in, int64_t n, int D, int W, const int32_t *nbrs, const float *nsc, int R, const uint64_t *marked,
                            const int32_t *tasks, int P, const int32_t *given, const int32_t *given_n, int G, int L, int32_t *list, float *lsc,
                            int32_t *ln, int32_t *cn, int wt)
{
    if (n < 1 || R < 1 || R > 64 || W < 1 || (wt != 0 && wt != W) || (given && (G < 1 || G > 64)) || (list && L < 1)) return -1;
    // a 16-byte aligned copy: rows of an even width are read as 16-byte words
    uint64_t *rows = (uint64_t *)aligned_alloc(64, ((sizeof(uint64_t) * (size_t)n * W + 63) / 64 + 1) * 64);
    memcpy(rows, rows_in, sizeof(uint64_t) * (size_t)n * W);
    jv::BxParams p{};
    p.rows = rows; p.n = n; p.D = D; p.W = W; p.nbrs = nbrs; p.nsc = nsc; p.R = R; p.marked = marked; p.tasks = (int32_t *)tasks; p.P = P;
    p.given = given; p.given_n = given_n; p.G = G; p.L = L; p.list = list; p.lsc = lsc; p.ln = ln; p.cn = cn;
    const size_t lds_bytes = jv::bx_lds_bytes(R, wt ? 0 : W);
    char *lds = (char *)aligned_alloc(64, (lds_bytes + 63) / 64 * 64 + 64);
    int rc = 0;
    for (int t = 0; t < P && rc == 0; ++t) {
        memset(lds, 0xa5, lds_bytes);         // stale LDS must never reach a result
        memset(lds + lds_bytes, 0x3c, 64);    // canary behind the block
        BxLaunch Ln{&p, 2, wt, t, lds};
        emu::run_wave(bx_lane_main, &Ln);
        for (int i = 0; i < 64; ++i)
            if (lds[lds_bytes + i] != 0x3c) rc = -3;
    }
    free(lds);
    free(rows);
    return rc;
}
