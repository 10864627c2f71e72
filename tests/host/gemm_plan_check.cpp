// Stand-alone check of csrc/gemm_plan.h, the host decisions of the GEMM entry points: no HIP, no GPU.  tests/test_gemm_plan_host.py builds it
// with -fsanitize=address,undefined and runs it; a sanitizer report or a failed invariant ends it with a non-zero status.
//   * sweeps every function of the header over the axes of tests/make_gemm_plan_golden.py (same order) and prints one line per case (one
//     per block of 7 hints x 32 argument bits for the NT schedule, run-length coded): the test compares them with the golden table, which
//     was recorded from the library;
//   * checks the invariants of every plan on the way (workspace layout, splits, launch geometry);
//   * enumerates the kernel keys nt_launch can return and compares the set with the list of instantiations, both ways.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../multi-modal-emotion_amd/csrc/gemm_plan.h"
#include "check.h"

using namespace tav::plan;

static const void* const PTR = (const void*)0x1000;   // stands for a device pointer: tested for NULL-ness only
static const int F32 = TAV_F32, BF16 = TAV_BF16, FP8 = TAV_FP8;

static tav_gemm_nt_args nt_args(int in, int out, int nzb, long M, long N, long kbytes, int hint, int bits) {
    tav_gemm_nt_args g;
    std::memset(&g, 0, sizeof g);
    g.A = g.B = PTR; g.C = (void*)PTR;
    g.M = M; g.N = N; g.K = kbytes * 128 / elem_size(in);
    g.lda = g.ldb = g.K;
    g.ldc = g.ld_pre = g.ld_gelu_in = g.ld_resid = N;
    g.in_dtype = in; g.out_dtype = out; g.nzb = nzb; g.nzg = 1; g.tile_m_hint = hint; g.alpha = 1.f;
    g.resid = (bits & 1) ? (const float*)PTR : nullptr;
    g.accumulate = (bits & 2) ? 1 : 0;
    g.act = (bits & 4) ? 1 : 0;
    g.gelu_in = (bits & 8) ? PTR : nullptr;
    g.C_pre = (bits & 16) ? (void*)PTR : nullptr;
    return g;
}

static std::vector<bool> key_seen(nt_num_keys, false);

// the launches tav_gemm_nt makes for a (validated) call: geometry invariants, and every key must be a kernel that exists
static void check_launches(const tav_gemm_nt_args& g) {
    int tm, rows_big, tm_rest;
    nt_plan(&g, &tm, &rows_big, &tm_rest);
    CHECK(tm == 2 || tm == 3 || tm == 4 || tm == 8 || tm == 16, "tile %d", tm);
    CHECK(rows_big > 0 && rows_big <= g.M, "rows_big %d of %ld", rows_big, (long)g.M);
    const bool mixed = rows_big < g.M;
    for (int part = 0; part < (mixed ? 2 : 1); ++part) {
        int M = mixed ? rows_big : (int)g.M, t = mixed ? 16 : tm;
        if (part == 1) {
            const NtSplit s = nt_split(&g, rows_big);
            CHECK(s.M_rest == g.M - rows_big && s.M_rest > 0 && s.a_bytes > 0 && s.c_bytes > 0, "split of %ld at %d", (long)g.M, rows_big);
            CHECK(rows_big % 256 == 0 && tm == 16 && tm_rest >= 2 && tm_rest <= 4, "mixed schedule %d + tile %d", rows_big, tm_rest);
            M = s.M_rest; t = tm_rest;
        }
        const NtLaunch L = nt_launch(&g, M, t);
        const int k = nt_key_index(L.key);
        CHECK(k >= 0, "no kernel <in %d, out %d, TM %d, NST %d, NW %d, TNW %d, EPI %d> (M %d N %ld hint %d act %d)", L.key.in, L.key.out, L.key.tm,
              L.key.nst, L.key.nw, L.key.tnw, L.key.epi, M, (long)g.N, g.tile_m_hint, g.act);
        if (k >= 0) key_seen[k] = true;
        CHECK(L.lds <= (size_t)160 * 1024 && L.lds > 0, "LDS %zu", L.lds);
        CHECK(L.block == 256 || L.block == 512, "block %u", L.block);
        CHECK(L.block == 64u * L.key.nw, "block %u for %d waves", L.block, L.key.nw);
        CHECK(L.grid_x > 0 && L.grid_y > 0 && L.tiles_m > 0 && L.tiles_n > 0, "grid %u x %u", L.grid_x, L.grid_y);
        const int bm = 8 * L.key.tm * L.key.nw, bn = 32 * L.key.tnw;              // the tile the kernel computes must cover what the grid assumes
        CHECK((long)L.tiles_m * bm >= M && (long)(L.tiles_m - 1) * bm < M, "tiles_m %d x %d rows for M %d", L.tiles_m, bm, M);
        CHECK((long)L.tiles_n * bn >= g.N && (long)(L.tiles_n - 1) * bn < g.N, "tiles_n %d x %d for N %ld", L.tiles_n, bn, (long)g.N);
    }
}

static void sweep_nt_schedule() {
    const int dtypes[6][2] = {{BF16, BF16}, {BF16, F32}, {F32, BF16}, {F32, F32}, {FP8, BF16}, {FP8, F32}};
    const int nzbs[] = {1, 3}, hints[] = {0, 2, 3, 4, 8, 16, 17};
    const long Ms[] = {1, 7, 128, 255, 256, 257, 1000, 4096, 11712, 23424, 46848, 46885, 255968}, Ns[] = {4, 128, 132, 256, 768, 2304, 3072};
    const long kbs[] = {1, 2, 6, 12, 36, 37, 48};
    for (auto& dt : dtypes) for (int nzb : nzbs) for (long M : Ms) for (long N : Ns) for (long kb : kbs) {
        std::string line, prev;
        int run = 0;
        for (int hint : hints) for (int bits = 0; bits < 32; ++bits) {
            const tav_gemm_nt_args g = nt_args(dt[0], dt[1], nzb, M, N, kb, hint, bits);
            int tile = 0, rows_first = 0, tile_rest = 0;
            const int rc = nt_validate(&g, false);
            if (rc == 0) {                                                        // (as tav_gemm_nt_schedule reports the plan)
                int tm, rb, tr;
                nt_plan(&g, &tm, &rb, &tr);
                tile = tm; rows_first = rb; tile_rest = rb < g.M ? tr : 0;
                check_launches(g);
            }
            char cur[64];
            std::snprintf(cur, sizeof cur, "%d,%d,%d,%d", rc, tile, rows_first, tile_rest);
            if (prev == cur) { ++run; continue; }
            if (run) line += " " + std::to_string(run) + "*" + prev;
            prev = cur; run = 1;
        }
        line += " " + std::to_string(run) + "*" + prev;
        std::printf("nt_schedule %d %d %d %ld %ld %ld :%s\n", dt[0], dt[1], nzb, M, N, kb, line.c_str());
    }
}

// every key nt_launch can return: operand x output type x all 32 tile hints x all 8 ring hints x every combination of the arguments the
// epilogue flavour looks at x grids below and above 256 workgroups (and a shape that takes the mixed schedule)
static void sweep_nt_keys() {
    const int dtypes[5][2] = {{BF16, BF16}, {BF16, F32}, {F32, F32}, {FP8, BF16}, {FP8, F32}};
    const long shapes[4][2] = {{128, 128}, {300, 256}, {46885, 768}, {4096, 3072}};
    long cases = 0;
    for (auto& dt : dtypes) for (auto& sh : shapes) for (int nzb = 1; nzb <= 3; nzb += 2) for (int tile = 0; tile < 32; ++tile) for (int ring = 0; ring < 8; ++ring)
        for (int ptrs = 0; ptrs < 16; ++ptrs) for (int act = 0; act < 8; ++act) {
            tav_gemm_nt_args g = nt_args(dt[0], dt[1], nzb, sh[0], sh[1], 12, tile | (ring << 5), 0);
            g.resid = (ptrs & 1) ? (const float*)PTR : nullptr;
            g.C_pre = (ptrs & 2) ? (void*)PTR : nullptr;
            g.gelu_in = (ptrs & 4) ? PTR : nullptr;
            g.accumulate = (ptrs & 8) ? 1 : 0;
            g.act = act;
            CHECK(nt_validate(&g, true) == 0, "key sweep case refused");
            check_launches(g);
            ++cases;
        }
    int reached = 0;
    std::string idle;
    for (int k = 0; k < nt_num_keys; ++k) {
        reached += key_seen[k] ? 1 : 0;
        if (!key_seen[k]) {
            const NtKey& q = nt_keys[k];
            char b[96];
            std::snprintf(b, sizeof b, " <in %d, out %d, TM %d, NST %d, NW %d, TNW %d, EPI %d>", q.in, q.out, q.tm, q.nst, q.nw, q.tnw, q.epi);
            idle += b;
        }
    }
    for (int k = 0; k < nt_num_keys; ++k)
        for (int j = 0; j < k; ++j) CHECK(!(nt_keys[k] == nt_keys[j]), "key %d repeats key %d", k, j);
    std::printf("nt_keys %d in the list, %d reached over %ld cases; compiled for nothing:%s\n", nt_num_keys, reached, cases, idle.empty() ? " none" : idle.c_str());
    CHECK(reached == nt_num_keys, "a kernel of the list that no argument set reaches (reported, to be removed by a later change):%s", idle.c_str());
}

static void sweep_tn_splits() {
    const long Ns[] = {4, 128, 136, 512, 768, 1536, 2304, 3072}, rows[] = {1, 63, 64, 255, 256, 257, 1464, 7999, 11712, 46848}, nbs[] = {1, 8, 32};
    for (long n1 : Ns) for (long n2 : Ns) for (long rpb : rows) for (long nb : nbs) {
        int32_t cr = 0, ns = 0;
        tn_splits(n1, n2, rpb, nb, &cr, &ns);
        std::printf("tn_splits %ld %ld %ld %ld : 0 %d %d\n", n1, n2, rpb, nb, cr, ns);
        const long cpb = ns / nb;
        CHECK(cr > 0 && cr % 64 == 0 && ns % nb == 0 && cpb >= 1, "chunk %d, %d splits", cr, ns);
        CHECK(cpb * cr >= rpb && (cpb - 1) * cr < rpb, "%ld chunks of %d rows for %ld rows: an empty or a missing chunk", cpb, cr, rpb);
        CHECK(cpb == (rpb + cr - 1) / cr, "chunks per batch as tav_gemm_tn derives them");
    }
}

static void make_problems(tav_gemm_tn_problem* p, const long (*shapes)[2], int n, bool bias) {
    for (int k = 0; k < n; ++k) {
        p[k].A = p[k].B = PTR; p[k].out = (float*)PTR; p[k].dbias = bias ? (float*)PTR : nullptr;
        p[k].N1 = shapes[k][0]; p[k].N2 = shapes[k][1]; p[k].lda = shapes[k][0]; p[k].ldb = shapes[k][1];
    }
}

static void check_layout(const tav_gemm_tn_problem* probs, int n, long rows, const TnGroupPlan& P, bool use_ws) {
    CHECK(P.chunk > 0 && P.chunk % 64 == 0 && P.nsplit >= 1 && (long)P.nsplit * P.chunk >= rows, "%d splits of %ld rows for %ld", P.nsplit, P.chunk, rows);
    CHECK(P.tw == (P.big ? 256 : 128) && (P.big || P.nsplit == 1), "tile width %d, %d splits", P.tw, P.nsplit);
    if (tn_has_empty_split(P, rows)) return;                                      // refused by the entry point
    CHECK((long)(P.nsplit - 1) * P.chunk < rows, "empty split");
    const TnGroupLayout L = tn_group_layout(probs, n, P, use_ws);
    long off = 0;
    for (int k = 0; k < n; ++k) {                                                 // slabs, back to back from 0 ...
        if (P.nsplit > 1) { CHECK(L.slab_off[k] == off, "slab %d at %ld, expected %ld", k, L.slab_off[k], off); off += (long)P.nsplit * probs[k].N1 * probs[k].N2; }
        else CHECK(L.slab_off[k] == -1, "slab %d in a workspace without splits", k);
    }
    for (int k = 0; k < n; ++k) {                                                 // ... then the bias partials
        if (use_ws && probs[k].dbias) { CHECK(L.bias_off[k] == off, "bias partials %d at %ld, expected %ld", k, L.bias_off[k], off); off += (long)L.nbias[k] * probs[k].N1; }
        else CHECK(L.bias_off[k] == -1, "bias partials %d without a place", k);
        CHECK(L.nbias[k] == P.nsplit * L.tiles_2[k], "bias slots");
    }
    CHECK(L.ws_floats == off && off == (use_ws ? P.ws_floats : 0), "workspace ends at %ld, layout says %ld, plan says %ld", off, L.ws_floats, P.ws_floats);
    int tiles = 0; long n4 = 0, n1 = 0;
    for (int k = 0; k < TN_PROBLEMS_MAX; ++k) {
        const tav_gemm_tn_problem& a = probs[k < n ? k : n - 1];
        CHECK((long)L.tiles_1[k] * P.tw >= a.N1 && (long)(L.tiles_1[k] - 1) * P.tw < a.N1 && (long)L.tiles_2[k] * P.tw >= a.N2 && (long)(L.tiles_2[k] - 1) * P.tw < a.N2, "tiles of %d", k);
        if (k < n) { tiles += L.tiles_1[k] * L.tiles_2[k]; n4 += a.N1 * a.N2 / 4; n1 += a.N1; }
        CHECK(L.tile_end[k] == tiles && L.end4[k] == n4, "prefix sums at %d", k);
        CHECK(k == 0 || (L.tile_end[k] >= L.tile_end[k - 1] && L.end4[k] >= L.end4[k - 1]), "prefix sums decrease at %d", k);
    }
    CHECK(L.total == tiles && tiles > 0 && L.total_n1 == n1, "totals");
}

static void sweep_tn_grouped() {
    static const long layer[4][2] = {{2304, 768}, {768, 768}, {3072, 768}, {768, 3072}}, ragged[4][2] = {{384, 136}, {136, 264}, {256, 512}, {520, 128}};
    const long rows[] = {100, 777, 2047, 2048, 5856, 12287, 12288, 46848};
    const int flags[] = {0, 1, 2, 1 | (1 << 8), 1 | (2 << 8), 1 | (3 << 8), 1 | (4 << 8)}, dts[] = {BF16, F32};
    for (int set = 0; set < 2; ++set) for (int n = 1; n <= 4; ++n) for (long r : rows) for (int dt : dts) for (int fl : flags) for (int bias = 1; bias >= 0; --bias) {
        tav_gemm_tn_problem probs[4];
        make_problems(probs, set == 0 ? layer : ragged, n, bias != 0);
        const TnGroupPlan P = tn_big_plan(probs, n, r, dt, fl);
        std::printf("tn_grouped_ws_bytes %s %d %ld %d %d %d : %ld\n", set == 0 ? "layer" : "ragged", n, r, dt, fl, bias, P.ws_floats * 4);
        CHECK(tn_validate_group(probs, n, r, dt) == 0, "valid problems refused");
        check_layout(probs, n, r, P, true);
        check_layout(probs, n, r, tn_plain_plan(r), false);
    }
}

static void sweep_validation() {
    CHECK(elem_size(F32) == 4 && elem_size(BF16) == 2 && elem_size(FP8) == 1, "element sizes");
    struct { const char* name; const void *A, *B, *out; long N1, N2, lda, ldb, a_zb, b_zb, rows, nbatch; int dtype, want; } cases[] = {
        {"valid bf16", PTR, PTR, PTR, 128, 128, 128, 128, 0, 0, 256, 1, BF16, 0},
        {"valid f32, batched", PTR, PTR, PTR, 132, 4, 132, 4, 132 * 256, 4 * 256, 256, 8, F32, 0},
        {"A NULL x N1 0", nullptr, PTR, PTR, 0, 128, 128, 128, 0, 0, 256, 1, BF16, TAV_ERR_NULL},
        {"nbatch 0 x dtype 9", PTR, PTR, PTR, 128, 128, 128, 128, 0, 0, 256, 0, 9, TAV_ERR_SHAPE},
        {"dtype fp8 x N1 132", PTR, PTR, PTR, 132, 128, 128, 128, 0, 0, 256, 1, FP8, TAV_ERR_DTYPE},
        {"N2 132 (bf16) x lda 132", PTR, PTR, PTR, 128, 132, 132, 128, 0, 0, 256, 1, BF16, TAV_ERR_SHAPE},
        {"b_zb 4 x staging offsets", PTR, PTR, PTR, 128, 128, 1l << 24, 128, 0, 4, 256, 1, BF16, TAV_ERR_ALIGN},
        {"staging offsets", PTR, PTR, PTR, 128, 128, 128, 1l << 24, 0, 0, 256, 1, BF16, TAV_ERR_SHAPE},
        {"one row below the staging limit", PTR, PTR, PTR, 128, 128, 128, 1l << 20, 0, 0, 1983, 1, BF16, 0},
        {"at the staging limit", PTR, PTR, PTR, 128, 128, 128, 1l << 20, 0, 0, 1984, 1, BF16, TAV_ERR_SHAPE},
    };
    for (auto& c : cases) {
        const int rc = tn_validate_problem(c.A, c.B, c.out, c.N1, c.N2, c.lda, c.ldb, c.a_zb, c.b_zb, c.rows, c.nbatch, c.dtype);
        std::printf("tn_validate_problem [%s] : %d\n", c.name, rc);
        CHECK(rc == c.want, "%s: %d, expected %d", c.name, rc, c.want);
    }
    tav_gemm_nt_args g = nt_args(BF16, BF16, 1, 256, 256, 2, 0, 0);
    CHECK(nt_validate(nullptr, true) == TAV_ERR_NULL && nt_validate(&g, true) == 0, "nt_validate");
    g.A = nullptr; g.M = 0;
    CHECK(nt_validate(&g, true) == TAV_ERR_NULL && nt_validate(&g, false) == TAV_ERR_SHAPE, "nt_validate: pointers before shapes");
    std::printf("nt_validate [A NULL x M 0] : %d / %d\n", nt_validate(&g, true), nt_validate(&g, false));
}

int main() {
    sweep_validation();
    sweep_nt_schedule();
    sweep_nt_keys();
    sweep_tn_splits();
    sweep_tn_grouped();
    return check_summary();
}
