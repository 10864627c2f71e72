// Stand-alone check of csrc/entry_plan.h, the host decisions of the entry points outside gemm.hip: no HIP, no GPU.
// tests/test_entry_plan_host.py builds it with -fsanitize=address,undefined and runs it; a sanitizer report or a failed invariant ends it
// with a non-zero status.
//   * "query NAME : v v ..." -- every size query of the ABI over the axes of tests/make_entry_plan_golden.py (same order): the test compares
//     the lines with the table recorded from the library;
//   * every validator over a sweep that includes its caps, accepted and refused dtype codes included, and wherever it accepts a shape the
//     invariants of the geometry: grid x work per block covers the problem, LDS within a CU's 160 KB, workspace offsets increasing and
//     ending at the advertised size, partial counts equal to what the query functions advertise;
//   * "finding NAME : first shape" -- an accepted shape whose grid does not fit dim3 (x below 2^31, y and z at most 65535) or whose size
//     query does not fit its int: the narrowing the enqueue then does loses bits.  The test holds the list of names.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../multi-modal-emotion_amd/csrc/entry_plan.h"
#include "check.h"

using namespace tav::plan;

static void* const PTR = (void*)0x1000;   // stands for a device pointer: tested for NULL-ness only
static const int F32 = TAV_F32, BF16 = TAV_BF16;
static const int64_t LDS_CU = 160 * 1024;
static const std::vector<int64_t> SZ = {1, 2, 4, 63, 64, 65, 255, 256, 257, 1000, 4096, 8192, 8193, 65535, 65536, 65537, 131072, 262144, 1 << 20, 1 << 24, 1ll << 31, 1ll << 40};
static const int CODES[] = {-1, 0, 1, 2, 3, 4, 7};

static std::map<std::string, std::string> findings;
static void finding(const char* name, const char* fmt, int64_t a = 0, int64_t b = 0, int64_t c = 0) {
    char buf[160];
    std::snprintf(buf, sizeof buf, fmt, (long long)a, (long long)b, (long long)c);
    findings.emplace(name, buf);
}
// geometry every launch must have: whole blocks, LDS of a CU; a grid beyond dim3 is a finding (the validator accepted the shape)
static void check_launch(const char* name, const Launch& L, int64_t a = 0, int64_t b = 0, int64_t c = 0) {
    CHECK(L.gx >= 1 && L.gy >= 1 && L.gz >= 1 && L.block >= 1 && L.block <= 1024, "%s grid %" PRId64 " %" PRId64 " %" PRId64 " block %d", name, L.gx, L.gy, L.gz, L.block);
    CHECK((int64_t)L.lds <= LDS_CU, "%s lds %zu", name, L.lds);
    if (L.gx >= (1ll << 31) || L.gy > 65535 || L.gz > 65535) finding(name, "grid past dim3 at (%lld, %lld, %lld)", a, b, c);
}
static bool fits_int(int64_t v) { return v >= INT32_MIN && v <= INT32_MAX; }
static std::vector<int64_t> around(int64_t x) { return {x - 1, x, x + 1}; }
static std::vector<int64_t> cat(std::vector<int64_t> a, const std::vector<int64_t>& b) { a.insert(a.end(), b.begin(), b.end()); return a; }

static void queries() {
    auto line = [](const char* name, const std::vector<int64_t>& v) {
        std::printf("query %s :", name);
        for (int64_t x : v) std::printf(" %" PRId64, x);
        std::printf("\n");
    };
    std::vector<int64_t> out;
    for (int64_t r : cat(cat(cat({0, 1}, around(LN_BWD_ROWS)), {46848}), cat(around(LN_BWD_ROWS * LN_MAX_BLOCKS), {1ll << 40}))) out.push_back(ln_blocks(r));
    line("tav_ln_bwd_partials", out); out.clear();
    for (int64_t b : {1, 4, 32}) for (int64_t c : {64, 512, 768}) out.push_back(gn_workspace_floats(b, c));
    line("tav_gn_workspace_floats", out); out.clear();
    for (int64_t b : {1, 4}) for (int64_t t : cat(cat(cat({1}, around(C0_BT)), around(2 * C0_BT)), {49999})) out.push_back(conv0_bwd_partials(b, t, 512, 10));
    line("tav_conv0_bwd_partials", out); out.clear();
    out.push_back(weight_norm_partials(768, 48)); out.push_back(weight_norm_partials(16, 16));
    for (int64_t r : cat(cat(cat({1}, around(WN_PART_ROWS)), around(WN_PART_ROWS * WN_MAX_PARTS)), {2 * WN_PART_ROWS * WN_MAX_PARTS})) out.push_back(weight_norm_partials(r, 1));
    line("tav_weight_norm_partials", out); out.clear();
    for (int64_t r : cat(cat(cat({1}, around(EMB_PART_ROWS)), around(EMB_PART_ROWS * EMB_MAX_PARTS)), {1ll << 40})) out.push_back(embed_add_bwd_parts(r));
    line("tav_embed_add_bwd_parts", out); out.clear();
    for (int n : {1, 7, 300, 65535}) out.push_back(sumsq_partials(n));
    line("tav_sumsq_partials", out);
    line("tav_optim_chunk_elems", {OPT_CHUNK});
    line("tav_optim_max_groups", {OPT_MAX_GROUPS});
    out = {fp8_amax_partials(1, 4), fp8_amax_partials(8, 1024), fp8_amax_partials(9, 1024), fp8_amax_partials(11712, 768)};
    for (int64_t r : around((int64_t)FP8_AMAX_BLOCK_GROUPS * FP8_AMAX_MAX_PARTS * 4 / 4096)) out.push_back(fp8_amax_partials(r, 4096));
    out.push_back(fp8_amax_partials(1ll << 30, 4096));
    line("tav_fp8_amax_partials", out); out.clear();
    for (int64_t r : cat(cat(cat({0, 1}, around(SPEC_ROWS)), around((int64_t)SPEC_ROWS * SPEC_MAX_PARTS)), {1ll << 40})) for (int64_t h : {0, 4, 768}) out.push_back(specaug_bwd_ws_bytes(r, h));
    line("tav_specaug_bwd_ws_bytes", out); out.clear();
    out = {audio_resample_tile(0, 1, 0), audio_resample_tile(1, 0, 0), audio_resample_tile(1, 1, -1)};
    for (int o : {1, 2, 3, 7, 30, 31, 32, 147, 441}) for (int n : {1, 160, 320}) for (int w : {0, 6, 17, 100, 4000}) out.push_back(audio_resample_tile(o, n, w));
    line("tav_audio_resample_tile", out);
}

// every validator with a dtype argument over every code (and pair of codes): "accepts NAME : codes" -- the test compares the sets with the
// recorded accepted_dtypes and with the dispatch lists of the .hip files; a refused code must give TAV_ERR_DTYPE, arguments otherwise valid
template <typename F> static void accepts(const char* name, F rc_of) {
    std::printf("accepts %s :", name);
    for (int a : CODES) {
        const int rc = rc_of(a);
        CHECK(rc == 0 || rc == TAV_ERR_DTYPE, "%s code %d gives %d", name, a, rc);
        if (rc == 0) std::printf(" %d", a);
    }
    std::printf("\n");
}
template <typename F> static void accepts2(const char* name, F rc_of) {
    std::printf("accepts %s :", name);
    for (int a : CODES) for (int b : CODES) {
        const int rc = rc_of(a, b);
        CHECK(rc == 0 || rc == TAV_ERR_DTYPE, "%s codes %d %d give %d", name, a, b, rc);
        if (rc == 0) std::printf(" %d>%d", a, b);
    }
    std::printf("\n");
}
static void dtypes() {
    accepts("tav_head_scale", [](int a) { return head_scale_validate(true, a, 0, 2, 8, 2, 128, 128, 128); });
    accepts("tav_gn_gelu_fwd tav_gn_gelu_bwd", [](int a) { return gn_validate(true, a, 2, 100, 64); });
    accepts("tav_gelu_fwd tav_gelu_bwd", [](int a) { return gelu_validate(true, a, 64); });
    accepts("tav_cast_weight", [](int a) { return cast_weight_validate(true, a, 8, 8); });
    accepts("tav_cast_conv_weight", [](int a) { return cast_conv_weight_validate(true, false, a, 8, 4, 3, 0); });
    accepts("tav_zero_pad_rows", [](int a) { return zero_pad_rows_validate(true, a, 2, 8, 8, 2); });
    accepts("tav_transpose2d", [](int a) { return transpose2d_validate(true, a, 8, 8, 2); });
    accepts("tav_patchify", [](int a) { return patchify_validate(true, a, 1, 2, 16, 16, 1); });
    accepts("tav_conv0_fwd", [](int a) { return conv0_fwd_validate(true, a, 1, 100, 19, 8, 10, 5); });
    accepts("tav_conv0_bwd_w", [](int a) { return conv0_bwd_validate(true, a, 1, 100, 19, 8, 10, 5); });
    accepts("tav_col2im_1d", [](int a) { return col2im_validate(true, a, 1, 100, 19, 8, 10, 5); });
    accepts("tav_weight_norm_fwd", [](int a) { return weight_norm_validate(true, a, 64, 16, 8); });
    accepts("tav_fp8_amax", [](int a) { return fp8_amax_validate(true, a, 8, 64, 64); });
    accepts("tav_fp8_quantize tav_fp8_quantize_delayed", [](int a) { return fp8_quantize_validate(true, true, false, a, 8, 64, 64, 64, 0, 0); });
    tav_attn_args at; std::memset(&at, 0, sizeof at);
    at.q = at.k = at.v = PTR; at.o = PTR; at.lse = (float*)PTR; at.B = 2; at.S = 128; at.nheads = 2;
    at.ld_q = at.ld_k = at.ld_v = at.ld_o = 128;
    accepts("tav_attn_fwd tav_attn_bwd tav_attn_fwd_len tav_attn_bwd_len", [&](int a) { at.dtype = a; return attn_validate(&at, ATTN_FWD); });
    accepts("tav_attn_probs", [&](int a) { at.dtype = a; return attn_validate(&at, ATTN_PROBS); });
    tav_ln_args ln; std::memset(&ln, 0, sizeof ln);
    ln.x = ln.dy = PTR; ln.gamma = ln.beta = (float*)PTR; ln.y_f32 = ln.mean = ln.rstd = ln.dx_f32 = (float*)PTR; ln.rows = 8; ln.W = 64;
    accepts("tav_ln_fwd", [&](int a) { ln.x_dtype = a; return ln_fwd_validate(&ln); });
    accepts2("tav_ln_bwd", [&](int a, int b) { ln.x_dtype = a; ln.dy_dtype = b; return ln_bwd_validate(&ln); });
    tav_clip_xform x; std::memset(&x, 0, sizeof x);
    x.T = 4; x.H = x.W = x.crop_h = x.crop_w = 32; x.nf = 1; x.out_h = x.out_w = 16;
    accepts("tav_video_clip_transform", [&](int a) { x.src_dtype = a; return video_clip_validate(true, &x); });
    tav_resample_args r; std::memset(&r, 0, sizeof r);
    r.C = 1; r.L = r.T_row = 1000; r.sL = 1; r.o = r.n = r.ntap = 1;
    ResamplePlan P;
    accepts("tav_audio_resample", [&](int a) { r.src_dtype = a; return audio_resample_validate(true, &r, &P); });
    accepts2("tav_cast2d", [](int a, int b) { return cast2d_validate(true, a, b, 8, 8, 4, 8); });
    accepts2("tav_group_pad", [](int a, int b) { return group_pad_validate(true, a, b, 1, 8, 64, 4, 1, 1); });
    for (int a : CODES) CHECK(lp_code(PTR, a) == (a == BF16 ? BF16 : F32) && lp_code(nullptr, a) == F32, "lp_code %d", a);
}

static void attention() {
    for (int dt : {BF16, F32}) for (int64_t B : {1ll, 4ll, 1000ll, 1ll << 20, 1ll << 31}) for (int64_t S : SZ) for (int64_t nh : {1, 12, 64}) {
        tav_attn_args a; std::memset(&a, 0, sizeof a);
        a.q = a.k = a.v = a.dout = PTR; a.o = a.dq = a.dk = a.dv = PTR; a.lse = a.delta = (float*)PTR;
        a.B = B; a.S = S; a.nheads = nh; a.dtype = dt; a.scale = 0.125f;
        a.ld_q = a.ld_k = a.ld_v = a.ld_o = a.ld_do = a.ld_dq = a.ld_dk = a.ld_dv = nh * 64;
        const int es = dt == BF16 ? 2 : 4;
        for (int bwd = 0; bwd < 2; ++bwd) {
            if (attn_validate(&a, bwd ? ATTN_BWD : ATTN_FWD) != 0) continue;
            for (int mode = 0; mode < 3; ++mode) for (int pre = 0; pre < 2; ++pre) {
                const Launch L = attn_launch(&a, bwd, bwd ? (mode == 0 && pre == 0 ? attn_dq_lds(es) : attn_dkdv_lds(es, mode, pre)) : attn_fwd_lds(es));
                check_launch(bwd ? "tav_attn_bwd" : "tav_attn_fwd", L, B, S, nh);
                CHECK(L.gx < (1ll << 31) && L.gx == (int64_t)attn_tiles(S, bwd) * nh * B && (int64_t)attn_tiles(S, bwd) * 128 >= S && L.block == 256, "attn grid");
                CHECK(fits_int(B) && fits_int(S) && fits_int(nh), "attn sizes travel as int: %" PRId64 " %" PRId64 " %" PRId64, B, S, nh);
            }
        }
        if (attn_validate(&a, ATTN_PROBS, true, 0) == 0) {
            if (!fits_int(B) || !fits_int(S)) { finding("tav_attn_probs sizes", "B or S does not fit the int it travels as at (%lld, %lld, %lld)", B, S, nh); continue; }
            const Launch L = attn_probs_launch(&a);
            check_launch("tav_attn_probs", L, B, S, nh);
            CHECK(L.gx * 4 >= B * nh * S, "probs rows");
        }
    }
}

static void norm() {
    for (int64_t rows : SZ) {
        const Launch F = ln_fwd_launch(rows), Bw = ln_bwd_launch(rows);
        check_launch("tav_ln_fwd", F, rows); check_launch("tav_ln_bwd", Bw, rows);
        CHECK(F.gx <= 2048 && (F.gx == 2048 || F.gx * 4 >= rows), "ln_fwd grid %" PRId64, rows);       // grid-stride beyond 2048 workgroups
        CHECK(Bw.gx == ln_blocks(rows) && Bw.gx <= LN_MAX_BLOCKS && (Bw.gx == LN_MAX_BLOCKS || Bw.gx * 16 >= rows), "ln_bwd blocks %" PRId64, rows);
    }
    for (int64_t W = 4; W <= LN_MAX_W; W += 4) { const Launch R = ln_reduce_launch(W, TAV_LN_REDUCE_MAX); check_launch("ln_reduce", R, W); CHECK(R.gx * 16 >= W && R.gy == TAV_LN_REDUCE_MAX, "ln_reduce %" PRId64, W); }
    tav_ln_reduce_item items[TAV_LN_REDUCE_MAX];
    for (auto& it : items) it = tav_ln_reduce_item{(float*)PTR, (float*)PTR, nullptr, LN_MAX_BLOCKS, 64, 0, 0};
    items[5].W = LN_MAX_W;
    int wmax = 0;
    CHECK(ln_reduce_validate(items, TAV_LN_REDUCE_MAX, &wmax) == 0 && wmax == LN_MAX_W, "ln_reduce_validate");
    CHECK(ln_reduce_validate(items, TAV_LN_REDUCE_MAX + 1, &wmax) == TAV_ERR_SHAPE && ln_reduce_validate(items, 5, &wmax) == 0 && wmax == 64, "ln_reduce_validate n");
    for (int64_t B : {1ll, 4ll, 65535ll, 65536ll}) for (int64_t T : SZ) for (int64_t C : {64, 512, 768, 4096}) {
        if (gn_validate(true, BF16, B, T, C) != 0) continue;
        const GnPlan P = gn_plan(B, T, C);
        check_launch("tav_gn_gelu B", P.stats, B, 0, C); check_launch("tav_gn_gelu T", Launch{P.apply.gx, P.apply.gy, 1, 256, 0}, 0, T, C);
        check_launch("tav_gn_gelu", P.pivot, B, T, C); check_launch("tav_gn_gelu", P.finalize, B, T, C); check_launch("tav_gn_gelu", P.param, B, T, C);
        CHECK(P.stats.gx * GN_CB >= C && P.stats.gy == GN_SPLIT && P.stats.gz == B && P.apply.gx == P.stats.gx && P.apply.gy * 4 * GN_AR >= T && P.apply.gz == B, "gn grids");
        CHECK(P.pivot.gx * 8 >= B * (C / 4) && P.finalize.gx * 256 >= B * C && P.param.gx * 256 >= C, "gn small grids");
        const GnLayout W = gn_layout(B, C);
        CHECK(W.part == 0 && W.sums - W.part == B * GN_SPLIT * C * 2 && W.piv - W.sums == B * C * 2 && W.end - W.piv == B * C, "gn layout");
        CHECK(fits_int(W.end) && gn_workspace_floats(B, C) == W.end, "gn workspace");
    }
}

static void elementwise() {
    for (int64_t n : SZ) {      // one thread (or wave, or block) per item
        for (int per : {4, 8, 64, 256}) { const Launch L = grid1(n, per); check_launch("one-dimensional element grid", L, n); CHECK(L.gx * per >= n && (L.gx - 1) * per < n, "grid1"); }
        const Launch F = fill_launch(n);
        check_launch("tav_fill_f32", F, n); CHECK(F.gx <= 4096 && (F.gx == 4096 || F.gx * 256 >= n), "fill");
        const Launch T = tile32_launch(n, 768);
        check_launch("tav_cast_weight R", T, n, 768); CHECK(T.gx * 32 >= 768 && T.gy * 32 >= n, "tile32");
        check_launch("tav_mean_pool_fwd B / tav_patchify B / tav_conv0 B", mean_pool_fwd_launch(n, 768), n); CHECK(mean_pool_fwd_launch(n, 768).gx * 64 >= 768, "mean_pool");
        if (embed_add_bwd_validate(true, n, 768, 3) == 0) {
            const PartsPlan P = embed_add_bwd_plan(n, 768, 3);
            check_launch("tav_embed_add_bwd", P.partial, n); check_launch("tav_embed_add_bwd", P.final_, n);
            if (!fits_int((n + P.parts - 1) / P.parts)) { finding("tav_embed_add_bwd rows per part", "does not fit int at rows %lld", n); continue; }
            CHECK(P.parts == embed_add_bwd_parts(n) && P.parts >= 1 && P.parts <= 256 && (int64_t)P.parts * P.rows_per_part >= n && P.partial.gy == P.parts &&
                  P.partial.gx * 256 >= 768 && P.final_.gx * 256 >= 3 * 768, "embed_add_bwd %" PRId64, n);
        }
        for (int64_t W : {64, 768, 1024})
            if (scatter_add_validate(true, n, W, 100) == 0) { check_launch("tav_scatter_add_rows", Launch{n, 1, 1, SCAT_T, scatter_add_lds(n, W)}, n, W); CHECK(scatter_add_lds(n, W) >= 256 + (size_t)n * 4 + 64 * W, "scatter lds"); }
    }
    for (int64_t S = 1; S <= 1024; ++S) { const int t = text_pos_threads(S); CHECK(t >= S && t >= 64 && t <= 1024 && (t & (t - 1)) == 0, "text_pos_threads %" PRId64, S); }
    CHECK(multi_tensor_validate(true, 65535) == 0 && multi_tensor_validate(true, 65536) == TAV_ERR_SHAPE && sumsq_partials(65535) == 65535 * SUMSQ_BLOCKS, "multi tensor");
    CHECK(chunked_validate(true, 1, 1, OPT_MAX_GROUPS) == 0 && chunked_validate(true, 1, 1, OPT_MAX_GROUPS + 1) == TAV_ERR_SHAPE, "groups");
    CHECK(cast_weights_multi_validate(true, 65535, 1) == 0 && cast_weights_multi_validate(true, 65536, 1) == TAV_ERR_SHAPE, "cast multi");
    CHECK(transpose2d_validate(true, BF16, 8, 8, 65535) == 0 && transpose2d_validate(true, BF16, 8, 8, 65536) == TAV_ERR_SHAPE, "transpose z");
}

static void audio_frontend() {
    for (int64_t B : {1ll, 4ll, 65536ll}) for (int64_t T : SZ) {
        if (conv0_fwd_validate(true, BF16, B, 5 * T + 10, T, 512, 10, 5) == 0) {
            const Launch F = conv0_fwd_launch(B, T);
            check_launch("tav_mean_pool_fwd B / tav_patchify B / tav_conv0 B", Launch{1, F.gy, 1, 256, 0}, B); check_launch("tav_conv0_fwd", Launch{F.gx, 1, 1, 256, 0}, T);
            CHECK(F.gx * C0_TT >= T && F.gy == B, "conv0 fwd");
        }
        if (conv0_bwd_validate(true, BF16, B, 5 * T + 10, T, 512, 10, 5) != 0) continue;
        const Conv0BwdPlan P = conv0_bwd_plan(B, T, 512, 10);
        check_launch("tav_conv0_bwd_w", Launch{P.partial.gx, 1, 1, 256, 0}, T); check_launch("tav_conv0_bwd_w", P.final_, T);
        CHECK((int64_t)P.chunks * C0_BT >= T && P.partial.gx == P.chunks && P.partial.gy == B && P.final_.gx * 64 >= 512 * 11, "conv0 bwd");
        CHECK(P.blocks == (int64_t)P.chunks * B && conv0_bwd_partials(B, T, 512, 10) == (int64_t)P.blocks * 512 * 11 && fits_int(B * cdiv(T, C0_BT) * 512 * 11), "conv0 partials");
    }
    for (int64_t Cg : {1, 16, 48, 128}) for (int64_t m : SZ) for (int64_t K : {1, 8, 128}) {
        const int64_t H = Cg * m;
        if (weight_norm_validate(true, BF16, H, Cg, K) != 0 || H > (1ll << 24)) continue;
        const WnPlan P = weight_norm_plan(H, Cg, K);
        check_launch("tav_weight_norm", P.partial, H, Cg, K); check_launch("tav_weight_norm", P.final_, H, Cg, K); check_launch("tav_weight_norm", P.apply, H, Cg, K);
        CHECK(P.parts == weight_norm_partials(H, Cg) && P.parts >= 1 && P.parts <= WN_MAX_PARTS && (int64_t)P.parts * P.rows_per_part >= P.rows && P.partial.gx == P.parts && P.apply.gx * 256 >= P.n, "wn parts");
        CHECK(P.ws_dw == 0 && P.ws_partials == H * Cg * K && P.ws_dots == P.ws_partials + (int64_t)P.parts * K && P.ws_end == H * Cg * K + (int64_t)weight_norm_partials(H, Cg) * K + K &&
              P.ws_dw < P.ws_partials && P.ws_partials < P.ws_dots && P.ws_dots < P.ws_end, "wn workspace");
    }
}

static void fp8_specaug_media() {
    for (int64_t rows : SZ) for (int64_t cols : {4, 64, 768, 4096}) {
        if (fp8_amax_validate(true, BF16, rows, cols, cols) != 0) continue;
        const int nb = fp8_amax_partials(rows, cols);
        CHECK(nb >= 1 && nb <= 2048, "amax partials");
        if (cols % 8 == 0 && fp8_can_stream(false, 0x1000, 0x1000, rows, cols, cols, cols)) { const Launch L = fp8_stream_launch(rows, cols); check_launch("tav_fp8_quantize", L, rows, cols); CHECK(L.gx <= 8192, "stream"); CHECK(fits_int(rows), "rows travel as unsigned"); }
        const Launch T = fp8_tile_launch(rows, cols);
        check_launch("tav_fp8_quantize rows", T, rows, cols); CHECK(T.gx * 64 >= cols && T.gy * 64 >= rows, "fp8 tiles");
    }
    for (int64_t B : {1ll, 4ll, 65536ll}) for (int64_t T : SZ) for (int64_t H : {4, 768, 1 << 20}) {
        if (specaug_bwd_validate(true, true, true, INT64_MAX, B, T, H) != 0) continue;
        const int64_t rows = B * T;
        const PartsPlan P = specaug_bwd_plan(rows, H);
        check_launch("tav_specaug_bwd", P.partial, rows, H); check_launch("tav_specaug_bwd", P.final_, rows, H);
        CHECK(P.parts == specaug_bwd_parts(rows) && P.parts <= SPEC_MAX_PARTS && (int64_t)P.parts * P.rows_per_part >= rows && P.partial.gy == P.parts && P.partial.gx * 256 >= H / 4 &&
              P.final_.gx * 64 >= H / 4 && specaug_bwd_ws_bytes(rows, H) == (int64_t)P.parts * H * 4, "specaug bwd");
        if (!fits_int((rows + P.parts - 1) / P.parts)) finding("tav_specaug_bwd rows per part", "does not fit int at rows %lld", rows);
        check_launch("tav_specaug_fwd", grid1(rows * (H / 4)), rows, H);
    }
    CHECK(specaug_draw_validate(true, 0x7fffffff, 1, 0.5f, 1, 0) == 0 && specaug_draw_validate(true, 2, 100, 0.05f, 10, SPEC_MAX_SPANS + 1) == 0 &&
          specaug_draw_validate(true, 2, 100000, 0.05f, 10, SPEC_MAX_SPANS + 1) == TAV_ERR_SHAPE, "specaug draw");
    for (int h : {1, 7, 8, 9, 224, VX_MAX}) for (int w : {1, 31, 32, 33, 224, VX_MAX}) for (int nf : {1, 16, 32}) {
        tav_clip_xform x; std::memset(&x, 0, sizeof x);
        x.src_dtype = TAV_U8; x.T = 4; x.H = x.W = x.crop_h = x.crop_w = 32; x.nf = nf; x.out_h = h; x.out_w = w;
        CHECK(video_clip_validate(true, &x) == 0, "video valid");
        const Launch L = video_clip_launch(&x);
        check_launch("tav_video_clip_transform", L, h, w, nf); CHECK(L.gx * VX_TW >= w && L.gy * VX_TH >= h && L.gz == nf && L.block == VX_TW * VX_TH, "video grid");
    }
    for (int o : {1, 2, 3, 7, 30, 31, 147, 441, 1 << 20}) for (int n : {1, 160, 320, 1 << 20}) for (int width : {0, 6, 17, 4000, 1 << 24}) for (int64_t L : {1ll, 1000ll, 1ll << 40}) {
        tav_resample_args a; std::memset(&a, 0, sizeof a);
        a.src_dtype = F32; a.C = 2; a.L = L; a.sC = L; a.sL = 1; a.o = o; a.n = n; a.width = width; a.ntap = 1; a.first_max = 0;
        a.T_row = ((int64_t)n * L + o - 1) / o;
        if (a.T_row > (1ll << 40)) a.T_row = 1ll << 40;
        ResamplePlan P;
        if (audio_resample_validate(true, &a, &P) != 0) continue;
        check_launch("tav_audio_resample", P.launch, o, n, L);
        CHECK(P.tile == audio_resample_tile(o, n, width) && P.tile >= AR_THREADS && P.tile <= AR_THREADS * AR_MAX_PER_THREAD && P.tile % AR_THREADS == 0 &&
              ar_span(P.tile, o, n, width) <= AR_SPAN_MAX && P.launch.gx * P.tile >= a.T_row && P.launch.gx < (1ll << 31) && P.launch.block == AR_THREADS, "resample plan");
        CHECK(!P.table_in_lds || (int64_t)n * ar_pitch(a.ntap) <= AR_TABLE_MAX, "table in lds");
    }
}

int main() {
    queries();
    dtypes();
    attention();
    norm();
    elementwise();
    audio_frontend();
    fp8_specaug_media();
    for (const auto& f : findings) std::printf("finding %s : %s\n", f.first.c_str(), f.second.c_str());
    return check_summary();
}
