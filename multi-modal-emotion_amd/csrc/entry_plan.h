// Host decisions of every entry point outside gemm.hip (gemm_plan.h holds those) as pure functions: argument checks, launch geometry, the
// size queries of the ABI, the layout of the workspaces the library carves up itself, and the constants all of these rest on.  Only the
// public ABI header and the standard library: any C++17 host compiler builds it (tests/host/entry_plan_check.cpp runs it under ASan +
// UBSan); the .hip files keep their kernels, pack() and an enqueue that reads validate, plan, dispatch, launch.
//
// A validator takes `have` = "every required pointer is there" (the entry forms it from its own arguments) and the sizes; the order of its
// tests is the order of the codes the entry points have always returned.  Geometry is computed in 64 bits: the enqueue narrows a grid
// to dim3's unsigned, entry_plan_check.cpp says for which accepted shapes that loses bits (profiles/entry_host_refactor.txt lists them).
#pragma once
#include <stdint.h>
#include <math.h>
#include <stddef.h>
#include "../../include/tavhip.h"

namespace tav {
namespace plan {

struct Launch {
    int64_t gx, gy, gz;
    int block;
    size_t lds;
};
inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline Launch grid1(int64_t n, int per_block = 256, int block = 256) { return Launch{cdiv(n, per_block), 1, 1, block, 0}; }   // one thread (or `per_block`-th of a block) per item
inline bool is_float(int dt) { return dt == TAV_BF16 || dt == TAV_F32; }
// the optional low-precision copy of the f32 entries: bf16 when asked for, any other code is read as f32
inline int lp_code(const void* lp_ptr, int lp_dtype) { return (lp_ptr && lp_dtype == TAV_BF16) ? TAV_BF16 : TAV_F32; }
// `have` alone: tav_clip_coef
inline int ptrs_validate(bool have) { return have ? 0 : TAV_ERR_NULL; }
// `have`, then n >= 1: tav_fill_f32, tav_tanh_*, tav_sum_partials, tav_fp8_roll_states
inline int count_validate(bool have, int64_t n) { return !have ? TAV_ERR_NULL : (n <= 0 ? TAV_ERR_SHAPE : 0); }

// ------------------------------------------------------------------------------------------------ attention.hip
constexpr int ATT_FWD_NQ = 2;        // 16-query tiles per wave: 32 queries per wave, 128 per workgroup
enum { ATTN_FWD = 0, ATTN_BWD = 1, ATTN_PROBS = 2 };
// tav_attn_fwd / _bwd, their _len forms and tav_attn_probs.  `extra`: the _len forms' seq_lens (tested last) or tav_attn_probs' output
// (tested with the first pointers); true where there is none.
inline int attn_validate(const tav_attn_args* a, int what, bool extra = true, int64_t hs_bstride = 0) {
    const bool probs = what == ATTN_PROBS;
    if (!a || !a->q || !a->k || !a->lse || (probs ? !extra : (!a->v || !a->o))) return TAV_ERR_NULL;
    if (a->B <= 0 || a->S <= 0 || a->nheads <= 0 || (probs && hs_bstride < 0)) return TAV_ERR_SHAPE;
    if (!probs) {     // the grid is one-dimensional (attn_tile): 64-query tiles x heads x batch below 2^31, factor by factor so that nothing overflows
        const int64_t lim = 1ll << 31;
        if (a->S >= lim * 64 || a->nheads >= lim || a->B >= lim) return TAV_ERR_SHAPE;
        const int64_t th = ((a->S + 63) / 64) * a->nheads;
        if (th >= lim || th * a->B >= lim) return TAV_ERR_SHAPE;
    }
    if (!is_float(a->dtype)) return TAV_ERR_DTYPE;
    if (a->mask_mode < 0 || a->mask_mode > 2) return TAV_ERR_SHAPE;
    if (a->mask_mode != 0 && !a->key_mask) return TAV_ERR_NULL;
    if (!probs && a->mask_mode == 2 && (!a->corr || !a->o_soft)) return TAV_ERR_NULL;
    const int pk = a->dtype == TAV_BF16 ? 8 : 4;
    if (a->ld_q % pk || a->ld_k % pk || (!probs && (a->ld_v % pk || a->ld_o % 4))) return TAV_ERR_ALIGN;
    if (probs) return 0;
    if (a->ld_q < a->nheads * 64 || a->ld_k < a->nheads * 64 || a->ld_v < a->nheads * 64 || a->ld_o < a->nheads * 64) return TAV_ERR_SHAPE;
    {   // the streamed tiles are addressed with 32-bit byte offsets inside one batch entry's slice
        const int64_t es = a->dtype == TAV_BF16 ? 2 : 4;
        int64_t ld = a->ld_q > a->ld_k ? a->ld_q : a->ld_k;
        ld = ld > a->ld_v ? ld : a->ld_v;
        if (what == ATTN_BWD && a->ld_do > ld) ld = a->ld_do;
        if (ld >= (1ll << 32) || a->S + 64 > ((1ll << 32) - 1) / (ld * es)) return TAV_ERR_SHAPE;      // (S + 64) * ld * es >= 2^32, without forming the product
    }
    if (what == ATTN_BWD) {
        if (!a->dout || !a->dq || !a->dk || !a->dv || !a->delta) return TAV_ERR_NULL;
        if (a->ld_do % pk || a->ld_dq % 4 || a->ld_dk % 4 || a->ld_dv % 4) return TAV_ERR_ALIGN;
    }
    return extra ? 0 : TAV_ERR_NULL;
}
// LDS bytes of the three kernels: attention.hip forms them from its device-only HD<T> and asserts them equal to these
constexpr int attn_rowb(int es) { return 64 * es; }
constexpr int attn_pitch_n(int es) { return 64 * es + (es == 2 ? 32 : 16); }
constexpr int attn_dkdv_bq(int es, int mode, bool pre) { return es == 2 ? ((mode == 0 && pre) ? 32 : 64) : 32; }
constexpr size_t attn_fwd_lds(int es) { return 2 * (64 * attn_rowb(es) + 64 * attn_pitch_n(es) + 2 * 64 * 4) + (256 + 64) * 4; }
constexpr size_t attn_dkdv_lds(int es, int mode, bool pre) {
    return 2 * (2 * attn_dkdv_bq(es, mode, pre) * attn_rowb(es) + (es == 2 ? 0 : 2 * attn_dkdv_bq(es, mode, pre) * attn_pitch_n(es)) + 2 * attn_dkdv_bq(es, mode, pre) * 4) + (256 + 64) * 4;
}
constexpr size_t attn_dq_lds(int es) { return 2 * (2 * 64 * attn_rowb(es) + (es == 2 ? 0 : 64 * attn_pitch_n(es)) + 64 * 4); }
// query tiles per (batch entry, head): 128 queries per workgroup, forward and backward (the _len forms keep the grid of the padded problem)
inline int attn_tiles(int64_t S, bool bwd) { return (int)((S + (bwd ? 128 : 64 * ATT_FWD_NQ) - 1) / (bwd ? 128 : 64 * ATT_FWD_NQ)); }
inline Launch attn_launch(const tav_attn_args* a, bool bwd, size_t lds) { return Launch{(int64_t)attn_tiles(a->S, bwd) * a->nheads * a->B, 1, 1, 256, lds}; }
inline Launch attn_probs_launch(const tav_attn_args* a) { return grid1(a->B * a->nheads * a->S, 4); }      // one wave per row
inline int head_scale_validate(bool have, int dt, int64_t hs_bstride, int64_t B, int64_t S, int64_t nheads, int64_t lda, int64_t ldb, int64_t ldo) {
    if (!have) return TAV_ERR_NULL;
    if (B <= 0 || S <= 0 || nheads <= 0 || hs_bstride < 0) return TAV_ERR_SHAPE;
    if (!is_float(dt)) return TAV_ERR_DTYPE;
    return (lda % 4 || ldb % 4 || ldo % 4) ? TAV_ERR_ALIGN : 0;
}

// ------------------------------------------------------------------------------------------------ norm.hip
constexpr int LN_MAX_W = 1024;         // norm.hip's 64 lanes x LN_MAXV float4 (it asserts that)
// cap on workgroups of the LN backward (= rows of the dgamma/dbeta partial buffer).  Measured at 11712 x 768: 256 -> 35.5 us,
// 512 -> 33.9 us, 1024 -> 38.0 us (more partial rows for ln_param_reduce); at 46848 x 768 (batch 32): 256 -> 157 us, 512 -> 106.5 us
// (4.7 TB/s), 1024 -> 131 us, 2048 -> 136 us: one workgroup per CU keeps too few bytes in flight, four pay for their partial rows.
constexpr int LN_MAX_BLOCKS = 512;
constexpr int LN_BWD_ROWS = 16;        // rows per workgroup of the LN backward below the cap
constexpr int LN_FWD_MAX_BLOCKS = 2048;   // the LN forward strides over the rows beyond this grid
inline int ln_blocks(int64_t rows) {    // tav_ln_bwd_partials
    const int64_t b = (rows + LN_BWD_ROWS - 1) / LN_BWD_ROWS;      // >= 4 rows per wave so the per-lane dgamma/dbeta partials amortise
    return (int)(b < 1 ? 1 : (b > LN_MAX_BLOCKS ? LN_MAX_BLOCKS : b));
}
inline int ln_fwd_validate(const tav_ln_args* a) {
    if (!a || !a->x || !a->gamma || !a->beta || (!a->y_f32 && !a->y_lp)) return TAV_ERR_NULL;
    if (a->rows <= 0 || a->W <= 0 || a->W > LN_MAX_W || a->W % 4) return TAV_ERR_SHAPE;
    if (a->ld_x % 4 || a->ld_y % 4) return TAV_ERR_ALIGN;
    return is_float(a->x_dtype) ? 0 : TAV_ERR_DTYPE;
}
inline int ln_bwd_validate(const tav_ln_args* a) {
    if (!a || !a->x || !a->gamma || !a->dy || !a->mean || !a->rstd || (!a->dx_f32 && !a->dx_lp)) return TAV_ERR_NULL;
    if (a->act == 1 && !a->beta) return TAV_ERR_NULL;
    if ((a->dgamma || a->dbeta) && !a->partials) return TAV_ERR_NULL;
    if (a->rows <= 0 || a->W <= 0 || a->W > LN_MAX_W || a->W % 4) return TAV_ERR_SHAPE;
    if (a->ld_x % 4 || a->ld_dy % 4 || a->ld_dx % 4) return TAV_ERR_ALIGN;
    if (a->defer_param_reduce && !a->partials) return TAV_ERR_NULL;
    return (is_float(a->x_dtype) && is_float(a->dy_dtype)) ? 0 : TAV_ERR_DTYPE;
}
inline Launch ln_fwd_launch(int64_t rows) { const int64_t want = (rows + 3) / 4; return Launch{want < LN_FWD_MAX_BLOCKS ? want : LN_FWD_MAX_BLOCKS, 1, 1, 256, 0}; }   // a wave per row, grid-stride
inline Launch ln_bwd_launch(int64_t rows) { return Launch{ln_blocks(rows), 1, 1, 256, 0}; }
inline Launch ln_reduce_launch(int64_t W, int n = 1) { return Launch{cdiv(W, 16), n, 1, 256, 0}; }
// *wmax: the widest item (the x extent of the launch)
inline int ln_reduce_validate(const tav_ln_reduce_item* items, int n, int* wmax) {
    if (!items) return TAV_ERR_NULL;
    if (n <= 0 || n > TAV_LN_REDUCE_MAX) return TAV_ERR_SHAPE;
    *wmax = 0;
    for (int i = 0; i < n; ++i) {
        const tav_ln_reduce_item& it = items[i];
        if (!it.partials || (!it.dgamma && !it.dbeta)) return TAV_ERR_NULL;
        if (it.W <= 0 || it.W > LN_MAX_W || it.W % 4 || it.nblocks <= 0 || it.nblocks > LN_MAX_BLOCKS) return TAV_ERR_SHAPE;
        *wmax = it.W > *wmax ? it.W : *wmax;
    }
    return 0;
}
constexpr int GN_SPLIT = 32;     // T-slices of the statistics pass
constexpr int GN_CB = 256;       // channels per workgroup of the statistics pass
constexpr int GN_AR = 16;        // rows per thread of the apply passes (a workgroup covers 4 * GN_AR rows x 256 channels)
// group-norm workspace, float offsets: [B][GN_SPLIT][C][2] partial sums, [B][C][2] sums of the backward, [B][C] pivots of the forward
struct GnLayout { int64_t part, sums, piv, end; };
inline GnLayout gn_layout(int64_t B, int64_t C) { return GnLayout{0, B * GN_SPLIT * C * 2, B * GN_SPLIT * C * 2 + B * C * 2, B * GN_SPLIT * C * 2 + B * C * 2 + B * C}; }
inline int gn_workspace_floats(int64_t B, int64_t C) { return (int)gn_layout(B, C).end; }
inline int gn_validate(bool have, int dt, int64_t B, int64_t T, int64_t C) {
    if (!have) return TAV_ERR_NULL;
    if (B <= 0 || T <= 0 || C <= 0 || C % 64) return TAV_ERR_SHAPE;
    // tav_gn_workspace_floats answers in an int: a caller that sized its workspace by a wrapped answer would have it written out of bounds
    if (B > INT32_MAX || C > INT32_MAX || B * C > INT32_MAX / (GN_SPLIT * 2 + 3)) return TAV_ERR_SHAPE;
    return is_float(dt) ? 0 : TAV_ERR_DTYPE;
}
struct GnPlan { Launch pivot, stats, finalize, param, apply; };
inline GnPlan gn_plan(int64_t B, int64_t T, int64_t C) {
    return GnPlan{grid1(B * (C / 4), 8), Launch{cdiv(C, GN_CB), GN_SPLIT, B, 256, 0}, grid1(B * C), grid1(C), Launch{cdiv(C, GN_CB), cdiv(T, 4 * GN_AR), B, 256, 0}};
}
inline int gelu_validate(bool have, int dt, int64_t n) {
    if (!have) return TAV_ERR_NULL;
    if (n <= 0 || n % 4) return TAV_ERR_SHAPE;
    return is_float(dt) ? 0 : TAV_ERR_DTYPE;
}

// ------------------------------------------------------------------------------------------------ elementwise.hip
constexpr int SCAT_T = 1024, SCAT_MAXW = 1024;
constexpr int SUMSQ_BLOCKS = 96;
constexpr int OPT_CHUNK = 16384;
constexpr int OPT_MAX_GROUPS = 64;
constexpr int ADAMW_MULTI_BLOCKS = 192;
constexpr int FILL_MAX_BLOCKS = 4096;                   // tav_fill_f32 strides beyond this grid
constexpr int EMB_PART_ROWS = 256, EMB_MAX_PARTS = 256;  // tav_embed_add_bwd: rows per part below the cap on parts

inline int cast_weight_validate(bool have, int dt, int64_t R, int64_t C) {
    if (!have) return TAV_ERR_NULL;
    if (R <= 0 || C <= 0) return TAV_ERR_SHAPE;
    return is_float(dt) ? 0 : TAV_ERR_DTYPE;
}
inline Launch tile32_launch(int64_t R, int64_t C, int64_t nbatch = 1) { return Launch{cdiv(C, 32), cdiv(R, 32), nbatch, 256, 0}; }   // tav_cast_weight, tav_transpose2d
inline int cast_weights_multi_validate(bool have, int64_t n, int64_t blocks_per_tensor) {
    if (!have) return TAV_ERR_NULL;
    return (n <= 0 || n > 65535 || blocks_per_tensor <= 0) ? TAV_ERR_SHAPE : 0;
}
inline int cast_conv_weight_validate(bool have, bool phase, int dt, int64_t co, int64_t ci, int64_t k, int64_t conv_stride) {
    if (!have) return TAV_ERR_NULL;
    if (co <= 0 || ci <= 0 || k <= 0) return TAV_ERR_SHAPE;
    if (phase && (conv_stride <= 0 || conv_stride > k)) return TAV_ERR_SHAPE;     // (stride > k would leave phases without a tap)
    return is_float(dt) ? 0 : TAV_ERR_DTYPE;
}
inline int zero_pad_rows_validate(bool have, int dt, int64_t B, int64_t T, int64_t C, int64_t pad) {
    if (!have) return TAV_ERR_NULL;
    if (B <= 0 || T <= 0 || C <= 0 || C % 4 || pad <= 0) return TAV_ERR_SHAPE;
    return is_float(dt) ? 0 : TAV_ERR_DTYPE;
}
inline int cast2d_validate(bool have, int sdt, int ddt, int64_t ld_src, int64_t ld_dst, int64_t R, int64_t C) {
    if (!have) return TAV_ERR_NULL;
    if (R <= 0 || C <= 0 || C % 4) return TAV_ERR_SHAPE;
    if (ld_src % 4 || ld_dst % 4) return TAV_ERR_ALIGN;
    return (is_float(sdt) && is_float(ddt)) ? 0 : TAV_ERR_DTYPE;
}
inline int transpose2d_validate(bool have, int dt, int64_t R, int64_t C, int64_t nbatch) {
    if (!have) return TAV_ERR_NULL;
    if (R <= 0 || C <= 0 || nbatch <= 0 || nbatch > 65535) return TAV_ERR_SHAPE;
    return is_float(dt) ? 0 : TAV_ERR_DTYPE;
}
inline int add_f32_validate(bool have, int64_t n) { return !have ? TAV_ERR_NULL : ((n <= 0 || n % 4) ? TAV_ERR_SHAPE : 0); }
inline Launch fill_launch(int64_t n) { const int64_t b = cdiv(n, 256); return Launch{b < FILL_MAX_BLOCKS ? b : FILL_MAX_BLOCKS, 1, 1, 256, 0}; }   // grid-stride
// tav_embed_add_fwd and tav_gather_rows
inline int table_rows_validate(bool have, int64_t rows, int64_t W, int64_t ntable) {
    if (!have) return TAV_ERR_NULL;
    return (rows <= 0 || W <= 0 || W % 4 || ntable <= 0) ? TAV_ERR_SHAPE : 0;
}
inline int embed_add_bwd_parts(int64_t rows) { const int64_t p = (rows + EMB_PART_ROWS - 1) / EMB_PART_ROWS; return (int)(p > EMB_MAX_PARTS ? EMB_MAX_PARTS : p); }
inline int embed_add_bwd_validate(bool have, int64_t rows, int64_t W, int64_t ntable) {
    if (!have) return TAV_ERR_NULL;
    return (rows <= 0 || W <= 0 || ntable <= 0 || ntable > 8) ? TAV_ERR_SHAPE : 0;
}
// A two-stage column sum: `parts` workgroup rows of `rows_per_part` rows each, then the parts in order
struct PartsPlan { int parts, rows_per_part; Launch partial, final_; };
inline PartsPlan embed_add_bwd_plan(int64_t rows, int64_t W, int64_t ntable) {
    const int np = embed_add_bwd_parts(rows);
    return PartsPlan{np, (int)((rows + np - 1) / np), Launch{cdiv(W, 256), np, 1, 256, 0}, grid1(ntable * W)};
}
// the LayerNorm tav_text_embed_fwd ends with, over its own pre-LN sum
inline tav_ln_args text_embed_ln(const tav_text_embed_args* a) {
    tav_ln_args ln = {};
    ln.x = a->pre; ln.x_dtype = TAV_F32; ln.gamma = a->gamma; ln.beta = a->beta; ln.y_f32 = a->y_f32; ln.y_lp = a->y_lp; ln.lp_dtype = a->lp_dtype;
    ln.mean = a->mean; ln.rstd = a->rstd; ln.rows = a->B * a->S; ln.W = a->W; ln.ld_x = a->W; ln.ld_y = a->W; ln.eps = a->eps;
    return ln;
}
inline int text_embed_validate(const tav_text_embed_args* a) {
    if (!a || !a->ids || !a->word || !a->pos || !a->type || !a->gamma || !a->beta || !a->pre || !a->pos_ids) return TAV_ERR_NULL;
    if (a->B <= 0 || a->S <= 0 || a->S > 1024 || a->W <= 0 || a->W % 4) return TAV_ERR_SHAPE;
    const tav_ln_args ln = text_embed_ln(a);
    return ln_fwd_validate(&ln);             // (once answered by tav_ln_fwd behind the first two launches: same codes, now in front of them)
}
inline int text_pos_threads(int64_t S) { int t = 64; while (t < S) t <<= 1; return t; }      // one thread per token: a power of two >= S
inline size_t scatter_add_lds(int64_t rows, int64_t W) { return 256 + (((size_t)rows * 4 + 15) & ~(size_t)15) + (size_t)16 * W * 4; }   // header + match list + 16 partial rows
inline int scatter_add_validate(bool have, int64_t rows, int64_t W, int64_t ntable) {
    if (!have) return TAV_ERR_NULL;
    if (rows <= 0 || W <= 0 || ntable <= 0 || W % 4 || W > SCAT_MAXW) return TAV_ERR_SHAPE;
    return scatter_add_lds(rows, W) > 150 * 1024 ? TAV_ERR_SHAPE : 0;                          // rows <= ~22 k tokens per call at W = 768
}
inline int patchify_validate(bool have, int dt, int64_t B, int64_t F, int64_t H, int64_t W, int64_t nkeep) {
    if (!have) return TAV_ERR_NULL;
    if (B <= 0 || F <= 0 || F % 2 || H % 16 || W % 16 || nkeep <= 0) return TAV_ERR_SHAPE;
    return is_float(dt) ? 0 : TAV_ERR_DTYPE;
}
inline int mask_to_index_validate(bool have, int64_t B, int64_t n, int64_t nkeep) {
    if (!have) return TAV_ERR_NULL;
    return (B <= 0 || n <= 0 || nkeep <= 0 || nkeep > n) ? TAV_ERR_SHAPE : 0;
}
inline int ragged_lens_validate(bool have, int64_t B, int64_t ntok, int64_t cap_true, int64_t cap_keep, int64_t base) {
    if (!have) return TAV_ERR_NULL;
    if (B <= 0 || ntok <= 0 || cap_true <= 0 || cap_true > ntok || cap_keep <= 0 || cap_keep > ntok || base < 0) return TAV_ERR_SHAPE;
    return (ntok > INT32_MAX / 2 || base > INT32_MAX / 2) ? TAV_ERR_SHAPE : 0;
}
inline int mean_pool_validate(bool have, int64_t B, int64_t S, int64_t W) {
    if (!have) return TAV_ERR_NULL;
    return (B <= 0 || S <= 0 || W <= 0 || W % 4) ? TAV_ERR_SHAPE : 0;
}
inline Launch mean_pool_fwd_launch(int64_t B, int64_t W) { return Launch{cdiv(W, 64), B, 1, 256, 0}; }
inline int head_validate(bool have, int64_t B, int64_t K, int64_t N, int64_t nmax) {
    if (!have) return TAV_ERR_NULL;
    return (B <= 0 || K <= 0 || N <= 0 || N > nmax) ? TAV_ERR_SHAPE : 0;
}
inline int classes_validate(bool have, int64_t B, int64_t C, int64_t bmax) {       // tav_cross_entropy, tav_step_stats (B <= INT32_MAX): one workgroup
    if (!have) return TAV_ERR_NULL;
    return (B <= 0 || B > bmax || C <= 0 || C > 64) ? TAV_ERR_SHAPE : 0;
}
inline int dropout_validate(bool have, int64_t n, float p) {
    if (!have) return TAV_ERR_NULL;
    return (n <= 0 || p < 0.f || p >= 1.f) ? TAV_ERR_SHAPE : 0;
}
inline int sumsq_partials(int ntensors) { return ntensors * SUMSQ_BLOCKS; }
inline int multi_tensor_validate(bool have, int ntensors) { return !have ? TAV_ERR_NULL : ((ntensors <= 0 || ntensors > 65535) ? TAV_ERR_SHAPE : 0); }   // y extent of the grid
inline int chunked_validate(bool have, int ntensors, int nchunks, int ngroups = 1) {
    if (!have) return TAV_ERR_NULL;
    return (ntensors <= 0 || nchunks <= 0 || ngroups < 1 || ngroups > OPT_MAX_GROUPS) ? TAV_ERR_SHAPE : 0;
}

// ------------------------------------------------------------------------------------------------ audio_frontend.hip
constexpr int C0_TT = 128;     // output steps per workgroup (conv0 forward): enough stores to amortise the weight loads of the prologue
constexpr int C0_BT = 512;     // output steps per workgroup of the conv0 weight gradient (4 time groups x 128 steps): half the partial blocks of 256 for the final reduce
constexpr int C0_MAXK = 16;
constexpr int WN_MAX_PARTS = 512, WN_PART_ROWS = 256, WN_MAXK = 128;   // weight norm: rows per part below the cap on parts; taps
inline int conv0_fwd_validate(bool have, int dt, int64_t B, int64_t T_in, int64_t T_out, int64_t C, int64_t K, int64_t stride) {
    if (!have) return TAV_ERR_NULL;
    if (B <= 0 || T_in <= 0 || T_out <= 0 || C <= 0 || C % 4 || K <= 0 || K > C0_MAXK || stride <= 0 || stride > 8) return TAV_ERR_SHAPE;
    if ((T_out - 1) * stride + K > T_in) return TAV_ERR_SHAPE;
    return is_float(dt) ? 0 : TAV_ERR_DTYPE;
}
inline Launch conv0_fwd_launch(int64_t B, int64_t T_out) { return Launch{cdiv(T_out, C0_TT), B, 1, 256, 0}; }
inline int conv0_bwd_validate(bool have, int dt, int64_t B, int64_t T_in, int64_t T_out, int64_t C, int64_t K, int64_t stride) {
    if (!have) return TAV_ERR_NULL;
    if (B <= 0 || T_in <= 0 || T_out <= 0 || C <= 0 || C % 8 || K <= 0 || K > 10 || stride <= 0 || stride > 8) return TAV_ERR_SHAPE;
    // tav_conv0_bwd_partials answers in an int (see gn_validate); factor by factor so that nothing overflows
    if (C > INT32_MAX || B > INT32_MAX / (C * (K + 1)) || (T_out - 1) / C0_BT + 1 > INT32_MAX / (B * C * (K + 1))) return TAV_ERR_SHAPE;
    return is_float(dt) ? 0 : TAV_ERR_DTYPE;
}
inline int conv0_bwd_partials(int64_t B, int64_t T_out, int64_t C, int64_t K) { return (int)(B * cdiv(T_out, C0_BT) * C * (K + 1)); }   // floats: [B * chunks][C][K + 1]
struct Conv0BwdPlan { int chunks, blocks; Launch partial, final_; };     // blocks = partial blocks the final kernel sums
inline Conv0BwdPlan conv0_bwd_plan(int64_t B, int64_t T_out, int64_t C, int64_t K) {
    const int64_t nc = cdiv(T_out, C0_BT);
    return Conv0BwdPlan{(int)nc, (int)(nc * B), Launch{nc, B, 1, 256, 0}, grid1(C * (K + 1), 64)};
}
inline int col2im_validate(bool have, int dt, int64_t B, int64_t T_in, int64_t T_out, int64_t C, int64_t K, int64_t stride) {
    if (!have) return TAV_ERR_NULL;
    if (B <= 0 || T_in <= 0 || T_out <= 0 || C <= 0 || C % 4 || K <= 0 || stride <= 0) return TAV_ERR_SHAPE;
    return is_float(dt) ? 0 : TAV_ERR_DTYPE;
}
inline int group_pad_validate(bool have, int sdt, int ddt, int64_t B, int64_t T, int64_t H, int64_t G, int64_t pad_l, int64_t pad_r) {
    if (!have) return TAV_ERR_NULL;
    if (B <= 0 || T <= 0 || H <= 0 || G <= 0 || H % G || (H / G) % 4 || pad_l < 0 || pad_r < 0) return TAV_ERR_SHAPE;
    return (is_float(sdt) && is_float(ddt) && !(sdt == TAV_BF16 && ddt == TAV_F32)) ? 0 : TAV_ERR_DTYPE;
}
inline int weight_norm_partials(int64_t H, int64_t Cg) { const int64_t nb = (H * Cg + WN_PART_ROWS - 1) / WN_PART_ROWS; return (int)(nb > WN_MAX_PARTS ? WN_MAX_PARTS : nb); }
inline int weight_norm_validate(bool have, int dt, int64_t H, int64_t Cg, int64_t K) {
    if (!have) return TAV_ERR_NULL;
    if (H <= 0 || Cg <= 0 || K <= 0 || K > WN_MAXK || H % Cg) return TAV_ERR_SHAPE;
    return is_float(dt) ? 0 : TAV_ERR_DTYPE;       // (tav_weight_norm_fwd once answered this behind its first two launches)
}
// both weight-norm entries: rows = H * Cg weight rows of K taps; workspace of the backward in float offsets: dw in the natural layout,
// the column-sum partials [parts][K], the K dots
struct WnPlan { int64_t rows, n; int parts, rows_per_part; Launch partial, final_, apply; int64_t ws_dw, ws_partials, ws_dots, ws_end; };
inline WnPlan weight_norm_plan(int64_t H, int64_t Cg, int64_t K) {
    const int64_t rows = H * Cg, n = rows * K;
    const int nb = weight_norm_partials(H, Cg);
    return WnPlan{rows, n, nb, (int)((rows + nb - 1) / nb), Launch{nb, 1, 1, 128, 0}, Launch{1, 1, 1, 128, 0}, grid1(n), 0, n, n + (int64_t)nb * K, n + (int64_t)nb * K + K};
}

// ------------------------------------------------------------------------------------------------ fp8.hip
constexpr int FP8_AMAX_BLOCK_GROUPS = 2048, FP8_AMAX_MAX_PARTS = 2048;       // groups of 4 per workgroup (>= 8 per thread) below the cap on workgroups
constexpr int FP8_STREAM_BLOCK_GROUPS = 1024, FP8_STREAM_MAX_BLOCKS = 8192;  // groups of 8 per workgroup of the streaming quantiser; it strides beyond
inline int fp8_amax_partials(int64_t rows, int64_t cols) {
    const int64_t nb = (rows * (cols / 4) + FP8_AMAX_BLOCK_GROUPS - 1) / FP8_AMAX_BLOCK_GROUPS;
    return (int)(nb < 1 ? 1 : (nb > FP8_AMAX_MAX_PARTS ? FP8_AMAX_MAX_PARTS : nb));
}
inline int fp8_amax_validate(bool have, int dt, int64_t rows, int64_t cols, int64_t ld) {
    if (!have) return TAV_ERR_NULL;
    if (rows <= 0 || cols <= 0 || cols % 4) return TAV_ERR_SHAPE;
    if (ld % 4) return TAV_ERR_ALIGN;
    return is_float(dt) ? 0 : TAV_ERR_DTYPE;
}
inline int fp8_quantize_validate(bool have, bool q, bool qt, int dt, int64_t rows, int64_t cols, int64_t ld, int64_t ld_q, int64_t ld_qt, int64_t rows_pad) {
    if (!have) return TAV_ERR_NULL;
    if (rows <= 0 || cols <= 0 || cols % 4) return TAV_ERR_SHAPE;
    if (ld % 4 || (q && ld_q % 4) || (qt && (ld_qt % 4 || rows_pad % 4 || rows_pad < rows || ld_qt < rows_pad))) return TAV_ERR_ALIGN;
    return is_float(dt) ? 0 : TAV_ERR_DTYPE;
}
// the streaming form (no transposed copy): 16-B aligned groups of 8 and 32-bit group indices
inline bool fp8_can_stream(bool qt, uintptr_t x, uintptr_t q, int64_t rows, int64_t cols, int64_t ld, int64_t ld_q) {
    return !qt && !(cols % 8 || ld % 8 || ld_q % 8 || rows * (cols / 8) >= (1ll << 31) || (x & 15) || (q & 7));
}
inline Launch fp8_stream_launch(int64_t rows, int64_t cols) { const int64_t nb = cdiv(rows * (cols / 8), FP8_STREAM_BLOCK_GROUPS); return Launch{nb < 1 ? 1 : (nb > FP8_STREAM_MAX_BLOCKS ? FP8_STREAM_MAX_BLOCKS : nb), 1, 1, 256, 0}; }
inline Launch fp8_tile_launch(int64_t rows_out, int64_t cols) { return Launch{cdiv(cols, 64), cdiv(rows_out, 64), 1, 256, 0}; }   // rows_out: rows_pad with a transposed copy
inline int splitk_reduce_validate(bool have, int nsplit, int64_t n_elems) {
    if (!have) return TAV_ERR_NULL;
    return (nsplit <= 0 || n_elems <= 0 || n_elems % 4) ? TAV_ERR_SHAPE : 0;
}

// ------------------------------------------------------------------------------------------------ specaug.hip
constexpr int SPEC_T = 256;              // threads of a draw workgroup
constexpr int SPEC_MAX_SPANS = 128;      // chosen starts kept in LDS
constexpr uint64_t SPEC_EPS_STRIDE = 1ull << 40;      // a tag owns the 2^40 indices behind it; its epsilon draw is the word after them
constexpr int SPEC_ROWS = 32;
constexpr int SPEC_MAX_PARTS = 1024;
inline bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
inline int specaug_draw_validate(bool have, int64_t B, int64_t L, float prob, int64_t length, int64_t min_masks) {
    if (!have) return TAV_ERR_NULL;
    if (B < 1 || L < 1 || length < 1 || min_masks < 0 || B > 0x7fffffff || L > 0x7fffffff || length > 0x7fffffff || min_masks > 0x7fffffff ||
        !(prob >= 0.f) || !(prob <= 1.f) || B * L > (int64_t)SPEC_EPS_STRIDE)
        return TAV_ERR_SHAPE;
    // the most spans a row can take: the kernel's n0 at len = L with eps replaced by its supremum (each rounded operation is monotone)
    const float top = floorf(((prob * (float)L) / (float)length) + 1.0f);
    int64_t cap = (int64_t)top > min_masks ? (int64_t)top : min_masks;
    if (L / length < cap) cap = L / length;
    return cap > SPEC_MAX_SPANS ? TAV_ERR_SHAPE : 0;
}
inline int specaug_shape(int64_t B, int64_t T, int64_t H) {
    return (B < 1 || T < 1 || H < 1 || H % 4 || H > 0x7fffffff || T > 0x7fffffff || B > 0x7fffffff || B * T > (int64_t)1 << 40) ? TAV_ERR_SHAPE : 0;
}
inline int specaug_fwd_validate(bool have, bool ptrs_aligned, int64_t B, int64_t T, int64_t H) {
    if (!have) return TAV_ERR_NULL;
    if (specaug_shape(B, T, H)) return TAV_ERR_SHAPE;
    return ptrs_aligned ? 0 : TAV_ERR_ALIGN;
}
inline int specaug_bwd_parts(int64_t rows) {
    const int64_t p = (rows + SPEC_ROWS - 1) / SPEC_ROWS;
    return (int)(p > SPEC_MAX_PARTS ? SPEC_MAX_PARTS : (p < 1 ? 1 : p));
}
inline int64_t specaug_bwd_ws_bytes(int64_t rows, int64_t H) { return (rows < 1 || H < 1) ? 0 : (int64_t)specaug_bwd_parts(rows) * H * (int64_t)sizeof(float); }
inline int specaug_bwd_validate(bool have, bool ptrs_aligned, bool dembed, int64_t workspace_bytes, int64_t B, int64_t T, int64_t H) {
    if (!have) return TAV_ERR_NULL;
    if (specaug_shape(B, T, H)) return TAV_ERR_SHAPE;
    if (dembed && workspace_bytes < specaug_bwd_ws_bytes(B * T, H)) return TAV_ERR_SHAPE;
    return ptrs_aligned ? 0 : TAV_ERR_ALIGN;
}
inline PartsPlan specaug_bwd_plan(int64_t rows, int64_t H) {
    const int np = specaug_bwd_parts(rows);
    return PartsPlan{np, (int)((rows + np - 1) / np), Launch{cdiv(H / 4, 256), np, 1, 256, 0}, grid1(H / 4, 64, 64)};
}

// ------------------------------------------------------------------------------------------------ video_transform.hip
constexpr int VX_TW = 32, VX_TH = 8;      // output tile of a workgroup: 32 columns (128-B store segments per channel plane) x 8 rows
constexpr int VX_MAX = 16384;             // sizes up to here keep (2 o + 1) n_in inside int32
inline bool vx_size_ok(int32_t v) { return v >= 1 && v <= VX_MAX; }
inline int video_clip_validate(bool have, const tav_clip_xform* x) {
    if (!have) return TAV_ERR_NULL;
    if (x->src_dtype != TAV_U8 && x->src_dtype != TAV_F32) return TAV_ERR_DTYPE;
    if (x->T < 1 || !vx_size_ok(x->H) || !vx_size_ok(x->W) || !vx_size_ok(x->out_h) || !vx_size_ok(x->out_w)) return TAV_ERR_SHAPE;
    if (x->sT < 0 || x->sH < 0 || x->sW < 0 || x->sC < 0) return TAV_ERR_SHAPE;
    if (x->nf < 1 || x->nf > 32) return TAV_ERR_SHAPE;
    for (int i = 0; i < x->nf; ++i)
        if (x->frame[i] < 0 || x->frame[i] >= x->T) return TAV_ERR_SHAPE;
    if (!vx_size_ok(x->crop_h) || !vx_size_ok(x->crop_w) || x->crop_top < 0 || x->crop_left < 0 || x->crop_top > x->H - x->crop_h ||
        x->crop_left > x->W - x->crop_w)
        return TAV_ERR_SHAPE;
    if (x->mid_h != 0 || x->mid_w != 0)
        if (!vx_size_ok(x->mid_h) || !vx_size_ok(x->mid_w)) return TAV_ERR_SHAPE;
    return 0;
}
inline Launch video_clip_launch(const tav_clip_xform* x) { return Launch{cdiv(x->out_w, VX_TW), cdiv(x->out_h, VX_TH), x->nf, VX_TW * VX_TH, 0}; }

// ------------------------------------------------------------------------------------------------ audio_resample.hip
constexpr int AR_THREADS = 256;
constexpr int AR_MAX_PER_THREAD = 4;      // a tile is 256, 512, 768 or 1024 outputs: the largest whose input span fits AR_SPAN_MAX
constexpr int AR_SPAN_MAX = 8192;         // f32 elements of LDS for the channel mean of a tile's input span (32 KiB)
constexpr int AR_TABLE_MAX = 6144;        // f32 elements of LDS for the compact table (24 KiB): 441/160 needs 160 x 35, 441/320 320 x 17
// Row pitch of the table in LDS.  The lanes of a wave make consecutive outputs, hence consecutive phases p at the same k: lane l reads
// p_l * pitch + k.  ds_read_b32 serves 32 lanes per cycle from 32 four-byte banks, so an odd pitch puts them on 32 different banks (ntap = 34
// itself would pair them up).
inline int ar_pitch(int ntap) { return ntap | 1; }
// the most input positions `tile` consecutive outputs read: they span at most (tile + n - 2) / n + 1 values of q
inline int64_t ar_span(int64_t tile, int64_t o, int64_t n, int64_t width) { return ((tile + n - 2) / n + 1) * o + 2 * width; }
// outputs per workgroup for a rate pair, 0 when not even 256 outputs' input span fits the LDS buffer (o / n beyond about 30)
inline int audio_resample_tile(int32_t o, int32_t n, int32_t width) {
    if (o < 1 || n < 1 || width < 0) return 0;
    for (int m = AR_MAX_PER_THREAD; m >= 1; --m)
        if (ar_span((int64_t)m * AR_THREADS, o, n, width) <= AR_SPAN_MAX) return m * AR_THREADS;
    return 0;
}
struct ResamplePlan { int64_t L_out; int tile, table_in_lds; Launch launch; };
// (the plan is part of the check: a rate pair without a tile, or more than 2^31 - 1 workgroups, is refused)
inline int audio_resample_validate(bool have, const tav_resample_args* a, ResamplePlan* P) {
    if (!have) return TAV_ERR_NULL;
    if (a->src_dtype != TAV_F32 && a->src_dtype != TAV_I16) return TAV_ERR_DTYPE;
    if (a->C < 1 || a->C > 32 || a->L < 1 || a->L > (1ll << 40) || a->sC < 0 || a->sL < 0) return TAV_ERR_SHAPE;
    if (a->o < 1 || a->n < 1 || a->ntap < 1 || a->width < 0 || a->o > (1 << 20) || a->n > (1 << 20) || a->width > (1 << 24)) return TAV_ERR_SHAPE;
    if ((int64_t)a->n * a->ntap > (1ll << 24)) return TAV_ERR_SHAPE;
    if (a->first_max < 0 || (int64_t)a->first_max + a->ntap > 2ll * a->width + a->o) return TAV_ERR_SHAPE;
    P->L_out = ((int64_t)a->n * a->L + a->o - 1) / a->o;
    if (a->T_row < P->L_out || a->T_row > (1ll << 40)) return TAV_ERR_SHAPE;
    P->tile = audio_resample_tile(a->o, a->n, a->width);
    if (P->tile == 0) return TAV_ERR_SHAPE;
    P->launch = Launch{(a->T_row + P->tile - 1) / P->tile, 1, 1, AR_THREADS, 0};
    if (P->launch.gx > 0x7fffffffll) return TAV_ERR_SHAPE;
    P->table_in_lds = (int64_t)a->n * ar_pitch(a->ntap) <= AR_TABLE_MAX;
    return 0;
}
}  // namespace plan
}  // namespace tav
