// Host decisions of the GEMM entry points (gemm.hip) as pure functions: argument checks, tile and split planners, launch geometry, the list of
// gemm_nt_kernel instantiations and the workspace layout of the grouped weight gradients.  Only the public ABI header and the standard
// library: any C++17 host compiler builds it (tests/host/gemm_plan_check.cpp runs it under ASan + UBSan); gemm.hip keeps the enqueue.
#pragma once
#include <stdint.h>
#include <algorithm>
#include "../../include/tavhip.h"

namespace tav {
namespace plan {

inline int elem_size(int dtype) { return dtype == TAV_FP8 ? 1 : (dtype == TAV_BF16 ? 2 : 4); }

// ------------------------------------------------------------------------------------------------ NT: checks
inline int nt_validate(const tav_gemm_nt_args* a, bool need_ptrs) {
    if (!a || (need_ptrs && (!a->A || !a->B || !a->C))) return TAV_ERR_NULL;
    if (a->M <= 0 || a->N <= 0 || a->K <= 0) return TAV_ERR_SHAPE;
    const int es = elem_size(a->in_dtype);
    if (a->in_dtype != TAV_BF16 && a->in_dtype != TAV_F32 && a->in_dtype != TAV_FP8) return TAV_ERR_DTYPE;
    if (a->in_dtype == TAV_F32 && a->out_dtype != TAV_F32) return TAV_ERR_DTYPE;
    if (a->out_dtype != TAV_F32 && a->out_dtype != TAV_BF16) return TAV_ERR_DTYPE;
    if ((a->K * es) % 128 != 0) return TAV_ERR_SHAPE;      // K-tile = 128 bytes
    if ((a->M * a->lda + a->K) * es >= (1ll << 32) || (a->N * a->ldb + a->K) * es >= (1ll << 32)) return TAV_ERR_SHAPE;   // 32-bit staging offsets per (zb, zg) slice
    if (a->N % 4 != 0) return TAV_ERR_SHAPE;
    {   // the epilogue addresses a tile's rows with 32-bit element offsets from the tile's first row
        const int64_t ldmax = std::max(std::max(a->ldc, a->C_pre ? a->ld_pre : 0), std::max(a->gelu_in ? a->ld_gelu_in : 0, a->resid ? a->ld_resid : 0));
        if (ldmax < 0 || 256 * ldmax + a->N >= (1ll << 30)) return TAV_ERR_SHAPE;
    }
    const int pk = 16 / es;
    if (a->lda % pk || a->ldb % pk || a->ldc % 4) return TAV_ERR_ALIGN;
    if (a->a_zb % pk || a->a_zg % pk || a->b_zb % pk || a->b_zg % pk || a->c_zb % 4 || a->c_zg % 4 || a->gelu_zb % 4) return TAV_ERR_ALIGN;
    return 0;
}

// ------------------------------------------------------------------------------------------------ NT: tile picker
// tile height: minimise (tiles per CU, rounded up) x (cost of one tile ~ TM + fixed overhead)
inline int nt_small_tile(int M, int N, int nz) {
    const int tiles_n = (N + 127) / 128;
    int tm = 4;
    double best = 1e30;
    for (int c = 4; c >= 2; --c) {
        const long tiles = (long)((M + 32 * c - 1) / (32 * c)) * tiles_n * nz;
        const double cost = (double)((tiles + 255) / 256) * (c + 0.8);
        if (cost < best - 1e-9) { best = cost; tm = c; }
    }
    return tm;
}
// Fitted launch times in microseconds: rounds x (K-tiles x time per K-tile + prologue and epilogue), constants from tools/gpu_ab.py `layer`
// at batch 32 and 8 with per-tile hints (profiles/r02_microbench_*; they reproduce its timings within ~5 %).  K-tiles beyond the 36th cost
// 1.3-1.6x (K = 3072 operands; not a channel-aliasing effect -- padding the row stride changes nothing).
// `epi`: bit 0 f32 residual / accumulate read, bit 1 f32 output, bit 2 GELU, bit 3 gelu' side input, bit 4 second output.
inline double nt_small_us(int M, int N, double nk, int nz, int tm, int epi) {
    static const double slots[5] = {0, 0, 768, 512, 512}, tk[5] = {0, 0, 0.56, 0.72, 0.85}, fix[5] = {0, 0, 3.6, 4.0, 4.4};
    const long t = (long)((M + 32 * tm - 1) / (32 * tm)) * ((N + 127) / 128) * nz;
    // two workgroups per CU hide one's epilogue behind the other's main loop: the residual read costs little after a short K loop
    const double e = ((epi & 1) ? 2.0 + 0.2 * nk : 0.0) + ((epi & 2) ? 2.0 : 0.0) + ((epi & 4) ? 2.0 : 0.0) + ((epi & 8) ? 1.0 : 0.0) + ((epi & 16) ? 2.5 : 0.0);
    const double kt = (nk <= 36.0 ? nk : 36.0 + 1.6 * (nk - 36.0)) * tk[tm];
    return (double)((long)((t + slots[tm] - 1) / slots[tm])) * (kt + fix[tm] + e * tm / 4.0);
}
inline double nt_big_round_us(double nk, int epi) {
    // (3 + 2 ring: 1.37-1.52 us per K-tile at every K measured)
    const double kt = nk * 1.45;
    return kt + 6.5 + ((epi & 1) ? 9.0 : 0.0) + ((epi & 2) ? 4.0 : 0.0) + ((epi & 4) ? 3.0 : 0.0) + ((epi & 8) ? 4.7 : 0.0) + ((epi & 16) ? 6.7 : 0.0);
}
// Returns the tile for the launch; when `rows_big` is given and a mixed schedule is faster, *rows_big < M is the number of leading rows that
// take the 256 x 256 tile (whole rounds of 256 workgroups) and *tm_rest the 128-wide tile of a second launch over the remaining rows.
inline int nt_pick_tile(int M, int N, int K, int nz, bool bf16_in, int epi, int* rows_big = nullptr, int* tm_rest = nullptr) {
    int tm = nt_small_tile(M, N, nz);
    if (rows_big) *rows_big = M;
    // 256x256 (8 waves, one workgroup per CU) against the 128-wide winner.  The big tile stages half the bytes per FLOP (1.35 PFLOP/s at
    // 4096^3 against 1.15) but nothing on its CU computes while it runs its epilogue, whereas two 128-wide workgroups per CU overlap one's
    // epilogue with the other's main loop: memory-heavy epilogues (f32 residual in, f32 out) favour the small tile, plain bf16 outputs the
    // big one.  A last, partly filled round of big tiles costs a whole round: when the grid is a few rounds long (N = 768 at batch 32:
    // 2.14 rounds) the rows of that last round go to a second launch with the small tile instead.
    if (bf16_in && M >= 256 && N >= 256) {
        const double nk = (double)K / 64.0;
        const long tn_big = (N + 255) / 256;
        const long t_big = (long)((M + 255) / 256) * tn_big * nz;
        const double us_small = nt_small_us(M, N, nk, nz, tm, epi);
        const double big_round = nt_big_round_us(nk, epi);
        const double us_big = (double)((t_big + 255) / 256) * big_round;
        double us_best = us_small;
        if (us_big < 0.98 * us_small) { tm = 16; us_best = us_big; }
        const long full = t_big / 256;
        if (rows_big && nz == 1 && full >= 1 && t_big % 256 != 0) {
            const long m_tiles = full * 256 / tn_big;
            const int rows_a = (int)(m_tiles * 256), m_rest = M - rows_a;
            if (m_tiles >= 1 && m_rest > 0) {
                const int tr = nt_small_tile(m_rest, N, 1);
                const double us_split = (double)((m_tiles * tn_big + 255) / 256) * big_round + nt_small_us(m_rest, N, nk, 1, tr, epi) + 2.0;   // + the seam between two launches
                if (us_split < 0.93 * us_best) { tm = 16; *rows_big = rows_a; *tm_rest = tr; }   // (the model is good to ~5 %: only clear wins)
            }
        }
    }
    return tm;
}
// The tile plan of one call: `tm` for the first `rows_big` rows (all of them unless a mixed schedule wins), `tm_rest` for the others.
inline void nt_plan(const tav_gemm_nt_args* a, int* tm_out, int* rows_big, int* tm_rest) {
    const int es = elem_size(a->in_dtype);
    const int nz = (int)((a->nzb > 0 ? a->nzb : 1) * (a->nzg > 0 ? a->nzg : 1));
    int tm = a->tile_m_hint & 31;                            // 2/3/4: 64/96/128 x 128 tiles (4 waves); 8: 256 x 128, 16: 256 x 256 (8 waves); 17: as 0 but one launch
    const bool may_split = tm == 0 && a->in_dtype == TAV_BF16 && nz == 1;
    *rows_big = (int)a->M; *tm_rest = 4;
    if (a->in_dtype == TAV_F32 && (tm == 8 || tm == 16)) tm = 4;
    if (tm != 8 && tm != 16 && (tm < 2 || tm > 4))
        tm = nt_pick_tile((int)a->M, (int)a->N, (int)(a->K * es / 2), nz, a->in_dtype != TAV_F32,
                          ((a->resid || a->accumulate) ? 1 : 0) | (a->out_dtype == TAV_F32 ? 2 : 0) | ((a->act & 3) ? 4 : 0) | (a->gelu_in ? 8 : 0) | (a->C_pre ? 16 : 0),
                          may_split ? rows_big : nullptr, tm_rest);
    if (a->in_dtype == TAV_FP8 && tm != 16) tm = 4;          // fp8 operands: the 128 x 128 and 256 x 256 tiles only
    *tm_out = tm;
}

// ------------------------------------------------------------------------------------------------ NT: the kernels that exist
// Epilogue flavours: the values of gemm.hip's NT_* (it asserts that).  The transformer layers' epilogues are straight-line code, everything
// else takes the generic one.
enum { EPI_GEN = 0, EPI_PLAIN = 1, EPI_RESID = 2, EPI_GELU_D = 3, EPI_MUL_D = 4 };

// THE list of gemm_nt_kernel<in, out, TM, NST, NW, TNW, EPI> instantiations: X(IN, OUT, TM, NST, NW, TNW, EPI) once per kernel.  gemm.hip
// attaches the function pointers in the same order; nt_launch() returns only keys from it (proved over every input by gemm_plan_check.cpp).
//   _TILES   : the 64 / 96 / 128 x 128 tiles (4 waves) at one ring depth
//   _FLAVOUR : one epilogue flavour where flavours exist -- the 256 x 256 tile and ring depths 4 and 2 of the 128-wide tiles
//   _FLAVOUR3: the same with, in between, what exists with the generic epilogue ONLY: the 256 x 128 tile and ring depth 3
// The order of the list is the order of the kernels in the code object.  It is the order in which the launch ladders this list replaced
// named them (hence fp8 first and _FLAVOUR3): the code object stayed byte-identical.  Nothing else depends on the order.
#define TAV_NT_TILES(X, IN, OUT, NST, EPI) X(IN, OUT, 4, NST, 4, 4, EPI) X(IN, OUT, 3, NST, 4, 4, EPI) X(IN, OUT, 2, NST, 4, 4, EPI)
#define TAV_NT_FLAVOUR(X, IN, OUT, EPI) X(IN, OUT, 4, 2, 8, 8, EPI) TAV_NT_TILES(X, IN, OUT, 4, EPI) TAV_NT_TILES(X, IN, OUT, 2, EPI)
#define TAV_NT_FLAVOUR3(X, IN, OUT, EPI) \
    X(IN, OUT, 4, 2, 8, 8, EPI) X(IN, OUT, 4, 3, 8, 4, GEN) TAV_NT_TILES(X, IN, OUT, 4, EPI) TAV_NT_TILES(X, IN, OUT, 3, GEN) TAV_NT_TILES(X, IN, OUT, 2, EPI)
#define TAV_NT_KERNELS(X)                                                                                                        \
    /* fp8: flavours only for the 256 x 256 tile (the one the video stack runs on); ring depth 2 */                              \
    X(FP8, BF16, 4, 2, 8, 8, PLAIN) X(FP8, BF16, 4, 2, 8, 8, GELU_D) X(FP8, BF16, 4, 2, 8, 8, MUL_D) X(FP8, BF16, 4, 2, 8, 8, GEN) \
    X(FP8, F32, 4, 2, 8, 8, PLAIN) X(FP8, F32, 4, 2, 8, 8, RESID) X(FP8, F32, 4, 2, 8, 8, GEN)                                    \
    X(FP8, BF16, 4, 2, 4, 4, GEN) X(FP8, F32, 4, 2, 4, 4, GEN)                                                                    \
    TAV_NT_FLAVOUR3(X, BF16, BF16, PLAIN) TAV_NT_FLAVOUR(X, BF16, BF16, GELU_D) TAV_NT_FLAVOUR(X, BF16, BF16, MUL_D) TAV_NT_FLAVOUR(X, BF16, BF16, GEN) \
    TAV_NT_FLAVOUR3(X, BF16, F32, PLAIN) TAV_NT_FLAVOUR(X, BF16, F32, RESID) TAV_NT_FLAVOUR(X, BF16, F32, GEN)                    \
    /* f32: generic epilogue, ring depth 2, 4 waves */                                                                           \
    X(F32, F32, 4, 2, 4, 4, GEN) X(F32, F32, 3, 2, 4, 4, GEN) X(F32, F32, 2, 2, 4, 4, GEN)

struct NtKey {
    int8_t in, out, tm, nst, nw, tnw, epi;                   // dtype codes and the template arguments TM, NST, NW, TNW, EPI
};
constexpr bool operator==(const NtKey& a, const NtKey& b) {
    return a.in == b.in && a.out == b.out && a.tm == b.tm && a.nst == b.nst && a.nw == b.nw && a.tnw == b.tnw && a.epi == b.epi;
}
#define TAV_NT_KEY(IN, OUT, TM, NST, NW, TNW, EPI) {TAV_##IN, TAV_##OUT, TM, NST, NW, TNW, EPI_##EPI},
constexpr NtKey nt_keys[] = {TAV_NT_KERNELS(TAV_NT_KEY)};
#undef TAV_NT_KEY
constexpr int nt_num_keys = (int)(sizeof(nt_keys) / sizeof(nt_keys[0]));
inline int nt_key_index(const NtKey& k) {                    // -1: no such kernel
    for (int i = 0; i < nt_num_keys; ++i)
        if (nt_keys[i] == k) return i;
    return -1;
}

// ------------------------------------------------------------------------------------------------ NT: one launch
struct NtLaunch {
    NtKey key;
    int tiles_m, tiles_n;
    unsigned grid_x, grid_y, block;
    size_t lds;
};
// Kernel and geometry of one launch: tile `tm` (as nt_plan gives it) over the M rows of this launch.
inline NtLaunch nt_launch(const tav_gemm_nt_args* a, int M, int tm) {
    const int in = a->in_dtype, out = a->out_dtype;
    const int nzb = a->nzb > 0 ? a->nzb : 1, nzg = a->nzg > 0 ? a->nzg : 1;
    const int bm = tm >= 8 ? 256 : 32 * tm, bn = tm == 16 ? 256 : 128;
    NtLaunch L;
    L.tiles_m = (M + bm - 1) / bm;
    L.tiles_n = ((int)a->N + bn - 1) / bn;
    const long wgs = (long)L.tiles_m * L.tiles_n * nzb * nzg;
    // Ring depth.  Large grids run two workgroups per CU and are bound by the L2->LDS intake, where depth changes nothing: 2.
    // A grid of at most one workgroup per CU (the text / audio / fusion branches' N = 768 GEMMs) is LATENCY bound instead -- a lone
    // workgroup waits out every DMA round trip -- and has the whole LDS to itself: 4 buffers (3 tiles in flight).
    int nst = (a->tile_m_hint >> 5) & 7;                     // tuning: LDS ring depth 2..4 (0 = let the library choose)
    if (tm == 8) nst = 3;
    else if (tm == 16) nst = 2;
    else if (nst < 2 || nst > 4) nst = (wgs <= 256 && in == TAV_BF16) ? 4 : 2;
    if (in != TAV_BF16) nst = 2;
    L.grid_x = (unsigned)(L.tiles_m * L.tiles_n); L.grid_y = (unsigned)(nzb * nzg); L.block = tm >= 8 ? 512 : 256;
    // 256x128: 3 x 48 KB (its f32 epilogue tile needs 128 KB); 256x256: 2 x 64 KB, or 3 A + 2 B images = 160 KB (bf16, R25)
    L.lds = (tm == 16 && in == TAV_BF16) ? (size_t)160 * 1024 : (size_t)nst * (bm + bn) * 128;
    // the epilogue flavour the arguments ask for ...
    const bool side = a->resid || a->C_pre || a->gelu_in || a->accumulate;
    int epi = EPI_GEN;
    if (!side && a->act == 0) epi = EPI_PLAIN;
    else if (a->resid && !a->C_pre && !a->gelu_in && !a->accumulate && a->act == 0 && out == TAV_F32) epi = EPI_RESID;
    else if (a->C_pre && (a->act & 3) == 3 && !a->resid && !a->gelu_in && !a->accumulate && out == TAV_BF16) epi = EPI_GELU_D;
    else if (a->gelu_in && (a->act & 4) && !(a->act & 3) && !a->resid && !a->C_pre && !a->accumulate && out == TAV_BF16) epi = EPI_MUL_D;
    // ... and where it exists: not at ring depth 3 (which includes the 256 x 128 tile), not for f32 operands, for fp8 only at 256 x 256
    if (nst == 3 || in == TAV_F32 || (in == TAV_FP8 && tm != 16)) epi = EPI_GEN;
    L.key = NtKey{(int8_t)in, (int8_t)out, (int8_t)(tm >= 8 ? 4 : tm), (int8_t)nst, (int8_t)(tm >= 8 ? 8 : 4), (int8_t)(tm == 16 ? 8 : 4), (int8_t)epi};
    return L;
}

// Second launch of a mixed schedule: rows [rows_big, M) -- byte offsets of its A, C, C_pre and gelu_in, element offset of its f32 resid.
struct NtSplit {
    int M_rest;
    long a_bytes, c_bytes, pre_bytes, gelu_bytes, resid_elems;
};
inline NtSplit nt_split(const tav_gemm_nt_args* a, int rows_big) {
    const long r = rows_big, es = elem_size(a->in_dtype), oes = elem_size(a->out_dtype);
    return NtSplit{(int)a->M - rows_big, r * a->lda * es, r * a->ldc * oes, r * a->ld_pre * oes, r * a->ld_gelu_in * es, r * a->ld_resid};
}

// ------------------------------------------------------------------------------------------------ TN: checks and planners
constexpr int TN_PROBLEMS_MAX = 4;                           // gemm.hip's TN_GROUP_MAX (it asserts that)

// One weight-gradient problem A [rows x N1], B [rows x N2] -> out, for tav_gemm_tn (its own batch strides and batch count) and for every
// problem of tav_gemm_tn_grouped / _grouped_ws (a_zb = b_zb = 0, nbatch = 1; rows and dtype were checked by the caller, so those two
// tests cannot fire there).  The order of the tests is the order of tav_gemm_tn's codes and is merely preserved.
inline int tn_validate_problem(const void* A, const void* B, const void* out, int64_t N1, int64_t N2, int64_t lda, int64_t ldb, int64_t a_zb,
                               int64_t b_zb, int64_t rows_per_batch, int64_t nbatch, int dtype) {
    if (!A || !B || !out) return TAV_ERR_NULL;
    if (N1 <= 0 || N2 <= 0 || rows_per_batch <= 0 || nbatch <= 0) return TAV_ERR_SHAPE;
    if (dtype != TAV_BF16 && dtype != TAV_F32) return TAV_ERR_DTYPE;
    const int es = elem_size(dtype), pk = 16 / es;
    if (N1 % pk || N2 % pk || N2 % 4) return TAV_ERR_SHAPE;
    if (lda % pk || ldb % pk || a_zb % pk || b_zb % pk) return TAV_ERR_ALIGN;
    if ((rows_per_batch + 64) * (lda > ldb ? lda : ldb) * es >= (1ll << 32)) return TAV_ERR_SHAPE;   // 32-bit staging offsets
    return 0;
}
inline int tn_validate_group(const tav_gemm_tn_problem* probs, int nprob, int64_t rows, int dtype) {
    for (int k = 0; k < nprob; ++k) {
        const tav_gemm_tn_problem& a = probs[k];
        const int rc = tn_validate_problem(a.A, a.B, a.out, a.N1, a.N2, a.lda, a.ldb, 0, 0, rows, 1, dtype);
        if (rc != 0) return rc;
    }
    return 0;
}

constexpr double TN_SPLIT_PENALTY = 0.06;   // per extra token split (slab traffic), tuned with the four branch streams running concurrently
// The chunking tav_gemm_tn wants for a shape (arguments already checked positive).
inline void tn_splits(int64_t n1, int64_t n2, int64_t rows_per_batch, int64_t nbatch, int32_t* chunk_rows, int32_t* nsplit) {
    const long tiles = ((n1 + 127) / 128) * ((n2 + 127) / 128);
    // The kernel is resident at 2 workgroups per CU = 512 slots.  Pick the number of token chunks per batch entry so that
    // tiles * splits fills whole rounds of 512 (a 576-workgroup launch costs two rounds), chunks stay >= 256 tokens, and among
    // equally efficient choices the one with fewer splits (less slab traffic) wins.
    const long SLOTS = 512;
    // (start: one chunk per batch entry -- it stays when no candidate's score gets above -1, i.e. at nbatch >= 17, where the penalty alone is larger)
    long best_cpb = 1, best_cr = ((rows_per_batch + 63) / 64) * 64; double best_score = -1.0;
    const long max_cpb = (rows_per_batch + 255) / 256 > 0 ? (rows_per_batch + 255) / 256 : 1;
    for (long cpb = 1; cpb <= max_cpb && cpb <= 64; ++cpb) {
        long cr = (rows_per_batch + cpb - 1) / cpb;
        cr = ((cr + 63) / 64) * 64;
        const long real_cpb = (rows_per_batch + cr - 1) / cr;
        const long wgs = tiles * real_cpb * nbatch;
        const long rounds = (wgs + SLOTS - 1) / SLOTS;
        // per-round cost grows with the chunk length; total ~ rounds * cr; smaller is better.  Normalise by the ideal.
        const double work = (double)rounds * (double)cr;
        const double ideal = (double)tiles * nbatch * rows_per_batch / SLOTS;
        const double score = ideal / work - TN_SPLIT_PENALTY * (double)(real_cpb * nbatch);      // penalty per split (slab bytes)
        // (cr is the chunk of real_cpb too: rows <= real_cpb * cr and cr is a multiple of 64, while rows > (real_cpb - 1) * cr)
        if (score > best_score + 1e-9) { best_score = score; best_cpb = real_cpb; best_cr = cr; }
    }
    *chunk_rows = (int32_t)best_cr;
    *nsplit = (int32_t)(best_cpb * nbatch);
}

// Plan of a grouped launch: 256-wide tiles + `nsplit` token chunks when the problems are large enough to pay for the slabs, else the
// 128-wide kernel (every tile sums over all rows, no workspace).  flags: bit 0 forces the 256-wide form, bit 1 the 128-wide one,
// bits 8..11 an explicit split count (tests / tuning).
struct TnGroupPlan {
    bool big;
    int tw, nsplit;            // tile width 256 / 128; token splits (1 unless big)
    long chunk;                // tokens per split (multiple of 64)
    long ws_floats;            // workspace: the slabs of a split launch, then the bias partials [nsplit][tiles_2][N1] of every problem that wants a bias gradient
};
inline TnGroupPlan tn_big_plan(const tav_gemm_tn_problem* probs, int nprob, long rows, int dtype, int flags) {
    TnGroupPlan P{false, 128, 1, 0, 0};
    const bool can_big = dtype == TAV_BF16 && !(flags & 2);
    long tiles = 0, elems = 0;
    for (int k = 0; k < nprob; ++k) {
        tiles += ((probs[k].N1 + 255) / 256) * ((probs[k].N2 + 255) / 256);
        elems += probs[k].N1 * probs[k].N2;
    }
    P.big = can_big && ((flags & 1) || (rows >= 12288 && tiles >= 48));  // below: the 128-wide tiles (slab traffic, 84 % fill) are as fast or faster
    if (P.big) {
        int best = 1; double best_score = -1.0;
        for (int s2 = 1; s2 <= 4; ++s2) {
            if (s2 > 1 && rows / s2 < 2048) break;
            const long wgs = tiles * s2;
            const double fill = (double)wgs / (double)(((wgs + 255) / 256) * 256);
            const double score = fill - 0.04 * (s2 - 1);             // each extra split writes and re-reads one more f32 copy of the gradients
            if (score > best_score + 1e-9) { best_score = score; best = s2; }
        }
        if ((flags >> 8) & 15) best = (flags >> 8) & 15;
        P.nsplit = best;
        P.tw = 256;
    }
    P.chunk = ((rows + P.nsplit - 1) / P.nsplit + 63) / 64 * 64;
    P.ws_floats = P.nsplit > 1 ? (long)P.nsplit * elems : 0;
    for (int k = 0; k < nprob; ++k)
        if (probs[k].dbias) P.ws_floats += (long)P.nsplit * ((probs[k].N2 + P.tw - 1) / P.tw) * probs[k].N1;
    return P;
}
// The workspace-free form of tav_gemm_tn_grouped: 128-wide tiles, every tile sums over all rows.
inline TnGroupPlan tn_plain_plan(long rows) { return TnGroupPlan{false, 128, 1, (rows + 63) / 64 * 64, 0}; }
// (an empty split would leave its slab unwritten)
inline bool tn_has_empty_split(const TnGroupPlan& P, long rows) { return (long)(P.nsplit - 1) * P.chunk >= rows; }

// Where everything of a grouped launch lies.  All TN_PROBLEMS_MAX slots are filled: slot k >= nprob repeats the last problem (the kernels
// take fixed-size arrays and never index past n), except that its slab offset is the end of the slabs.
struct TnGroupLayout {
    int tiles_1[TN_PROBLEMS_MAX], tiles_2[TN_PROBLEMS_MAX];
    int tile_end[TN_PROBLEMS_MAX];         // prefix sums of tiles_1 * tiles_2 over the real problems
    long n4[TN_PROBLEMS_MAX], end4[TN_PROBLEMS_MAX];   // N1 * N2 / 4 and its prefix sums
    int nbias[TN_PROBLEMS_MAX];            // bias partial slots: nsplit * tiles_2
    long slab_off[TN_PROBLEMS_MAX];        // float offset of the slabs in the workspace; -1: the tiles write `out` (one split)
    long bias_off[TN_PROBLEMS_MAX];        // float offset of the bias partials (behind all slabs); -1: none
    int total, total_n1;                   // tiles, and the N1 of all real problems
    bool any_bias;
    long ws_floats;                        // end of the last workspace item (0 without workspace)
};
// `use_ws`: bias partials in the workspace, shared by the tiles of a tile row (tav_gemm_tn_grouped_ws); without it the t2 == 0 tiles sum
// the bias gradient straight into dbias and nothing lies in a workspace (then nsplit must be 1).
inline TnGroupLayout tn_group_layout(const tav_gemm_tn_problem* probs, int nprob, const TnGroupPlan& P, bool use_ws) {
    TnGroupLayout L;
    L.total = 0; L.total_n1 = 0; L.any_bias = false;
    long off = 0, end4 = 0;
    for (int k = 0; k < TN_PROBLEMS_MAX; ++k) {
        const tav_gemm_tn_problem& a = probs[k < nprob ? k : nprob - 1];
        L.tiles_1[k] = ((int)a.N1 + P.tw - 1) / P.tw; L.tiles_2[k] = ((int)a.N2 + P.tw - 1) / P.tw;
        L.slab_off[k] = P.nsplit > 1 ? off : -1;
        L.bias_off[k] = -1;
        L.n4[k] = a.N1 * a.N2 / 4;
        L.nbias[k] = P.nsplit * L.tiles_2[k];
        if (k < nprob) {
            if (P.nsplit > 1) off += (long)P.nsplit * a.N1 * a.N2;
            L.total += L.tiles_1[k] * L.tiles_2[k];
            end4 += L.n4[k]; L.total_n1 += (int)a.N1; L.any_bias |= a.dbias != nullptr;
        }
        L.tile_end[k] = L.total;
        L.end4[k] = end4;
    }
    for (int k = 0; use_ws && k < nprob; ++k) {                         // bias partials behind all slabs
        if (!probs[k].dbias) continue;
        L.bias_off[k] = off;
        off += (long)L.nbias[k] * probs[k].N1;
    }
    L.ws_floats = off;
    return L;
}
}  // namespace plan
}  // namespace tav
