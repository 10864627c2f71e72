// Host decisions of the forced-alignment entry points (ctc_align.hip, include/tavhip_align.h) as pure functions: argument checks, the launch
// plan of tav_ctc_align, its LDS carve-up and its workspace.  Only the public headers and the standard library, no HIP type: any C++17 host
// compiler builds it (tests/host/align_plan_check.cpp runs it under ASan + UBSan).  entry_plan.h has the same role for the other entries.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "../../include/tavhip_align.h"

namespace tav {
namespace plan {

constexpr int ALIGN_ABI_VERSION = 1;
constexpr int64_t ALIGN_MAX_T = 4096;         // frames of one utterance (82 s of wav2vec2 frames)
constexpr int64_t ALIGN_MAX_N = 2048;         // tokens of one transcript
constexpr int64_t ALIGN_MAX_V = 128;          // labels
constexpr int64_t ALIGN_MAX_B = 65535;
constexpr int ALIGN_MAX_BLOCK = 1024;         // threads: beyond N + 1 = 1024 columns a thread keeps 2 or 3 of them
constexpr int ALIGN_MAX_TPT = 3;
constexpr int ALIGN_STAGE_ELEMS = 2048;       // f32 elements of one emission stage: 64 frames of 32 labels (8 KiB); a thread of the smallest
constexpr int ALIGN_PREFETCH = 32;            // workgroup (64) holds the next stage in ALIGN_STAGE_ELEMS / 64 registers while it runs this one
constexpr int ALIGN_SMALL_BLOCK = 256;        // up to here the kernel is built for 256 threads (512 VGPRs a lane); beyond, for 1024 (128 VGPRs),
constexpr int ALIGN_PREFETCH_BIG = 8;         // where 320 or more threads hold a stage in 8 registers each
constexpr int64_t ALIGN_LDS_MAX = 128 * 1024; // of the CU's 160 KiB
constexpr int64_t LSM_MAX_V = 65536;          // tav_ctc_log_softmax: columns of a row
constexpr int LSM_ROWS = 4;                   // rows (waves) per workgroup

inline int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

inline int log_softmax_validate(bool have, int64_t R, int64_t V, int64_t ld_in, int64_t ld_out) {
    if (!have) return TAV_ERR_NULL;
    if (R <= 0 || R > (int64_t)0x7fffffff * LSM_ROWS || V <= 0 || V > LSM_MAX_V || ld_in < V || ld_out < V) return TAV_ERR_SHAPE;
    return 0;
}
inline int64_t log_softmax_blocks(int64_t R) { return (R + LSM_ROWS - 1) / LSM_ROWS; }

// LDS of a tav_ctc_align workgroup, byte offsets (each a multiple of 16), and the launch shape
struct AlignPlan {
    int block, tpt, stage_frames, nwords, bits_frames;
    int64_t off_stage, off_seam, off_misc, off_path, off_prob, off_segs, off_bits, lds_bytes;
    int64_t ws_row_bytes;       // decision words of one utterance in the workspace: [T][nwords] of 8 bytes; 0 when they stay in LDS
};
inline int align_shape_validate(int64_t T, int64_t N, int64_t V) {
    return (T < 1 || T > ALIGN_MAX_T || N < 1 || N > ALIGN_MAX_N || V < 1 || V > ALIGN_MAX_V) ? TAV_ERR_SHAPE : 0;
}
// (T, N: the longest row of the batch; the shape must have passed align_shape_validate)
inline AlignPlan align_plan(int64_t T, int64_t N, int64_t V) {
    AlignPlan P = {};
    const int64_t cols = N + 1;
    P.tpt = (int)((cols + ALIGN_MAX_BLOCK - 1) / ALIGN_MAX_BLOCK);
    P.block = (int)align_up((cols + P.tpt - 1) / P.tpt, 64);
    P.nwords = P.block / 64 * P.tpt;                       // one ballot word per wave, column slot and frame
    int s = 64;
    while (s > 1 && s * V > ALIGN_STAGE_ELEMS) s >>= 1;
    P.stage_frames = s;
    int64_t o = 0;
    P.off_stage = o; o += align_up(2 * (int64_t)s * V * 4, 16);
    P.off_seam = o;  o += 2 * 16 * 4;                      // [2][waves <= 16] f32
    P.off_misc = o;  o += 16 * 4;
    P.off_path = o;  o += align_up(T * 2, 16);             // u16 per frame: token index | changed << 15
    P.off_prob = o;  o += align_up(T * 4, 16);
    P.off_segs = o;  o += align_up((N + 1) * 4, 16);
    P.off_bits = o;
    const int64_t per_frame = (int64_t)P.nwords * 8, room = (ALIGN_LDS_MAX - o) / per_frame;
    if (T <= room) {
        P.bits_frames = (int)T;
        P.ws_row_bytes = 0;
    } else {
        P.bits_frames = (int)room;
        P.ws_row_bytes = T * per_frame;
    }
    P.lds_bytes = o + (int64_t)P.bits_frames * per_frame;
    return P;
}
inline int64_t align_ws_bytes(int64_t B, int64_t T, int64_t N, int64_t V) {
    if (B < 1 || B > ALIGN_MAX_B) return TAV_ERR_SHAPE;
    if (const int rc = align_shape_validate(T, N, V)) return rc;
    return B * align_plan(T, N, V).ws_row_bytes;
}
// the order of the tests is the order of the codes: pointers, sizes, then strides
inline int align_validate(const tav_ctc_align_args* a, AlignPlan* P) {
    if (!a || !a->emission || !a->tokens || !a->n_frames || !a->n_tokens || !a->path_token || !a->path_prob || !a->seg || !a->seg_score || !a->span)
        return TAV_ERR_NULL;
    if (a->B < 1 || a->B > ALIGN_MAX_B) return TAV_ERR_SHAPE;
    if (const int rc = align_shape_validate(a->Tmax, a->Nmax, a->V)) return rc;
    if (a->ld < a->V || a->ld > (1ll << 24) || a->blank_id < 0 || a->blank_id >= a->V) return TAV_ERR_SHAPE;
    if (a->ld % 4) return TAV_ERR_ALIGN;
    *P = align_plan(a->Tmax, a->Nmax, a->V);
    if (P->ws_row_bytes) {
        if (!a->workspace) return TAV_ERR_NULL;
        if (a->workspace_bytes < a->B * P->ws_row_bytes) return TAV_ERR_SHAPE;
        if ((uintptr_t)a->workspace % 8) return TAV_ERR_ALIGN;
    }
    return 0;
}
inline void align_plan_public(const AlignPlan& P, tav_align_plan* out) {
    out->block = P.block;
    out->tokens_per_thread = P.tpt;
    out->frames_per_stage = P.stage_frames;
    out->bits_frames = P.bits_frames;
    out->lds_bytes = P.lds_bytes;
    out->ws_bytes_per_row = P.ws_row_bytes;
}
}  // namespace plan
}  // namespace tav
