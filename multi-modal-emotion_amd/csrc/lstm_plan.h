// Host decisions of the recurrent entry points (lstm.hip, include/tavhip_rnn.h) as pure functions: argument checks, the launch plan of
// tav_lstm_fwd / tav_lstm_bwd, their LDS carve-up and the workspace the forward leaves for the backward.  Only the public headers and the
// standard library, no HIP type: any C++17 host compiler builds it (tests/host/lstm_plan_check.cpp runs it under ASan + UBSan).
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "../../include/tavhip_rnn.h"

namespace tav {
namespace plan {

constexpr int RNN_ABI_VERSION = 1;
constexpr int LSTM_ROWS = 16;                    // batch rows of a workgroup: the N of one 16x16 MFMA tile
constexpr int LSTM_MAX_WAVES = 16;
constexpr int LSTM_MAX_TPW = 4;                  // 16-unit tiles per wave: 16 waves x 4 tiles x 16 units = Hp 1024
constexpr int64_t LSTM_HP_QUANT = 64;            // Hp = ceil(H / 64) 64: K elem_size % 128 == 0 for the GEMMs around the recurrence in bf16
constexpr int64_t LSTM_LDS_MAX = 160 * 1024;
constexpr int64_t LSTM_MAX_T = 1 << 16;
constexpr int64_t LSTM_MAX_B = 1 << 20;
constexpr int64_t LSTM_MAX_STRIDE = (int64_t)1 << 40;
constexpr int64_t LSTM_WS_ALIGN = 256;

inline int64_t lstm_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }
inline int lstm_elem_size(int dtype) { return dtype == TAV_BF16 ? 2 : 4; }

// LDS of the two kernels and the launch shape.  Pitches are in bytes; each row is padded by 16 bytes so that the 16 rows of a fragment
// read start in different banks.
struct LstmPlan {
    int block, waves, tpw, ntiles, Hp, es;
    int64_t h_pitch, bias_off, fwd_lds;   // forward: h_{t-1} of the tile, [2][LSTM_ROWS] rows of Hp elements (two images: one barrier a step), then b_hh [4 Hp] f32
    int64_t dz_pitch, bwd_lds;       // backward: dZ_t of the tile, [LSTM_ROWS] rows of 4 Hp elements
    int64_t lds_bytes;
    int64_t ws_gates_off, ws_cell_off, ws_bytes;
};

inline int lstm_shape_validate(int64_t B, int64_t T, int64_t H, int dtype) {
    if (dtype != TAV_BF16 && dtype != TAV_F32) return TAV_ERR_DTYPE;
    if (B < 1 || B > LSTM_MAX_B || T < 1 || T > LSTM_MAX_T || H < 1) return TAV_ERR_SHAPE;
    if (H > LSTM_MAX_WAVES * LSTM_MAX_TPW * 16) return TAV_ERR_SHAPE;
    const int64_t Hp = lstm_up(H, LSTM_HP_QUANT), es = lstm_elem_size(dtype);
    if (LSTM_ROWS * (4 * Hp * es + 16) > LSTM_LDS_MAX) return TAV_ERR_SHAPE;
    if ((T + 1) * B * 4 * Hp * 4 > ((int64_t)1 << 40)) return TAV_ERR_SHAPE;
    return 0;
}
// (the shape must have passed lstm_shape_validate)
inline LstmPlan lstm_plan(int64_t B, int64_t T, int64_t H, int dtype) {
    LstmPlan P = {};
    P.es = lstm_elem_size(dtype);
    P.Hp = (int)lstm_up(H, LSTM_HP_QUANT);
    P.ntiles = P.Hp / 16;
    P.tpw = (P.ntiles + LSTM_MAX_WAVES - 1) / LSTM_MAX_WAVES;
    P.waves = (P.ntiles + P.tpw - 1) / P.tpw;
    P.block = P.waves * 64;
    P.h_pitch = (int64_t)P.Hp * P.es + 16;
    P.bias_off = 2 * LSTM_ROWS * P.h_pitch;
    P.fwd_lds = P.bias_off + 4 * (int64_t)P.Hp * 4;
    P.dz_pitch = 4 * (int64_t)P.Hp * P.es + 16;
    P.bwd_lds = LSTM_ROWS * P.dz_pitch;
    P.lds_bytes = P.fwd_lds > P.bwd_lds ? P.fwd_lds : P.bwd_lds;
    P.ws_gates_off = 0;
    P.ws_cell_off = lstm_up(T * B * 4 * P.Hp * 4, LSTM_WS_ALIGN);
    P.ws_bytes = P.ws_cell_off + lstm_up((T + 1) * B * P.Hp * 4, LSTM_WS_ALIGN);
    return P;
}
inline int64_t lstm_blocks(int64_t B) { return (B + LSTM_ROWS - 1) / LSTM_ROWS; }
inline int64_t lstm_ws_bytes(int64_t B, int64_t T, int64_t H, int dtype) {
    if (const int rc = lstm_shape_validate(B, T, H, dtype)) return rc;
    return lstm_plan(B, T, H, dtype).ws_bytes;
}
inline void lstm_plan_public(const LstmPlan& P, tav_lstm_plan* out) {
    out->block = P.block;
    out->rows_per_wg = LSTM_ROWS;
    out->Hp = P.Hp;
    out->tiles_per_wave = P.tpw;
    out->lds_bytes = P.lds_bytes;
    out->ws_gates_off = P.ws_gates_off;
    out->ws_cell_off = P.ws_cell_off;
    out->ws_bytes = P.ws_bytes;
}
// a stride of (b, t) over rows of `width` elements: 16-byte vector access in either dtype, rows that do not overlap within one index
inline int lstm_stride_validate(int64_t sb, int64_t st, int64_t width) {
    if (sb < width || st < width || sb > LSTM_MAX_STRIDE || st > LSTM_MAX_STRIDE) return TAV_ERR_SHAPE;
    return 0;
}
// the order of the tests is the order of the codes: pointers, dtype, sizes, then strides and alignment
inline int lstm_fwd_validate(const tav_lstm_fwd_args* a, LstmPlan* P) {
    if (!a || !a->xproj || !a->w_hh || !a->y || !a->workspace) return TAV_ERR_NULL;
    if (const int rc = lstm_shape_validate(a->B, a->T, a->H, a->dtype)) return rc;
    *P = lstm_plan(a->B, a->T, a->H, a->dtype);
    if (const int rc = lstm_stride_validate(a->xp_stride_b, a->xp_stride_t, 4 * (int64_t)P->Hp)) return rc;
    if (a->workspace_bytes < P->ws_bytes) return TAV_ERR_SHAPE;
    if (a->xp_stride_b % 8 || a->xp_stride_t % 8) return TAV_ERR_ALIGN;
    if ((uintptr_t)a->xproj % 16 || (uintptr_t)a->w_hh % 16 || (uintptr_t)a->y % 16 || (uintptr_t)a->workspace % 16 || (uintptr_t)a->b_hh % 16 ||
        (uintptr_t)a->h0 % 16 || (uintptr_t)a->c0 % 16)
        return TAV_ERR_ALIGN;
    return 0;
}
inline int lstm_bwd_validate(const tav_lstm_bwd_args* a, LstmPlan* P) {
    if (!a || !a->dy || !a->w_hh_t || !a->workspace || !a->dz) return TAV_ERR_NULL;
    if (const int rc = lstm_shape_validate(a->B, a->T, a->H, a->dtype)) return rc;
    *P = lstm_plan(a->B, a->T, a->H, a->dtype);
    if (const int rc = lstm_stride_validate(a->dy_stride_b, a->dy_stride_t, P->Hp)) return rc;
    if (const int rc = lstm_stride_validate(a->dz_stride_b, a->dz_stride_t, 4 * (int64_t)P->Hp)) return rc;
    if (a->workspace_bytes < P->ws_bytes) return TAV_ERR_SHAPE;
    if (a->dy_stride_b % 8 || a->dy_stride_t % 8 || a->dz_stride_b % 8 || a->dz_stride_t % 8) return TAV_ERR_ALIGN;
    if ((uintptr_t)a->dy % 16 || (uintptr_t)a->w_hh_t % 16 || (uintptr_t)a->workspace % 16 || (uintptr_t)a->dz % 16 || (uintptr_t)a->dh_T % 16 ||
        (uintptr_t)a->dc_T % 16 || (uintptr_t)a->dh0 % 16 || (uintptr_t)a->dc0 % 16 || (uintptr_t)a->dc_trace % 16)
        return TAV_ERR_ALIGN;
    return 0;
}
inline int logsigmoid_validate(bool have, int64_t n) {
    if (!have) return TAV_ERR_NULL;
    return (n < 1 || n > ((int64_t)1 << 38)) ? TAV_ERR_SHAPE : 0;
}
inline int64_t logsigmoid_blocks(int64_t n) { return (n + 255) / 256; }

}  // namespace plan
}  // namespace tav
