// csrc/lstm_plan.h alone, as a host program (tests/test_lstm_host.py builds it with ASan + UBSan): sweeps B, T, every H up to past the limit and
// both dtypes, and checks what a launch relies on.  Prints "FAILED ..." per broken invariant and ends with "ok: 0 failed checks".
#include <stdio.h>
#include <vector>
#include "../../multi-modal-emotion_amd/csrc/lstm_plan.h"
#include "check.h"

using namespace tav::plan;

int main() {
    long plans = 0, refused = 0;
    for (int dtype : {TAV_BF16, TAV_F32}) {
        const int64_t es = dtype == TAV_BF16 ? 2 : 4, hp_max = dtype == TAV_BF16 ? 1024 : 576;
        for (int64_t H = 1; H <= 1100; ++H) {
            const int64_t Hp = (H + 63) / 64 * 64;
            for (int64_t T : {(int64_t)1, (int64_t)2, (int64_t)70, (int64_t)512})
                for (int64_t B = 1; B <= 80; ++B) {
                    const int rc = lstm_shape_validate(B, T, H, dtype);
                    if (Hp > hp_max) {
                        ++refused;
                        CHECK(rc == TAV_ERR_SHAPE && lstm_ws_bytes(B, T, H, dtype) == TAV_ERR_SHAPE, "H %ld dtype %d accepted", (long)H, dtype);
                        continue;
                    }
                    CHECK(rc == 0, "H %ld T %ld B %ld dtype %d refused: %d", (long)H, (long)T, (long)B, dtype, rc);
                    if (rc) continue;
                    const LstmPlan P = lstm_plan(B, T, H, dtype);
                    ++plans;
                    CHECK(P.Hp == Hp && P.es == es && P.ntiles * 16 == Hp, "Hp %d for H %ld", P.Hp, (long)H);
                    CHECK(P.block == P.waves * 64 && P.block >= 64 && P.block <= 1024, "block %d", P.block);
                    CHECK(P.tpw >= 1 && P.tpw <= LSTM_MAX_TPW && P.waves * P.tpw >= P.ntiles && (P.waves - 1) * P.tpw < P.ntiles, "waves %d x %d tiles for %d", P.waves, P.tpw, P.ntiles);
                    CHECK(P.fwd_lds <= 160 * 1024 && P.bwd_lds <= 160 * 1024 && P.lds_bytes == (P.fwd_lds > P.bwd_lds ? P.fwd_lds : P.bwd_lds), "lds %ld %ld", (long)P.fwd_lds, (long)P.bwd_lds);
                    // forward LDS: two images of LSTM_ROWS rows, then the bias; the last byte a lane reads or writes lies inside its area
                    CHECK(P.h_pitch % 16 == 0 && P.h_pitch >= Hp * es && P.bias_off == 2 * LSTM_ROWS * P.h_pitch && P.bias_off % 16 == 0 &&
                              P.fwd_lds - P.bias_off == 4 * Hp * 4, "forward carve-up");
                    CHECK((2 * LSTM_ROWS - 1) * P.h_pitch + Hp * es <= P.bias_off, "h image");
                    CHECK(P.dz_pitch % 16 == 0 && P.dz_pitch >= 4 * Hp * es && (LSTM_ROWS - 1) * P.dz_pitch + 4 * Hp * es <= P.bwd_lds, "dz image");
                    // K loops: the forward steps by KSTEP, the backward by up to 4 KSTEP
                    const int64_t kstep = dtype == TAV_BF16 ? 32 : 16;
                    CHECK(Hp % kstep == 0 && (4 * Hp) % (4 * kstep) == 0, "K steps");
                    // workspace: gates [T][B][4 Hp] then cells [T + 1][B][Hp], f32, no overlap, inside ws_bytes
                    const int64_t gates_end = P.ws_gates_off + T * B * 4 * Hp * 4, cells_end = P.ws_cell_off + (T + 1) * B * Hp * 4;
                    CHECK(P.ws_gates_off == 0 && gates_end <= P.ws_cell_off && P.ws_cell_off % 256 == 0 && cells_end <= P.ws_bytes && P.ws_bytes % 256 == 0,
                          "workspace %ld %ld %ld", (long)P.ws_gates_off, (long)P.ws_cell_off, (long)P.ws_bytes);
                    CHECK(lstm_ws_bytes(B, T, H, dtype) == P.ws_bytes, "ws_bytes");
                    CHECK(lstm_blocks(B) * LSTM_ROWS >= B && (lstm_blocks(B) - 1) * LSTM_ROWS < B, "grid");
                    tav_lstm_plan pub;
                    lstm_plan_public(P, &pub);
                    CHECK(pub.block == P.block && pub.rows_per_wg == LSTM_ROWS && pub.Hp == P.Hp && pub.tiles_per_wave == P.tpw && pub.lds_bytes == P.lds_bytes &&
                              pub.ws_gates_off == P.ws_gates_off && pub.ws_cell_off == P.ws_cell_off && pub.ws_bytes == P.ws_bytes, "public plan");
                }
        }
    }
    CHECK(plans > 0 && refused > 0, "%ld plans, %ld refused", plans, refused);
    CHECK(lstm_shape_validate(1, 1, 64, TAV_FP8) == TAV_ERR_DTYPE && lstm_shape_validate(1, 1, 64, 7) == TAV_ERR_DTYPE, "dtype");
    CHECK(lstm_shape_validate(0, 1, 64, TAV_F32) == TAV_ERR_SHAPE && lstm_shape_validate(1, 0, 64, TAV_F32) == TAV_ERR_SHAPE && lstm_shape_validate(1, 1, 0, TAV_F32) == TAV_ERR_SHAPE &&
              lstm_shape_validate(LSTM_MAX_B + 1, 1, 64, TAV_F32) == TAV_ERR_SHAPE && lstm_shape_validate(1, LSTM_MAX_T + 1, 64, TAV_F32) == TAV_ERR_SHAPE &&
              lstm_shape_validate(1, 1, 577, TAV_F32) == TAV_ERR_SHAPE && lstm_shape_validate(1, 1, 577, TAV_BF16) == 0 && lstm_shape_validate(1, 1, 1025, TAV_BF16) == TAV_ERR_SHAPE &&
              lstm_shape_validate(LSTM_MAX_B, LSTM_MAX_T, 1024, TAV_BF16) == TAV_ERR_SHAPE, "limits");
    // the validators: pointers, dtype, sizes, strides, workspace, alignment
    {
        alignas(16) static char dummy[64];
        tav_lstm_fwd_args a = {};
        LstmPlan P;
        CHECK(lstm_fwd_validate(nullptr, &P) == TAV_ERR_NULL && lstm_fwd_validate(&a, &P) == TAV_ERR_NULL, "null");
        a.xproj = a.w_hh = dummy; a.y = a.workspace = dummy;
        a.B = 5; a.T = 70; a.H = 300; a.dtype = TAV_BF16; a.xp_stride_b = 70 * 1280; a.xp_stride_t = 1280;
        a.workspace_bytes = lstm_ws_bytes(5, 70, 300, TAV_BF16);
        CHECK(lstm_fwd_validate(&a, &P) == 0 && P.Hp == 320 && P.block == 640 && P.tpw == 2, "plain: %d", lstm_fwd_validate(&a, &P));
        tav_lstm_fwd_args b = a; b.y = nullptr;          CHECK(lstm_fwd_validate(&b, &P) == TAV_ERR_NULL, "y");
        b = a; b.dtype = TAV_FP8;                        CHECK(lstm_fwd_validate(&b, &P) == TAV_ERR_DTYPE, "dtype");
        b = a; b.H = 1025;                               CHECK(lstm_fwd_validate(&b, &P) == TAV_ERR_SHAPE, "H");
        b = a; b.xp_stride_t = 1272;                     CHECK(lstm_fwd_validate(&b, &P) == TAV_ERR_SHAPE, "stride below the row");
        b = a; b.xp_stride_t = 1284;                     CHECK(lstm_fwd_validate(&b, &P) == TAV_ERR_ALIGN, "stride not a multiple of 8");
        b = a; b.workspace_bytes -= 1;                   CHECK(lstm_fwd_validate(&b, &P) == TAV_ERR_SHAPE, "workspace small");
        b = a; b.h0 = (const float*)(dummy + 4);         CHECK(lstm_fwd_validate(&b, &P) == TAV_ERR_ALIGN, "h0 misaligned");
        tav_lstm_bwd_args c = {};
        CHECK(lstm_bwd_validate(nullptr, &P) == TAV_ERR_NULL && lstm_bwd_validate(&c, &P) == TAV_ERR_NULL, "bwd null");
        c.dy = c.w_hh_t = c.workspace = dummy; c.dz = dummy;
        c.B = 5; c.T = 70; c.H = 300; c.dtype = TAV_F32; c.dy_stride_b = 320; c.dy_stride_t = 5 * 320; c.dz_stride_b = 1280; c.dz_stride_t = 5 * 1280;
        c.workspace_bytes = lstm_ws_bytes(5, 70, 300, TAV_F32);
        CHECK(lstm_bwd_validate(&c, &P) == 0, "bwd plain");
        tav_lstm_bwd_args d = c; d.dz = nullptr;         CHECK(lstm_bwd_validate(&d, &P) == TAV_ERR_NULL, "dz");
        d = c; d.dy_stride_b = 316;                      CHECK(lstm_bwd_validate(&d, &P) == TAV_ERR_SHAPE, "dy stride");
        d = c; d.dz_stride_b = 1284;                     CHECK(lstm_bwd_validate(&d, &P) == TAV_ERR_ALIGN, "dz stride");
        d = c; d.workspace_bytes = 16;                   CHECK(lstm_bwd_validate(&d, &P) == TAV_ERR_SHAPE, "bwd workspace");
        d = c; d.dc_trace = (float*)(dummy + 8);         CHECK(lstm_bwd_validate(&d, &P) == TAV_ERR_ALIGN, "trace misaligned");
    }
    CHECK(logsigmoid_validate(false, 1) == TAV_ERR_NULL && logsigmoid_validate(true, 0) == TAV_ERR_SHAPE && logsigmoid_validate(true, 4097) == 0, "log-sigmoid");
    CHECK(logsigmoid_blocks(1) == 1 && logsigmoid_blocks(256) == 1 && logsigmoid_blocks(257) == 2, "log-sigmoid grid");
    printf("plans %ld refused %ld\n", plans, refused);
    return check_summary();
}
