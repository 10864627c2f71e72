/* libtavhip, recurrent layers -- the third public header of libtavhip.so.
 *
 * The reference's SingleModels/models/text.py::LSTMClassifier runs nn.LSTM(hidden, hidden, num_layers, batch_first=True) and ends in
 * nn.LogSigmoid.  The entry points below are the recurrence of one LSTM layer in one direction, forward and backward, and the log-sigmoid.
 * They follow the rules of include/tavhip.h (extern "C", device pointers and sizes, `stream` a hipStream_t passed as void*, no allocation,
 * no synchronisation, TAV_ERR_* codes) and live in the same shared object.  They have a header of their own for the reason
 * tavhip_align.h has one: the symbol set of tavhip.h is pinned by a recorded table.  tav_rnn_version() is bumped on any signature change.
 *
 * What is NOT here, on purpose: the input projection xproj = x W_ih^T + b_ih (one tav_gemm_nt over the B T rows), the weight gradient
 * dW_hh = sum_{b,t} dZ[b,t]^T h_{t-1}[b] (one tav_gemm_tn over the B T rows: h_{t-1} and h_t are the two contiguous views [0, T) and
 * [1, T] of the forward's y), db_hh (tav_colsum of dZ) and everything of W_ih (the projection's own backward on dZ).
 *
 * PADDING RULE.  The GEMMs around the recurrence need K * elem_size % 128 == 0, so the hidden size H is carried as
 *     Hp = ceil(H / 64) * 64                                   (300 -> 320)
 * and each of the four gate blocks (PyTorch's order i, f, g, o) is padded to Hp rows: W_hh is [4 Hp][Hp], gate q's unit u is row q Hp + u.
 * The caller keeps the pad rows AND pad columns of W_hh, the pads of b_hh, of xproj (that is: of W_ih's rows and of b_ih) and of h0 / c0
 * at zero.  A padded unit then has z = 0 exactly in all four gates, so c = 0 and h = 0 at every step, its dZ is exactly 0 in all
 * four gates, and dh0 / dc0 are 0 there.  The kernels do not mask: they rely on those zeros.
 */
#ifndef TAVHIP_RNN_H
#define TAVHIP_RNN_H
#include <stdint.h>
#include "tavhip.h"

#ifdef __cplusplus
extern "C" {
#endif

int tav_rnn_version(void);

/* The launch plan of tav_lstm_fwd / tav_lstm_bwd for a batch of B rows, T steps and hidden size H (host arithmetic).  dtype: TAV_BF16 or
 * TAV_F32, the operand type of xproj, W_hh, y, dY and dZ.  TAV_ERR_SHAPE for a shape the kernels cannot hold (H beyond what one
 * workgroup's LDS takes: Hp <= 1024 in bf16, Hp <= 576 in f32), TAV_ERR_DTYPE for any other dtype. */
typedef struct tav_lstm_plan {
    int32_t block;              /* threads of a workgroup                                                                       */
    int32_t rows_per_wg;        /* batch rows a workgroup owns for all T steps (the grid is ceil(B / rows_per_wg))              */
    int32_t Hp;                 /* padded hidden size                                                                           */
    int32_t tiles_per_wave;     /* 16-unit column tiles a wave computes all four gates of                                       */
    int64_t lds_bytes;          /* dynamic LDS of the larger of the two launches                                                */
    int64_t ws_gates_off;       /* workspace: the gate activations, f32 [T][B][4 Hp]                                            */
    int64_t ws_cell_off;        /* workspace: the cell states, f32 [T + 1][B][Hp], c0 in slot 0, c_T in slot T                  */
    int64_t ws_bytes;           /* workspace bytes the forward fills and the backward reads                                     */
} tav_lstm_plan;
int tav_lstm_get_plan(int64_t B, int64_t T, int64_t H, int32_t dtype, tav_lstm_plan* plan);
/* ws_bytes of that plan, or a negative TAV_ERR_* for a refused shape. */
int64_t tav_lstm_ws_bytes(int64_t B, int64_t T, int64_t H, int32_t dtype);

/* One layer, one direction, PyTorch's semantics, for t = 0 .. T-1:
 *     z_t = xproj[b, t, :] + b_hh + W_hh h_{t-1}          i = s(z_i)  f = s(z_f)  g = tanh(z_g)  o = s(z_o)       s(z) = 1 / (1 + expf(-z))
 *     c_t = f c_{t-1} + i g                               h_t = o tanh(c_t)
 * Element (b, t, n) of xproj is xproj[b xp_stride_b + t xp_stride_t + n], n < 4 Hp (both strides in elements, multiples of 8), so the
 * projection may be batch-major [B][T][4 Hp] or time-major [T][B][4 Hp].
 * y: [T + 1][B][Hp] in `dtype`, time-major, written in full: slot 0 = h0 (zeros when NULL), slot t + 1 = h_t; slot T is h_T.  The
 * recurrence itself carries h_t as it is stored (rounded to bf16 under TAV_BF16), c in f32.
 * workspace (tav_lstm_ws_bytes, 256-byte aligned): gate activations and cell states as laid out by the plan; slot T of the cells is c_T.
 * Rows of the batch are independent: a row's bits depend on nothing but its own inputs and the weights. */
typedef struct tav_lstm_fwd_args {
    const void* xproj;
    const void* w_hh;           /* [4 Hp][Hp] dense, `dtype` */
    const float* b_hh;          /* optional [4 Hp] */
    const float* h0;            /* optional [B][Hp] */
    const float* c0;            /* optional [B][Hp] */
    void* y;
    void* workspace;
    int64_t workspace_bytes;
    int64_t B, T, H;
    int64_t xp_stride_b, xp_stride_t;
    int32_t dtype;
    int32_t reserved;
} tav_lstm_fwd_args;
int tav_lstm_fwd(const tav_lstm_fwd_args* args, void* stream);

/* The reverse recurrence, for t = T-1 .. 0, with dh = dY[b, t] + W_hh^T dZ_{t+1} (dh_T at t = T-1) and the carry dc (dc_T at t = T-1):
 *     dz_o = dh tanh(c_t) o (1 - o)                 dc  += dh o (1 - tanh(c_t)^2)
 *     dz_i = dc g i (1 - i)      dz_f = dc c_{t-1} f (1 - f)      dz_g = dc i (1 - g^2)      carry to t-1: dc f
 * dZ element (b, t, n) is written at dz[b dz_stride_b + t dz_stride_t + n], n < 4 Hp, in `dtype`; it is the gradient of the
 * pre-activations, hence of xproj, and column-summed of b_hh.  The product W_hh^T dZ_{t+1} uses dZ as it is stored.
 * dY element (b, t, u) is read at dy[b dy_stride_b + t dy_stride_t + u], u < Hp (strides multiples of 8).
 * w_hh_t is the TRANSPOSE of the forward's operand, [Hp][4 Hp] dense (the weight cache's transposed copy).
 * dh0 / dc0 (optional, f32 [B][Hp]) receive the gradients of the initial state.  dc_trace (optional, f32 [T][B][Hp], NULL in
 * production) receives the carry that leaves step t, dc_t f_t -- what step t-1 adds to; slot 0 equals dc0. */
typedef struct tav_lstm_bwd_args {
    const void* dy;
    const float* dh_T;          /* optional [B][Hp] */
    const float* dc_T;          /* optional [B][Hp] */
    const void* w_hh_t;         /* [Hp][4 Hp] dense, `dtype` */
    const void* workspace;      /* as the forward left it */
    int64_t workspace_bytes;
    void* dz;
    float* dh0;                 /* optional */
    float* dc0;                 /* optional */
    float* dc_trace;            /* optional */
    int64_t B, T, H;
    int64_t dy_stride_b, dy_stride_t, dz_stride_b, dz_stride_t;
    int32_t dtype;
    int32_t reserved;
} tav_lstm_bwd_args;
int tav_lstm_bwd(const tav_lstm_bwd_args* args, void* stream);

/* y = min(x, 0) - log1p(exp(-|x|)) and dx = dy s(-x) from the stored x; f32, any element count n >= 1. */
int tav_logsigmoid_fwd(const float* x, float* y, int64_t n, void* stream);
int tav_logsigmoid_bwd(const float* x, const float* dy, float* dx, int64_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif
