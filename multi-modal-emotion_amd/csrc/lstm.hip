// One LSTM layer's recurrence, forward and backward (reference SingleModels/models/text.py::LSTMClassifier -> nn.LSTM), and nn.LogSigmoid.
//
// A workgroup owns LSTM_ROWS = 16 rows of the batch and runs the whole time loop for them; workgroups never wait for each other (no
// flags, no atomics, no cooperative launch).  A wave owns `TPW` tiles of 16 hidden units and computes all four gates of them, so the gate
// update needs no exchange: after the product, lane (g, i) holds z of units u0 + 4g .. + 3 of batch row i in all four gates.
//
// Forward, step t:  z[unit][row] = sum_k W_hh[unit][k] h_{t-1}[row][k]  as  mma16(a = W_hh rows streamed from global memory (L2) straight
// into registers, b = h_{t-1} of the tile read from LDS), K = Hp in ascending steps of KSTEP from a zero accumulator:
//   bf16 policy: v_mfma_f32_16x16x32_bf16, Hp / 32 chained MFMAs, products exact, f32 accumulation;
//   f32 policy : v_mfma_f32_16x16x4_f32 (common.h mma16<float>: four per 16 k-values), Hp / 4 chained MFMAs.  An output element is
//                one chain of Hp products either way; tests/lstm_ref.py charges (Hp + 2) u of sum |w h| for it.
// Then z = acc + (xproj + b_hh), the gates with the device library's expf / tanhf, c = fma(f, c, i g) in f32 registers, h = o tanhf(c).
// h_t goes to the other LDS image in the operand type (what the next step multiplies is what y stores) -- one barrier a step.
// xproj of step t + 1 is loaded before the gate math of step t; the stores of h_t, the gates and c_t are issued after the LDS write and
// nothing waits for them.
// Backward, step t: the gate derivatives from the saved activations, dZ_t to LDS and to global memory, then
// dh[unit][row] = sum_n W_hh^T[unit][n] dZ_t[row][n] (K = 4 Hp, same chain rules) for step t - 1.  Two barriers a step (one dZ image).
// Rows past B are clamped on every load and masked on every store; the pad units rely on the zero pads (include/tavhip_rnn.h).
// The order of every sum is fixed by the plan and a batch row is one MFMA column: its bits depend on no other row.
#include "common.h"
#include "tavhip_internal.h"
#include "lstm_plan.h"

namespace tav {
using plan::LstmPlan, plan::LSTM_ROWS;

TAV_DEV float sigmoid_f(float z) { return 1.0f / (1.0f + expf(-z)); }

template <typename T> TAV_DEV uint4 ldg16(const T* p) { return *reinterpret_cast<const uint4*>(p); }

template <typename T, int TPW, int MAXB>
__global__ __launch_bounds__(MAXB) void lstm_fwd_kernel(const tav_lstm_fwd_args a, const LstmPlan P) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int PK = ET<T>::PK, KSTEP = ET<T>::KSTEP, ES = ET<T>::ES;
    // xproj of step t + 1 is requested a step ahead where its 16 TPW registers fit next to the accumulators without scratch
    constexpr bool AHEAD = TPW == 1 || (TPW == 2 && MAXB <= 768);
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), g = lane >> 4, i = lane & 15;
    const int Hp = P.Hp, ntiles = P.ntiles, pitch = (int)P.h_pitch;
    const long B = a.B, T_ = a.T;
    const long row = (long)blockIdx.x * LSTM_ROWS + i;
    const bool live = row < B;
    const long b = live ? row : B - 1;                  // (loads of a row past the batch read the last row; nothing of it is stored)
    const T* const xp = reinterpret_cast<const T*>(a.xproj) + b * a.xp_stride_b;
    const T* const W = reinterpret_cast<const T*>(a.w_hh);
    T* const y = reinterpret_cast<T*>(a.y);
    float* const gates = reinterpret_cast<float*>(reinterpret_cast<char*>(a.workspace) + P.ws_gates_off);
    float* const cells = reinterpret_cast<float*>(reinterpret_cast<char*>(a.workspace) + P.ws_cell_off);

    // ---- this lane's units: tile j of the wave starts at unit u0[j]; the lane holds units u0 + 4g .. + 3 of row i
    int uu[TPW];
    bool on[TPW];
    f32x4 c[TPW], xn[TPW][4];
    float* const bias = reinterpret_cast<float*>(smem + P.bias_off);          // b_hh (zeros when absent), [4 Hp] f32
    for (int n = threadIdx.x * 4; n < 4 * Hp; n += blockDim.x * 4) st4(bias + n, a.b_hh ? ld4(a.b_hh + n) : f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
        const int tile = w * TPW + j;
        on[j] = tile < ntiles;                         // (wave-uniform)
        uu[j] = (on[j] ? tile : 0) * 16 + 4 * g;
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        f32x4 h = zero;
        c[j] = zero;
        if (on[j]) {
            if (a.h0) h = ld4(a.h0 + b * Hp + uu[j]);
            if (a.c0) c[j] = ld4(a.c0 + b * Hp + uu[j]);
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (AHEAD) xn[j][q] = ld4(xp + q * Hp + uu[j]);
            st4(reinterpret_cast<T*>(smem + i * pitch) + uu[j], h);
            if (live) {
                st4(y + b * Hp + uu[j], h);
                st4(cells + b * Hp + uu[j], c[j]);
            }
        }
    }
    __syncthreads();

    for (long t = 0; t < T_; ++t) {
        const char* const hcur = smem + (t & 1) * LSTM_ROWS * pitch + i * pitch + PK * g * ES;
        char* const hnext = smem + ((t + 1) & 1) * LSTM_ROWS * pitch + i * pitch;
        f32x4 acc[TPW][4];
#pragma unroll
        for (int j = 0; j < TPW; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[j][q] = f32x4{0.f, 0.f, 0.f, 0.f};
        // ---- the product: W_hh rows from L2, h_{t-1} from LDS
        for (int k0 = 0; k0 < Hp; k0 += KSTEP) {
            const uint4 hf = *reinterpret_cast<const uint4*>(hcur + k0 * ES);
#pragma unroll
            for (int j = 0; j < TPW; ++j) {
                if (on[j]) {
                    const int u = uu[j] - 4 * g + i;   // the row of W this lane supplies: unit u0 + i
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const uint4 wf = ldg16(W + (long)(q * Hp + u) * Hp + k0 + PK * g);
                        mma16<T>(wf, hf, acc[j][q]);
                    }
                }
            }
        }
        // ---- gates.  z = acc + (xproj + b_hh); a tile's xproj registers are free once its z exists, so the rows of step t + 1 are
        // requested there, ahead of the transcendentals
#pragma unroll
        for (int j = 0; j < TPW; ++j) {
            if (on[j]) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (!AHEAD) xn[j][q] = ld4(xp + t * a.xp_stride_t + q * Hp + uu[j]);
                    const f32x4 bq = ld4(bias + q * Hp + uu[j]);
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[j][q][r] += xn[j][q][r] + bq[r];
                }
                if (AHEAD && t + 1 < T_) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) xn[j][q] = ld4(xp + (t + 1) * a.xp_stride_t + q * Hp + uu[j]);
                }
                f32x4 gi, gf, gg, go, h;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    gi[r] = sigmoid_f(acc[j][0][r]);
                    gf[r] = sigmoid_f(acc[j][1][r]);
                    gg[r] = tanhf(acc[j][2][r]);
                    go[r] = sigmoid_f(acc[j][3][r]);
                    c[j][r] = fmaf(gf[r], c[j][r], gi[r] * gg[r]);
                    h[r] = go[r] * tanhf(c[j][r]);
                }
                st4(reinterpret_cast<T*>(hnext) + uu[j], h);
                if (live) {
                    const long at = (t * B + b) * 4 * Hp + uu[j];
                    st4(gates + at, gi);
                    st4(gates + at + Hp, gf);
                    st4(gates + at + 2 * Hp, gg);
                    st4(gates + at + 3 * Hp, go);
                    st4(cells + ((t + 1) * B + b) * Hp + uu[j], c[j]);
                    st4(y + ((t + 1) * B + b) * Hp + uu[j], h);
                }
            }
        }
        __syncthreads();
    }
}

template <typename T, int TPW, int MAXB>
__global__ __launch_bounds__(MAXB) void lstm_bwd_kernel(const tav_lstm_bwd_args a, const LstmPlan P) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int PK = ET<T>::PK, KSTEP = ET<T>::KSTEP, ES = ET<T>::ES;
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), g = lane >> 4, i = lane & 15;
    const int Hp = P.Hp, ntiles = P.ntiles, pitch = (int)P.dz_pitch, K = 4 * Hp;
    const long B = a.B, T_ = a.T;
    const long row = (long)blockIdx.x * LSTM_ROWS + i;
    const bool live = row < B;
    const long b = live ? row : B - 1;
    const T* const dy = reinterpret_cast<const T*>(a.dy) + b * a.dy_stride_b;
    T* const dz = reinterpret_cast<T*>(a.dz) + b * a.dz_stride_b;
    const T* const Wt = reinterpret_cast<const T*>(a.w_hh_t);
    const float* const gates = reinterpret_cast<const float*>(reinterpret_cast<const char*>(a.workspace) + P.ws_gates_off);
    const float* const cells = reinterpret_cast<const float*>(reinterpret_cast<const char*>(a.workspace) + P.ws_cell_off);
    char* const zrow = smem + i * pitch;

    int uu[TPW];
    bool on[TPW];
    f32x4 dh[TPW], dc[TPW];
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
        const int tile = w * TPW + j;
        on[j] = tile < ntiles;
        uu[j] = (on[j] ? tile : 0) * 16 + 4 * g;
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        dh[j] = (on[j] && a.dh_T) ? ld4(a.dh_T + b * Hp + uu[j]) : zero;
        dc[j] = (on[j] && a.dc_T) ? ld4(a.dc_T + b * Hp + uu[j]) : zero;
    }

    for (long t = T_ - 1; t >= 0; --t) {
        // ---- gate derivatives of step t
#pragma unroll
        for (int j = 0; j < TPW; ++j) {
            if (on[j]) {
                const long at = (t * B + b) * 4 * Hp + uu[j];
                const f32x4 gi = ld4(gates + at), gf = ld4(gates + at + Hp), gg = ld4(gates + at + 2 * Hp), go = ld4(gates + at + 3 * Hp);
                const f32x4 ct = ld4(cells + ((t + 1) * B + b) * Hp + uu[j]), cp = ld4(cells + (t * B + b) * Hp + uu[j]);
                const f32x4 dyt = ld4(dy + t * a.dy_stride_t + uu[j]);
                f32x4 zi, zf, zg, zo, carry;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float d = dyt[r] + dh[j][r];
                    const float tc = tanhf(ct[r]);
                    zo[r] = d * tc * (go[r] * (1.0f - go[r]));
                    const float dct = fmaf(d * go[r], 1.0f - tc * tc, dc[j][r]);
                    zi[r] = dct * gg[r] * (gi[r] * (1.0f - gi[r]));
                    zf[r] = dct * cp[r] * (gf[r] * (1.0f - gf[r]));
                    zg[r] = dct * gi[r] * (1.0f - gg[r] * gg[r]);
                    carry[r] = dct * gf[r];
                }
                dc[j] = carry;
                T* const zl = reinterpret_cast<T*>(zrow);
                st4(zl + uu[j], zi);
                st4(zl + Hp + uu[j], zf);
                st4(zl + 2 * Hp + uu[j], zg);
                st4(zl + 3 * Hp + uu[j], zo);
                if (live) {
                    T* const zt = dz + t * a.dz_stride_t + uu[j];
                    st4(zt, zi);
                    st4(zt + Hp, zf);
                    st4(zt + 2 * Hp, zg);
                    st4(zt + 3 * Hp, zo);
                    if (a.dc_trace) st4(a.dc_trace + (t * B + b) * Hp + uu[j], carry);
                }
            }
        }
        __syncthreads();
        // ---- dh of step t - 1: W_hh^T rows from L2, dZ_t from LDS
        f32x4 acc[TPW];
#pragma unroll
        for (int j = 0; j < TPW; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        constexpr int U = TPW == 1 ? 4 : (TPW == 2 ? 2 : 1);     // (K / KSTEP is a multiple of 8) steps whose loads are in flight together
        for (int k0 = 0; k0 < K; k0 += U * KSTEP) {
            uint4 wf[U][TPW], zfr[U];
#pragma unroll
            for (int s = 0; s < U; ++s) {
                zfr[s] = *reinterpret_cast<const uint4*>(zrow + (k0 + s * KSTEP + PK * g) * ES);
#pragma unroll
                for (int j = 0; j < TPW; ++j)
                    if (on[j]) wf[s][j] = ldg16(Wt + (long)(uu[j] - 4 * g + i) * K + k0 + s * KSTEP + PK * g);
            }
#pragma unroll
            for (int s = 0; s < U; ++s)
#pragma unroll
                for (int j = 0; j < TPW; ++j)
                    if (on[j]) mma16<T>(wf[s][j], zfr[s], acc[j]);
        }
#pragma unroll
        for (int j = 0; j < TPW; ++j) dh[j] = acc[j];
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
        if (on[j] && live) {
            if (a.dh0) st4(a.dh0 + b * Hp + uu[j], dh[j]);
            if (a.dc0) st4(a.dc0 + b * Hp + uu[j], dc[j]);
        }
    }
}

__global__ __launch_bounds__(256) void logsigmoid_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, const long n) {
    const long k = (long)blockIdx.x * 256 + threadIdx.x;
    if (k < n) {
        const float v = x[k];
        y[k] = fminf(v, 0.0f) - log1pf(expf(-fabsf(v)));
    }
}
__global__ __launch_bounds__(256) void logsigmoid_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ dx, const long n) {
    const long k = (long)blockIdx.x * 256 + threadIdx.x;
    if (k < n) {
        const float v = x[k], e = expf(-fabsf(v));       // s(-x) = e / (1 + e) for x >= 0, 1 / (1 + e) for x < 0: no overflow on either side
        dx[k] = dy[k] * ((v >= 0.0f ? e : 1.0f) / (1.0f + e));
    }
}

template <typename T> struct LstmLaunch {
    template <int TPW, int MAXB> static int fwd(const tav_lstm_fwd_args& a, const LstmPlan& P, const plan::Launch& L, void* stream) {
        TAV_LAUNCH((lstm_fwd_kernel<T, TPW, MAXB>), L, stream, a, P);
        return 0;
    }
    template <int TPW, int MAXB> static int bwd(const tav_lstm_bwd_args& a, const LstmPlan& P, const plan::Launch& L, void* stream) {
        TAV_LAUNCH((lstm_bwd_kernel<T, TPW, MAXB>), L, stream, a, P);
        return 0;
    }
};

// builds by tiles per wave and by the most threads (256: 512 registers a lane, 768: 168, 1024: 128)
#define TAV_LSTM_PICK(which, T)                                                                     \
    do {                                                                                            \
        using LL = LstmLaunch<T>;                                                                   \
        const bool mid = P.block <= 768;                                                            \
        if (P.tpw == 1 && P.block <= 256) return LL::template which<1, 256>(*a, P, L, stream);      \
        if (P.tpw == 1) return mid ? LL::template which<1, 768>(*a, P, L, stream) : LL::template which<1, 1024>(*a, P, L, stream); \
        if (P.tpw == 2) return mid ? LL::template which<2, 768>(*a, P, L, stream) : LL::template which<2, 1024>(*a, P, L, stream); \
        if (P.tpw == 3) return mid ? LL::template which<3, 768>(*a, P, L, stream) : LL::template which<3, 1024>(*a, P, L, stream); \
        return LL::template which<4, 1024>(*a, P, L, stream);                                       \
    } while (0)

}  // namespace tav
using namespace tav;

extern "C" int tav_rnn_version(void) { return plan::RNN_ABI_VERSION; }

extern "C" int tav_lstm_get_plan(int64_t B, int64_t T, int64_t H, int32_t dtype, tav_lstm_plan* out) {
    if (!out) return TAV_ERR_NULL;
    if (const int rc = plan::lstm_shape_validate(B, T, H, dtype)) return rc;
    plan::lstm_plan_public(plan::lstm_plan(B, T, H, dtype), out);
    return 0;
}

extern "C" int64_t tav_lstm_ws_bytes(int64_t B, int64_t T, int64_t H, int32_t dtype) { return plan::lstm_ws_bytes(B, T, H, dtype); }

extern "C" int tav_lstm_fwd(const tav_lstm_fwd_args* a, void* stream) {
    LstmPlan P;
    if (const int rc = plan::lstm_fwd_validate(a, &P)) return rc;
    const plan::Launch L{plan::lstm_blocks(a->B), 1, 1, P.block, (size_t)P.fwd_lds};
    return floats::dispatch(a->dtype, [&](auto tag) -> int {
        using T = decltype(tag);
        TAV_LSTM_PICK(fwd, T);
    });
}

extern "C" int tav_lstm_bwd(const tav_lstm_bwd_args* a, void* stream) {
    LstmPlan P;
    if (const int rc = plan::lstm_bwd_validate(a, &P)) return rc;
    const plan::Launch L{plan::lstm_blocks(a->B), 1, 1, P.block, (size_t)P.bwd_lds};
    return floats::dispatch(a->dtype, [&](auto tag) -> int {
        using T = decltype(tag);
        TAV_LSTM_PICK(bwd, T);
    });
}

extern "C" int tav_logsigmoid_fwd(const float* x, float* y, int64_t n, void* stream) {
    if (const int rc = plan::logsigmoid_validate(x && y, n)) return rc;
    const plan::Launch L{plan::logsigmoid_blocks(n), 1, 1, 256, 0};
    TAV_LAUNCH(logsigmoid_fwd_kernel, L, stream, x, y, (long)n);
    return 0;
}

extern "C" int tav_logsigmoid_bwd(const float* x, const float* dy, float* dx, int64_t n, void* stream) {
    if (const int rc = plan::logsigmoid_validate(x && dy && dx, n)) return rc;
    const plan::Launch L{plan::logsigmoid_blocks(n), 1, 1, 256, 0};
    TAV_LAUNCH(logsigmoid_bwd_kernel, L, stream, x, dy, dx, (long)n);
    return 0;
}
