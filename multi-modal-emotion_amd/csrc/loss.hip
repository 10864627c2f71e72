// Soft F-beta / soft precision loss over a batch of logits (tavhip_loss.h): loss and dlogits from one launch of ONE workgroup.
//
// The per-class sums tp, fp, fn run over all B rows, so the loss couples the batch: it is a kernel of its own and not an epilogue of
// cross_entropy_kernel.  No atomics, no second workgroup to wait for.
//
// Pass 1   thread i takes rows i, i + 256, ... in ascending order: the row's softmax in f32 (max subtracted, expf, the C terms summed in
//          class order, one division per class), then its 3 C terms promoted to f64 and added to per-thread f64 partials (registers).
// Reduce   per value a 64-lane xor butterfly (every lane ends with the same bits: each level adds the same two numbers on both sides),
//          lane 0 of each wave to LDS, then the four waves in wave order.  The order is fixed by the launch shape alone.
// Classes  thread k < C: P, R, F, the clamp decision, dloss/dtp, dloss/dfp, dloss/dfn, all in f64.  The upper clamp edge 1 - eps sits 1e-7
//          under 1.0, less than two f32 steps (2^-24) away, and F would carry several f32 roundings: an f32 class stage cannot take the
//          clamp branch an fp64 model takes.  Values are rounded to f32 ONCE, where they are stored: stats, the two gradient
//          coefficients of a class (to LDS) and the loss.
// Pass 2   the row's softmax again from the logits (the same function, the same bits), dlogits = grad_scale p (g - sum_j p_j g_j) in f32.
//
// A NaN or +Inf logit makes its row's probabilities NaN, every class sum that row touches NaN -- that is every class -- and with them the
// loss and every coefficient: nothing is laundered.  -Inf gives p = 0.  A target outside [0, C) selects no class.
#include "common.h"
#include "tavhip_internal.h"
#include "loss_plan.h"

namespace tav {
using plan::SOFT_F_BLOCK, plan::SOFT_F_WAVES;
constexpr int SOFT_F_C = TAV_SOFT_F_MAX_C;

TAV_DEV double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// p[k] = softmax(z)[k] for k < C (0 beyond).  fmaxf drops a NaN, so m stays finite next to one and expf(NaN - m) carries it; m = +Inf
// gives Inf - Inf = NaN for the infinite logit; a row of -Inf gives NaN as well.
TAV_DEV void soft_f_row(const float* __restrict__ z, int C, float (&p)[SOFT_F_C]) {
    float m = z[0];
#pragma unroll
    for (int k = 1; k < SOFT_F_C; ++k)
        if (k < C) m = fmaxf(m, z[k]);
    float se = 0.f;
#pragma unroll
    for (int k = 0; k < SOFT_F_C; ++k) {
        p[k] = k < C ? expf(z[k] - m) : 0.f;
        if (k < C) se = k == 0 ? p[0] : se + p[k];
    }
#pragma unroll
    for (int k = 0; k < SOFT_F_C; ++k)
        if (k < C) p[k] = p[k] / se;
}

__global__ __launch_bounds__(SOFT_F_BLOCK) void soft_f_loss_kernel(const tav_soft_f_args a) {
    __shared__ double s_part[SOFT_F_WAVES][3][SOFT_F_C];
    __shared__ double s_term[SOFT_F_C];
    __shared__ float s_g_own[SOFT_F_C], s_g_other[SOFT_F_C];      // dloss/dtp - dloss/dfn, dloss/dfp
    const int C = (int)a.C, B = (int)a.B;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float p[SOFT_F_C];

    double tp[SOFT_F_C], fp[SOFT_F_C], fn[SOFT_F_C];
#pragma unroll
    for (int k = 0; k < SOFT_F_C; ++k) tp[k] = fp[k] = fn[k] = 0.0;
    for (int r = threadIdx.x; r < B; r += SOFT_F_BLOCK) {
        soft_f_row(a.logits + (long)r * a.ld, C, p);
        const int64_t t64 = a.target[r];
        const int t = (t64 >= 0 && t64 < C) ? (int)t64 : -1;
#pragma unroll
        for (int k = 0; k < SOFT_F_C; ++k) {
            if (k < C) {
                const double pk = (double)p[k];
                if (k == t) { tp[k] += pk; fn[k] += 1.0 - pk; }
                else fp[k] += pk;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < SOFT_F_C; ++k) {
        if (k < C) {                                   // (uniform)
            const double s0 = wave_sum_f64(tp[k]), s1 = wave_sum_f64(fp[k]), s2 = wave_sum_f64(fn[k]);
            if (lane == 0) { s_part[wave][0][k] = s0; s_part[wave][1][k] = s1; s_part[wave][2][k] = s2; }
        }
    }
    __syncthreads();

    if ((int)threadIdx.x < C) {
        const int k = threadIdx.x;
        double TP = s_part[0][0][k], FP = s_part[0][1][k], FN = s_part[0][2][k];
        for (int w = 1; w < SOFT_F_WAVES; ++w) { TP += s_part[w][0][k]; FP += s_part[w][1][k]; FN += s_part[w][2][k]; }
        const double eps = a.eps, b2 = a.beta * a.beta, wk = a.weight ? (double)a.weight[k] : 1.0;
        const double dp = TP + FP + eps, dr = TP + FN + eps;
        const double P = TP / dp, R = TP / dr;
        const double dP_tp = (FP + eps) / (dp * dp), dP_fp = -TP / (dp * dp);
        const double dR_tp = (FN + eps) / (dr * dr), dR_fn = -TP / (dr * dr);
        double F, dF_tp, dF_fp, dF_fn;
        if (a.mode == TAV_SOFT_F_PRECISION) {
            F = P; dF_tp = dP_tp; dF_fp = dP_fp; dF_fn = 0.0;
        } else {
            const double Q = b2 * P + R + eps;
            F = (1.0 + b2) * P * R / Q;
            const double dF_P = (1.0 + b2) * R * (R + eps) / (Q * Q), dF_R = (1.0 + b2) * P * (b2 * P + eps) / (Q * Q);
            dF_tp = dF_P * dP_tp + dF_R * dR_tp; dF_fp = dF_P * dP_fp; dF_fn = dF_R * dR_fn;
        }
        // torch.clamp: the value is held at the edge it crossed, the gradient passes on [eps, 1 - eps] and stops outside.  A NaN is
        // neither below nor above: it stays, and so do its derivatives.
        const double hi = 1.0 - eps;
        const bool below = F < eps, above = F > hi;
        s_term[k] = wk * (below ? eps : (above ? hi : F));
        const double ga = (below || above) ? 0.0 : -wk * dF_tp, gb = (below || above) ? 0.0 : -wk * dF_fp, gc = (below || above) ? 0.0 : -wk * dF_fn;
        s_g_own[k] = (float)(ga - gc);
        s_g_other[k] = (float)gb;
        if (a.stats) { a.stats[k] = (float)TP; a.stats[C + k] = (float)FP; a.stats[2 * C + k] = (float)FN; }
    }
    __syncthreads();
    if (threadIdx.x == 0 && a.loss) {
        double s = s_term[0];
        for (int k = 1; k < C; ++k) s += s_term[k];
        a.loss[0] = (float)(1.0 - s);
    }
    if (!a.dlogits) return;

    float g_own[SOFT_F_C], g_other[SOFT_F_C];
#pragma unroll
    for (int k = 0; k < SOFT_F_C; ++k) {
        g_own[k] = k < C ? s_g_own[k] : 0.f;
        g_other[k] = k < C ? s_g_other[k] : 0.f;
    }
    for (int r = threadIdx.x; r < B; r += SOFT_F_BLOCK) {
        soft_f_row(a.logits + (long)r * a.ld, C, p);
        const int64_t t64 = a.target[r];
        const int t = (t64 >= 0 && t64 < C) ? (int)t64 : -1;
        float g[SOFT_F_C], s = 0.f;
#pragma unroll
        for (int k = 0; k < SOFT_F_C; ++k) {
            g[k] = k == t ? g_own[k] : g_other[k];
            if (k < C) s = k == 0 ? p[0] * g[0] : s + p[k] * g[k];
        }
        float* const d = a.dlogits + (long)r * C;
#pragma unroll
        for (int k = 0; k < SOFT_F_C; ++k)
            if (k < C) d[k] = (a.grad_scale * p[k]) * (g[k] - s);
    }
}

extern "C" int tav_loss_version(void) { return plan::LOSS_ABI_VERSION; }

extern "C" int tav_soft_f_loss(const tav_soft_f_args* a, void* stream) {
    if (const int rc = plan::soft_f_validate(a)) return rc;
    const plan::Launch L{1, 1, 1, SOFT_F_BLOCK, 0};
    TAV_LAUNCH(soft_f_loss_kernel, L, stream, *a);
    return 0;
}

}  // namespace tav
