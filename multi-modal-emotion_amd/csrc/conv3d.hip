// Dense 3x3x3 convolution, forward / input gradient / weight gradient, the flatten + Linear behind it and the sigmoid (reference
// SingleModels/models/visual.py::VisualClassification).  include/tavhip_conv.h states layouts, the padding rule and where values are rounded;
// conv3d_plan.h holds every host decision.
//
// Forward (tav_conv3d_fwd) is an implicit GEMM on the MFMA: M = output voxels, N = Cout, K = 27 Cin_p with k = tap Cin_p + ci.  A workgroup
// owns a 32 x TH patch of one output plane (b, d).  It stages the 34 x (TH + 2) x 3 halo of the input into LDS -- voxels outside the input read
// as zero there, which is all that distinguishes the forward (pad 0) from the input gradient (pad 2, flipped transposed weights) -- and every
// tap is then a shifted window of that one image: the 16-byte chunk c of K lies at table[c] bytes behind a voxel's own address (the table is
// built once per workgroup; the three taps along W are neighbours of a channels-last row).  A voxel's pitch in LDS is Cin_p es + 16 bytes, an
// odd number of 16-byte slots, so the 16 voxels of a fragment read start in 16 different slots of the 256-byte bank row.  Wave w owns patch row
// w: two 16-voxel tiles times NT 16-channel tiles of accumulators.  The weight rows stream from global memory (L2 / L1) into MFMA operands as
// in the LSTM recurrence; each feeds the two voxel tiles.  mma16(a = weights, b = voxels): lane (g, i) ends with channels 4g .. 4g + 3 of voxel
// i, which is one vector store of a channels-last row.  Epilogue: + bias, gelu / gelu' through common.h's gelu_both4_t.
//
// Weight gradient (tav_conv3d_wgrad): dW[tap][ci][co] = sum_v X[v + tap][ci] dZ[v][co], the voxels as MFMA k.  Both operands are k-strided
// reads (frag_kstrided: ds_read_b64_tr_b16 pairs in bf16) of the same halo image and of the staged dZ patch; dZ voxels past the output edge
// are staged as zero.  The four waves of a workgroup deal the 27 taps (wave w holds taps w, w + 4, ...: seven slots); the one free slot, "tap 27"
// of wave 3, multiplies a fragment of ones and so sums db on the MFMA as well.  blockIdx.x = slab: a contiguous range of patches summed into
// f32 accumulators that live in registers for the whole range and are stored once; blockIdx.y = the channel block CIT x COT tiles.  A second
// launch adds the slabs in ascending order into the parameter's torch layout.  No atomics anywhere.
#include "common.h"
#include "tavhip_internal.h"
#include "conv3d_plan.h"

namespace tav {
using plan::ConvPlan;
constexpr int CTW = plan::CONV_TW, CROW = plan::CONV_TW + 2, CSLOTS = plan::CONV_WG_SLOTS;

template <typename T> TAV_DEV uint4 cldg16(const T* p) { return *reinterpret_cast<const uint4*>(p); }

struct Patch { long b, d, h0, w0; };
TAV_DEV Patch patch_of(long p, const ConvPlan& P) {
    Patch q;
    q.w0 = (p % P.pw) * CTW; p /= P.pw;
    q.h0 = (p % P.ph) * P.th; p /= P.ph;
    q.d = p % P.od;
    q.b = p / P.od;
    return q;
}

// LDS voxel (kd, r, s) of the halo <- x[b][d + kd - pad][h0 + r - pad][w0 + s - pad][0 .. cin_p), zeros outside the input
template <typename T>
TAV_DEV void stage_halo(char* smem, const T* x, const ConvPlan& P, const Patch q, long D, long H, long W, int pad) {
    const int cpv = P.cin_p * ET<T>::ES / 16, rows = P.th + 2, total = 3 * rows * CROW * cpv;
    for (int it = threadIdx.x; it < total; it += blockDim.x) {
        const int c = it % cpv, v = it / cpv, s = v % CROW, rr = v / CROW, r = rr % rows, kd = rr / rows;
        const long di = q.d + kd - pad, hi = q.h0 + r - pad, wi = q.w0 + s - pad;
        uint4 val = {0u, 0u, 0u, 0u};
        if (di >= 0 && di < D && hi >= 0 && hi < H && wi >= 0 && wi < W)
            val = cldg16(x + (((q.b * D + di) * H + hi) * W + wi) * P.cin_p + c * ET<T>::PK);
        *reinterpret_cast<uint4*>(smem + (long)v * P.x_pitch + c * 16) = val;
    }
}

template <typename T, int NT>
__global__ __launch_bounds__(256) void conv3d_fwd_kernel(const tav_conv3d_fwd_args a, const ConvPlan P) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int PK = ET<T>::PK, KSTEP = ET<T>::KSTEP, ES = ET<T>::ES;
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), g = lane >> 4, i = lane & 15;
    const Patch q = patch_of(blockIdx.x, P);
    int* const table = reinterpret_cast<int*>(smem + P.table_off);
    for (int c = threadIdx.x; c < 4 * P.k_steps; c += blockDim.x) {
        int off = -1;                                   // (a chunk of the K pad: the fragment is zero, and so is the weight)
        if (c < P.n_chunks) {
            const int k = c * PK, tap = k / P.cin_p, ci = k - tap * P.cin_p, kd = tap / 9, kh = (tap / 3) % 3, kw = tap % 3;
            off = ((kd * (P.th + 2) + kh) * CROW + kw) * (int)P.x_pitch + ci * ES;
        }
        table[c] = off;
    }
    stage_halo<T>(smem, reinterpret_cast<const T*>(a.x), P, q, a.D, a.H, a.W, a.pad);
    __syncthreads();

    const T* const Wt = reinterpret_cast<const T*>(a.w);
    T* const y = reinterpret_cast<T*>(a.y);
    T* const gd = reinterpret_cast<T*>(a.g);
    const char* const vbase = smem + (long)(w * CROW + i) * P.x_pitch;       // voxel (kd 0, row w, column i): the window's origin of tile 0
    const long step16 = 16 * P.x_pitch;
    const long h = q.h0 + w;
    const int ntiles = P.cout_p / 16;
    for (int pass = 0; pass < P.n_passes; ++pass) {
        f32x4 acc[2][NT];
        bool on[NT];
        const T* wrow[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int tile = pass * P.n_tiles + j;
            on[j] = j < P.n_tiles && tile < ntiles;                           // (wave-uniform)
            wrow[j] = Wt + (long)((on[j] ? tile : 0) * 16 + i) * P.kp + PK * g;
            acc[0][j] = acc[1][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        for (int ks = 0; ks < P.k_steps; ++ks) {
            const int off = table[4 * ks + g];
            uint4 x0 = {0u, 0u, 0u, 0u}, x1 = {0u, 0u, 0u, 0u};
            if (off >= 0) {
                x0 = *reinterpret_cast<const uint4*>(vbase + off);
                x1 = *reinterpret_cast<const uint4*>(vbase + off + step16);
            }
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                if (on[j]) {
                    const uint4 wf = cldg16(wrow[j] + ks * KSTEP);
                    mma16<T>(wf, x0, acc[0][j]);
                    mma16<T>(wf, x1, acc[1][j]);
                }
            }
        }
        // ---- epilogue: lane (g, i) holds channels tile 16 + 4g .. + 3 of voxel i of each of the two tiles
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const long col = q.w0 + 16 * m + i;
            const bool live = h < P.oh && col < P.ow;
            const long at = (((q.b * P.od + q.d) * P.oh + h) * P.ow + col) * P.cout_p;
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                if (on[j] && live) {
                    const int co = (pass * P.n_tiles + j) * 16 + 4 * g;
                    f32x4 z = acc[m][j];
                    if (a.bias) {
                        const f32x4 bq = ld4(a.bias + co);
#pragma unroll
                        for (int r = 0; r < 4; ++r) z[r] += bq[r];
                    }
                    if (a.gelu) {
                        f32x4 yv, dv;
                        gelu_both4_t<T>(z, yv, dv);
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (co + r >= a.Cout) dv[r] = 0.f;              // gelu'(0) = 0.5 is not what a pad channel carries
                        st4(y + at + co, yv);
                        if (gd) st4(gd + at + co, dv);
                    } else {
                        st4(y + at + co, z);
                    }
                }
            }
        }
    }
}

template <typename T> TAV_DEV uint4 ones_frag();
template <> TAV_DEV uint4 ones_frag<bf16>() { return make_uint4(0x3F803F80u, 0x3F803F80u, 0x3F803F80u, 0x3F803F80u); }
template <> TAV_DEV uint4 ones_frag<float>() { return make_uint4(0x3F800000u, 0x3F800000u, 0x3F800000u, 0x3F800000u); }

template <typename T, int CIT, int COT>
__global__ __launch_bounds__(256) void conv3d_wgrad_kernel(const tav_conv3d_wgrad_args a, const ConvPlan P, const int nslabs) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int KSTEP = ET<T>::KSTEP, ES = ET<T>::ES, PK = ET<T>::PK;
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), g = lane >> 4, i = lane & 15;
    const int ncog = (P.cout_p / 16) / COT, cig = blockIdx.y / ncog, cog = blockIdx.y % ncog;
    const int ci0 = cig * CIT * 16, co0 = cog * COT * 16;
    const long s = blockIdx.x;
    const long pb = P.patches * s / nslabs, pe = P.patches * (s + 1) / nslabs;
    const int xp = (int)P.x_pitch, zp = (int)P.z_pitch;
    char* const zt = smem + P.wg_z_off;
    const T* const dz = reinterpret_cast<const T*>(a.dz);

    int tapoff[CSLOTS];                                  // slot j of this wave is tap w + 4 j: its window's byte offset in the halo (wave-uniform)
    f32x4 acc[CSLOTS][CIT][COT];
#pragma unroll
    for (int j = 0; j < CSLOTS; ++j) {
        const int tap = w + 4 * j, kd = tap / 9, kh = (tap / 3) % 3, kw = tap % 3;
        tapoff[j] = tap < plan::CONV_TAPS ? ((kd * (P.th + 2) + kh) * CROW + kw) * xp : 0;
#pragma unroll
        for (int m = 0; m < CIT; ++m)
#pragma unroll
            for (int n = 0; n < COT; ++n) acc[j][m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const uint4 ones = ones_frag<T>();
    const int zcpv = P.cout_p * ES / 16, ztotal = P.th * CTW * zcpv;

    for (long p = pb; p < pe; ++p) {
        const Patch q = patch_of(p, P);
        __syncthreads();                                 // the previous patch's fragment reads are done
        stage_halo<T>(smem, reinterpret_cast<const T*>(a.x), P, q, a.D, a.H, a.W, 0);
        for (int it = threadIdx.x; it < ztotal; it += blockDim.x) {
            const int c = it % zcpv, v = it / zcpv, sx = v % CTW, r = v / CTW;
            const long hi = q.h0 + r, wi = q.w0 + sx;
            uint4 val = {0u, 0u, 0u, 0u};                // a voxel past the output edge adds nothing
            if (hi < P.oh && wi < P.ow) val = cldg16(dz + (((q.b * P.od + q.d) * P.oh + hi) * P.ow + wi) * P.cout_p + c * PK);
            *reinterpret_cast<uint4*>(zt + (long)v * zp + c * 16) = val;
        }
        __syncthreads();
        for (int r = 0; r < P.th; ++r) {
#pragma unroll
            for (int v0 = 0; v0 < CTW; v0 += KSTEP) {
                uint4 zf[COT];
#pragma unroll
                for (int n = 0; n < COT; ++n) zf[n] = frag_kstrided<T>(zt + (r * CTW + v0) * zp, zp, 0, co0 + n * 16, lane);
                const char* const xrow = smem + (r * CROW + v0) * xp;
#pragma unroll
                for (int j = 0; j < CSLOTS; ++j) {
                    const int tap = w + 4 * j;           // (wave-uniform: the k-strided bf16 read needs every lane)
                    if (tap < plan::CONV_TAPS) {
#pragma unroll
                        for (int m = 0; m < CIT; ++m) {
                            const uint4 xf = frag_kstrided<T>(xrow + tapoff[j], xp, 0, ci0 + m * 16, lane);
#pragma unroll
                            for (int n = 0; n < COT; ++n) mma16<T>(xf, zf[n], acc[j][m][n]);
                        }
                    } else if (tap == plan::CONV_TAPS) {
#pragma unroll
                        for (int n = 0; n < COT; ++n) mma16<T>(ones, zf[n], acc[j][0][n]);
                    }
                }
            }
        }
    }
    // ---- the slab: [28][cin_p][cout_p] f32; lane (g, i) holds rows ci = 4g .. 4g + 3, column co = i of each tile
    float* const slab = reinterpret_cast<float*>(a.workspace) + s * P.slab_floats;
#pragma unroll
    for (int j = 0; j < CSLOTS; ++j) {
        const int tap = w + 4 * j;
        if (tap > plan::CONV_TAPS || (tap == plan::CONV_TAPS && cig != 0)) continue;
#pragma unroll
        for (int m = 0; m < CIT; ++m) {
            if (tap == plan::CONV_TAPS && m > 0) continue;
#pragma unroll
            for (int n = 0; n < COT; ++n)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    slab[((long)tap * P.cin_p + ci0 + m * 16 + 4 * g + r) * P.cout_p + co0 + n * 16 + i] = acc[j][m][n][r];
        }
    }
}

__global__ __launch_bounds__(256) void conv3d_slab_sum_kernel(const float* __restrict__ ws, float* __restrict__ dw, float* __restrict__ db, const int nslabs,
                                                               const long slab_floats, const int Cin, const int Cout, const int cin_p, const int cout_p) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x, nw = (long)Cout * Cin * plan::CONV_TAPS;
    long at;
    float* dst;
    if (idx < nw) {
        const int co = (int)(idx / (Cin * plan::CONV_TAPS)), rem = (int)(idx % (Cin * plan::CONV_TAPS)), ci = rem / plan::CONV_TAPS, tap = rem % plan::CONV_TAPS;
        at = ((long)tap * cin_p + ci) * cout_p + co;
        dst = dw + idx;
    } else if (idx < nw + Cout && db) {
        at = (long)plan::CONV_TAPS * cin_p * cout_p + (idx - nw);
        dst = db + (idx - nw);
    } else {
        return;
    }
    float sum = 0.f;
    for (int s = 0; s < nslabs; ++s) sum += ws[s * slab_floats + at];
    *dst = sum;
}

template <typename T>
__global__ __launch_bounds__(256) void conv3d_dz_kernel(const T* __restrict__ dy, const T* __restrict__ g, T* __restrict__ dz, const long n4) {
    const long k = (long)blockIdx.x * 256 + threadIdx.x;
    if (k < n4) {
        f32x4 v = ld4(dy + 4 * k);
        if (g) {
            const f32x4 gv = ld4(g + 4 * k);
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] *= gv[r];
        }
        st4(dz + 4 * k, v);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void conv3d_pack_input_kernel(const float* __restrict__ src, T* __restrict__ dst, const long B, const int C, const long S, const int cp) {
    const long v = (long)blockIdx.x * 256 + threadIdx.x;          // voxel b S + s: reads run along s per channel, the row of cp channels is this thread's
    if (v >= B * S) return;
    const long b = v / S, s = v % S;
    for (int c = 0; c < cp; c += 4) {
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (c + j < C) ? src[(b * C + c + j) * S + s] : 0.f;
        st4(dst + v * cp + c, o);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void conv3d_pack_weight_kernel(const float* __restrict__ wsrc, T* __restrict__ dst, const int Cout, const int Cin, const int flip,
                                                                  const int rows, const int cin_inner_p, const long kp) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * kp) return;
    const int row = (int)(idx / kp), k = (int)(idx % kp), t = k / cin_inner_p, inner = k % cin_inner_p;
    float v = 0.f;
    if (t < plan::CONV_TAPS) {
        const int co = flip ? inner : row, ci = flip ? row : inner, tap = flip ? plan::CONV_TAPS - 1 - t : t;
        if (co < Cout && ci < Cin) v = wsrc[((long)co * Cin + ci) * plan::CONV_TAPS + tap];
    }
    ET<T>::st(dst + idx, v);
}

// ---- flatten + Linear: thread = voxel s (reads of w run along s for each channel; the voxel's channels-last row is the thread's own)
template <typename T>
__global__ __launch_bounds__(256) void flat_fwd_kernel(const tav_flat_linear_fwd_args a, const int nparts) {
    __shared__ float red[4][plan::FLAT_MAX_O];
    const long b = blockIdx.y, p = blockIdx.x, S = a.S, F = a.C * S;
    const long s0 = S * p / nparts, s1 = S * (p + 1) / nparts;
    const int C = (int)a.C, O = (int)a.O, cp = (int)((a.C + 15) / 16 * 16);
    const T* const x = reinterpret_cast<const T*>(a.x);
    float acc[plan::FLAT_MAX_O];
#pragma unroll
    for (int o = 0; o < plan::FLAT_MAX_O; ++o) acc[o] = 0.f;
    for (long s = s0 + threadIdx.x; s < s1; s += 256) {
        const T* const xv = x + (b * S + s) * cp;
        for (int c = 0; c < C; c += 4) {
            const f32x4 x4 = ld4(xv + c);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (c + j < C) {
                    const float* const wp = a.w + (long)(c + j) * S + s;
#pragma unroll
                    for (int o = 0; o < plan::FLAT_MAX_O; ++o)
                        if (o < O) acc[o] = fmaf(x4[j], wp[o * F], acc[o]);
                }
            }
        }
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 0; o < plan::FLAT_MAX_O; ++o) {
        const float v = wave_sum(acc[o]);
        if (lane == 0) red[w][o] = v;
    }
    __syncthreads();
    if ((int)threadIdx.x < O) {
        const int o = threadIdx.x;
        reinterpret_cast<float*>(a.workspace)[(b * nparts + p) * O + o] = ((red[0][o] + red[1][o]) + red[2][o]) + red[3][o];
    }
}

__global__ __launch_bounds__(256) void flat_sum_kernel(const float* __restrict__ part, const float* __restrict__ bias, float* __restrict__ out, const long B, const int O,
                                                        const int nparts) {
    const long k = (long)blockIdx.x * 256 + threadIdx.x;
    if (k >= B * O) return;
    const long b = k / O;
    const int o = (int)(k % O);
    float sum = 0.f;
    for (int p = 0; p < nparts; ++p) sum += part[(b * nparts + p) * O + o];
    out[k] = sum + (bias ? bias[o] : 0.f);
}

template <typename T>
__global__ __launch_bounds__(256) void flat_bwd_kernel(const tav_flat_linear_bwd_args a) {
    const long s = (long)blockIdx.x * 256 + threadIdx.x, S = a.S, F = a.C * S, B = a.B;
    const int C = (int)a.C, O = (int)a.O, cp = (int)((a.C + 15) / 16 * 16);
    if (a.db && blockIdx.x == 0 && (int)threadIdx.x < O) {
        float sum = 0.f;
        for (long b = 0; b < B; ++b) sum += a.dy[b * O + threadIdx.x];
        a.db[threadIdx.x] = sum;
    }
    if (s >= S) return;
    const T* const x = reinterpret_cast<const T*>(a.x);
    T* const dx = reinterpret_cast<T*>(a.dx);
    for (int c = 0; c < cp; c += 4) {
        float wv[plan::FLAT_MAX_O][4], dwv[plan::FLAT_MAX_O][4];
#pragma unroll
        for (int o = 0; o < plan::FLAT_MAX_O; ++o)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                wv[o][j] = (o < O && c + j < C) ? a.w[o * F + (long)(c + j) * S + s] : 0.f;
                dwv[o][j] = 0.f;
            }
        for (long b = 0; b < B; ++b) {
            const f32x4 x4 = ld4(x + (b * S + s) * cp + c);
            f32x4 d4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int o = 0; o < plan::FLAT_MAX_O; ++o) {
                if (o < O) {
                    const float d = a.dy[b * O + o];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        d4[j] = fmaf(d, wv[o][j], d4[j]);
                        dwv[o][j] = fmaf(d, x4[j], dwv[o][j]);
                    }
                }
            }
            if (dx) st4(dx + (b * S + s) * cp + c, d4);
        }
#pragma unroll
        for (int o = 0; o < plan::FLAT_MAX_O; ++o)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (o < O && c + j < C) a.dw[o * F + (long)(c + j) * S + s] = dwv[o][j];
    }
}

__global__ __launch_bounds__(256) void sigmoid_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, const long n) {
    const long k = (long)blockIdx.x * 256 + threadIdx.x;
    if (k < n) y[k] = 1.0f / (1.0f + expf(-x[k]));
}
__global__ __launch_bounds__(256) void sigmoid_bwd_kernel(const float* __restrict__ y, const float* __restrict__ dy, float* __restrict__ dx, const long n) {
    const long k = (long)blockIdx.x * 256 + threadIdx.x;
    if (k < n) dx[k] = dy[k] * (y[k] * (1.0f - y[k]));
}

template <typename T> struct ConvLaunch {
    template <int NT> static int fwd(const tav_conv3d_fwd_args& a, const ConvPlan& P, const plan::Launch& L, void* stream) {
        TAV_LAUNCH((conv3d_fwd_kernel<T, NT>), L, stream, a, P);
        return 0;
    }
    template <int CIT, int COT> static int wgrad(const tav_conv3d_wgrad_args& a, const ConvPlan& P, int nslabs, const plan::Launch& L, void* stream) {
        TAV_LAUNCH((conv3d_wgrad_kernel<T, CIT, COT>), L, stream, a, P, nslabs);
        return 0;
    }
};

}  // namespace tav
using namespace tav;

extern "C" int tav_conv_version(void) { return plan::CONV_ABI_VERSION; }

extern "C" int tav_conv3d_get_plan(int64_t B, int64_t D, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int32_t pad, int32_t dtype, tav_conv3d_plan* out) {
    if (!out) return TAV_ERR_NULL;
    if (const int rc = plan::conv_shape_validate(B, D, H, W, Cin, Cout, pad, dtype)) return rc;
    plan::conv_plan_public(plan::conv_plan(B, D, H, W, Cin, Cout, pad, dtype), out);
    return 0;
}

extern "C" int64_t tav_conv3d_wgrad_ws_bytes(int64_t B, int64_t D, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int32_t dtype, int32_t nslabs) {
    return plan::conv_wgrad_ws_bytes(B, D, H, W, Cin, Cout, dtype, nslabs);
}

extern "C" int tav_conv3d_pack_input(const float* src, void* dst, int64_t B, int64_t C, int64_t D, int64_t H, int64_t W, int32_t dtype, void* stream) {
    if (const int rc = plan::conv_pack_input_validate(src && dst, B, C, D, H, W, dtype)) return rc;
    const long S = D * H * W;
    const plan::Launch L = plan::grid1(B * S);
    return floats::dispatch(dtype, [&](auto tag) -> int {
        using T = decltype(tag);
        TAV_LAUNCH(conv3d_pack_input_kernel<T>, L, stream, src, reinterpret_cast<T*>(dst), (long)B, (int)C, S, (int)plan::conv_cp(C));
        return 0;
    });
}

extern "C" int tav_conv3d_pack_weight(const float* w, void* dst, int64_t Cout, int64_t Cin, int32_t flip_transpose, int32_t dtype, void* stream) {
    if (const int rc = plan::conv_pack_weight_validate(w && dst, Cout, Cin, flip_transpose, dtype)) return rc;
    const int rows = (int)plan::conv_cp(flip_transpose ? Cin : Cout), inner_p = (int)plan::conv_cp(flip_transpose ? Cout : Cin);
    const long kp = plan::conv_kp(flip_transpose ? Cout : Cin, dtype);
    const plan::Launch L = plan::grid1(rows * kp);
    return floats::dispatch(dtype, [&](auto tag) -> int {
        using T = decltype(tag);
        TAV_LAUNCH(conv3d_pack_weight_kernel<T>, L, stream, w, reinterpret_cast<T*>(dst), (int)Cout, (int)Cin, (int)flip_transpose, rows, inner_p, kp);
        return 0;
    });
}

extern "C" int tav_conv3d_fwd(const tav_conv3d_fwd_args* a, void* stream) {
    ConvPlan P;
    if (const int rc = plan::conv_fwd_validate(a, &P)) return rc;
    const plan::Launch L{P.patches, 1, 1, P.block, (size_t)P.lds_bytes};
    return floats::dispatch(a->dtype, [&](auto tag) -> int {
        using LL = ConvLaunch<decltype(tag)>;
        switch (P.n_tiles) {
            case 1: return LL::template fwd<1>(*a, P, L, stream);
            case 2: return LL::template fwd<2>(*a, P, L, stream);
            case 3: return LL::template fwd<3>(*a, P, L, stream);
            default: return LL::template fwd<4>(*a, P, L, stream);
        }
    });
}

extern "C" int tav_conv3d_dz(const void* dy, const void* g, void* dz, int64_t n, int32_t dtype, void* stream) {
    if (const int rc = plan::conv_dz_validate(dy && dz, n, dtype)) return rc;
    if ((uintptr_t)dy % 16 || (uintptr_t)g % 16 || (uintptr_t)dz % 16) return TAV_ERR_ALIGN;
    const plan::Launch L = plan::grid1(n / 4);
    return floats::dispatch(dtype, [&](auto tag) -> int {
        using T = decltype(tag);
        TAV_LAUNCH(conv3d_dz_kernel<T>, L, stream, reinterpret_cast<const T*>(dy), reinterpret_cast<const T*>(g), reinterpret_cast<T*>(dz), (long)(n / 4));
        return 0;
    });
}

extern "C" int tav_conv3d_wgrad(const tav_conv3d_wgrad_args* a, void* stream) {
    ConvPlan P;
    int nslabs = 0;
    if (const int rc = plan::conv_wgrad_validate(a, &P, &nslabs)) return rc;
    const plan::Launch L{nslabs, P.wg_groups, 1, 64 * plan::CONV_WG_WAVES, (size_t)P.wg_lds_bytes};
    const int rc = floats::dispatch(a->dtype, [&](auto tag) -> int {
        using LL = ConvLaunch<decltype(tag)>;
        if (P.wg_cit == 2) return LL::template wgrad<2, 2>(*a, P, nslabs, L, stream);
        if (P.wg_cot == 3) return LL::template wgrad<1, 3>(*a, P, nslabs, L, stream);
        if (P.wg_cot == 2) return LL::template wgrad<1, 2>(*a, P, nslabs, L, stream);
        return LL::template wgrad<1, 1>(*a, P, nslabs, L, stream);
    });
    if (rc) return rc;
    const plan::Launch R = plan::grid1(a->Cout * a->Cin * plan::CONV_TAPS + a->Cout);
    TAV_LAUNCH(conv3d_slab_sum_kernel, R, stream, reinterpret_cast<const float*>(a->workspace), a->dw, a->db, nslabs, (long)P.slab_floats, (int)a->Cin, (int)a->Cout,
               P.cin_p, P.cout_p);
    return 0;
}

extern "C" int32_t tav_flat_linear_parts(int64_t S) { return plan::flat_parts(S); }
extern "C" int64_t tav_flat_linear_ws_bytes(int64_t B, int64_t S, int64_t O, int32_t nparts) { return plan::flat_ws_bytes(B, S, O, nparts); }

extern "C" int tav_flat_linear_fwd(const tav_flat_linear_fwd_args* a, void* stream) {
    int nparts = 0;
    if (const int rc = plan::flat_fwd_validate(a, &nparts)) return rc;
    const plan::Launch L{nparts, a->B, 1, 256, 0};
    const int rc = floats::dispatch(a->dtype, [&](auto tag) -> int {
        TAV_LAUNCH(flat_fwd_kernel<decltype(tag)>, L, stream, *a, nparts);
        return 0;
    });
    if (rc) return rc;
    const plan::Launch R = plan::grid1(a->B * a->O);
    TAV_LAUNCH(flat_sum_kernel, R, stream, reinterpret_cast<const float*>(a->workspace), a->bias, a->out, (long)a->B, (int)a->O, nparts);
    return 0;
}

extern "C" int tav_flat_linear_bwd(const tav_flat_linear_bwd_args* a, void* stream) {
    if (const int rc = plan::flat_bwd_validate(a)) return rc;
    const plan::Launch L = plan::grid1(a->S);
    return floats::dispatch(a->dtype, [&](auto tag) -> int {
        TAV_LAUNCH(flat_bwd_kernel<decltype(tag)>, L, stream, *a);
        return 0;
    });
}

extern "C" int tav_sigmoid_fwd(const float* x, float* y, int64_t n, void* stream) {
    if (const int rc = plan::sigmoid_validate(x && y, n)) return rc;
    const plan::Launch L = plan::grid1(n);
    TAV_LAUNCH(sigmoid_fwd_kernel, L, stream, x, y, (long)n);
    return 0;
}

extern "C" int tav_sigmoid_bwd(const float* y, const float* dy, float* dx, int64_t n, void* stream) {
    if (const int rc = plan::sigmoid_validate(y && dy && dx, n)) return rc;
    const plan::Launch L = plan::grid1(n);
    TAV_LAUNCH(sigmoid_bwd_kernel, L, stream, y, dy, dx, (long)n);
    return 0;
}
