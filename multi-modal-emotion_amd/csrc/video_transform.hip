// Video clip transform (reference models/tav.py:51-121, videoMAE_features): decoded frames -> the f32 [nf][3][out_h][out_w] clip tav_patchify reads.
//   subsample (frame[] from the host) -> /255, normalise -> crop -> bilinear to (mid_h, mid_w) -> bilinear to (out_h, out_w) -> flips
// One launch per clip, one thread per output pixel and its three channels.  The two resize levels are fused: an output pixel is the bilinear
// mix of 2 x 2 pixels of the intermediate image, each the bilinear mix of 2 x 2 source pixels, and the intermediate image is never stored.  A flip
// mirrors the output coordinate.  The interpolation weights of a pixel sum to 1, so the affine normalisation is applied once, last, on the raw
// value: y = v * scale[c] - shift[c].  Source coordinates are exact integers (tests/video_transform_ref.py is the host model):
//   num = max(0, (2 o + 1) n_in - n_out),  i0 = num / (2 n_out),  i1 = min(i0 + 1, n_in - 1),  lam = float(num - i0 * 2 n_out) / float(2 n_out)
// No reduction, no atomic: the result does not depend on the launch geometry.
#include "common.h"
#include "tavhip_internal.h"

namespace tav {
// defined with the host decisions (entry_plan.h)
using plan::VX_TW, plan::VX_TH;

// the source taps of one output coordinate along one axis: n = 2 intermediate pixels (1 without a first resize), each with two source indices
struct VxAxis {
    int i0[2], i1[2];     // source indices, crop offset added, clamped into the frame
    float l1[2];          // weight of i1 against i0
    float l2;             // weight of intermediate pixel 1 against 0
};

TAV_DEV void vx_coord(int o, int n_in, int n_out, int& i0, int& i1, float& lam) {
    int num = (2 * o + 1) * n_in - n_out;
    num = num < 0 ? 0 : num;
    const int den = 2 * n_out;
    i0 = num / den;
    lam = __fdiv_rn((float)(num - i0 * den), (float)den);
    i0 = i0 < n_in - 1 ? i0 : n_in - 1;
    i1 = i0 + 1 < n_in - 1 ? i0 + 1 : n_in - 1;
}

TAV_DEV int vx_clamp(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

// o: output coordinate before the flip; n_src: cropped size; off: crop offset; lim: frame size (every index is clamped into [0, lim))
TAV_DEV VxAxis vx_axis(int o, int n_src, int mid, int n_out, int off, int lim) {
    VxAxis a;
    if (mid > 0) {
        int j0, j1;
        vx_coord(o, mid, n_out, j0, j1, a.l2);
        vx_coord(j0, n_src, mid, a.i0[0], a.i1[0], a.l1[0]);
        vx_coord(j1, n_src, mid, a.i0[1], a.i1[1], a.l1[1]);
    } else {
        vx_coord(o, n_src, n_out, a.i0[0], a.i1[0], a.l1[0]);
        a.i0[1] = a.i0[0]; a.i1[1] = a.i1[0]; a.l1[1] = a.l1[0]; a.l2 = 0.f;
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        a.i0[k] = vx_clamp(a.i0[k] + off, lim);
        a.i1[k] = vx_clamp(a.i1[k] + off, lim);
    }
    return a;
}

// torch's upsample_bilinear2d form: h0 * (w0 * p00 + w1 * p01) + h1 * (w0 * p10 + w1 * p11), w0 = 1 - w1, h0 = 1 - h1
TAV_DEV float vx_mix(float p00, float p01, float p10, float p11, float w1, float h1) {
    const float w0 = 1.f - w1, h0 = 1.f - h1;
    return h0 * (w0 * p00 + w1 * p01) + h1 * (w0 * p10 + w1 * p11);
}

template <typename TS, int NMID>      // NMID: intermediate pixels per axis, 2 with a first resize and 1 without
__global__ __launch_bounds__(VX_TW * VX_TH) void video_clip_transform_kernel(const TS* __restrict__ src, float* __restrict__ dst, const tav_clip_xform x) {
    __shared__ VxAxis s_x[VX_TW], s_y[VX_TH];
    const int tid = threadIdx.x, tx = tid & (VX_TW - 1), ty = tid / VX_TW;
    const int ox = blockIdx.x * VX_TW + tx, oy = blockIdx.y * VX_TH + ty, f = blockIdx.z;
    if (tid < VX_TW) {
        const int o = blockIdx.x * VX_TW + tid;
        if (o < x.out_w) s_x[tid] = vx_axis(x.hflip ? x.out_w - 1 - o : o, x.crop_w, x.mid_w, x.out_w, x.crop_left, x.W);
    } else if (tid < VX_TW + VX_TH) {
        const int o = blockIdx.y * VX_TH + (tid - VX_TW);
        if (o < x.out_h) s_y[tid - VX_TW] = vx_axis(x.vflip ? x.out_h - 1 - o : o, x.crop_h, x.mid_h, x.out_h, x.crop_top, x.H);
    }
    __syncthreads();
    if (ox >= x.out_w || oy >= x.out_h) return;
    const VxAxis ax = s_x[tx], ay = s_y[ty];
    const TS* frame = src + (long)vx_clamp(x.frame[f], x.T) * x.sT;
    float m[NMID][NMID][3];              // the intermediate pixels [row][column][channel]
#pragma unroll
    for (int r = 0; r < NMID; ++r) {
        const TS* row0 = frame + (long)ay.i0[r] * x.sH;
        const TS* row1 = frame + (long)ay.i1[r] * x.sH;
#pragma unroll
        for (int q = 0; q < NMID; ++q) {
            const long c0 = (long)ax.i0[q] * x.sW, c1 = (long)ax.i1[q] * x.sW;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const long oc = c * x.sC;
                m[r][q][c] = vx_mix((float)row0[c0 + oc], (float)row0[c1 + oc], (float)row1[c0 + oc], (float)row1[c1 + oc], ax.l1[q], ay.l1[r]);
            }
        }
    }
    float* out = dst + ((long)f * 3 * x.out_h + oy) * x.out_w + ox;
    const long plane = (long)x.out_h * x.out_w;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float v = NMID == 2 ? vx_mix(m[0][0][c], m[0][NMID - 1][c], m[NMID - 1][0][c], m[NMID - 1][NMID - 1][c], ax.l2, ay.l2) : m[0][0][c];
        out[c * plane] = v * x.scale[c] - x.shift[c];
    }
}

}  // namespace tav
using namespace tav;

extern "C" int tav_video_clip_transform(const void* src, float* dst, const tav_clip_xform* x, void* stream) {
    if (const int rc = plan::video_clip_validate(src && dst && x, x)) return rc;
    const plan::Launch L = plan::video_clip_launch(x);
    return dtypes<on<TAV_U8>, on<TAV_F32>>::dispatch(x->src_dtype, [&](auto t) {
        using T = decltype(t);
        if (x->mid_h != 0) TAV_LAUNCH((video_clip_transform_kernel<T, 2>), L, stream, (const T*)src, dst, *x);      // two resizes
        else TAV_LAUNCH((video_clip_transform_kernel<T, 1>), L, stream, (const T*)src, dst, *x);
        return 0;
    });
}
