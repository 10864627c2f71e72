// SpecAugment (reference models/tav.py:269-306): the span sampler, the masked copy and its backward.
//   draw : one workgroup per row turns (seed, tag) into a uint8 span mask -- the sampler DESIGN.md §"Dropout RNG invariant" specifies
//   fwd  : y = fmask ? 0 : (tmask ? embed : x)                                  (pure select: bit-exact)
//   bwd  : dx = (tmask | fmask) ? 0 : dy, dembed = column sums of dy over the time-masked rows, in a fixed order (partials + second stage)
#include "common.h"
#include "tavhip_internal.h"

namespace tav {
// defined with the host decisions (entry_plan.h)
using plan::SPEC_T, plan::SPEC_MAX_SPANS, plan::SPEC_EPS_STRIDE;

struct SpecKey { uint64_t key; int s; };
TAV_DEV bool spec_less(uint64_t ka, int sa, uint64_t kb, int sb) { return ka < kb || (ka == kb && sa < sb); }

// floor(prob * len / length + eps) in f32, every operation rounded to nearest on its own (tests/specaug_ref.py is the host model)
TAV_DEV int spec_n0(float prob, int len, int length, float eps) {
    return (int)floorf(__fadd_rn(__fdiv_rn(__fmul_rn(prob, (float)len), (float)length), eps));
}

__global__ __launch_bounds__(SPEC_T) void specaug_draw_kernel(const uint8_t* __restrict__ valid, uint8_t* __restrict__ mask, int32_t* __restrict__ nspans,
                                                              int L, float prob, int length, int min_masks, uint64_t seed,
                                                              const uint64_t* __restrict__ seed_state, uint64_t tag) {
    __shared__ int s_cnt[SPEC_T / 64];
    __shared__ uint64_t s_key[SPEC_T / 64];
    __shared__ int s_pos[SPEC_T / 64];
    __shared__ int s_starts[SPEC_MAX_SPANS];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (seed_state) seed = seed_state[0];
    // len = non-zero bytes of the row's `valid`
    int len = L;
    if (valid) {
        int c = 0;
        for (int t = tid; t < L; t += SPEC_T) c += valid[(long)row * L + t] != 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
        if (lane == 0) s_cnt[wave] = c;
        __syncthreads();
        len = 0;
#pragma unroll
        for (int w = 0; w < SPEC_T / 64; ++w) len += s_cnt[w];
    }
    const float eps = (float)(mix64(seed ^ mix64(tag + SPEC_EPS_STRIDE)) >> 40) * (1.f / 16777216.f);       // one per call: every row computes the same
    int n = max(spec_n0(prob, len, length, eps), min_masks);
    const int nstarts = max(len - (length - 1), 0);
    n = min(min(n, nstarts), min(L / length, SPEC_MAX_SPANS));
    // the n smallest (key, s) pairs, one per pass: the smallest pair greater than the one chosen last
    const uint64_t base = tag + (uint64_t)row * (uint64_t)L;
    uint64_t last_key = 0;
    int last_s = -1;
    for (int k = 0; k < n; ++k) {
        uint64_t bk = ~0ull;
        int bs = 0x7fffffff;
        for (int s = tid; s < nstarts; s += SPEC_T) {
            const uint64_t key = mix64(seed ^ mix64(base + (uint64_t)s));
            if ((k == 0 || spec_less(last_key, last_s, key, s)) && spec_less(key, s, bk, bs)) { bk = key; bs = s; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint64_t ok = __shfl_xor(bk, o, 64);
            const int os = __shfl_xor(bs, o, 64);
            if (spec_less(ok, os, bk, bs)) { bk = ok; bs = os; }
        }
        __syncthreads();                    // (the previous pass's reads of s_key / s_pos are done)
        if (lane == 0) { s_key[wave] = bk; s_pos[wave] = bs; }
        __syncthreads();
        bk = s_key[0];
        bs = s_pos[0];
#pragma unroll
        for (int w = 1; w < SPEC_T / 64; ++w)
            if (spec_less(s_key[w], s_pos[w], bk, bs)) { bk = s_key[w]; bs = s_pos[w]; }
        last_key = bk;
        last_s = bs;
        if (tid == 0) s_starts[k] = bs;
    }
    __syncthreads();
    for (int t = tid; t < L; t += SPEC_T) {
        uint8_t m = 0;
        for (int k = 0; k < n; ++k) {
            const int s = s_starts[k];
            m |= (s <= t && t < s + length) ? 1 : 0;
        }
        mask[(long)row * L + t] = m;
    }
    if (nspans && tid == 0) nspans[row] = n;
}

// four channels of one frame per thread
__global__ void specaug_fwd_kernel(const float* __restrict__ x, const uint8_t* __restrict__ tmask, const uint8_t* __restrict__ fmask,
                                   const float* __restrict__ embed, float* __restrict__ y, long n4, int T, int H4) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const long r = i / H4;
    const int c4 = (int)(i - r * H4);
    f32x4 v = (tmask && tmask[r]) ? ld4(embed + 4 * c4) : ld4(x + 4 * i);
    if (fmask) {
        const uchar4 f = *reinterpret_cast<const uchar4*>(fmask + (r / T) * (4L * H4) + 4 * c4);
        if (f.x) v[0] = 0.f;
        if (f.y) v[1] = 0.f;
        if (f.z) v[2] = 0.f;
        if (f.w) v[3] = 0.f;
    }
    st4(y + 4 * i, v);
}

// Workgroup (x, p): four channels per thread, the rows [p * rpb, (p + 1) * rpb) in order.  Writes dx and, with `partials`, the part's column
// sums over the time-masked rows; the final kernel adds the parts in order -- no atomics, the same bits on every run.
__global__ __launch_bounds__(256) void specaug_bwd_kernel(const float* __restrict__ dy, const uint8_t* __restrict__ tmask, const uint8_t* __restrict__ fmask,
                                                          float* __restrict__ dx, float* __restrict__ partials, long rows, int T, int H4, int rpb) {
    const int c4 = blockIdx.x * 256 + threadIdx.x;
    if (c4 >= H4) return;
    const long r0 = (long)blockIdx.y * rpb;
    const long r1 = r0 + rpb < rows ? r0 + rpb : rows;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (long r = r0; r < r1; ++r) {
        f32x4 v = ld4(dy + (r * H4 + c4) * 4);
        if (fmask) {
            const uchar4 f = *reinterpret_cast<const uchar4*>(fmask + (r / T) * (4L * H4) + 4 * c4);
            if (f.x) v[0] = 0.f;
            if (f.y) v[1] = 0.f;
            if (f.z) v[2] = 0.f;
            if (f.w) v[3] = 0.f;
        }
        const bool tm = tmask && tmask[r];
        if (tm) acc += v;
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        st4(dx + (r * H4 + c4) * 4, tm ? zero : v);
    }
    if (partials) st4(partials + ((long)blockIdx.y * H4 + c4) * 4, acc);
}
__global__ void specaug_bwd_final_kernel(const float* __restrict__ partials, float* __restrict__ dembed, int nparts, int H4) {
    const int c4 = blockIdx.x * blockDim.x + threadIdx.x;
    if (c4 >= H4) return;
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
    for (int p = 0; p < nparts; ++p) a += ld4(partials + ((long)p * H4 + c4) * 4);
    st4(dembed + 4 * c4, a);
}

}  // namespace tav
using namespace tav;

extern "C" int tav_specaug_draw(const uint8_t* valid, uint8_t* mask, int32_t* nspans, int64_t B, int64_t L, float prob, int64_t length,
                                int64_t min_masks, uint64_t seed, uint64_t tag, void* stream) {
    if (const int rc = plan::specaug_draw_validate(mask, B, L, prob, length, min_masks)) return rc;
    TAV_LAUNCH(specaug_draw_kernel, (plan::Launch{B, 1, 1, SPEC_T, 0}), stream, valid, mask, nspans, (int)L, prob, (int)length, (int)min_masks, seed,
               (const uint64_t*)nullptr, tag);
    return 0;
}
extern "C" int tav_specaug_draw_dev(const uint8_t* valid, uint8_t* mask, int32_t* nspans, int64_t B, int64_t L, float prob, int64_t length,
                                    int64_t min_masks, const uint64_t* seed_state, uint64_t tag, void* stream) {
    if (const int rc = plan::specaug_draw_validate(seed_state && mask, B, L, prob, length, min_masks)) return rc;
    TAV_LAUNCH(specaug_draw_kernel, (plan::Launch{B, 1, 1, SPEC_T, 0}), stream, valid, mask, nspans, (int)L, prob, (int)length, (int)min_masks, (uint64_t)0,
               seed_state, tag);
    return 0;
}

extern "C" int tav_specaug_fwd(const float* x, const uint8_t* tmask, const uint8_t* fmask, const float* embed, float* y, int64_t B, int64_t T,
                               int64_t H, void* stream) {
    const bool al = plan::aligned(x, 16) && plan::aligned(y, 16) && plan::aligned(embed, 16) && plan::aligned(fmask, 4);
    if (const int rc = plan::specaug_fwd_validate(x && y && (!tmask || embed), al, B, T, H)) return rc;
    const long n4 = B * T * (H / 4);
    TAV_LAUNCH(specaug_fwd_kernel, plan::grid1(n4), stream, x, tmask, fmask, embed, y, n4, (int)T, (int)(H / 4));
    return 0;
}

extern "C" int64_t tav_specaug_bwd_ws_bytes(int64_t rows, int64_t H) { return plan::specaug_bwd_ws_bytes(rows, H); }
extern "C" int tav_specaug_bwd(const float* dy, const uint8_t* tmask, const uint8_t* fmask, float* dx, float* dembed, void* workspace,
                               int64_t workspace_bytes, int64_t B, int64_t T, int64_t H, void* stream) {
    const bool al = plan::aligned(dy, 16) && plan::aligned(dx, 16) && plan::aligned(dembed, 16) && plan::aligned(workspace, 16) && plan::aligned(fmask, 4);
    if (const int rc = plan::specaug_bwd_validate(dy && dx && (!dembed || workspace), al, dembed, workspace_bytes, B, T, H)) return rc;
    const int64_t rows = B * T;
    const plan::PartsPlan P = plan::specaug_bwd_plan(rows, H);
    float* partials = dembed ? (float*)workspace : nullptr;
    TAV_LAUNCH(specaug_bwd_kernel, P.partial, stream, dy, tmask, fmask, dx, partials, (long)rows, (int)T, (int)(H / 4), P.rows_per_part);
    if (dembed) TAV_LAUNCH(specaug_bwd_final_kernel, P.final_, stream, (const float*)partials, dembed, P.parts, (int)(H / 4));
    return 0;
}
