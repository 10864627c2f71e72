// Audio waveform transform (reference models/tav.py:165-169, speech_file_to_array_fn after the decoder): decoded PCM -> one row of the
// [B, T] f32 batch the audio front-end reads and one row of its 0/1 mask.  torchaudio's Resample(sr, target) (sinc_interp_hann, width 6,
// rolloff 0.99), .squeeze() and the mean over the channels:
//   y[q n + p] = sum_k h[p][k] * mean_c xpad_c[q o + k],   xpad = x with `width` zeros in front and `width + o` behind,  L_out = ceil(n L / o)
// (the filter is linear, so the channel mean is formed once on the input; tests/audio_resample_ref.py is the host model and keeps the
// reference's order).  torchaudio's conv1d runs all 2 width + o taps of a phase; only the taps inside the Hann window are non-zero in f32,
// and the host hands over just those: table[p][0..ntap) starts at tap first[p].  One launch per utterance.  A workgroup makes `tile`
// consecutive outputs: it forms the channel mean of the input span they read in LDS, once (ascending channel sum, then * 1.0f / C; positions
// outside [0, L) are the zero padding: a predicate, the load itself is clamped into the buffer), copies the compact table into LDS when it
// fits, and every thread runs fmaf over ascending k from 0 for its outputs.  No atomic, no cross-thread reduction: the bits do not depend
// on the launch.  Row elements [L_out, T_row) are written 0 (mask 0) by the same launch.
#include "common.h"
#include "tavhip_internal.h"

namespace tav {
// defined with the host decisions (entry_plan.h)
using plan::AR_THREADS, plan::AR_SPAN_MAX, plan::AR_TABLE_MAX;

TAV_DEV float ar_load(const float* p) { return *p; }
TAV_DEV float ar_load(const int16_t* p) { return (float)*p * 0x1p-15f; }          // exact: what torchaudio.load makes of a 16-bit file

template <typename TS>
__global__ __launch_bounds__(AR_THREADS) void audio_resample_kernel(const TS* __restrict__ src, const float* __restrict__ table,
                                                                    const int32_t* __restrict__ first, float* __restrict__ values,
                                                                    float* __restrict__ mask, const tav_resample_args a, const long L_out,
                                                                    const int tile, const int table_in_lds, const float inv_c) {
    __shared__ float s_x[AR_SPAN_MAX];
    __shared__ float s_h[AR_TABLE_MAX];
    const int tid = threadIdx.x;
    const long i0 = (long)blockIdx.x * tile;
    if (i0 >= L_out) {                     // a workgroup of the tail only (the whole workgroup takes this branch)
        for (int j = tid; j < tile; j += AR_THREADS) {
            const long i = i0 + j;
            if (i < a.T_row) {
                values[i] = 0.f;
                if (mask) mask[i] = 0.f;
            }
        }
        return;
    }
    const int o = a.o, n = a.n, ntap = a.ntap, pitch = ntap | 1;
    const long last = (i0 + tile < L_out ? i0 + tile : L_out) - 1;       // the last sample of this tile
    const long q_lo = i0 / n;
    const int nq = (int)(last / n - q_lo) + 1;
    const int span = (nq - 1) * o + 2 * a.width + o;                     // <= ar_span(tile) <= AR_SPAN_MAX: the host chose the tile so
    const long x_lo = q_lo * o - a.width;                                // input position of s_x[0]
    for (int t = tid; t < span; t += AR_THREADS) {
        const long pos = x_lo + t;
        const long cp = pos < 0 ? 0 : (pos >= a.L ? a.L - 1 : pos);
        const TS* s = src + cp * a.sL;
        float sum = 0.f;
        for (int c = 0; c < a.C; ++c) sum += ar_load(s + c * a.sC);
        s_x[t] = (pos >= 0 && pos < a.L) ? sum * inv_c : 0.f;
    }
    if (table_in_lds)
        for (int t = tid; t < n * ntap; t += AR_THREADS) s_h[(t / ntap) * pitch + t % ntap] = table[t];
    __syncthreads();
    const int first_max = 2 * a.width + o - ntap;                        // the host checked a.first_max against it; the device array is clamped besides
    const int r0 = (int)(i0 - q_lo * n);                                 // < n
    for (int j = tid; j < tile; j += AR_THREADS) {
        const long i = i0 + j;
        if (i >= a.T_row) break;
        float acc = 0.f;
        if (i < L_out) {
            const int r = r0 + j, qr = r / n, p = r - qr * n;
            int f = first[p];
            f = f < 0 ? 0 : (f > first_max ? first_max : f);
            const float* x = s_x + qr * o + f;                           // qr * o + f + ntap <= (nq - 1) * o + 2 width + o = span
            if (table_in_lds) {
                const float* h = s_h + p * pitch;
                for (int k = 0; k < ntap; ++k) acc = fmaf(h[k], x[k], acc);
            } else {
                const float* h = table + (long)p * ntap;
                for (int k = 0; k < ntap; ++k) acc = fmaf(h[k], x[k], acc);
            }
        }
        values[i] = acc;
        if (mask) mask[i] = i < L_out ? 1.f : 0.f;
    }
}

}  // namespace tav
using namespace tav;

extern "C" int tav_audio_resample_tile(int32_t o, int32_t n, int32_t width) { return plan::audio_resample_tile(o, n, width); }

extern "C" int tav_audio_resample(const void* src, const float* table, const int32_t* first, float* values, float* mask,
                                  const tav_resample_args* a, void* stream) {
    plan::ResamplePlan P;
    if (const int rc = plan::audio_resample_validate(src && values && table && first && a, a, &P)) return rc;
    const float inv_c = 1.0f / (float)a->C;
    return dtypes<on<TAV_I16>, on<TAV_F32>>::dispatch(a->src_dtype, [&](auto t) {
        using T = decltype(t);
        TAV_LAUNCH(audio_resample_kernel<T>, P.launch, stream, (const T*)src, table, first, values, mask, *a, (long)P.L_out, P.tile, P.table_in_lds, inv_c);
        return 0;
    });
}
