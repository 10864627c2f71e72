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

constexpr int AR_THREADS = 256;
constexpr int AR_MAX_PER_THREAD = 4;      // a tile is 256, 512, 768 or 1024 outputs: the largest whose input span fits AR_SPAN_MAX
constexpr int AR_SPAN_MAX = 8192;         // f32 elements of LDS for the channel mean of a tile's input span (32 KiB)
constexpr int AR_TABLE_MAX = 6144;        // f32 elements of LDS for the compact table (24 KiB): 441/160 needs 160 x 35, 441/320 320 x 17

// Row pitch of the table in LDS.  The lanes of a wave make consecutive outputs, hence consecutive phases p at the same k: lane l reads
// p_l * pitch + k.  ds_read_b32 serves 32 lanes per cycle from 32 four-byte banks, so an odd pitch puts them on 32 different banks (ntap = 34
// itself would pair them up).
static inline int ar_pitch(int ntap) { return ntap | 1; }

// the most input positions `tile` consecutive outputs read: they span at most (tile + n - 2) / n + 1 values of q
static inline long ar_span(long tile, long o, long n, long width) { return ((tile + n - 2) / n + 1) * o + 2 * width; }

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

// outputs per workgroup for a rate pair, 0 when not even 256 outputs' input span fits the LDS buffer (o / n beyond about 30)
extern "C" int tav_audio_resample_tile(int32_t o, int32_t n, int32_t width) {
    if (o < 1 || n < 1 || width < 0) return 0;
    for (int m = AR_MAX_PER_THREAD; m >= 1; --m)
        if (ar_span((long)m * AR_THREADS, o, n, width) <= AR_SPAN_MAX) return m * AR_THREADS;
    return 0;
}

extern "C" int tav_audio_resample(const void* src, const float* table, const int32_t* first, float* values, float* mask,
                                  const tav_resample_args* a, void* stream) {
    if (!src || !values || !table || !first || !a) return TAV_ERR_NULL;
    if (a->src_dtype != TAV_F32 && a->src_dtype != TAV_I16) return TAV_ERR_DTYPE;
    if (a->C < 1 || a->C > 32 || a->L < 1 || a->L > (1L << 40) || a->sC < 0 || a->sL < 0) return TAV_ERR_SHAPE;
    if (a->o < 1 || a->n < 1 || a->ntap < 1 || a->width < 0 || a->o > (1 << 20) || a->n > (1 << 20) || a->width > (1 << 24)) return TAV_ERR_SHAPE;
    if ((long)a->n * a->ntap > (1L << 24)) return TAV_ERR_SHAPE;
    if (a->first_max < 0 || (long)a->first_max + a->ntap > 2L * a->width + a->o) return TAV_ERR_SHAPE;
    const long L_out = ((long)a->n * a->L + a->o - 1) / a->o;
    if (a->T_row < L_out || a->T_row > (1L << 40)) return TAV_ERR_SHAPE;
    const int tile = tav_audio_resample_tile(a->o, a->n, a->width);
    if (tile == 0) return TAV_ERR_SHAPE;
    const long blocks = (a->T_row + tile - 1) / tile;
    if (blocks > 0x7fffffffL) return TAV_ERR_SHAPE;
    const int in_lds = (long)a->n * ar_pitch(a->ntap) <= AR_TABLE_MAX;
    const float inv_c = 1.0f / (float)a->C;
    const hipStream_t st = (hipStream_t)stream;
    if (a->src_dtype == TAV_I16)
        hipLaunchKernelGGL(audio_resample_kernel<int16_t>, dim3((unsigned)blocks), dim3(AR_THREADS), 0, st, (const int16_t*)src, table, first,
                           values, mask, *a, L_out, tile, in_lds, inv_c);
    else
        hipLaunchKernelGGL(audio_resample_kernel<float>, dim3((unsigned)blocks), dim3(AR_THREADS), 0, st, (const float*)src, table, first, values,
                           mask, *a, L_out, tile, in_lds, inv_c);
    return tav_last_error();
}
