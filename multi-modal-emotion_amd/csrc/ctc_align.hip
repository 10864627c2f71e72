// CTC forced alignment (reference run_scripts/get_times.py: get_trellis, backtrack and the grouping merge_repeats means) and the row
// log-softmax in front of it.  f32 only.
//
// tav_ctc_align: one workgroup per utterance.  The recurrence is T dependent steps of N + 1 independent updates, so a frame's cost is the
// length of its dependency chain; everything that does not depend on the recurrence is taken out of it:
//   * emission rows are staged in LDS, `stage_frames` at a time and two stages deep: the rows of the next stage are loaded from global
//     memory into registers before the frames of the current one run and are written to LDS behind them, and the values a step needs
//     (the blank's and the token's log-probability) are read from LDS a group of four frames ahead of the steps that add them;
//   * a thread keeps `TPT` consecutive trellis columns in registers for all frames.  The left neighbour of its first column comes from
//     the lane below by two DPP moves (row_shr:1, row_bcast:15 for the first lane of a row of 16) and, for the first lane of a wave, from
//     one LDS slot per wave that the wave below wrote at the end of the previous frame (double-buffered: one barrier per frame, none
//     when the workgroup is a single wave);
//   * `changed > stayed` is the comparison the max itself makes; its ballot word (one per wave, column slot and frame) is all the
//     walk back needs, so the trellis is never read again.  The words stay in LDS when they fit; otherwise they go to the caller's
//     workspace and come back to LDS a window of frames at a time, so that the one lane that walks always reads at LDS latency;
//   * the walk leaves (token, changed) per frame in LDS; path_prob, seg and seg_score are then formed by all threads.
// Columns right of N_b compute on clamped tokens and are never stored: a column depends only on columns to its left.
// Every index is clamped; no atomics; scratch is 0.
#include "common.h"
#include "tavhip_internal.h"
#include "align_plan.h"
#include <type_traits>

namespace tav {
using plan::AlignPlan, plan::LSM_ROWS;

constexpr int ALIGN_AHEAD = 4;     // frames of a group: the next group's emissions are read from LDS while this group's steps run

TAV_DEV int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// value of the lane below; lane 0 of the wave gets `seam`.  Every lane of the wave must be active.
TAV_DEV float from_lane_below(float v, float seam, int lane) {
    const int vi = __float_as_int(v);
    const int sh = __builtin_amdgcn_update_dpp(__float_as_int(seam), vi, 0x111 /* row_shr:1 */, 0xf, 0xf, false);   // lanes 0, 16, 32, 48 keep `seam`
    const int bc = __builtin_amdgcn_update_dpp(sh, vi, 0x142 /* row_bcast:15 */, 0xe, 0xf, false);                 // rows 1..3: lane 15 of the row below
    return __int_as_float((lane & 15) == 0 ? bc : sh);
}

// MAXB: the most threads of a launch; PRE: registers a thread holds the next stage in (PRE * threads >= ALIGN_STAGE_ELEMS); MULTI: more
// than one wave (a seam slot and a barrier per frame)
template <int TPT, int MAXB, int PRE, bool MULTI>
__global__ __launch_bounds__(MAXB) void ctc_align_kernel(const tav_ctc_align_args a, const AlignPlan P) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* const stage = reinterpret_cast<float*>(smem + P.off_stage);
    float* const seam = reinterpret_cast<float*>(smem + P.off_seam);
    int* const misc = reinterpret_cast<int*>(smem + P.off_misc);
    uint16_t* const path = reinterpret_cast<uint16_t*>(smem + P.off_path);
    float* const prob = reinterpret_cast<float*>(smem + P.off_prob);
    int* const segs = reinterpret_cast<int*>(smem + P.off_segs);
    unsigned long long* const bits = reinterpret_cast<unsigned long long*>(smem + P.off_bits);

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nthreads = blockDim.x, nw = nthreads >> 6;
    const int Tmax = (int)a.Tmax, Nmax = (int)a.Nmax, V = (int)a.V, ld = (int)a.ld, blank = a.blank_id;
    const int T = clampi(a.n_frames[b], 0, Tmax), N = clampi(a.n_tokens[b], 0, Nmax);
    const int S = P.stage_frames, nwords = P.nwords;
    const bool in_lds = P.ws_row_bytes == 0;
    const float* const em = a.emission + (long)b * Tmax * ld;
    const int32_t* const tok = a.tokens + (long)b * Nmax;
    float* const tr = a.trellis ? a.trellis + (long)b * (Tmax + 1) * (Nmax + 1) : nullptr;
    unsigned long long* const wsb = in_lds ? nullptr : reinterpret_cast<unsigned long long*>(a.workspace) + (long)b * Tmax * nwords;

    // ---- this thread's columns and tokens
    const int col0 = tid * TPT;
    int tk[TPT];
    float v[TPT];
    int bad = 0;
#pragma unroll
    for (int k = 0; k < TPT; ++k) {
        const int col = col0 + k;
        int id = 0;
        if (col >= 1 && col <= N) {
            id = tok[col - 1];
            if (id < 0 || id >= V) { bad = 1; id = clampi(id, 0, V - 1); }
        }
        tk[k] = id;
        v[k] = col == 0 ? 0.f : -INFINITY;
        if (tr && col <= N) tr[col] = v[k];
    }
    float best = v[TPT - 1];                       // of column N, for its owner: the first maximum over t
    int best_t = 0;
    int own = -1;                                  // the slot that holds column N, if this thread owns it
#pragma unroll
    for (int k = 0; k < TPT; ++k)
        if (col0 + k == N) { own = k; best = v[k]; }
    if (MULTI && lane == 63) seam[w] = v[TPT - 1];
    const int status_bad = __syncthreads_or(bad);  // (also orders the seam slot and the first stage)

    // ---- forward
    const int nchunks = (T + S - 1) / S;
    float pre[PRE];
    // element i = tid + r nthreads of a stage is (frame i / V, label i % V): one division, then steps of nthreads
    const int step_f = nthreads / V, step_x = nthreads - step_f * V;
    auto fetch = [&](int c) {                      // rows [c S, c S + nf) -> registers
        const int nf = (T - c * S < S ? T - c * S : S), n = nf * V;
        const float* src = em + (long)c * S * ld;
        int f = tid / V, x = tid - f * V;
#pragma unroll
        for (int r = 0; r < PRE; ++r) {
            if (tid + r * nthreads < n) pre[r] = src[f * ld + x];
            f += step_f;
            x += step_x;
            if (x >= V) { x -= V; ++f; }
        }
    };
    auto park = [&](int c) {                       // registers -> stage c & 1
        const int nf = (T - c * S < S ? T - c * S : S), n = nf * V;
        float* dst = stage + (c & 1) * S * V;
#pragma unroll
        for (int r = 0; r < PRE; ++r) {
            const int i = tid + r * nthreads;
            if (i < n) dst[i] = pre[r];
        }
    };
    // the blank's and the tokens' log-probabilities of the frames [f0, f0 + ALIGN_AHEAD) of a stage (rows past its last frame are
    // clamped into it: read, never used)
    auto gather = [&](const float* st, int f0, float (&eb)[ALIGN_AHEAD], float (&et)[ALIGN_AHEAD][TPT]) {
#pragma unroll
        for (int u = 0; u < ALIGN_AHEAD; ++u) {
            const float* row = st + (f0 + u < S ? f0 + u : S - 1) * V;
            eb[u] = row[blank];
#pragma unroll
            for (int k = 0; k < TPT; ++k) et[u][k] = row[tk[k]];
        }
    };
    bool is_own[TPT];
#pragma unroll
    for (int k = 0; k < TPT; ++k) is_own[k] = k == own;
    if (nchunks > 0) { fetch(0); park(0); }
    __syncthreads();
    for (int c = 0; c < nchunks; ++c) {
        if (c + 1 < nchunks) fetch(c + 1);
        const int nf = (T - c * S < S ? T - c * S : S);
        const float* st = stage + (c & 1) * S * V;
        float eb[ALIGN_AHEAD], et[ALIGN_AHEAD][TPT], ebn[ALIGN_AHEAD], etn[ALIGN_AHEAD][TPT];
        gather(st, 0, eb, et);
        // one group of ALIGN_AHEAD frames; `full`: all of them exist (no test per frame), else the stage's last, short group;
        // `with_trellis`: the caller wants the trellis rows
        auto group = [&](const int f0, auto full, auto with_trellis) {
            constexpr bool FULL = decltype(full)::value, TR = decltype(with_trellis)::value;
            gather(st, f0 + ALIGN_AHEAD, ebn, etn);        // the next group's, under this group's steps
            unsigned long long mm[ALIGN_AHEAD][TPT];
#pragma unroll
            for (int u = 0; u < ALIGN_AHEAD; ++u) {
                if (FULL || f0 + u < nf) {         // (uniform)
                    const int t = c * S + f0 + u;
                    float below = 0.f;
                    if (MULTI) below = (w > 0) ? seam[(t & 1) * 16 + w - 1] : 0.f;
                    const float left0 = from_lane_below(v[TPT - 1], below, lane);
#pragma unroll
                    for (int k = TPT - 1; k >= 0; --k) {
                        const float left = k ? v[k - 1] : left0;
                        const float stayed = v[k] + eb[u], changed = left + et[u][k];
                        const bool ch = changed > stayed;
                        mm[u][k] = __ballot(ch);
                        float nv = ch ? changed : stayed;
                        if (col0 + k == 0) nv = 0.f;
                        v[k] = nv;
                        if (TR && col0 + k <= N) tr[(long)(t + 1) * (Nmax + 1) + col0 + k] = nv;
                        const bool up = is_own[k] && nv > best;
                        best = up ? nv : best;
                        best_t = up ? t + 1 : best_t;
                    }
                    if (MULTI) {
                        if (lane == 63) seam[((t + 1) & 1) * 16 + w] = v[TPT - 1];
                        __syncthreads();
                    }
                }
            }
            if (lane == 0) {                       // the group's decision words, one masked region
                const long at = (long)(c * S + f0) * nwords + w * TPT;
                if (in_lds) {
#pragma unroll
                    for (int u = 0; u < ALIGN_AHEAD; ++u)
                        if (FULL || f0 + u < nf) {
#pragma unroll
                            for (int k = 0; k < TPT; ++k) bits[at + u * nwords + k] = mm[u][k];
                        }
                } else {
#pragma unroll
                    for (int u = 0; u < ALIGN_AHEAD; ++u)
                        if (FULL || f0 + u < nf) {
#pragma unroll
                            for (int k = 0; k < TPT; ++k) wsb[at + u * nwords + k] = mm[u][k];
                        }
                }
            }
#pragma unroll
            for (int u = 0; u < ALIGN_AHEAD; ++u) {
                eb[u] = ebn[u];
#pragma unroll
                for (int k = 0; k < TPT; ++k) et[u][k] = etn[u][k];
            }
        };
        const int nfull = nf & ~(ALIGN_AHEAD - 1);
        if (tr) {
            for (int f0 = 0; f0 < nfull; f0 += ALIGN_AHEAD) group(f0, std::true_type(), std::true_type());
            if (nfull < nf) group(nfull, std::false_type(), std::true_type());
        } else {
            for (int f0 = 0; f0 < nfull; f0 += ALIGN_AHEAD) group(f0, std::true_type(), std::false_type());
            if (nfull < nf) group(nfull, std::false_type(), std::false_type());
        }
        if (c + 1 < nchunks) park(c + 1);
        __syncthreads();
    }
    if (own >= 0) misc[0] = best_t;
    if (tid == 0) { misc[1] = 1; misc[2] = 0; misc[4] = N; }
    __syncthreads();

    // ---- the walk back: windows of the decision words in LDS, one lane walks
    const int t_start = N == 0 ? 0 : clampi(misc[0], 0, T);
    {
        int hi = t_start;                          // frames [lo, hi) are the window; the walk is at trellis time hi
        while (hi > 0) {
            const int lo = in_lds ? 0 : (hi - P.bits_frames > 0 ? hi - P.bits_frames : 0);
            if (!in_lds) {
                const long n = (long)(hi - lo) * nwords;
                for (long i = tid; i < n; i += nthreads) bits[i] = wsb[(long)lo * nwords + i];
                __syncthreads();
            }
            if (tid == 0) {
                int j = misc[4], t = hi, failed = 1;
                for (; t > lo; --t) {
                    const int i = j / TPT, k = j - i * TPT;
                    const unsigned long long m = bits[(long)(t - 1 - lo) * nwords + (i >> 6) * TPT + k];
                    const int ch = (int)((m >> (i & 63)) & 1ull);
                    path[t - 1] = (uint16_t)((j - 1) | (ch << 15));
                    if (ch && --j == 0) { failed = 0; --t; break; }
                }
                misc[1] = failed;                  // still walking, or out of frames
                misc[2] = t;                       // on success: the first frame of the path
                misc[3] = (failed && t > 0) ? t : 0;      // where the next window ends
                misc[4] = j;
            }
            __syncthreads();
            hi = misc[3];
            __syncthreads();
        }
    }
    const int failed = misc[1], first = misc[2];
    const int status = (failed ? 1 : 0) | (status_bad ? 2 : 0);

    // ---- outputs, every row in full
    int32_t* const o_tok = a.path_token + (long)b * Tmax;
    float* const o_prob = a.path_prob + (long)b * Tmax;
    for (int t = tid; t < Tmax; t += nthreads) {
        int pt = -1;
        float pp = 0.f;
        if (!failed && t >= first && t < t_start) {
            const unsigned p = path[t];
            const int jm = clampi((int)(p & 0x7fffu), 0, N - 1), ch = (int)(p >> 15);
            const int id = ch ? clampi(tok[jm], 0, V - 1) : blank;
            pp = expf(em[(long)t * ld + id]);
            pt = jm;
            prob[t] = pp;
            if (ch) segs[jm] = t;
        }
        o_tok[t] = pt;
        o_prob[t] = pp;
    }
    if (tid == 0) {
        segs[N] = t_start;
        int32_t* sp = a.span + (long)b * 4;
        sp[0] = failed ? -1 : first;
        sp[1] = failed ? -1 : t_start;
        sp[2] = failed ? 0 : t_start - first;
        sp[3] = status;
    }
    __syncthreads();
    int32_t* const o_seg = a.seg + (long)b * Nmax * 2;
    float* const o_score = a.seg_score + (long)b * Nmax;
    for (int j = tid; j < Nmax; j += nthreads) {
        int s = -1, e = -1;
        float score = 0.f;
        if (!failed && j < N) {
            s = clampi(segs[j], 0, T);
            e = clampi(segs[j + 1], s, T);
            double acc = 0.0;
            for (int t = s; t < e; ++t) acc += (double)prob[t];
            score = (float)(acc / (double)(e - s));
        }
        o_seg[2 * j] = s;
        o_seg[2 * j + 1] = e;
        o_score[j] = score;
    }
}

// one wave per row; lane l takes columns l, l + 64, ... in ascending order, the waves' partials meet in a fixed butterfly
__global__ __launch_bounds__(64 * LSM_ROWS) void ctc_log_softmax_kernel(const float* __restrict__ x, float* __restrict__ y, const long R, const int V,
                                                                         const long ld_in, const long ld_out) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * LSM_ROWS + (threadIdx.x >> 6);
    if (row >= R) return;                          // (whole waves)
    const float* xr = x + row * ld_in;
    float* yr = y + row * ld_out;
    float m = -INFINITY;
    for (int c = lane; c < V; c += 64) m = fmaxf(m, xr[c]);
    m = wave_max(m);
    float s = 0.f;
    for (int c = lane; c < V; c += 64) s += expf(xr[c] - m);
    s = wave_sum(s);
    const float ls = logf(s);
    for (int c = lane; c < V; c += 64) yr[c] = (xr[c] - m) - ls;
}

}  // namespace tav
using namespace tav;

extern "C" int tav_align_version(void) { return plan::ALIGN_ABI_VERSION; }

extern "C" int tav_ctc_log_softmax(const float* logits, float* out, int64_t R, int64_t V, int64_t ld_in, int64_t ld_out, void* stream) {
    if (const int rc = plan::log_softmax_validate(logits && out, R, V, ld_in, ld_out)) return rc;
    const plan::Launch L{plan::log_softmax_blocks(R), 1, 1, 64 * LSM_ROWS, 0};
    TAV_LAUNCH(ctc_log_softmax_kernel, L, stream, logits, out, (long)R, (int)V, (long)ld_in, (long)ld_out);
    return 0;
}

extern "C" int tav_ctc_align_plan(int64_t T, int64_t N, int64_t V, tav_align_plan* out) {
    if (!out) return TAV_ERR_NULL;
    if (const int rc = plan::align_shape_validate(T, N, V)) return rc;
    plan::align_plan_public(plan::align_plan(T, N, V), out);
    return 0;
}

extern "C" int64_t tav_ctc_align_ws_bytes(int64_t B, int64_t T, int64_t N, int64_t V) { return plan::align_ws_bytes(B, T, N, V); }

extern "C" int tav_ctc_align(const tav_ctc_align_args* a, void* stream) {
    AlignPlan P;
    if (const int rc = plan::align_validate(a, &P)) return rc;
    const plan::Launch L{a->B, 1, 1, P.block, (size_t)P.lds_bytes};
    constexpr int SMALL = plan::ALIGN_SMALL_BLOCK, BIG = plan::ALIGN_MAX_BLOCK;
    static_assert(64 * plan::ALIGN_PREFETCH >= plan::ALIGN_STAGE_ELEMS && (SMALL + 64) * plan::ALIGN_PREFETCH_BIG >= plan::ALIGN_STAGE_ELEMS, "a stage fits the registers");
    if (P.block == 64) TAV_LAUNCH((ctc_align_kernel<1, 64, plan::ALIGN_PREFETCH, false>), L, stream, *a, P);
    else if (P.block <= SMALL) TAV_LAUNCH((ctc_align_kernel<1, SMALL, plan::ALIGN_PREFETCH, true>), L, stream, *a, P);
    else if (P.tpt == 1) TAV_LAUNCH((ctc_align_kernel<1, BIG, plan::ALIGN_PREFETCH_BIG, true>), L, stream, *a, P);
    else if (P.tpt == 2) TAV_LAUNCH((ctc_align_kernel<2, BIG, plan::ALIGN_PREFETCH_BIG, true>), L, stream, *a, P);
    else TAV_LAUNCH((ctc_align_kernel<3, BIG, plan::ALIGN_PREFETCH_BIG, true>), L, stream, *a, P);
    return 0;
}
