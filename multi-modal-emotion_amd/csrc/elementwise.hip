// HBM-bound support kernels of the TAV path: weight casts (+ transposed copies for dgrad), casts/adds, modality and
// text embeddings, video patch gather, pooling, classifier head, cross-entropy, dropout, grad-norm and AdamW.
// Every kernel is coalesced along the feature axis and vectorised 4-wide where the shape allows.
#include "common.h"
#include "tavhip_internal.h"

namespace tav {
// defined with the host decisions (entry_plan.h)
using plan::SCAT_T, plan::SUMSQ_BLOCKS, plan::OPT_CHUNK, plan::OPT_MAX_GROUPS;

// ------------------------------------------------------------------------------------------------ weight casts
template <typename TD>
__global__ void cast_weight_kernel(const float* __restrict__ src, TD* __restrict__ dst, long ld_n, TD* __restrict__ dst_t, long ld_t, int R, int C) {
    __shared__ float tile[32][33];
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
    for (int k = ty; k < 32; k += 8) {
        const int r = r0 + k, c = c0 + tx;
        float v = 0.f;
        if (r < R && c < C) { v = src[(long)r * C + c]; if (dst) ET<TD>::st(dst + (long)r * ld_n + c, v); }
        tile[k][tx] = v;
    }
    __syncthreads();
    if (dst_t) {
        for (int k = ty; k < 32; k += 8) {
            const int c = c0 + k, r = r0 + tx;
            if (r < R && c < C) ET<TD>::st(dst_t + (long)c * ld_t + r, tile[tx][k]);
        }
    }
}

// Multi-tensor form: blockIdx.y selects a descriptor (one launch refreshes every operand copy of a transformer layer).
struct CastDesc { const float* src; void* dst; void* dst_t; long ld_n, ld_t; int R, C, dtype; float scale_n; };   // scale_n: factor on the values written to dst (not dst_t)
// bf16 matrices with R, C multiples of 64 and both copies wanted (every GEMM weight): 64x64 tiles, 16-B loads, 8-B stores (128-B row
// segments) -- the 32x32 / 2-B-store form below ran at 2.1 TB/s
__device__ void cast_weight_tile64(const CastDesc& d, float (*tile)[65], int t, int tiles_c) {
    const int c0 = (t % tiles_c) * 64, r0 = (t / tiles_c) * 64;
    const int q = threadIdx.x & 15, h = threadIdx.x >> 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = h + 16 * i;
        const f32x4 v = ld4(d.src + (long)(r0 + row) * d.C + c0 + 4 * q);
        st4((bf16*)d.dst + (long)(r0 + row) * d.ld_n + c0 + 4 * q, v * d.scale_n);
        tile[row][4 * q] = v[0]; tile[row][4 * q + 1] = v[1]; tile[row][4 * q + 2] = v[2]; tile[row][4 * q + 3] = v[3];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = h + 16 * i;
        const f32x4 v = {tile[4 * q][c], tile[4 * q + 1][c], tile[4 * q + 2][c], tile[4 * q + 3][c]};
        st4((bf16*)d.dst_t + (long)(c0 + c) * d.ld_t + r0 + 4 * q, v);
    }
    __syncthreads();
}
__global__ void cast_weight_multi_kernel(const CastDesc* __restrict__ descs) {
    __shared__ float tile[64][65];
    const CastDesc d = descs[blockIdx.y];
    if (d.dtype == TAV_BF16 && d.dst && d.dst_t && (d.R & 63) == 0 && (d.C & 63) == 0 && (d.ld_n & 3) == 0 && (d.ld_t & 3) == 0) {
        const int tc = d.C >> 6, nt = tc * (d.R >> 6);
        for (int t = blockIdx.x; t < nt; t += gridDim.x) cast_weight_tile64(d, tile, t, tc);      // block-uniform loop
        return;
    }
    const int tiles_c = (d.C + 31) >> 5, tiles_r = (d.R + 31) >> 5;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int t = blockIdx.x; t < tiles_c * tiles_r; t += gridDim.x) {      // block-uniform loop
        const int c0 = (t % tiles_c) * 32, r0 = (t / tiles_c) * 32;
        for (int k = ty; k < 32; k += 8) {
            const int r = r0 + k, c = c0 + tx;
            float v = 0.f;
            if (r < d.R && c < d.C) {
                v = d.src[(long)r * d.C + c];
                if (d.dst) { if (d.dtype == TAV_BF16) ET<bf16>::st((bf16*)d.dst + (long)r * d.ld_n + c, v * d.scale_n); else ((float*)d.dst)[(long)r * d.ld_n + c] = v * d.scale_n; }
            }
            tile[k][tx] = v;
        }
        __syncthreads();
        if (d.dst_t) {
            for (int k = ty; k < 32; k += 8) {
                const int c = c0 + k, r = r0 + tx;
                if (r < d.R && c < d.C) {
                    if (d.dtype == TAV_BF16) ET<bf16>::st((bf16*)d.dst_t + (long)c * d.ld_t + r, tile[tx][k]); else ((float*)d.dst_t)[(long)c * d.ld_t + r] = tile[tx][k];
                }
            }
        }
        __syncthreads();
    }
}

// nn.Conv1d weight [co][ci][k] -> dst[co][k*CI + ci] (forward/wgrad operand) and dst_t[k*CI + ci][co] (dgrad operand)
// ... and (v5) dst_ph: the input-gradient operands BY OUTPUT PHASE.  dx[s*m + r] = sum over the taps j = r + q*s of dy[m - q] . W[:, :, j]: for every
// residue r of the input position, one NT GEMM whose A row is the Q_r = ceil((K - r) / s) CONSECUTIVE dy rows m - (Q_r - 1) .. m (overlapping
// rows, lda = CO) and whose B operand is  ph_r[ci][q' * CO + co] = W[co][ci][r + (Q_r - 1 - q') * s]  -- the blocks ph_0 | ph_1 | ... stand
// one after the other (CI * Q_r * CO elements each, CO * CI * K in all).  No [T_out, K * CI] column buffer and no col2im pass.
template <typename TD>
__global__ void cast_conv_weight_kernel(const float* __restrict__ src, TD* __restrict__ dst, TD* __restrict__ dst_t, TD* __restrict__ dst_ph, int CO, int CI,
                                        int K, int stride) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long n = (long)CO * CI * K;
    if (idx >= n) return;
    const int co = (int)(idx / ((long)CI * K));
    const int rem = (int)(idx - (long)co * CI * K);
    const int kk = rem / CI, ci = rem - kk * CI;          // idx enumerates dst order [co][kk][ci]
    const float v = src[((long)co * CI + ci) * K + kk];
    if (dst) ET<TD>::st(dst + idx, v);
    if (dst_t) ET<TD>::st(dst_t + ((long)kk * CI + ci) * CO + co, v);
    if (dst_ph) {
        const int r = kk % stride, q = kk / stride;
        long off = 0;                                       // elements of the phases before r
        for (int rp = 0; rp < r; ++rp) off += (long)CI * CO * ((K - rp + stride - 1) / stride);
        const int Q = (K - r + stride - 1) / stride;
        ET<TD>::st(dst_ph + off + ((long)ci * Q + (Q - 1 - q)) * CO + co, v);
    }
}

// dst[z][c][r] = src[z][r][c]  (batched 2-D transpose through a padded LDS tile; both sides coalesced)
template <typename T>
__global__ void transpose2d_kernel(const T* __restrict__ src, T* __restrict__ dst, int R, int C) {
    __shared__ float tile[32][33];
    const long zoff = (long)blockIdx.z * R * C;
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int k = ty; k < 32; k += 8) {
        const int r = r0 + k, c = c0 + tx;
        tile[k][tx] = (r < R && c < C) ? ET<T>::ld(src + zoff + (long)r * C + c) : 0.f;
    }
    __syncthreads();
    for (int k = ty; k < 32; k += 8) {
        const int c = c0 + k, r = r0 + tx;
        if (r < R && c < C) ET<T>::st(dst + zoff + (long)c * R + r, tile[tx][k]);
    }
}

template <typename TS, typename TD>
__global__ void cast2d_kernel(const TS* __restrict__ src, long ld_src, TD* __restrict__ dst, long ld_dst, long R, int C4) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= R * C4) return;
    const long r = idx / C4; const int c = (int)(idx - r * C4) * 4;
    st4(dst + r * ld_dst + c, ld4(src + r * ld_src + c));
}

template <typename TL>
__global__ void add_f32_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ y, TL* __restrict__ y_lp, long n4) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const f32x4 v = ld4(a + 4 * i) + ld4(b + 4 * i);
    if (y) st4(y + 4 * i, v);
    if (y_lp) st4(y_lp + 4 * i, v);
}

__global__ void fill_f32_kernel(float* p, float v, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) p[i] = v;
}

// ------------------------------------------------------------------------------------------------ modality embedding add
__global__ void embed_add_fwd_kernel(const float* __restrict__ x, const int64_t* __restrict__ ids, const float* __restrict__ table,
                                     float* __restrict__ out, long rows, int W4) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= rows * W4) return;
    const long r = idx / W4; const int c = (int)(idx - r * W4) * 4;
    const long W = (long)W4 * 4;
    st4(out + r * W + c, ld4(x + r * W + c) + ld4(table + ids[r] * W + c));
}
// partial[block][t][c] = sum over this block's rows with ids == t
__global__ void embed_add_bwd_partial_kernel(const float* __restrict__ dy, const int64_t* __restrict__ ids, float* __restrict__ partial, long rows,
                                             int W, int ntable, int rows_per_block) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= W) return;
    const long r0 = (long)blockIdx.y * rows_per_block;
    long r1 = r0 + rows_per_block; r1 = r1 < rows ? r1 : rows;
    float acc[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) acc[t] = 0.f;
    for (long r = r0; r < r1; ++r) {
        const int t = (int)ids[r];
        const float v = dy[r * W + c];
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] += (k == t) ? v : 0.f;
    }
    for (int t = 0; t < ntable; ++t) partial[((long)blockIdx.y * ntable + t) * W + c] = acc[t];
}
__global__ void embed_add_bwd_final_kernel(const float* __restrict__ partial, float* dtable, int nparts, int ntable, int W, int accumulate) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= ntable * W) return;
    float s = 0.f;
    for (int k = 0; k < nparts; ++k) s += partial[(long)k * ntable * W + idx];
    dtable[idx] = accumulate ? dtable[idx] + s : s;
}

// ------------------------------------------------------------------------------------------------ text embeddings
__global__ void text_pos_ids_kernel(const int64_t* __restrict__ ids, int64_t* __restrict__ pos_ids, int S, int pad_id) {
    __shared__ int scan[1024];
    const int b = blockIdx.x, s = threadIdx.x;
    const bool in = s < S;
    const int id = in ? (int)ids[(long)b * S + s] : pad_id;
    const int nonpad = (pad_id >= 0) ? (id != pad_id ? 1 : 0) : 1;
    scan[s] = in ? nonpad : 0;
    __syncthreads();
    for (int off = 1; off < (int)blockDim.x; off <<= 1) {
        const int v = (s >= off) ? scan[s - off] : 0;
        __syncthreads();
        scan[s] += v;
        __syncthreads();
    }
    if (in) pos_ids[(long)b * S + s] = (pad_id >= 0) ? (long)(scan[s] * nonpad + pad_id) : (long)s;
}
__global__ void text_embed_sum_kernel(const int64_t* __restrict__ ids, const int64_t* __restrict__ pos_ids, const float* __restrict__ word,
                                      const float* __restrict__ pos, const float* __restrict__ type, float* __restrict__ pre, long rows, int W4) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= rows * W4) return;
    const long r = idx / W4; const int c = (int)(idx - r * W4) * 4;
    const long W = (long)W4 * 4;
    st4(pre + r * W + c, ld4(word + ids[r] * W + c) + ld4(pos + pos_ids[r] * W + c) + ld4(type + c));
}
// dtable[idx[r]][:] += d[r][:] without atomics (bitwise reproducible): one workgroup per token row r.  Every workgroup lists, in
// ascending order, the rows that carry the same index (rows <= a few thousand: rows/1024 compares per thread); only the workgroup
// of the FIRST such row goes on and adds their sum to the table row.  Wave w sums matches w, w+16, ... (fixed order), the 16
// partial rows meet in LDS in wave order.  A padding token shared by a quarter of the batch costs rows/64 serial row reads.
__global__ __launch_bounds__(SCAT_T) void scatter_add_rows_kernel(const float* __restrict__ d, const int64_t* __restrict__ idx, float* __restrict__ dtable,
                                                                  int rows, int W, long ntable) {
    extern __shared__ __attribute__((aligned(16))) char scat_smem[];
    // all LDS in the dynamic region (a static __shared__ object in front would move its base off 16-B alignment)
    int* wcount = reinterpret_cast<int*>(scat_smem);                   // [16]
    int* wbase = wcount + 16;                                          // [16]
    int& total = wcount[32];
    int& dup_before = wcount[33];
    int* match = reinterpret_cast<int*>(scat_smem + 256);              // [rows] worst case
    const int r = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t id = idx[r];
    if (t == 0) dup_before = 0;
    __syncthreads();
    const int per = (rows + SCAT_T - 1) / SCAT_T, i0 = t * per;
    int i1 = i0 + per; i1 = i1 < rows ? i1 : rows;
    int cnt = 0;
    for (int i = i0; i < i1; ++i) if (idx[i] == id) { ++cnt; if (i < r) dup_before = 1; }      // benign race: every writer stores 1
    __syncthreads();
    if (dup_before || id < 0 || id >= ntable) return;                  // not the first row with this index (or an index outside the table)
    // ordered compaction of the matching rows: exclusive scan of cnt over the threads (wave scan + 16 wave totals)
    int incl = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int v = __shfl_up(incl, o, 64); if (lane >= o) incl += v; }
    if (lane == 63) wcount[wave] = incl;
    __syncthreads();
    if (t == 0) { int a = 0; for (int w = 0; w < 16; ++w) { wbase[w] = a; a += wcount[w]; } total = a; }
    __syncthreads();
    int pos = wbase[wave] + incl - cnt;
    for (int i = i0; i < i1; ++i) if (idx[i] == id) match[pos++] = i;
    __syncthreads();
    const int n = total;
    float* part = reinterpret_cast<float*>(scat_smem + 256 + (((size_t)rows * 4 + 15) & ~(size_t)15));   // [16][W]
    // lane owns float4 columns lane, lane+64, ... (W <= 1024: at most 4)
    f32x4 acc[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int W4 = W / 4;
    for (int m = wave; m < n; m += 16) {
        const float* src = d + (long)match[m] * W;
#pragma unroll
        for (int k = 0; k < 4; ++k) { const int c = lane + 64 * k; if (c < W4) acc[k] += ld4(src + 4 * c); }
    }
    const int nw = n < 16 ? n : 16;                                      // waves that hold a partial sum
    if (nw > 1) {
        if (wave < nw) {
#pragma unroll
            for (int k = 0; k < 4; ++k) { const int c = lane + 64 * k; if (c < W4) st4(part + (long)wave * W + 4 * c, acc[k]); }
        }
        __syncthreads();
    }
    if (wave == 0) {
        float* dst = dtable + id * W;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = lane + 64 * k;
            if (c < W4) {
                f32x4 v = acc[k];
                for (int w = 1; w < nw; ++w) v += ld4(part + (long)w * W + 4 * c);
                st4(dst + 4 * c, ld4(dst + 4 * c) + v);
            }
        }
    }
}
// indices are clamped into the table: a caller's bad index must read a wrong row, never fault the device
__global__ void gather_rows_kernel(const float* __restrict__ table, const int32_t* __restrict__ idx, float* __restrict__ out, long rows, int W4, int ntable) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * W4) return;
    const long r = i / W4; const int c = (int)(i - r * W4) * 4;
    const long W = (long)W4 * 4;
    int t = idx[r]; t = t < 0 ? 0 : (t >= ntable ? ntable - 1 : t);
    st4(out + r * W + c, ld4(table + (long)t * W + c));
}

// ------------------------------------------------------------------------------------------------ video patches
// one workgroup per kept token; patch element order = Conv3d weight order (c, dt, dh, dw)
template <typename TD>
__global__ __launch_bounds__(256) void patchify_kernel(const float* __restrict__ video, const int32_t* __restrict__ keep_idx, TD* __restrict__ out,
                                                       int F, int Hh, int Ww, int nkeep) {
    const int j = blockIdx.x, b = blockIdx.y;
    const int gw = Ww / 16, gh = Hh / 16, ntok = (F / 2) * gh * gw;
    int tok = keep_idx[(long)b * nkeep + j];
    tok = tok < 0 ? 0 : (tok >= ntok ? ntok - 1 : tok);       // never index outside the clip (a short row of the mask repeats its last token)
    const int tt = tok / (gh * gw), rem = tok - tt * gh * gw, hh = rem / gw, ww = rem - hh * gw;
    TD* orow = out + ((long)b * nkeep + j) * 1536;
    for (int v = threadIdx.x; v < 384; v += 256) {           // 384 float4 = 3*2*16 rows of 16 pixels
        const int dw4 = v & 3, rowi = v >> 2;                // rowi = (c*2 + dt)*16 + dh
        const int dh = rowi & 15, cd = rowi >> 4, dt = cd & 1, c = cd >> 1;
        const float* srcp = video + ((((long)b * F + (2 * tt + dt)) * 3 + c) * Hh + (16 * hh + dh)) * Ww + 16 * ww + 4 * dw4;
        st4(orow + rowi * 16 + 4 * dw4, ld4(srcp));
    }
}
__global__ __launch_bounds__(256) void mask_to_index_kernel(const uint8_t* __restrict__ mask, int keep_value, int32_t* __restrict__ keep_idx,
                                                            int32_t* __restrict__ counts, int n, int nkeep) {
    __shared__ int scan[256];
    const int b = blockIdx.x, t = threadIdx.x;
    const int per = (n + 255) / 256, i0 = t * per;
    int i1 = i0 + per; i1 = i1 < n ? i1 : n;
    int cnt = 0;
    for (int i = i0; i < i1; ++i) cnt += ((mask[(long)b * n + i] != 0) == (keep_value != 0)) ? 1 : 0;
    scan[t] = cnt;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const int v = (t >= off) ? scan[t - off] : 0;
        __syncthreads();
        scan[t] += v;
        __syncthreads();
    }
    int pos = scan[t] - cnt;
    for (int i = i0; i < i1; ++i)
        if (((mask[(long)b * n + i] != 0) == (keep_value != 0))) { if (pos < nkeep) keep_idx[(long)b * nkeep + pos] = i; ++pos; }
    if (t == 255 && counts) counts[b] = scan[255];
    // a row with fewer than nkeep kept tokens: the unwritten slots repeat the row's last kept index (0 if it has none), so every
    // consumer reads valid memory; the caller decides from counts[] whether that is an error
    const int found = scan[255];
    if (found < nkeep) {
        __shared__ int last_kept;
        if (t == 0) last_kept = 0;
        __syncthreads();
        if (cnt > 0 && scan[t] == found) {                       // the thread that owns the last kept element
            int last = 0;
            for (int i = i0; i < i1; ++i) if (((mask[(long)b * n + i] != 0) == (keep_value != 0))) last = i;
            last_kept = last;
        }
        __syncthreads();
        for (int k = found + t; k < nkeep; k += 256) keep_idx[(long)b * nkeep + k] = last_kept;
    }
}
// ragged rows at a fixed capacity: one workgroup per row of the video mask counts its True tokens and writes the row's lengths, clamped to
// the capacities the shapes were built for, so whatever mask sits in the buffer the length-aware kernels stay inside their rows.  A row that
// does not fit ORs its bit into *status (an ordinary device atomic, at most once per row); the caller zeroes the word and reads it at its sync.
__global__ __launch_bounds__(256) void ragged_lens_kernel(const uint8_t* __restrict__ mask, int32_t* __restrict__ true_cnt, int32_t* __restrict__ vid_lens,
                                                          int32_t* __restrict__ av_lens, int32_t* __restrict__ status, int ntok, int cap_true, int cap_keep,
                                                          int base) {
    __shared__ int red[256];
    const int b = blockIdx.x, t = threadIdx.x;
    int cnt = 0;
    for (int i = t; i < ntok; i += 256) cnt += mask[(long)b * ntok + i] != 0 ? 1 : 0;
    red[t] = cnt;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (t < off) red[t] += red[t + off];
        __syncthreads();
    }
    if (t == 0) {
        const int n = red[0], kept = ntok - n;
        true_cnt[b] = n;
        vid_lens[b] = kept < cap_keep ? kept : cap_keep;
        av_lens[b] = base + (n < cap_true ? n : cap_true);
        const int bits = (n > cap_true ? TAV_RAGGED_OVER_TRUE : 0) | ((kept > cap_keep || n == 0) ? TAV_RAGGED_OVER_KEEP : 0);
        if (bits) atomicOr(status, bits);
    }
}

// ------------------------------------------------------------------------------------------------ pooling / head / loss
// block = 16 float4 columns x 16 row groups: every thread sums rows rg, rg+16, ... of its 4 columns (16-B loads, S/16 iterations)
__global__ __launch_bounds__(256) void mean_pool_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int S, int W) {
    __shared__ f32x4 red[16][16];
    const int b = blockIdx.y, cq = threadIdx.x & 15, rg = threadIdx.x >> 4;
    const int c = (blockIdx.x * 16 + cq) * 4;
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
    if (c < W) for (int s = rg; s < S; s += 16) a += ld4(x + ((long)b * S + s) * W + c);
    red[rg][cq] = a;
    __syncthreads();
    if (rg == 0 && c < W) {
#pragma unroll
        for (int k = 1; k < 16; ++k) a += red[k][cq];
        st4(y + (long)b * W + c, a * (1.f / (float)S));
    }
}
template <typename TL>
__global__ void mean_pool_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, TL* __restrict__ dx_lp, long n4, int S, int W4) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const long row = i / W4; const int c = (int)(i - row * W4) * 4;
    const long b = row / S;
    const f32x4 v = ld4(dy + b * W4 * 4 + c) * (1.f / (float)S);
    if (dx) st4(dx + 4 * i, v);
    if (dx_lp) st4(dx_lp + 4 * i, v);
}
// length-aware forms: batch entry b averages its first L_b = clamp(lens[b], 0, S) rows of an S-row slice, in the order of
// mean_pool_fwd_kernel on S = L_b (bitwise equal to it); L_b = 0 gives y = 0.  Backward: dy[b]/L_b on those rows, 0 on the rest.
__device__ inline int pool_len(const int* lens, int b, int S) { const int L = lens[b]; return L < 0 ? 0 : (L > S ? S : L); }
__global__ __launch_bounds__(256) void mean_pool_fwd_len_kernel(const float* __restrict__ x, float* __restrict__ y, const int* __restrict__ lens, int S, int W) {
    __shared__ f32x4 red[16][16];
    const int b = blockIdx.y, cq = threadIdx.x & 15, rg = threadIdx.x >> 4;
    const int c = (blockIdx.x * 16 + cq) * 4, L = pool_len(lens, b, S);
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
    if (c < W) for (int s = rg; s < L; s += 16) a += ld4(x + ((long)b * S + s) * W + c);
    red[rg][cq] = a;
    __syncthreads();
    if (rg == 0 && c < W) {
#pragma unroll
        for (int k = 1; k < 16; ++k) a += red[k][cq];
        st4(y + (long)b * W + c, L > 0 ? a * (1.f / (float)L) : f32x4{0.f, 0.f, 0.f, 0.f});
    }
}
template <typename TL>
__global__ void mean_pool_bwd_len_kernel(const float* __restrict__ dy, float* __restrict__ dx, TL* __restrict__ dx_lp, const int* __restrict__ lens, long n4,
                                         int S, int W4) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const long row = i / W4; const int c = (int)(i - row * W4) * 4;
    const long b = row / S;
    const int s = (int)(row - b * S), L = pool_len(lens, (int)b, S);
    const f32x4 v = s < L ? ld4(dy + b * W4 * 4 + c) * (1.f / (float)L) : f32x4{0.f, 0.f, 0.f, 0.f};
    if (dx) st4(dx + 4 * i, v);
    if (dx_lp) st4(dx_lp + 4 * i, v);
}

__global__ void head_fwd_kernel(const float* __restrict__ x, const float* __restrict__ Wt, const float* __restrict__ bias, float* __restrict__ y,
                                int Bn, int K, int N) {
    const int lane = threadIdx.x & 63, o = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (o >= Bn * N) return;
    const int b = o / N, n = o - b * N;
    float a = 0.f;
    for (int k = lane; k < K; k += 64) a += x[(long)b * K + k] * Wt[(long)n * K + k];
    a = wave_sum(a);
    if (lane == 0) y[o] = a + (bias ? bias[n] : 0.f);
}
__global__ void head_bwd_kernel(const float* __restrict__ x, const float* __restrict__ Wt, const float* __restrict__ dy, float* __restrict__ dx,
                                float* __restrict__ dW, float* __restrict__ db, int Bn, int K, int N, int accumulate) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < K) {
        if (dx)
            for (int b = 0; b < Bn; ++b) {
                float a = 0.f;
                for (int n = 0; n < N; ++n) a += dy[b * N + n] * Wt[(long)n * K + k];
                dx[(long)b * K + k] = a;
            }
        for (int n = 0; n < N; ++n) {
            float a = 0.f;
            for (int b = 0; b < Bn; ++b) a += dy[b * N + n] * x[(long)b * K + k];
            dW[(long)n * K + k] = accumulate ? dW[(long)n * K + k] + a : a;
        }
    }
    if (db && blockIdx.x == 0 && threadIdx.x < N) {
        float a = 0.f;
        for (int b = 0; b < Bn; ++b) a += dy[b * N + threadIdx.x];
        db[threadIdx.x] = accumulate ? db[threadIdx.x] + a : a;
    }
}
__global__ void tanh_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = tanhf(x[i]);
}
__global__ void tanh_bwd_kernel(const float* __restrict__ y, const float* __restrict__ dy, float* __restrict__ dx, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dx[i] = dy[i] * (1.f - y[i] * y[i]);
}

// single workgroup: B samples, C classes (C <= 32)
__global__ __launch_bounds__(256) void cross_entropy_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                                            const float* __restrict__ cw, float* __restrict__ loss, float* __restrict__ dlogits,
                                                            int Bn, int C, float grad_scale) {
    __shared__ float s_num[256], s_den[256];
    float num = 0.f, den = 0.f;
    for (int i = threadIdx.x; i < Bn; i += 256) {
        const float* z = logits + (long)i * C;
        float m = z[0];
        for (int c = 1; c < C; ++c) m = fmaxf(m, z[c]);
        float se = 0.f;
        for (int c = 0; c < C; ++c) se += expf(z[c] - m);
        const int t = (int)target[i];
        const float w = cw ? cw[t] : 1.f;
        num += w * (m + logf(se) - z[t]);
        den += w;
    }
    s_num[threadIdx.x] = num; s_den[threadIdx.x] = den;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) { s_num[threadIdx.x] += s_num[threadIdx.x + off]; s_den[threadIdx.x] += s_den[threadIdx.x + off]; }
        __syncthreads();
    }
    const float wsum = s_den[0];
    if (threadIdx.x == 0 && loss) loss[0] = s_num[0] / wsum;
    if (dlogits)
        for (int i = threadIdx.x; i < Bn; i += 256) {
            const float* z = logits + (long)i * C;
            float m = z[0];
            for (int c = 1; c < C; ++c) m = fmaxf(m, z[c]);
            float se = 0.f;
            for (int c = 0; c < C; ++c) se += expf(z[c] - m);
            const int t = (int)target[i];
            const float w = (cw ? cw[t] : 1.f) * grad_scale / wsum;
            for (int c = 0; c < C; ++c) dlogits[(long)i * C + c] = w * (expf(z[c] - m) / se - (c == t ? 1.f : 0.f));
        }
}

// single workgroup, one lane per row (C <= 64): confusion-matrix bins in an LDS histogram (ds_add_u32), then plain 64-bit adds into cm --
// launches on one stream are ordered and there is one workgroup, so nothing here needs a global atomic.  Lane 0 updates the loop accumulator.
__global__ __launch_bounds__(256) void step_stats_kernel(const float* __restrict__ logits, const int64_t* __restrict__ preds,
                                                         const int64_t* __restrict__ target, int64_t* __restrict__ cm,
                                                         const float* __restrict__ loss, const int32_t* __restrict__ status,
                                                         tav_loop_acc* __restrict__ acc, int Bn, int C) {
    __shared__ unsigned s_bins[64 * 64];
    __shared__ unsigned s_bad;
    const int nbins = C * C;
    if (cm)
        for (int i = threadIdx.x; i < nbins; i += 256) s_bins[i] = 0u;
    if (threadIdx.x == 0) s_bad = 0u;
    __syncthreads();
    for (long r = threadIdx.x; r < Bn; r += 256) {
        const long t = (long)target[r];
        long p;
        if (logits) {
            // torch.argmax: first index of the maximum, NaN greater than everything (once the best is a NaN nothing replaces it)
            const float* z = logits + r * C;
            float best = z[0];
            int bi = 0;
            for (int c = 1; c < C; ++c) {
                const float v = z[c];
                if (best == best && (v != v || v > best)) { best = v; bi = c; }
            }
            p = bi;
        } else {
            p = (long)preds[r];
        }
        if (t < 0 || t >= C || p < 0 || p >= C) atomicAdd(&s_bad, 1u);
        else if (cm) atomicAdd(&s_bins[(int)t * C + (int)p], 1u);
    }
    __syncthreads();
    if (cm)
        for (int i = threadIdx.x; i < nbins; i += 256) {
            const unsigned n = s_bins[i];
            if (n) cm[i] += (int64_t)n;
        }
    if (acc && threadIdx.x == 0) {
        const int64_t step = acc->steps;
        if (loss) {
            const float l = loss[0];
            acc->loss_sum += (double)l;
            if ((__float_as_uint(l) & 0x7f800000u) == 0x7f800000u) acc->nonfinite += 1;
        }
        acc->steps = step + 1;
        acc->rows += (int64_t)Bn;
        acc->bad_rows += (int64_t)s_bad;
        if (status) {
            const int32_t w = status[0];
            if (w) {
                if (acc->first_bad_step < 0) acc->first_bad_step = (int32_t)(step < INT32_MAX ? step : INT32_MAX);
                acc->status |= w;
            }
        }
    }
}

TAV_DEV void dropout_one(const float* __restrict__ x, float* __restrict__ y, uint8_t* __restrict__ mask, long i, float p, uint64_t seed, uint64_t offset) {
    const uint64_t r = mix64(seed ^ mix64(offset + (uint64_t)i));
    const float u = (float)(r >> 40) * (1.f / 16777216.f);
    const bool keep = u >= p;
    mask[i] = keep ? 1 : 0;
    y[i] = keep ? x[i] / (1.f - p) : 0.f;
}
__global__ void dropout_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, uint8_t* __restrict__ mask, long n, float p, uint64_t seed,
                                   uint64_t offset) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    dropout_one(x, y, mask, i, p, seed, offset);
}
// ABI v7: the same draw with the seed read from device memory when the kernel runs, so that a captured launch takes the seed the host
// wrote into that word before the replay instead of the one baked into the graph at capture time.
__global__ void dropout_fwd_dev_kernel(const float* __restrict__ x, float* __restrict__ y, uint8_t* __restrict__ mask, long n, float p,
                                       const uint64_t* __restrict__ seed_state, uint64_t offset) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    dropout_one(x, y, mask, i, p, seed_state[0], offset);
}
__global__ void dropout_bwd_kernel(const float* __restrict__ dy, const uint8_t* __restrict__ mask, float* __restrict__ dx, long n, float p) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dx[i] = mask[i] ? dy[i] / (1.f - p) : 0.f;
}

// ------------------------------------------------------------------------------------------------ optimiser
__global__ __launch_bounds__(256) void sumsq_multi_kernel(const float* const* __restrict__ ptrs, const int64_t* __restrict__ sizes, float* __restrict__ partials) {
    __shared__ float red[256];
    const int t = blockIdx.y;
    const float* p = ptrs[t];
    const long n = sizes[t];
    float a = 0.f;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)SUMSQ_BLOCKS * 256) { const float v = p[i]; a += v * v; }
    red[threadIdx.x] = a;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) { if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off]; __syncthreads(); }
    if (threadIdx.x == 0) partials[(long)t * SUMSQ_BLOCKS + blockIdx.x] = red[0];
}
__global__ __launch_bounds__(256) void sum_final_kernel(const float* __restrict__ partials, long n, float* out) {
    __shared__ float red[256];
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;            // ~19 k partials in one workgroup: four loads in flight per thread
    long i = threadIdx.x;
    for (; i + 768 < n; i += 1024) { a0 += partials[i]; a1 += partials[i + 256]; a2 += partials[i + 512]; a3 += partials[i + 768]; }
    for (; i < n; i += 256) a0 += partials[i];
    const float a = (a0 + a1) + (a2 + a3);
    red[threadIdx.x] = a;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) { if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off]; __syncthreads(); }
    if (threadIdx.x == 0) out[0] = red[0];
}
__global__ void clip_coef_kernel(const float* sumsq, float max_norm, float* coef, float* norm_out) {
    const float norm = sqrtf(sumsq[0]);
    if (norm_out) norm_out[0] = norm;
    float c = max_norm / (norm + 1e-6f);            // torch.nn.utils.clip_grad_norm_
    coef[0] = c > 1.f ? 1.f : c;                    // clamp(max=1): a NaN norm gives a NaN coefficient (as torch does), never a silent 1
}
// step counter lives on the device so that a captured hipGraph replays with the right bias correction
__global__ void adam_tick_kernel(int* step, float b1, float b2, float* bc) {
    const int s = step[0] + 1;
    step[0] = s;
    bc[0] = 1.f - powf(b1, (float)s);
    bc[1] = 1.f - powf(b2, (float)s);
}
__global__ __launch_bounds__(256) void adamw_multi_kernel(float* const* __restrict__ params, const float* const* __restrict__ grads,
                                                          float* const* __restrict__ m1, float* const* __restrict__ m2, const int64_t* __restrict__ sizes,
                                                          const float* __restrict__ clip_coef, const float* __restrict__ lr_dev, float b1, float b2, float eps,
                                                          float wd, const float* __restrict__ bc) {
    const float lr = lr_dev[0], bc1 = bc[0], bc2 = bc[1];
    const int t = blockIdx.y;
    float* p = params[t]; const float* g = grads[t]; float* ea = m1[t]; float* es = m2[t];
    const long n = sizes[t];
    const float cc = clip_coef ? clip_coef[0] : 1.f;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const float gr = g[i] * cc;
        float w = p[i] * (1.f - lr * wd);
        const float a = ea[i] * b1 + (1.f - b1) * gr;
        const float s = es[i] * b2 + (1.f - b2) * gr * gr;
        ea[i] = a; es[i] = s;
        const float denom = sqrtf(s) / sqrtf(bc2) + eps;
        w -= (lr / bc1) * a / denom;
        p[i] = w;
    }
}

// ---- chunked forms: block c handles chunk c of the concatenation of all tensors (chunk_prefix[t] = first chunk of tensor t, built once
// on the host since the sizes are static).  Every block has OPT_CHUNK elements of work (except a tensor's last chunk): no empty blocks
// for the ~400 small tensors, enough parallelism for the large ones, float4 accesses.
TAV_DEV int chunk_owner(const int32_t* __restrict__ prefix, int ntensors, int c) {
    int lo = 0, hi = ntensors - 1;
    while (lo < hi) {                               // last t with prefix[t] <= c
        const int mid = (lo + hi + 1) >> 1;
        if (prefix[mid] <= c) lo = mid; else hi = mid - 1;
    }
    return lo;
}
__global__ __launch_bounds__(256) void sumsq_chunk_kernel(const float* const* __restrict__ ptrs, const int64_t* __restrict__ sizes,
                                                          const int32_t* __restrict__ prefix, int ntensors, float* __restrict__ partials) {
    __shared__ float red[4];
    const int c = blockIdx.x, t = chunk_owner(prefix, ntensors, c);
    const long off = (long)(c - prefix[t]) * OPT_CHUNK;
    const float* p = ptrs[t] + off;
    long n = sizes[t] - off; n = n < OPT_CHUNK ? n : OPT_CHUNK;
    float a = 0.f;
    if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) {
        const long n4 = n >> 2;
        for (long i = threadIdx.x; i < n4; i += 256) { const f32x4 v = *reinterpret_cast<const f32x4*>(p + 4 * i); a += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3]; }
        for (long i = 4 * n4 + threadIdx.x; i < n; i += 256) a += p[i] * p[i];
    } else {
        for (long i = threadIdx.x; i < n; i += 256) a += p[i] * p[i];
    }
    a = wave_sum(a);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) partials[c] = red[0] + red[1] + red[2] + red[3];
}
// One chunk of one tensor (n <= OPT_CHUNK elements from p / g / ea / es) with the learning rate and the weight decay of that tensor: the body of
// adamw_chunk_kernel (one lr, one wd for the launch) and of adamw_chunk_groups_kernel (a pair per parameter group), so the two cannot drift apart.
TAV_DEV void adamw_chunk_update(float* p, const float* g, float* ea, float* es, long n, float cc, float lr,
                                float wd, float b1, float b2, float eps, float bc1, float bc2) {
    const float decay = 1.f - lr * wd, step = lr / bc1, rs2 = 1.f / sqrtf(bc2), omb1 = 1.f - b1, omb2 = 1.f - b2;
    // One arithmetic for every element, whichever of the loops below it falls into: contraction is OFF and the three multiply-adds are written
    // out, so the 16-byte and the scalar form agree bit for bit.  (With the compiler free to contract, the two forms differed in the last bit of
    // some weights -- harmless alone, but an optimizer sharded over ranks cuts the tensors elsewhere than the replicated one, lands elements in the
    // other form, and Adam's m / sqrt(v) turns last-bit differences of near-zero gradients into lr-sized ones within a few steps.)
    auto upd = [&](float& w, float gr, float& a, float& s2) {
#pragma clang fp contract(off)
        gr = gr * cc;
        w = w * decay;
        a = __builtin_fmaf(a, b1, omb1 * gr);
        s2 = __builtin_fmaf(s2, b2, (omb2 * gr) * gr);
        const float den = __builtin_fmaf(sqrtf(s2), rs2, eps);
        const float q = (step * a) / den;
        w = w - q;
    };
    const bool al = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(ea) | reinterpret_cast<uintptr_t>(es)) & 15) == 0;
    long done = 0;
    if (al) {
        const long n4 = n >> 2;
        constexpr int U = 4;                        // 16 independent 16-B loads in flight per thread before the first use
        long i = threadIdx.x;
        for (; i + (U - 1) * 256 < n4; i += U * 256) {
            f32x4 w[U], a[U], s2[U], gr[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {                // every byte is touched exactly once per step: non-temporal both ways
                const long j = 4 * (i + u * 256);
                w[u] = __builtin_nontemporal_load(reinterpret_cast<f32x4*>(p + j)); gr[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(g + j));
                a[u] = __builtin_nontemporal_load(reinterpret_cast<f32x4*>(ea + j)); s2[u] = __builtin_nontemporal_load(reinterpret_cast<f32x4*>(es + j));
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float wk = w[u][k], ak = a[u][k], sk = s2[u][k];
                    upd(wk, gr[u][k], ak, sk);
                    w[u][k] = wk; a[u][k] = ak; s2[u][k] = sk;
                }
                const long j = 4 * (i + u * 256);
                *reinterpret_cast<f32x4*>(p + j) = w[u];         // the updated weights are read again right away (operand casts): default policy
                __builtin_nontemporal_store(a[u], reinterpret_cast<f32x4*>(ea + j)); __builtin_nontemporal_store(s2[u], reinterpret_cast<f32x4*>(es + j));
            }
        }
        for (; i < n4; i += 256) {
            f32x4 w = *reinterpret_cast<f32x4*>(p + 4 * i), a = *reinterpret_cast<f32x4*>(ea + 4 * i), s2 = *reinterpret_cast<f32x4*>(es + 4 * i);
            const f32x4 gr = *reinterpret_cast<const f32x4*>(g + 4 * i);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float wk = w[k], ak = a[k], sk = s2[k];
                upd(wk, gr[k], ak, sk);
                w[k] = wk; a[k] = ak; s2[k] = sk;
            }
            *reinterpret_cast<f32x4*>(p + 4 * i) = w; *reinterpret_cast<f32x4*>(ea + 4 * i) = a; *reinterpret_cast<f32x4*>(es + 4 * i) = s2;
        }
        done = 4 * n4;
    }
    for (long i = done + threadIdx.x; i < n; i += 256) upd(p[i], g[i], ea[i], es[i]);
}
__global__ __launch_bounds__(256) void adamw_chunk_kernel(float* const* __restrict__ params, const float* const* __restrict__ grads,
                                                          float* const* __restrict__ m1, float* const* __restrict__ m2, const int64_t* __restrict__ sizes,
                                                          const int32_t* __restrict__ prefix, int ntensors, const float* __restrict__ clip_coef,
                                                          const float* __restrict__ lr_dev, float b1, float b2, float eps, float wd, const float* __restrict__ bc) {
    const float lr = lr_dev[0], bc1 = bc[0], bc2 = bc[1];
    const int c = blockIdx.x, t = chunk_owner(prefix, ntensors, c);
    const long off = (long)(c - prefix[t]) * OPT_CHUNK;
    float* p = params[t] + off; const float* g = grads[t] + off; float* ea = m1[t] + off; float* es = m2[t] + off;
    long n = sizes[t] - off; n = n < OPT_CHUNK ? n : OPT_CHUNK;
    const float cc = clip_coef ? clip_coef[0] : 1.f;
    adamw_chunk_update(p, g, ea, es, n, cc, lr, wd, b1, b2, eps, bc1, bc2);
}
// Parameter groups: the same walk; tensor t belongs to group group_of[t] (clamped into the table) and takes that group's {lr, wd} from the
// device table `hyper` -- three more block-uniform loads per chunk, all of them before the element loops.
__global__ __launch_bounds__(256) void adamw_chunk_groups_kernel(float* const* __restrict__ params, const float* const* __restrict__ grads,
                                                                 float* const* __restrict__ m1, float* const* __restrict__ m2,
                                                                 const int64_t* __restrict__ sizes, const int32_t* __restrict__ prefix, int ntensors,
                                                                 const float* __restrict__ clip_coef, const int32_t* __restrict__ group_of,
                                                                 const float* __restrict__ hyper, int ngroups, float b1, float b2, float eps,
                                                                 const float* __restrict__ bc) {
    const float bc1 = bc[0], bc2 = bc[1];
    const int c = blockIdx.x, t = chunk_owner(prefix, ntensors, c);
    int gi = group_of[t];
    gi = gi < 0 ? 0 : (gi >= ngroups ? ngroups - 1 : gi);
    const float lr = hyper[2 * gi], wd = hyper[2 * gi + 1];
    const long off = (long)(c - prefix[t]) * OPT_CHUNK;
    float* p = params[t] + off; const float* g = grads[t] + off; float* ea = m1[t] + off; float* es = m2[t] + off;
    long n = sizes[t] - off; n = n < OPT_CHUNK ? n : OPT_CHUNK;
    const float cc = clip_coef ? clip_coef[0] : 1.f;
    adamw_chunk_update(p, g, ea, es, n, cc, lr, wd, b1, b2, eps, bc1, bc2);
}

}  // namespace tav
using namespace tav;

extern "C" int tav_version(void) { return TAV_ABI_VERSION; }
extern "C" const char* tav_error_string(int code) {
    switch (code) {
        case 0: return "ok";
        case TAV_ERR_NULL: return "required pointer is NULL";
        case TAV_ERR_SHAPE: return "unsupported shape";
        case TAV_ERR_DTYPE: return "unsupported dtype";
        case TAV_ERR_ALIGN: return "stride/offset not 16-byte aligned";
        case TAV_ERR_NO_RCCL: return "RCCL not available (librccl could not be loaded)";
        default: return code > 0 ? hipGetErrorString((hipError_t)code) : "unknown";
    }
}

extern "C" int tav_cast_weight(const float* src, int64_t R, int64_t C, void* dst, int64_t ld_dst, void* dst_t, int64_t ld_dst_t, int32_t dt, void* stream) {
    if (const int rc = plan::cast_weight_validate(src && (dst || dst_t), dt, R, C)) return rc;
    const long ld_n = ld_dst > 0 ? ld_dst : C, ld_t = ld_dst_t > 0 ? ld_dst_t : R;
    return floats::dispatch(dt, [&](auto t) {
        using T = decltype(t);
        TAV_LAUNCH((cast_weight_kernel<T>), plan::tile32_launch(R, C), stream, src, (T*)dst, ld_n, (T*)dst_t, ld_t, (int)R, (int)C);
        return 0;
    });
}
extern "C" int tav_cast_weights_multi(const void* descs_dev, int32_t n, int32_t blocks_per_tensor, void* stream) {
    if (const int rc = plan::cast_weights_multi_validate(descs_dev, n, blocks_per_tensor)) return rc;
    TAV_LAUNCH(cast_weight_multi_kernel, (plan::Launch{blocks_per_tensor, n, 1, 256, 0}), stream, (const CastDesc*)descs_dev);
    return 0;
}
extern "C" int tav_cast_conv_weight(const float* src, int64_t co, int64_t ci, int64_t k, void* dst, void* dst_t, void* dst_phase, int64_t conv_stride,
                                    int32_t dt, void* stream) {
    if (const int rc = plan::cast_conv_weight_validate(src && (dst || dst_t || dst_phase), dst_phase, dt, co, ci, k, conv_stride)) return rc;
    const int cs = dst_phase ? (int)conv_stride : 1;
    return floats::dispatch(dt, [&](auto t) {
        using T = decltype(t);
        TAV_LAUNCH((cast_conv_weight_kernel<T>), plan::grid1(co * ci * k), stream, src, (T*)dst, (T*)dst_t, (T*)dst_phase, (int)co, (int)ci, (int)k, cs);
        return 0;
    });
}
// v5: zero rows [0, pad) and [pad + T, T + 2 pad) of every [T + 2 pad][C] batch entry (the zero frame around a padded gradient buffer)
template <typename T> __global__ void zero_pad_rows_kernel(T* __restrict__ buf, long n4, int Tn, int C, int pad) {
    const long i4 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i4 >= n4) return;
    const int c4 = C / 4;
    const long row = i4 / c4;                                // (b, pad row 0 .. 2 pad - 1)
    const int col = (int)(i4 - row * c4) * 4;
    const long b = row / (2 * pad);
    const int pr = (int)(row - b * 2 * pad);
    const long trow = b * ((long)Tn + 2 * pad) + (pr < pad ? pr : Tn + pr);
    st4(buf + trow * C + col, f32x4{0.f, 0.f, 0.f, 0.f});
}
extern "C" int tav_zero_pad_rows(void* buf, int32_t dt, int64_t B, int64_t T, int64_t C, int64_t pad, void* stream) {
    if (const int rc = plan::zero_pad_rows_validate(buf, dt, B, T, C, pad)) return rc;
    const long n4 = B * 2 * pad * (C / 4);
    return floats::dispatch(dt, [&](auto t) {
        using E = decltype(t);
        TAV_LAUNCH((zero_pad_rows_kernel<E>), plan::grid1(n4), stream, (E*)buf, n4, (int)T, (int)C, (int)pad);
        return 0;
    });
}
extern "C" int tav_cast2d(const void* src, int32_t sdt, int64_t ld_src, void* dst, int32_t ddt, int64_t ld_dst, int64_t R, int64_t C, void* stream) {
    if (const int rc = plan::cast2d_validate(src && dst, sdt, ddt, ld_src, ld_dst, R, C)) return rc;
    using cases = dtypes<on<TAV_F32, TAV_BF16>, on<TAV_BF16, TAV_F32>, on<TAV_F32, TAV_F32>, on<TAV_BF16, TAV_BF16>>;
    return cases::dispatch(sdt, ddt, [&](auto ts, auto td) {
        using S = decltype(ts); using D = decltype(td);
        TAV_LAUNCH((cast2d_kernel<S, D>), plan::grid1(R * (C / 4)), stream, (const S*)src, (long)ld_src, (D*)dst, (long)ld_dst, (long)R, (int)(C / 4));
        return 0;
    });
}
extern "C" int tav_transpose2d(const void* src, void* dst, int32_t dt, int64_t R, int64_t C, int64_t nbatch, void* stream) {
    if (const int rc = plan::transpose2d_validate(src && dst, dt, R, C, nbatch)) return rc;
    return floats::dispatch(dt, [&](auto t) {
        using T = decltype(t);
        TAV_LAUNCH((transpose2d_kernel<T>), plan::tile32_launch(R, C, nbatch), stream, (const T*)src, (T*)dst, (int)R, (int)C);
        return 0;
    });
}
extern "C" int tav_add_f32(const float* a, const float* b, float* y, void* y_lp, int32_t lp, int64_t n, void* stream) {
    if (const int rc = plan::add_f32_validate(a && b && (y || y_lp), n)) return rc;
    return floats::dispatch(plan::lp_code(y_lp, lp), [&](auto t) {
        using T = decltype(t);
        TAV_LAUNCH((add_f32_kernel<T>), plan::grid1(n / 4), stream, a, b, y, (T*)y_lp, n / 4);
        return 0;
    });
}
extern "C" int tav_fill_f32(float* p, float v, int64_t n, void* stream) {
    if (const int rc = plan::count_validate(p, n)) return rc;
    TAV_LAUNCH(fill_f32_kernel, plan::fill_launch(n), stream, p, v, (long)n);
    return 0;
}
extern "C" int tav_embed_add_fwd(const float* x, const int64_t* ids, const float* table, float* out, int64_t rows, int64_t W, int64_t ntable, void* stream) {
    if (const int rc = plan::table_rows_validate(x && ids && table && out, rows, W, ntable)) return rc;
    TAV_LAUNCH(embed_add_fwd_kernel, plan::grid1(rows * (W / 4)), stream, x, ids, table, out, (long)rows, (int)(W / 4));
    return 0;
}
extern "C" int tav_embed_add_bwd_parts(int64_t rows) { return plan::embed_add_bwd_parts(rows); }
extern "C" int tav_embed_add_bwd(const float* dy, const int64_t* ids, float* dtable, float* partials, int64_t rows, int64_t W, int64_t ntable,
                                 int32_t accumulate, void* stream) {
    if (const int rc = plan::embed_add_bwd_validate(dy && ids && dtable && partials, rows, W, ntable)) return rc;
    const plan::PartsPlan P = plan::embed_add_bwd_plan(rows, W, ntable);
    TAV_LAUNCH(embed_add_bwd_partial_kernel, P.partial, stream, dy, ids, partials, (long)rows, (int)W, (int)ntable, P.rows_per_part);
    TAV_LAUNCH(embed_add_bwd_final_kernel, P.final_, stream, partials, dtable, P.parts, (int)ntable, (int)W, accumulate);
    return 0;
}
extern "C" int tav_ln_fwd(const tav_ln_args* a, void* stream);
extern "C" int tav_text_embed_fwd(const tav_text_embed_args* a, void* stream) {
    if (const int rc = plan::text_embed_validate(a)) return rc;
    const tav_ln_args ln = plan::text_embed_ln(a);
    TAV_LAUNCH(text_pos_ids_kernel, (plan::Launch{a->B, 1, 1, plan::text_pos_threads(a->S), 0}), stream, a->ids, a->pos_ids, (int)a->S, a->pad_id);
    TAV_LAUNCH(text_embed_sum_kernel, plan::grid1(ln.rows * (a->W / 4)), stream, a->ids, a->pos_ids, a->word, a->pos, a->type, a->pre, (long)ln.rows, (int)(a->W / 4));
    return tav_ln_fwd(&ln, stream);
}
extern "C" int tav_scatter_add_rows(const float* d, const int64_t* idx, float* dtable, int64_t rows, int64_t W, int64_t ntable, void* stream) {
    if (const int rc = plan::scatter_add_validate(d && idx && dtable, rows, W, ntable)) return rc;
    TAV_LAUNCH(scatter_add_rows_kernel, (plan::Launch{rows, 1, 1, SCAT_T, plan::scatter_add_lds(rows, W)}), stream, d, idx, dtable, (int)rows, (int)W, (long)ntable);
    return 0;
}
extern "C" int tav_gather_rows(const float* table, const int32_t* idx, float* out, int64_t rows, int64_t W, int64_t ntable, void* stream) {
    if (const int rc = plan::table_rows_validate(table && idx && out, rows, W, ntable)) return rc;
    TAV_LAUNCH(gather_rows_kernel, plan::grid1(rows * (W / 4)), stream, table, idx, out, (long)rows, (int)(W / 4), (int)ntable);
    return 0;
}
extern "C" int tav_patchify(const float* video, const int32_t* keep_idx, void* patches, int32_t dt, int64_t B, int64_t F, int64_t H, int64_t W, int64_t nkeep,
                            void* stream) {
    if (const int rc = plan::patchify_validate(video && keep_idx && patches, dt, B, F, H, W, nkeep)) return rc;
    return floats::dispatch(dt, [&](auto t) {
        using T = decltype(t);
        TAV_LAUNCH((patchify_kernel<T>), (plan::Launch{nkeep, B, 1, 256, 0}), stream, video, keep_idx, (T*)patches, (int)F, (int)H, (int)W, (int)nkeep);
        return 0;
    });
}
extern "C" int tav_mask_to_index(const uint8_t* mask, int32_t keep_value, int32_t* keep_idx, int32_t* counts, int64_t B, int64_t n, int64_t nkeep, void* stream) {
    if (const int rc = plan::mask_to_index_validate(mask && keep_idx, B, n, nkeep)) return rc;
    TAV_LAUNCH(mask_to_index_kernel, (plan::Launch{B, 1, 1, 256, 0}), stream, mask, keep_value, keep_idx, counts, (int)n, (int)nkeep);
    return 0;
}
extern "C" int tav_ragged_lens(const uint8_t* mask, int32_t* true_cnt, int32_t* vid_lens, int32_t* av_lens, int32_t* status, int64_t B, int64_t ntok,
                               int64_t cap_true, int64_t cap_keep, int64_t base, void* stream) {
    if (const int rc = plan::ragged_lens_validate(mask && true_cnt && vid_lens && av_lens && status, B, ntok, cap_true, cap_keep, base)) return rc;
    TAV_LAUNCH(ragged_lens_kernel, (plan::Launch{B, 1, 1, 256, 0}), stream, mask, true_cnt, vid_lens, av_lens, status, (int)ntok, (int)cap_true, (int)cap_keep, (int)base);
    return 0;
}
extern "C" int tav_mean_pool_fwd(const float* x, float* y, int64_t B, int64_t S, int64_t W, void* stream) {
    if (const int rc = plan::mean_pool_validate(x && y, B, S, W)) return rc;
    TAV_LAUNCH(mean_pool_fwd_kernel, plan::mean_pool_fwd_launch(B, W), stream, x, y, (int)S, (int)W);
    return 0;
}
extern "C" int tav_mean_pool_bwd(const float* dy, float* dx, void* dx_lp, int32_t lp, int64_t B, int64_t S, int64_t W, void* stream) {
    if (const int rc = plan::mean_pool_validate(dy && (dx || dx_lp), B, S, W)) return rc;
    const long n4 = B * S * W / 4;
    return floats::dispatch(plan::lp_code(dx_lp, lp), [&](auto t) {
        using T = decltype(t);
        TAV_LAUNCH((mean_pool_bwd_kernel<T>), plan::grid1(n4), stream, dy, dx, (T*)dx_lp, n4, (int)S, (int)(W / 4));
        return 0;
    });
}
extern "C" int tav_mean_pool_fwd_len(const float* x, float* y, const int32_t* seq_lens, int64_t B, int64_t S, int64_t W, void* stream) {
    if (const int rc = plan::mean_pool_validate(x && y && seq_lens, B, S, W)) return rc;
    TAV_LAUNCH(mean_pool_fwd_len_kernel, plan::mean_pool_fwd_launch(B, W), stream, x, y, seq_lens, (int)S, (int)W);
    return 0;
}
extern "C" int tav_mean_pool_bwd_len(const float* dy, float* dx, void* dx_lp, int32_t lp, const int32_t* seq_lens, int64_t B, int64_t S, int64_t W,
                                     void* stream) {
    if (const int rc = plan::mean_pool_validate(dy && (dx || dx_lp) && seq_lens, B, S, W)) return rc;
    const long n4 = B * S * W / 4;
    return floats::dispatch(plan::lp_code(dx_lp, lp), [&](auto t) {
        using T = decltype(t);
        TAV_LAUNCH((mean_pool_bwd_len_kernel<T>), plan::grid1(n4), stream, dy, dx, (T*)dx_lp, seq_lens, n4, (int)S, (int)(W / 4));
        return 0;
    });
}
extern "C" int tav_head_fwd(const float* x, const float* W, const float* b, float* y, int64_t B, int64_t K, int64_t N, void* stream) {
    if (const int rc = plan::head_validate(x && W && y, B, K, N, INT64_MAX)) return rc;
    TAV_LAUNCH(head_fwd_kernel, plan::grid1(B * N, 4), stream, x, W, b, y, (int)B, (int)K, (int)N);      // one wave per output
    return 0;
}
extern "C" int tav_head_bwd(const float* x, const float* W, const float* dy, float* dx, float* dW, float* db, int64_t B, int64_t K, int64_t N,
                            int32_t accumulate, void* stream) {
    if (const int rc = plan::head_validate(x && W && dy && dW, B, K, N, 256)) return rc;
    TAV_LAUNCH(head_bwd_kernel, plan::grid1(K), stream, x, W, dy, dx, dW, db, (int)B, (int)K, (int)N, accumulate);
    return 0;
}
extern "C" int tav_tanh_fwd(const float* x, float* y, int64_t n, void* stream) {
    if (const int rc = plan::count_validate(x && y, n)) return rc;
    TAV_LAUNCH(tanh_fwd_kernel, plan::grid1(n), stream, x, y, (long)n);
    return 0;
}
extern "C" int tav_tanh_bwd(const float* y, const float* dy, float* dx, int64_t n, void* stream) {
    if (const int rc = plan::count_validate(y && dy && dx, n)) return rc;
    TAV_LAUNCH(tanh_bwd_kernel, plan::grid1(n), stream, y, dy, dx, (long)n);
    return 0;
}
static const plan::Launch ONE_BLOCK = {1, 1, 1, 256, 0}, ONE_THREAD = {1, 1, 1, 1, 0};
extern "C" int tav_cross_entropy(const float* logits, const int64_t* target, const float* cw, float* loss, float* dlogits, int64_t B, int64_t C,
                                 float grad_scale, void* stream) {
    if (const int rc = plan::classes_validate(logits && target && (loss || dlogits), B, C, INT64_MAX)) return rc;
    TAV_LAUNCH(cross_entropy_kernel, ONE_BLOCK, stream, logits, target, cw, loss, dlogits, (int)B, (int)C, grad_scale);
    return 0;
}
extern "C" int tav_step_stats(const float* logits, const int64_t* preds, const int64_t* target, int64_t* cm, const float* loss,
                              const int32_t* status, tav_loop_acc* acc, int64_t B, int64_t C, void* stream) {
    if (const int rc = plan::classes_validate(target && (!logits) != (!preds) && (cm || acc), B, C, INT32_MAX)) return rc;
    TAV_LAUNCH(step_stats_kernel, ONE_BLOCK, stream, logits, preds, target, cm, loss, status, acc, (int)B, (int)C);
    return 0;
}
extern "C" int tav_dropout_fwd(const float* x, float* y, uint8_t* mask, int64_t n, float p, uint64_t seed, uint64_t offset, void* stream) {
    if (const int rc = plan::dropout_validate(x && y && mask, n, p)) return rc;
    TAV_LAUNCH(dropout_fwd_kernel, plan::grid1(n), stream, x, y, mask, (long)n, p, seed, offset);
    return 0;
}
extern "C" int tav_dropout_fwd_dev(const float* x, float* y, uint8_t* mask, int64_t n, float p, const uint64_t* seed_state, uint64_t offset,
                                   void* stream) {
    if (const int rc = plan::dropout_validate(x && y && mask && seed_state, n, p)) return rc;
    TAV_LAUNCH(dropout_fwd_dev_kernel, plan::grid1(n), stream, x, y, mask, (long)n, p, seed_state, offset);
    return 0;
}
extern "C" int tav_dropout_bwd(const float* dy, const uint8_t* mask, float* dx, int64_t n, float p, void* stream) {
    if (const int rc = plan::dropout_validate(dy && mask && dx, n, p)) return rc;
    TAV_LAUNCH(dropout_bwd_kernel, plan::grid1(n), stream, dy, mask, dx, (long)n, p);
    return 0;
}
extern "C" int tav_sumsq_partials(int32_t ntensors) { return plan::sumsq_partials(ntensors); }
extern "C" int tav_sumsq_multi(const float* const* ptrs, const int64_t* sizes, int32_t ntensors, float* partials, float* out_sumsq, void* stream) {
    if (const int rc = plan::multi_tensor_validate(ptrs && sizes && partials && out_sumsq, ntensors)) return rc;
    TAV_LAUNCH(sumsq_multi_kernel, (plan::Launch{SUMSQ_BLOCKS, ntensors, 1, 256, 0}), stream, ptrs, sizes, partials);
    TAV_LAUNCH(sum_final_kernel, ONE_BLOCK, stream, partials, (long)plan::sumsq_partials(ntensors), out_sumsq);
    return 0;
}
extern "C" int tav_optim_chunk_elems(void) { return OPT_CHUNK; }
extern "C" int tav_sumsq_chunked(const float* const* ptrs, const int64_t* sizes, const int32_t* chunk_prefix, int32_t ntensors, int32_t nchunks,
                                 float* partials, float* out_sumsq, void* stream) {
    if (const int rc = plan::chunked_validate(ptrs && sizes && chunk_prefix && partials && out_sumsq, ntensors, nchunks)) return rc;
    TAV_LAUNCH(sumsq_chunk_kernel, (plan::Launch{nchunks, 1, 1, 256, 0}), stream, ptrs, sizes, chunk_prefix, ntensors, partials);
    TAV_LAUNCH(sum_final_kernel, ONE_BLOCK, stream, partials, (long)nchunks, out_sumsq);
    return 0;
}
// second stage of tav_sumsq_chunked on its own: a sharded optimizer computes the partials of the chunks it owns, the ranks exchange them, and every
// rank adds the complete array here -- same kernel, same order, hence the same norm bit for bit as the replicated optimizer's
extern "C" int tav_sum_partials(const float* partials, int64_t n, float* out, void* stream) {
    if (const int rc = plan::count_validate(partials && out, n)) return rc;
    TAV_LAUNCH(sum_final_kernel, ONE_BLOCK, stream, partials, (long)n, out);
    return 0;
}
extern "C" int tav_adamw_chunked(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq, const int64_t* sizes,
                                 const int32_t* chunk_prefix, int32_t ntensors, int32_t nchunks, const float* clip_coef, const float* lr, float beta1,
                                 float beta2, float eps, float weight_decay, int32_t* step, float* bias_corr, void* stream) {
    if (const int rc = plan::chunked_validate(params && grads && exp_avg && exp_avg_sq && sizes && chunk_prefix && lr && step && bias_corr, ntensors, nchunks)) return rc;
    TAV_LAUNCH(adam_tick_kernel, ONE_THREAD, stream, step, beta1, beta2, bias_corr);
    TAV_LAUNCH(adamw_chunk_kernel, (plan::Launch{nchunks, 1, 1, 256, 0}), stream, params, grads, exp_avg, exp_avg_sq, sizes, chunk_prefix, ntensors, clip_coef, lr,
               beta1, beta2, eps, weight_decay, (const float*)bias_corr);
    return 0;
}
extern "C" int tav_optim_max_groups(void) { return OPT_MAX_GROUPS; }
extern "C" int tav_adamw_chunked_groups(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                                        const int64_t* sizes, const int32_t* chunk_prefix, int32_t ntensors, int32_t nchunks, const float* clip_coef,
                                        const int32_t* group_of, const float* hyper, int32_t ngroups, float beta1, float beta2, float eps, int32_t* step,
                                        float* bias_corr, void* stream) {
    if (const int rc = plan::chunked_validate(params && grads && exp_avg && exp_avg_sq && sizes && chunk_prefix && group_of && hyper && step && bias_corr, ntensors,
                                              nchunks, ngroups))
        return rc;
    TAV_LAUNCH(adam_tick_kernel, ONE_THREAD, stream, step, beta1, beta2, bias_corr);
    TAV_LAUNCH(adamw_chunk_groups_kernel, (plan::Launch{nchunks, 1, 1, 256, 0}), stream, params, grads, exp_avg, exp_avg_sq, sizes, chunk_prefix, ntensors, clip_coef,
               group_of, hyper, (int)ngroups, beta1, beta2, eps, (const float*)bias_corr);
    return 0;
}
extern "C" int tav_clip_coef(const float* sumsq, float max_norm, float* coef_out, float* norm_out, void* stream) {
    if (const int rc = plan::ptrs_validate(sumsq && coef_out)) return rc;
    TAV_LAUNCH(clip_coef_kernel, ONE_THREAD, stream, sumsq, max_norm, coef_out, norm_out);
    return 0;
}
extern "C" int tav_adamw_multi(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq, const int64_t* sizes,
                               int32_t ntensors, const float* clip_coef, const float* lr, float beta1, float beta2, float eps, float weight_decay,
                               int32_t* step, float* bias_corr, void* stream) {
    if (const int rc = plan::multi_tensor_validate(params && grads && exp_avg && exp_avg_sq && sizes && lr && step && bias_corr, ntensors)) return rc;
    TAV_LAUNCH(adam_tick_kernel, ONE_THREAD, stream, step, beta1, beta2, bias_corr);
    TAV_LAUNCH(adamw_multi_kernel, (plan::Launch{plan::ADAMW_MULTI_BLOCKS, ntensors, 1, 256, 0}), stream, params, grads, exp_avg, exp_avg_sq, sizes, clip_coef, lr, beta1,
               beta2, eps, weight_decay, (const float*)bias_corr);
    return 0;
}
