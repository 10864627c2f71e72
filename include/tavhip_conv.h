/* libtavhip, dense 3-D convolution -- the fourth public header of libtavhip.so.
 *
 * The reference's SingleModels/models/visual.py::VisualClassification is Conv3d(3) -> GELU -> [Conv3d(3) -> GELU]* -> flatten -> Linear ->
 * Sigmoid.  The entry points below are that arithmetic: the 3x3x3 convolution forward (which, with a halo of 2 and the flipped, transposed
 * weight copy, is also its input gradient), its weight gradient, the flatten + Linear over tens of millions of features, and the sigmoid.
 * They follow the rules of include/tavhip.h (extern "C", device pointers and sizes, `stream` a hipStream_t passed as void*, no allocation,
 * no synchronisation, TAV_ERR_* codes, arguments validated on the host before anything touches the device) and live in the same shared
 * object.  They have a header of their own for the reason tavhip_align.h and tavhip_rnn.h have one: the symbol set of tavhip.h is pinned by
 * a recorded table.  tav_conv_version() is bumped on any signature change.
 *
 * Fixed: kernel 3x3x3, stride 1, dilation 1, groups 1.  dtype is TAV_BF16 or TAV_F32 (TAV_ERR_DTYPE otherwise): the type of activations,
 * weight operands, dY, g and dZ.  Accumulation is f32.
 *
 * LAYOUT AND PADDING RULE.  Activations are channels-last, [B][D][H][W][Cp] in `dtype`, with the channel count carried padded:
 *     Cp = ceil(C / 16) * 16                  for every C in 1 .. 128, hidden widths and input_dim alike
 * (input_dim 1 .. 4 goes to 16, not 4: a 16-channel tile is what one MFMA row block of the weight gradient holds, and the forward's K-step
 * of 32 bf16 values then covers two taps).  The caller keeps the pad channels of the input, of the weight operands (pad rows AND pad
 * columns) and of the bias at zero; tav_conv3d_pack_input / tav_conv3d_pack_weight write them so.  A pad output channel then has z = 0
 * exactly, gelu(0) = 0, and the kernels store g = 0 there: pad channels of every output (y, g, dX, dZ) are exactly zero.
 *
 * WHERE VALUES ARE ROUNDED to `dtype` (nothing under TAV_F32): y = gelu(z) and g = gelu'(z) when stored by tav_conv3d_fwd (z itself is
 * never stored); dX when stored by the pad = 2 launch; dZ = dY * g once, by tav_conv3d_dz, from the stored dY and g -- the input gradient
 * and the weight gradient read those same bits.  tav_flat_linear_bwd rounds its dx once when it stores it.
 */
#ifndef TAVHIP_CONV_H
#define TAVHIP_CONV_H
#include <stdint.h>
#include "tavhip.h"

#ifdef __cplusplus
extern "C" {
#endif

int tav_conv_version(void);

/* The launch plan (host arithmetic) of tav_conv3d_fwd on an input of B x D x H x W voxels, Cin -> Cout channels, halo `pad` in {0, 2}, and
 * -- for pad = 0 -- of tav_conv3d_wgrad on the same geometry.  TAV_ERR_SHAPE: Cin or Cout outside 1 .. 128, a size below 3 - 2 pad or above
 * 4096, B above 65536, pad not 0 or 2, or channel widths whose halo does not fit the 160 KiB of LDS (Cin above 112 under TAV_F32). */
typedef struct tav_conv3d_plan {
    int32_t cin_p, cout_p;      /* padded channel counts                                                                         */
    int32_t tw, th;             /* the patch of one output plane a workgroup owns: tw x th voxels (tw = 32; th in 4, 2, 1 by LDS) */
    int32_t block;              /* threads of a forward workgroup: one wave per patch row, two 16-voxel tiles a wave             */
    int32_t n_tiles, n_passes;  /* 16-channel output tiles a wave holds at a time, and passes over them                          */
    int32_t k_steps;            /* MFMA K-steps of one output element: ceil(27 cin_p / (32 bf16 | 16 f32))                       */
    int64_t kp;                 /* row length of the weight operand [cout_p][kp], kp = k_steps * (32 | 16), k = tap cin_p + ci   */
    int64_t lds_bytes;          /* dynamic LDS of the forward launch: the (tw + 2)(th + 2) x 3 halo and the tap offset table      */
    int64_t od, oh, ow;         /* output size: D + 2 pad - 2, ...                                                               */
    int64_t patches;            /* = the forward grid: B od ceil(oh / th) ceil(ow / tw)                                           */
    int32_t wg_block;           /* weight gradient (pad = 0 only, zeros otherwise): threads of a workgroup                       */
    int32_t wg_ci_tiles, wg_co_tiles;   /* 16-channel tiles of Cin x Cout one workgroup column holds for its taps                */
    int32_t wg_groups;          /* workgroup columns (grid.y): channel blocks of wg_ci_tiles x wg_co_tiles                        */
    int32_t wg_nslabs;          /* the plan's slab count (grid.x) when the caller passes nslabs = 0                              */
    int32_t reserved;
    int64_t wg_lds_bytes;       /* halo of X and the dZ patch                                                                    */
    int64_t wg_slab_floats;     /* f32 words of one slab: 28 cin_p cout_p (27 taps and the bias row block)                       */
} tav_conv3d_plan;
int tav_conv3d_get_plan(int64_t B, int64_t D, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int32_t pad, int32_t dtype, tav_conv3d_plan* plan);
/* Workspace bytes of tav_conv3d_wgrad for `nslabs` slabs (0 = the plan's choice), or a negative TAV_ERR_*. */
int64_t tav_conv3d_wgrad_ws_bytes(int64_t B, int64_t D, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int32_t dtype, int32_t nslabs);

/* NCDHW f32 [B][C][D][H][W] -> channels-last [B][D][H][W][Cp] in `dtype`, pad channels zero. */
int tav_conv3d_pack_input(const float* src, void* dst, int64_t B, int64_t C, int64_t D, int64_t H, int64_t W, int32_t dtype, void* stream);
/* torch's Conv3d weight, f32 [Cout][Cin][3][3][3], -> the operand of tav_conv3d_fwd in `dtype`, pads zero:
 *   flip_transpose = 0:  dst [cout_p][kp(Cin)],  dst[co][tap cin_p + ci]          = w[co][ci][tap]           the forward's operand
 *   flip_transpose = 1:  dst [cin_p][kp(Cout)],  dst[ci][(26 - tap) cout_p + co]  = w[co][ci][tap]           the input gradient's
 * with tap = 9 kd + 3 kh + kw and kp(C) the plan's kp for C input channels. */
int tav_conv3d_pack_weight(const float* w, void* dst, int64_t Cout, int64_t Cin, int32_t flip_transpose, int32_t dtype, void* stream);

/* z[b][d][h][w][co] = bias[co] + sum_{kd, kh, kw, ci} x[b][d + kd - pad][h + kh - pad][w + kw - pad][ci] W[co][ci][kd][kh][kw], voxels of x
 * outside [0, D) x [0, H) x [0, W) reading as zero (they are zero-filled when the halo is staged into LDS, never in memory).
 *   pad = 0: the forward.  pad = 2 with the flip_transpose weight copy and x = dZ: the input gradient (Cin and Cout are then those of
 *   THIS launch: Cin = the channels of dZ).
 * gelu = 0: y = z.  gelu = 1: y = gelu(z) with the exact erf form (TAV_F32: erff; TAV_BF16: the library's gelu_parts_fast, |erf error|
 * <= 1.5e-7), and, when g is given, g = gelu'(z), zero in the pad channels.
 * An output element is one chain of k_steps MFMA steps in ascending k from a zero accumulator; the bias is added after it.  A voxel is
 * one MFMA column: its bits depend on no other voxel of the batch. */
typedef struct tav_conv3d_fwd_args {
    const void* x;              /* [B][D][H][W][cin_p] */
    const void* w;              /* [cout_p][kp] */
    const float* bias;          /* optional [cout_p] f32 */
    void* y;                    /* [B][od][oh][ow][cout_p] */
    void* g;                    /* optional, like y; needs gelu = 1 */
    int64_t B, D, H, W, Cin, Cout;
    int32_t pad, gelu, dtype, reserved;
} tav_conv3d_fwd_args;
int tav_conv3d_fwd(const tav_conv3d_fwd_args* args, void* stream);

/* dz[k] = dy[k] * g[k] (g NULL: a copy), n elements of `dtype`, n a multiple of 4; rounded once. */
int tav_conv3d_dz(const void* dy, const void* g, void* dz, int64_t n, int32_t dtype, void* stream);

/* dw[co][ci][kd][kh][kw] = sum_{b, d, h, w} x[b][d + kd][h + kh][w + kw][ci] dz[b][d][h][w][co]   and   db[co] = sum dz[b][d][h][w][co],
 * x [B][D][H][W][cin_p], dz [B][D-2][H-2][W-2][cout_p]; dw is f32 in the parameter's own torch layout [Cout][Cin][3][3][3] (no pads), db f32
 * [Cout], both overwritten.  `nslabs` workgroup rows (0 = the plan's choice; at most 4096) each sum a contiguous range of the patches -- slab
 * s takes patches [s P / nslabs, (s + 1) P / nslabs), possibly none -- into an f32 slab of the workspace, voxels of a patch in ascending
 * (h, w) as MFMA k; a second launch adds the slabs in ascending s.  No atomics: the result is bitwise repeatable for one nslabs. */
typedef struct tav_conv3d_wgrad_args {
    const void* x;
    const void* dz;
    void* workspace;            /* tav_conv3d_wgrad_ws_bytes, 16-byte aligned */
    int64_t workspace_bytes;
    float* dw;
    float* db;                  /* optional */
    int64_t B, D, H, W, Cin, Cout;
    int32_t nslabs, dtype;
} tav_conv3d_wgrad_args;
int tav_conv3d_wgrad(const tav_conv3d_wgrad_args* args, void* stream);

/* flatten + Linear.  x is channels-last [B][S][cp] in `dtype` (S = D H W voxels, cp = ceil(C / 16) 16), w is f32 [O][C S] exactly as
 * torch.nn.Linear holds it after x.view(B, -1) on NCDHW: feature f = c S + s; pad channels are skipped.  1 <= O <= 16.
 *   out[b][o] = bias[o] + sum_f x[b][f] w[o][f]        f32 [B][O]
 * Forward: `nparts` workgroups a batch row (0 = tav_flat_linear_parts(S); at most 4096) each sum the voxels [p S / nparts, (p + 1) S / nparts)
 * into f32 partials [B][nparts][O] in the workspace; a second launch adds them in ascending p.  All index arithmetic is 64-bit. */
int32_t tav_flat_linear_parts(int64_t S);
int64_t tav_flat_linear_ws_bytes(int64_t B, int64_t S, int64_t O, int32_t nparts);
typedef struct tav_flat_linear_fwd_args {
    const void* x;
    const float* w;
    const float* bias;          /* optional [O] */
    float* out;
    void* workspace;
    int64_t workspace_bytes;
    int64_t B, S, C, O;
    int32_t nparts, dtype;
} tav_flat_linear_fwd_args;
int tav_flat_linear_fwd(const tav_flat_linear_fwd_args* args, void* stream);
/* One pass over x, w and dy [B][O] f32:  dx[b][s][c] = sum_o dy[b][o] w[o][c S + s] in `dtype` (pad channels zero; optional),
 * dw[o][c S + s] = sum_b dy[b][o] x[b][s][c] in ascending b (f32 [O][C S], overwritten), db[o] = sum_b dy[b][o] (optional). */
typedef struct tav_flat_linear_bwd_args {
    const void* x;
    const float* w;
    const float* dy;
    void* dx;                   /* optional */
    float* dw;
    float* db;                  /* optional */
    int64_t B, S, C, O;
    int32_t dtype, reserved;
} tav_flat_linear_bwd_args;
int tav_flat_linear_bwd(const tav_flat_linear_bwd_args* args, void* stream);

/* y = 1 / (1 + exp(-x)) and dx = dy y (1 - y) from the stored y; f32, any element count n >= 1. */
int tav_sigmoid_fwd(const float* x, float* y, int64_t n, void* stream);
int tav_sigmoid_bwd(const float* y, const float* dy, float* dx, int64_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif
