// Host decisions of the dense 3-D convolution entry points (conv3d.hip, include/tavhip_conv.h) as pure functions: argument checks, the patch
// a workgroup owns per dtype and channel width, LDS carve-ups, grids, the weight gradient's slabs and the flat linear's parts.  Only the public
// headers and the standard library, no HIP type: any C++17 host compiler builds it (tests/host/conv3d_plan_check.cpp runs it under ASan + UBSan).
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "../../include/tavhip_conv.h"

namespace tav {
namespace plan {

constexpr int CONV_ABI_VERSION = 1;
constexpr int CONV_TAPS = 27;
constexpr int CONV_TW = 32;                       // patch width: two 16-voxel MFMA tiles a wave
constexpr int CONV_MAX_C = 128;
constexpr int64_t CONV_C_QUANT = 16;              // Cp = ceil(C / 16) 16 (include/tavhip_conv.h, padding rule)
constexpr int64_t CONV_MAX_DIM = 4096;
constexpr int64_t CONV_MAX_B = 65536;
constexpr int64_t CONV_LDS_MAX = 160 * 1024;
constexpr int64_t CONV_LDS_SHARE = 64 * 1024;     // a patch that leaves room for a second workgroup on the CU is preferred
constexpr int CONV_MAX_SLABS = 4096;
constexpr int CONV_WG_WAVES = 4;                  // weight gradient: the 27 taps (and the bias row block, "tap" 27) dealt over four waves
constexpr int CONV_WG_SLOTS = 7;                  // taps a wave holds: slot j of wave w is tap w + 4 j
constexpr int FLAT_MAX_O = 16;
constexpr int FLAT_MAX_PARTS = 4096;

inline int64_t conv_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }
inline int conv_es(int dtype) { return dtype == TAV_BF16 ? 2 : 4; }
inline int conv_kstep(int dtype) { return dtype == TAV_BF16 ? 32 : 16; }      // ET<T>::KSTEP
inline int conv_pk(int dtype) { return dtype == TAV_BF16 ? 8 : 4; }           // ET<T>::PK: elements of one 16-byte chunk
inline int64_t conv_cp(int64_t C) { return conv_up(C, CONV_C_QUANT); }
inline int64_t conv_kp(int64_t C, int dtype) { return conv_up(CONV_TAPS * conv_cp(C), conv_kstep(dtype)); }

struct ConvPlan {
    int es, cin_p, cout_p, th, block, n_tiles, n_passes, k_steps, n_chunks;
    int64_t kp, x_pitch, halo_bytes, table_off, lds_bytes;      // voxel pitch in bytes: cin_p es + 16, an odd number of 16-byte slots
    int64_t od, oh, ow, ph, pw, patches;
    // weight gradient (pad = 0)
    int wg_cit, wg_cot, wg_groups, wg_nslabs;
    int64_t z_pitch, wg_z_off, wg_lds_bytes, slab_floats;
};

inline int64_t conv_halo_bytes(int th, int64_t x_pitch) { return 3 * (int64_t)(th + 2) * (CONV_TW + 2) * x_pitch; }

inline int conv_shape_validate(int64_t B, int64_t D, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int pad, int dtype) {
    if (dtype != TAV_BF16 && dtype != TAV_F32) return TAV_ERR_DTYPE;
    if (pad != 0 && pad != 2) return TAV_ERR_SHAPE;
    if (Cin < 1 || Cin > CONV_MAX_C || Cout < 1 || Cout > CONV_MAX_C || B < 1 || B > CONV_MAX_B) return TAV_ERR_SHAPE;
    const int64_t lo = 3 - 2 * pad;
    if (D < lo || H < lo || W < lo || D > CONV_MAX_DIM || H > CONV_MAX_DIM || W > CONV_MAX_DIM) return TAV_ERR_SHAPE;
    // the narrowest patch must fit: forward halo + table, and for pad = 0 the weight gradient's halo + dZ patch
    const int64_t xp = conv_cp(Cin) * conv_es(dtype) + 16, zp = conv_cp(Cout) * conv_es(dtype) + 16;
    const int64_t table = conv_kp(Cin, dtype) / conv_pk(dtype) * 4;
    if (conv_halo_bytes(1, xp) + table > CONV_LDS_MAX) return TAV_ERR_SHAPE;
    if (pad == 0 && conv_halo_bytes(1, xp) + CONV_TW * zp > CONV_LDS_MAX) return TAV_ERR_SHAPE;
    const int64_t od = D + 2 * pad - 2, oh = H + 2 * pad - 2, ow = W + 2 * pad - 2;
    if (B * od * conv_up(oh, 1) * ((ow + CONV_TW - 1) / CONV_TW) >= ((int64_t)1 << 31)) return TAV_ERR_SHAPE;      // the grid at th = 1
    return 0;
}
// (the shape must have passed conv_shape_validate)
inline ConvPlan conv_plan(int64_t B, int64_t D, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int pad, int dtype) {
    ConvPlan P = {};
    P.es = conv_es(dtype);
    P.cin_p = (int)conv_cp(Cin);
    P.cout_p = (int)conv_cp(Cout);
    P.kp = conv_kp(Cin, dtype);
    P.k_steps = (int)(P.kp / conv_kstep(dtype));
    P.n_chunks = CONV_TAPS * P.cin_p / conv_pk(dtype);
    P.x_pitch = (int64_t)P.cin_p * P.es + 16;
    P.z_pitch = (int64_t)P.cout_p * P.es + 16;
    const int64_t table = (int64_t)P.k_steps * 4 * 4;
    // the tallest patch of 4, 2, 1 rows whose LDS (the larger of the forward's and, for pad = 0, the weight gradient's) leaves room for a
    // second workgroup; failing that, the tallest that fits at all
    auto need = [&](int th) {
        const int64_t f = conv_halo_bytes(th, P.x_pitch) + table, w = conv_halo_bytes(th, P.x_pitch) + (int64_t)th * CONV_TW * P.z_pitch;
        return (pad == 0 && w > f) ? w : f;
    };
    P.th = 1;
    for (const int64_t cap : {CONV_LDS_SHARE, CONV_LDS_MAX}) {
        bool found = false;
        for (const int th : {4, 2, 1})
            if (need(th) <= cap) { P.th = th; found = true; break; }
        if (found) break;
    }
    P.block = 64 * P.th;
    const int nt = P.cout_p / 16;
    P.n_passes = (nt + 3) / 4;
    P.n_tiles = (nt + P.n_passes - 1) / P.n_passes;
    P.halo_bytes = conv_halo_bytes(P.th, P.x_pitch);
    P.table_off = P.halo_bytes;
    P.lds_bytes = P.halo_bytes + table;
    P.od = D + 2 * pad - 2;
    P.oh = H + 2 * pad - 2;
    P.ow = W + 2 * pad - 2;
    P.ph = (P.oh + P.th - 1) / P.th;
    P.pw = (P.ow + CONV_TW - 1) / CONV_TW;
    P.patches = B * P.od * P.ph * P.pw;
    if (pad == 0) {
        const int cit = P.cin_p / 16, cot = P.cout_p / 16;
        if (cit % 2 == 0 && cot % 2 == 0) { P.wg_cit = 2; P.wg_cot = 2; }
        else if (cot % 3 == 0) { P.wg_cit = 1; P.wg_cot = 3; }
        else if (cot % 2 == 0) { P.wg_cit = 1; P.wg_cot = 2; }
        else { P.wg_cit = 1; P.wg_cot = 1; }
        P.wg_groups = (cit / P.wg_cit) * (cot / P.wg_cot);
        P.wg_z_off = P.halo_bytes;
        P.wg_lds_bytes = P.halo_bytes + (int64_t)P.th * CONV_TW * P.z_pitch;
        P.slab_floats = (int64_t)(CONV_TAPS + 1) * P.cin_p * P.cout_p;
        const int64_t want = 1024 / P.wg_groups > 0 ? 1024 / P.wg_groups : 1;          // about four workgroups a CU
        P.wg_nslabs = (int)(P.patches < want ? P.patches : want);
    }
    return P;
}
inline void conv_plan_public(const ConvPlan& P, tav_conv3d_plan* o) {
    *o = tav_conv3d_plan{};
    o->cin_p = P.cin_p; o->cout_p = P.cout_p; o->tw = CONV_TW; o->th = P.th; o->block = P.block;
    o->n_tiles = P.n_tiles; o->n_passes = P.n_passes; o->k_steps = P.k_steps; o->kp = P.kp; o->lds_bytes = P.lds_bytes;
    o->od = P.od; o->oh = P.oh; o->ow = P.ow; o->patches = P.patches;
    if (P.wg_groups) {
        o->wg_block = 64 * CONV_WG_WAVES; o->wg_ci_tiles = P.wg_cit; o->wg_co_tiles = P.wg_cot; o->wg_groups = P.wg_groups;
        o->wg_nslabs = P.wg_nslabs; o->wg_lds_bytes = P.wg_lds_bytes; o->wg_slab_floats = P.slab_floats;
    }
}
inline int conv_nslabs(const ConvPlan& P, int nslabs) { return nslabs == 0 ? P.wg_nslabs : nslabs; }
inline int64_t conv_wgrad_ws_bytes(int64_t B, int64_t D, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int dtype, int nslabs) {
    if (const int rc = conv_shape_validate(B, D, H, W, Cin, Cout, 0, dtype)) return rc;
    if (nslabs < 0 || nslabs > CONV_MAX_SLABS) return TAV_ERR_SHAPE;
    const ConvPlan P = conv_plan(B, D, H, W, Cin, Cout, 0, dtype);
    return (int64_t)conv_nslabs(P, nslabs) * P.slab_floats * 4;
}

// the order of the tests is the order of the codes: pointers, dtype, sizes, then alignment
inline int conv_fwd_validate(const tav_conv3d_fwd_args* a, ConvPlan* P) {
    if (!a || !a->x || !a->w || !a->y) return TAV_ERR_NULL;
    if (const int rc = conv_shape_validate(a->B, a->D, a->H, a->W, a->Cin, a->Cout, a->pad, a->dtype)) return rc;
    if ((a->gelu != 0 && a->gelu != 1) || (a->g && !a->gelu)) return TAV_ERR_SHAPE;
    *P = conv_plan(a->B, a->D, a->H, a->W, a->Cin, a->Cout, a->pad, a->dtype);
    if ((uintptr_t)a->x % 16 || (uintptr_t)a->w % 16 || (uintptr_t)a->y % 16 || (uintptr_t)a->g % 16 || (uintptr_t)a->bias % 16) return TAV_ERR_ALIGN;
    return 0;
}
inline int conv_wgrad_validate(const tav_conv3d_wgrad_args* a, ConvPlan* P, int* nslabs) {
    if (!a || !a->x || !a->dz || !a->workspace || !a->dw) return TAV_ERR_NULL;
    if (const int rc = conv_shape_validate(a->B, a->D, a->H, a->W, a->Cin, a->Cout, 0, a->dtype)) return rc;
    if (a->nslabs < 0 || a->nslabs > CONV_MAX_SLABS) return TAV_ERR_SHAPE;
    *P = conv_plan(a->B, a->D, a->H, a->W, a->Cin, a->Cout, 0, a->dtype);
    *nslabs = conv_nslabs(*P, a->nslabs);
    if (a->workspace_bytes < (int64_t)*nslabs * P->slab_floats * 4) return TAV_ERR_SHAPE;
    if ((uintptr_t)a->x % 16 || (uintptr_t)a->dz % 16 || (uintptr_t)a->workspace % 16 || (uintptr_t)a->dw % 4 || (uintptr_t)a->db % 4) return TAV_ERR_ALIGN;
    return 0;
}
inline int conv_dz_validate(bool have, int64_t n, int dtype) {
    if (!have) return TAV_ERR_NULL;
    if (dtype != TAV_BF16 && dtype != TAV_F32) return TAV_ERR_DTYPE;
    return (n < 4 || n % 4 || n > ((int64_t)1 << 40)) ? TAV_ERR_SHAPE : 0;
}
inline int conv_pack_input_validate(bool have, int64_t B, int64_t C, int64_t D, int64_t H, int64_t W, int dtype) {
    if (!have) return TAV_ERR_NULL;
    if (dtype != TAV_BF16 && dtype != TAV_F32) return TAV_ERR_DTYPE;
    if (B < 1 || B > CONV_MAX_B || C < 1 || C > CONV_MAX_C || D < 1 || H < 1 || W < 1 || D > CONV_MAX_DIM || H > CONV_MAX_DIM || W > CONV_MAX_DIM) return TAV_ERR_SHAPE;
    return 0;
}
inline int conv_pack_weight_validate(bool have, int64_t Cout, int64_t Cin, int flip, int dtype) {
    if (!have) return TAV_ERR_NULL;
    if (dtype != TAV_BF16 && dtype != TAV_F32) return TAV_ERR_DTYPE;
    if (Cin < 1 || Cin > CONV_MAX_C || Cout < 1 || Cout > CONV_MAX_C || (flip != 0 && flip != 1)) return TAV_ERR_SHAPE;
    return 0;
}

// ---- flatten + Linear
inline int flat_parts(int64_t S) { return (int)(S < 1 ? 0 : (S + 1023) / 1024 > 1024 ? 1024 : (S + 1023) / 1024); }      // about a thousand voxels a part, at most 1024 parts
inline int flat_shape_validate(int64_t B, int64_t S, int64_t C, int64_t O, int dtype) {
    if (dtype != TAV_BF16 && dtype != TAV_F32) return TAV_ERR_DTYPE;
    if (B < 1 || B > CONV_MAX_B || S < 1 || S > ((int64_t)1 << 36) || C < 1 || C > CONV_MAX_C || O < 1 || O > FLAT_MAX_O) return TAV_ERR_SHAPE;
    if (S * conv_cp(C) > ((int64_t)1 << 40)) return TAV_ERR_SHAPE;
    return 0;
}
inline int flat_nparts(int64_t S, int nparts) { return nparts == 0 ? flat_parts(S) : nparts; }
inline int64_t flat_ws_bytes(int64_t B, int64_t S, int64_t O, int nparts) {
    if (B < 1 || B > CONV_MAX_B || S < 1 || O < 1 || O > FLAT_MAX_O || nparts < 0 || nparts > FLAT_MAX_PARTS) return TAV_ERR_SHAPE;
    return B * flat_nparts(S, nparts) * O * 4;
}
inline int flat_fwd_validate(const tav_flat_linear_fwd_args* a, int* nparts) {
    if (!a || !a->x || !a->w || !a->out || !a->workspace) return TAV_ERR_NULL;
    if (const int rc = flat_shape_validate(a->B, a->S, a->C, a->O, a->dtype)) return rc;
    if (a->nparts < 0 || a->nparts > FLAT_MAX_PARTS) return TAV_ERR_SHAPE;
    *nparts = flat_nparts(a->S, a->nparts);
    if (a->workspace_bytes < a->B * *nparts * a->O * 4) return TAV_ERR_SHAPE;
    if ((uintptr_t)a->x % 16 || (uintptr_t)a->w % 4 || (uintptr_t)a->out % 4 || (uintptr_t)a->workspace % 4 || (uintptr_t)a->bias % 4) return TAV_ERR_ALIGN;
    return 0;
}
inline int flat_bwd_validate(const tav_flat_linear_bwd_args* a) {
    if (!a || !a->x || !a->w || !a->dy || !a->dw) return TAV_ERR_NULL;
    if (const int rc = flat_shape_validate(a->B, a->S, a->C, a->O, a->dtype)) return rc;
    if ((uintptr_t)a->x % 16 || (uintptr_t)a->dx % 16 || (uintptr_t)a->w % 4 || (uintptr_t)a->dy % 4 || (uintptr_t)a->dw % 4 || (uintptr_t)a->db % 4) return TAV_ERR_ALIGN;
    return 0;
}
inline int sigmoid_validate(bool have, int64_t n) {
    if (!have) return TAV_ERR_NULL;
    return (n < 1 || n > ((int64_t)1 << 38)) ? TAV_ERR_SHAPE : 0;
}

}  // namespace plan
}  // namespace tav
