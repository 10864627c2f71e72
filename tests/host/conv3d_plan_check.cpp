// csrc/conv3d_plan.h alone, as a host program (tests/test_conv3d_host.py builds it with ASan + UBSan): sweeps every channel pair, both halos and
// both dtypes over a set of sizes, and checks what a launch relies on.  Prints "FAILED ..." per broken invariant and ends with
// "ok: 0 failed checks".
#include <stdio.h>
#include <vector>
#include "../../multi-modal-emotion_amd/csrc/conv3d_plan.h"
#include "check.h"

using namespace tav::plan;

int main() {
    long plans = 0, refused = 0;
    const int64_t sizes[][4] = {{1, 3, 3, 3}, {3, 4, 6, 35}, {8, 16, 224, 224}, {8, 14, 222, 222}, {2, 5, 9, 67}, {1, 1, 1, 1}, {65536, 3, 3, 3}, {1, 4096, 3, 4096}};
    for (int dtype : {TAV_BF16, TAV_F32}) {
        const int64_t es = dtype == TAV_BF16 ? 2 : 4, ks = dtype == TAV_BF16 ? 32 : 16, pk = 16 / es;
        for (int pad : {0, 2})
            for (int64_t Cin = 1; Cin <= 130; ++Cin)
                for (int64_t Cout = 1; Cout <= 130; Cout += (Cin % 16 == 0 ? 1 : 7))
                    for (const auto& s : sizes) {
                        const int64_t B = s[0], D = s[1], H = s[2], W = s[3];
                        const int rc = conv_shape_validate(B, D, H, W, Cin, Cout, pad, dtype);
                        const int64_t cin_p = (Cin + 15) / 16 * 16, cout_p = (Cout + 15) / 16 * 16;
                        const bool small = pad == 0 && (D < 3 || H < 3 || W < 3);
                        const bool wide = Cin > 128 || Cout > 128 || (dtype == TAV_F32 && cin_p > 112);
                        if (small || wide) {
                            ++refused;
                            CHECK(rc == TAV_ERR_SHAPE, "Cin %ld Cout %ld pad %d dtype %d size %ld accepted: %d", (long)Cin, (long)Cout, pad, dtype, (long)W, rc);
                            continue;
                        }
                        if (rc) {      // only the grid limit may refuse what is left
                            ++refused;
                            CHECK(rc == TAV_ERR_SHAPE && B * (D + 2 * pad - 2) * (H + 2 * pad - 2) * ((W + 2 * pad - 2 + 31) / 32) >= ((int64_t)1 << 31), "refused %d", rc);
                            continue;
                        }
                        const ConvPlan P = conv_plan(B, D, H, W, Cin, Cout, pad, dtype);
                        ++plans;
                        CHECK(P.cin_p == cin_p && P.cout_p == cout_p && P.es == es, "pads %d %d", P.cin_p, P.cout_p);
                        CHECK(P.th == 4 || P.th == 2 || P.th == 1, "th %d", P.th);
                        CHECK(P.block == 64 * P.th && P.block <= 256, "block %d", P.block);
                        CHECK(P.kp % ks == 0 && P.kp >= 27 * cin_p && P.kp < 27 * cin_p + ks && P.k_steps * ks == P.kp, "kp %ld", (long)P.kp);
                        CHECK(P.n_chunks * pk == 27 * cin_p && P.n_chunks <= 4 * P.k_steps, "chunks %d", P.n_chunks);
                        CHECK(P.n_tiles >= 1 && P.n_tiles <= 4 && P.n_tiles * P.n_passes >= cout_p / 16 && P.n_tiles * (P.n_passes - 1) < cout_p / 16, "tiles %d x %d", P.n_tiles, P.n_passes);
                        // a voxel's pitch: whole 16-byte slots, an odd number of them, room for every channel
                        CHECK(P.x_pitch % 16 == 0 && (P.x_pitch / 16) % 2 == 1 && P.x_pitch >= cin_p * es, "x pitch %ld", (long)P.x_pitch);
                        CHECK(P.halo_bytes == 3 * (int64_t)(P.th + 2) * 34 * P.x_pitch && P.table_off == P.halo_bytes && P.table_off % 16 == 0, "halo");
                        CHECK(P.lds_bytes == P.halo_bytes + 16 * (int64_t)P.k_steps && P.lds_bytes <= CONV_LDS_MAX, "lds %ld", (long)P.lds_bytes);
                        // the last byte a forward lane reads: tap (2, 2, 2) of the window of row th - 1, column 31
                        CHECK(((int64_t)((2 * (P.th + 2) + P.th - 1 + 2) * 34 + 31 + 2)) * P.x_pitch + cin_p * es <= P.halo_bytes, "window");
                        CHECK(P.od == D + 2 * pad - 2 && P.oh == H + 2 * pad - 2 && P.ow == W + 2 * pad - 2 && P.od >= 1 && P.oh >= 1 && P.ow >= 1, "output size");
                        CHECK(P.ph * P.th >= P.oh && (P.ph - 1) * P.th < P.oh && P.pw * 32 >= P.ow && (P.pw - 1) * 32 < P.ow, "patches per plane");
                        CHECK(P.patches == B * P.od * P.ph * P.pw && P.patches < ((int64_t)1 << 31), "grid %ld", (long)P.patches);
                        tav_conv3d_plan pub;
                        conv_plan_public(P, &pub);
                        CHECK(pub.tw == 32 && pub.th == P.th && pub.kp == P.kp && pub.patches == P.patches && pub.lds_bytes == P.lds_bytes, "public plan");
                        if (pad == 0) {
                            const int cit = P.cin_p / 16, cot = P.cout_p / 16;
                            CHECK(P.wg_cit * P.wg_cot <= 4 && cit % P.wg_cit == 0 && cot % P.wg_cot == 0 && P.wg_groups == (cit / P.wg_cit) * (cot / P.wg_cot), "channel block %d x %d", P.wg_cit, P.wg_cot);
                            CHECK(P.z_pitch % 16 == 0 && (P.z_pitch / 16) % 2 == 1 && P.wg_z_off == P.halo_bytes, "z pitch");
                            CHECK(P.wg_lds_bytes == P.halo_bytes + (int64_t)P.th * 32 * P.z_pitch && P.wg_lds_bytes <= CONV_LDS_MAX, "wgrad lds %ld", (long)P.wg_lds_bytes);
                            CHECK(P.slab_floats == 28 * (int64_t)P.cin_p * P.cout_p, "slab");
                            CHECK(P.wg_nslabs >= 1 && P.wg_nslabs <= CONV_MAX_SLABS && P.wg_nslabs <= P.patches, "nslabs %d", P.wg_nslabs);
                            for (int ns : {0, 1, 2, 7, CONV_MAX_SLABS}) {
                                const int eff = conv_nslabs(P, ns);
                                CHECK(conv_wgrad_ws_bytes(B, D, H, W, Cin, Cout, dtype, ns) == (int64_t)eff * P.slab_floats * 4, "workspace");
                                // the slabs' patch ranges tile [0, patches) in order
                                int64_t at = 0;
                                for (int sl = 0; sl < eff && sl < 9; ++sl) {
                                    CHECK(P.patches * sl / eff == at, "slab %d starts at %ld", sl, (long)at);
                                    at = P.patches * (sl + 1) / eff;
                                }
                                CHECK(P.patches * eff / eff == P.patches, "last slab");
                            }
                            CHECK(conv_wgrad_ws_bytes(B, D, H, W, Cin, Cout, dtype, CONV_MAX_SLABS + 1) == TAV_ERR_SHAPE && conv_wgrad_ws_bytes(B, D, H, W, Cin, Cout, dtype, -1) == TAV_ERR_SHAPE, "slab count limits");
                        } else {
                            CHECK(P.wg_groups == 0 && pub.wg_block == 0 && pub.wg_nslabs == 0, "no weight gradient for pad 2");
                        }
                    }
    }
    CHECK(conv_shape_validate(1, 5, 5, 5, 3, 32, 1, TAV_BF16) == TAV_ERR_SHAPE && conv_shape_validate(1, 5, 5, 5, 3, 32, 0, TAV_FP8) == TAV_ERR_DTYPE, "pad / dtype");
    CHECK(conv_shape_validate(0, 5, 5, 5, 3, 32, 0, TAV_BF16) == TAV_ERR_SHAPE && conv_shape_validate(1, 4097, 5, 5, 3, 32, 0, TAV_BF16) == TAV_ERR_SHAPE, "B / size limits");
    // argument structs: pointers, dtype, sizes, then alignment
    {
        tav_conv3d_fwd_args a = {};
        ConvPlan P;
        a.x = a.w = (const void*)4096; a.y = (void*)4096;
        a.B = 2; a.D = 5; a.H = 6; a.W = 40; a.Cin = 3; a.Cout = 32; a.dtype = TAV_BF16;
        CHECK(conv_fwd_validate(&a, &P) == 0 && conv_fwd_validate(nullptr, &P) == TAV_ERR_NULL, "forward args");
        a.g = (void*)4096;
        CHECK(conv_fwd_validate(&a, &P) == TAV_ERR_SHAPE, "g without gelu");
        a.gelu = 1;
        CHECK(conv_fwd_validate(&a, &P) == 0, "g with gelu");
        a.x = (const void*)4100;
        CHECK(conv_fwd_validate(&a, &P) == TAV_ERR_ALIGN, "alignment");
        a.Cin = 129;
        CHECK(conv_fwd_validate(&a, &P) == TAV_ERR_SHAPE, "sizes before alignment");
        a.y = nullptr;
        CHECK(conv_fwd_validate(&a, &P) == TAV_ERR_NULL, "pointers first");
    }
    // flatten + Linear
    for (int64_t S : {(int64_t)1, (int64_t)105, (int64_t)1024, (int64_t)1025, (int64_t)580800, (int64_t)1 << 30}) {
        const int n = flat_parts(S);
        CHECK(n >= 1 && n <= 1024 && n <= S && (S <= 1024 ? n == 1 : true), "parts %d for S %ld", n, (long)S);
        CHECK(flat_ws_bytes(8, S, 7, 0) == 8 * (int64_t)n * 7 * 4 && flat_ws_bytes(8, S, 7, 200) == 8 * 200 * 7 * 4, "flat workspace");
    }
    CHECK(flat_ws_bytes(8, 100, 17, 0) == TAV_ERR_SHAPE && flat_ws_bytes(8, 100, 7, FLAT_MAX_PARTS + 1) == TAV_ERR_SHAPE && flat_parts(0) == 0, "flat limits");
    CHECK(flat_shape_validate(8, 580800, 32, 7, TAV_BF16) == 0 && flat_shape_validate(8, 580800, 32, 17, TAV_BF16) == TAV_ERR_SHAPE &&
              flat_shape_validate(8, 580800, 32, 7, TAV_FP8) == TAV_ERR_DTYPE, "flat shapes");
    CHECK(sigmoid_validate(true, 1) == 0 && sigmoid_validate(false, 1) == TAV_ERR_NULL && sigmoid_validate(true, 0) == TAV_ERR_SHAPE, "sigmoid");
    CHECK(conv_dz_validate(true, 64, TAV_F32) == 0 && conv_dz_validate(true, 6, TAV_F32) == TAV_ERR_SHAPE && conv_dz_validate(false, 64, TAV_F32) == TAV_ERR_NULL, "dz");
    printf("%ld plans checked, %ld shapes refused\n", plans, refused);
    return check_summary();
}
