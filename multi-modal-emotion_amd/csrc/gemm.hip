// MFMA GEMMs of the TAV hot path.
//
//   gemm_nt : C[z][m][n] = epi( sum_k A[z][m][k] * B[z][n][k] )        forward linears, dgrad (with W^T copies),
//                                                                       conv1d-as-GEMM (overlapping A rows), grouped pos-conv
//   gemm_tn : S[s][n1][n2] = sum_{m in split s} A[m][n1] * B[m][n2]     wgrad (dW = dY^T X), split over the token axis,
//             followed by splitk_reduce (deterministic, no atomics)
//
// Replaces the ATen/cuBLAS call sites listed in SURVEY.md §2.1 (reference utils/TAVFormer.py:348-350,393-439;
// HF roberta/wav2vec2/videomae linears; wav2vec2 conv stack).
//
// NT tiles: 64/96/128 x 128 (4 waves as 2x2, 2 workgroups per CU) or 256 x 256 (8 waves as 4x2, each a 64 x 128 block of 16x16 MFMA tiles, one
// workgroup per CU), K-tile = 128 bytes per row (64 bf16 / 32 f32 / 128 e4m3), staged by LDS-DMA (global_load_lds_dwordx4 from inline asm) into a
// 2- to 4-deep ring with the next tile's DMA pieces issued between the MFMA groups, one barrier per K-tile (the 256 x 256 tiles of both kernels:
// five 32 KB images = 160 KB, three for the activation-side operand, which is issued two K-tiles ahead, two for the other).  The host picks the tile -- or a mix of
// both over disjoint row ranges -- per call from a fitted cost model (nt_pick_tile, tav_gemm_nt_schedule) and the epilogue flavour (EPI) from the
// arguments: every such host decision is a pure function of gemm_plan.h, this file keeps the kernels and the enqueue.  TN tiles: 128 x 128 (4 waves) or 256 x 256 (8 waves, token axis split into f32 slabs), 64-token K-tiles, transposed fragment reads.
// LDS image of the NT kernel: [row][8 chunks of 16 B], chunk index XOR-swizzled with (row>>1)&7 so that the
// ds_read_b128 fragment reads (16 rows x one chunk per 16-lane group) are bank-conflict free.
#include "common.h"
#include <type_traits>
#include "tavhip_internal.h"
#include "gemm_plan.h"

namespace tav {

// ------------------------------------------------------------------------------------------------
struct GemmNT {
    const char* A; const char* B; char* C; char* Cpre; const float* bias; const char* gelu_in; const float* resid;
    int M, N, K;
    long lda, ldb, ldc, ld_pre, ld_gelu, ld_resid;   // row strides in elements
    int nzg;
    long a_zb, a_zg, b_zb, b_zg, c_zb, c_zg, bias_zg;  // batch strides in elements (C strides apply to Cpre/gelu_in/resid too)
    long g_zb;                                         // ... except that gelu_in takes this zb stride (= c_zb unless the caller says otherwise: ABI v5 gelu_zb)
    int act, accumulate;
    float alpha;
    int tiles_m, tiles_n;
    const float* sa; const float* sb;                   // fp8 operands: device scalars multiplied into alpha (the dequantisation factors)
};

TAV_DEV int swz(int row, int chunk) { return chunk ^ ((row >> 1) & 7); }

// TM = 16-row MFMA tiles per wave along M (2, 3 or 4); NW = waves per workgroup (4 or 8), arranged (NW/2) x 2, each wave a
// (16*TM) x 64 block: the workgroup tile is (8*TM*NW) x 128 = 64/96/128 x 128 (NW = 4) or 256 x 128 (NW = 8, TM = 4).
// The host picks the shape per launch:
//  * the kernel is bound by what one CU can pull from L2 into LDS (~70-90 GB/s per CU measured: 4096^3 tops out at 1.15 PF
//    with 128x128 tiles = 64 FLOP per staged byte, and a deeper ring at equal occupancy changes nothing), so the 256x128 tile
//    (85 FLOP/B, one 8-wave workgroup per CU) is faster wherever its coarser tile grid still fills the chip;
//  * the tile count must divide well over the 256 CUs (M = 11712, N = 768: 552 tiles of 128 rows leave 28 % of the chip idle in
//    the last round, 732 tiles of 96 rows do not) and small-M problems must still produce enough workgroups.
enum { NT_GEN = 0, NT_PLAIN = 1, NT_RESID = 2, NT_GELU_D = 3, NT_MUL_D = 4 };   // epilogue flavours (see the epilogue)
template <typename T, typename TO, int TM, int NST, int NW, int TNW, int EPI = NT_GEN>
__global__ __launch_bounds__(64 * NW, NW == 4 ? 2 : 1) __attribute__((amdgpu_waves_per_eu(2, 2))) void gemm_nt_kernel(const GemmNT p) {
    constexpr int ES = ET<T>::ES;
    constexpr bool F8 = std::is_same<T, fp8>::value;      // e4m3 operands: 128 k-values per 128-byte K-tile, one block-scaled MFMA per 16x16 tile
    using TS = typename std::conditional<F8, bf16, T>::type;   // dtype of the epilogue's side input / activation flavour
    constexpr int BM = 8 * TM * NW, BN = 32 * TNW;        // TNW = 16-column MFMA tiles per wave along N (4: BN = 128, 8: BN = 256)
    constexpr int PB = BN / 8 / NW;                       // DMA pieces of the B image per wave (the A image: TM per wave)
    constexpr int NP = TM + PB;                           // DMA pieces per wave per K-tile
    constexpr int TILE_A = BM * 128, TILE_B = BN * 128;   // bytes per K-tile image
    // R25 (256 x 256 tile): the 160 KB of LDS hold FIVE 32 KB images -- three A slots and two B slots.  With two whole K-tile slots a DMA must
    // be issued and land within ONE K-tile time and the ring is empty at every wait (the loop then runs at issue + round trip per K-tile: the
    // MFMA-free build takes as long as the full one).  With the fifth image, A(kt+2) is issued while tile kt is multiplied: one image is still
    // in flight at every wait, B(kt+1) goes out first in the iteration (most of a K-tile time to land), A(kt+2) has a K-tile time more.
    constexpr bool R25 = NW == 8 && TNW == 8 && NST == 2 && !F8 && ES == 2;
    constexpr int NSA = R25 ? 3 : NST;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* sA = smem;                  // [NSA][BM][128B]  activations (m)
    char* sB = smem + NSA * TILE_A;   // [NST][BN][128B]  weights (n)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, i = lane & 15;
    const int wm = wave >> 1, wn = wave & 1;

    // tile order: XCD band (xcd_remap), then super-tiles of GROUP_M m-tiles walked m-fastest (L2 locality)
    constexpr int GROUP_M = 8;
    const int tile = xcd_remap(blockIdx.x, p.tiles_m * p.tiles_n);
    const int gsz = GROUP_M * p.tiles_n;
    const int first_m = (tile / gsz) * GROUP_M;
    const int gm = (p.tiles_m - first_m) < GROUP_M ? (p.tiles_m - first_m) : GROUP_M;
    const int rem = tile % gsz;
    // (uniform integer divisions run on the VALU; to_sgpr pins their results -- and every address derived from them -- back to SGPRs)
    const int tm_idx = to_sgpr(first_m + rem % gm), tn_idx = to_sgpr(rem / gm);
    const int m0 = tm_idx * BM, n0 = tn_idx * BN;
    const int z = blockIdx.y, zb = to_sgpr(z / p.nzg), zg = z - zb * p.nzg;

    const char* Ab = p.A + (zb * p.a_zb + zg * p.a_zg) * ES;
    const char* Bb = p.B + (zb * p.b_zb + zg * p.b_zg) * ES;
    // LDS-DMA staging (global_load_lds_dwordx4): one wave instruction fills 64 consecutive 16-B slots = 8 rows x 8 chunk
    // slots of the image; the LDS side is linear (wave-uniform base + lane*16), so the XOR swizzle is applied to the SOURCE
    // chunk each lane fetches.  Wave w stages rows [8*TM*w, +8*TM) of A and [8*PB*w, +8*PB) of B.
    const int lr = lane >> 3, lc = lane & 7;
    // per-lane 32-bit byte offsets from the wave-uniform operand bases (the host checks M*lda and N*ldb fit): advancing a
    // K-tile is one v_add_u32 per DMA instruction
    unsigned ga[TM], gb[PB];
#pragma unroll
    for (int j = 0; j < TM; ++j) {
        const int r = wave * 8 * TM + j * 8 + lr;
        int ra = m0 + r; ra = ra < p.M ? ra : p.M - 1;
        ga[j] = (unsigned)((long)ra * p.lda * ES + swz(r, lc) * 16);     // slot lc of row r holds chunk lc ^ f(r)
    }
#pragma unroll
    for (int j = 0; j < PB; ++j) {
        const int r = wave * 8 * PB + j * 8 + lr;
        int rb = n0 + r; rb = rb < p.N ? rb : p.N - 1;
        gb[j] = (unsigned)((long)rb * p.ldb * ES + swz(r, lc) * 16);
    }
    const unsigned ldsA = __builtin_amdgcn_readfirstlane(lds_addr(sA) + wave * 8 * TM * 128);
    const unsigned ldsB = __builtin_amdgcn_readfirstlane(lds_addr(sB) + wave * 8 * PB * 128);
    // piece pc of the next K-tile image: TM pieces of A, then PB of B.  The K offset rides on the SCALAR operand base (one 64-bit scalar add
    // per operand and K-tile); the lane offsets ga / gb never change, so a piece is {scalar add for the LDS address, M0, nop, DMA}.
    auto stage_a = [&](int j, unsigned ko, int buf) { glds16_m0(Ab + ko, ga[j], ldsA + buf * TILE_A + j * 1024); };
    auto stage_b = [&](int j, unsigned ko, int buf) { glds16_m0(Bb + ko, gb[j], ldsB + buf * TILE_B + j * 1024); };
    auto stage_piece = [&](int pc, unsigned ko, int buf) {
        if (pc < TM) stage_a(pc, ko, buf);
        else stage_b(pc - TM, ko, buf);
    };

    f32x4 acc[TNW][TM];  // [tn][tm]
#pragma unroll
    for (int a = 0; a < TNW; ++a)
#pragma unroll
        for (int b = 0; b < TM; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nk = p.K * ES / 128;
    int off_a[2][TM], off_b[2][TNW];
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
#pragma unroll
        for (int t = 0; t < TM; ++t) { const int r = wm * 16 * TM + t * 16 + i; off_a[s2][t] = r * 128 + swz(r, 4 * s2 + g) * 16; }
#pragma unroll
        for (int t = 0; t < TNW; ++t) { const int r = wn * 16 * TNW + t * 16 + i; off_b[s2][t] = r * 128 + swz(r, 4 * s2 + g) * 16; }
    }
    uint4 fa0[TM], fb0[TNW], fa1[TM], fb1[TNW];
    // One K-tile: wait for the image, read both fragment sets, then the MFMAs.  The TM+4 DMA pieces of the NEXT image are
    // issued between the MFMA groups of the first fragment set (a DMA costs the issuing wave 60-180 cycles of issue time;
    // spread out they run under the matrix pipe, and the second set's MFMAs give them time to land before the next wait).
    // NST-deep ring: while tile kt is multiplied, tiles kt+1 .. kt+NST-2 are in flight and tile kt+NST-1 is being issued, so a
    // DMA has NST-1 tile times to land (an L2 hit takes longer than one 128x128x64 tile's MFMAs).  vmcnt counts in issue
    // order: tile kt has landed once at most (NST-2) younger tiles x NP pieces are outstanding.
    auto ktile = [&](int kt, int cur, auto prefetch) {
        if constexpr (decltype(prefetch)::value) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NST - 2) * NP) : "memory");
        else wait_vmcnt0();                                 // tail: fewer tiles in flight than the constant assumes
        __syncthreads();                                    // everybody's pieces landed; the buffer refilled below is no longer read
        const char* cA = sA + cur * TILE_A;
        const char* cB = sB + cur * TILE_B;
        const unsigned ko = (unsigned)(kt + NST - 1) * 128u;
        const int nxt = (cur + NST - 1) % NST;
#pragma unroll
        for (int t = 0; t < TM; ++t) fa0[t] = *reinterpret_cast<const uint4*>(cA + off_a[0][t]);
#pragma unroll
        for (int t = 0; t < TNW; ++t) fb0[t] = *reinterpret_cast<const uint4*>(cB + off_b[0][t]);
#pragma unroll
        for (int t = 0; t < TM; ++t) fa1[t] = *reinterpret_cast<const uint4*>(cA + off_a[1][t]);
#pragma unroll
        for (int t = 0; t < TNW; ++t) fb1[t] = *reinterpret_cast<const uint4*>(cB + off_b[1][t]);
        __builtin_amdgcn_sched_barrier(0);                  // keep all 16 fragment reads in flight ahead of the MFMAs
#pragma unroll
        for (int tn = 0; tn < TNW; ++tn) {
#pragma unroll
            for (int tm = 0; tm < TM; ++tm) {
                if constexpr (F8) mma16_fp8(fb0[tn], fb1[tn], fa0[tm], fa1[tm], acc[tn][tm]);
                else mma16<T>(fb0[tn], fa0[tm], acc[tn][tm]);
            }
            if constexpr (decltype(prefetch)::value) {
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int pc = tn * NP / TNW; pc < (tn + 1) * NP / TNW; ++pc) stage_piece(pc, ko, nxt);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if constexpr (!F8) {
#pragma unroll
            for (int tn = 0; tn < TNW; ++tn)
#pragma unroll
                for (int tm = 0; tm < TM; ++tm) mma16<T>(fb1[tn], fa1[tm], acc[tn][tm]);
        }
    };
    // R25 iteration: ISSUE_B = B(kt+1) goes out (kt + 1 < nk), ISSUE_A = A(kt+2) goes out (kt + 2 < nk).  Issue order per iteration: B(kt+1),
    // then A(kt+2); at the next wait the TM youngest pieces are exactly A(kt+2)'s and may stay in flight.
    // (cl / cs: current slot of A (three slots) / of B (two slots); issue_s: B's image of tile kt+1 goes out, issue_l: A's image of tile kt+2)
    auto ktile25 = [&](int kt, int cl, int cs, auto issue_s, auto issue_l) {
        constexpr bool IS = decltype(issue_s)::value, IL = decltype(issue_l)::value;
        if constexpr (IS) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(TM) : "memory");   // A(kt+1) was issued after B(kt): it may still fly
        else wait_vmcnt0();
        __syncthreads();
        const char* cA = sA + cl * TILE_A;
        const char* cB = sB + cs * TILE_B;
        const int nl = cl == 0 ? 2 : cl - 1;                  // slot of A(kt-1) = slot of A(kt+2)
        const int ns = cs ^ 1;
#pragma unroll
        for (int t = 0; t < TM; ++t) fa0[t] = *reinterpret_cast<const uint4*>(cA + off_a[0][t]);
#pragma unroll
        for (int t = 0; t < TNW; ++t) fb0[t] = *reinterpret_cast<const uint4*>(cB + off_b[0][t]);
#pragma unroll
        for (int t = 0; t < TM; ++t) fa1[t] = *reinterpret_cast<const uint4*>(cA + off_a[1][t]);
#pragma unroll
        for (int t = 0; t < TNW; ++t) fb1[t] = *reinterpret_cast<const uint4*>(cB + off_b[1][t]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int tn = 0; tn < TNW; ++tn) {
#pragma unroll
            for (int tm = 0; tm < TM; ++tm) mma16<T>(fb0[tn], fa0[tm], acc[tn][tm]);
            if constexpr (IS || IL) {
                __builtin_amdgcn_sched_barrier(0);
                // one piece per MFMA group: B's PB pieces first, then A's TM
                if constexpr (IS) {
                    if (tn < PB) stage_b(tn, (unsigned)(kt + 1) * 128u, ns);
                }
                if constexpr (IL) {
                    if (tn >= PB && tn - PB < TM) stage_a(tn - PB, (unsigned)(kt + 2) * 128u, nl);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
#pragma unroll
        for (int tn = 0; tn < TNW; ++tn)
#pragma unroll
            for (int tm = 0; tm < TM; ++tm) mma16<T>(fb1[tn], fa1[tm], acc[tn][tm]);
    };
    if constexpr (R25) {
        static_assert(!R25 || PB + TM <= TNW, "one DMA piece per MFMA group");
        auto stage_l = [&](unsigned ko, int slot) {
#pragma unroll
            for (int j = 0; j < TM; ++j) stage_a(j, ko, slot);
        };
        auto stage_s = [&](unsigned ko, int slot) {
#pragma unroll
            for (int j = 0; j < PB; ++j) stage_b(j, ko, slot);
        };
        stage_l(0u, 0);
        stage_s(0u, 0);
        if (nk > 1) stage_l(128u, 1);
        int cl = 0, cs = 0, kt = 0;
        for (; kt + 2 < nk; ++kt) { ktile25(kt, cl, cs, std::true_type{}, std::true_type{}); cl = cl == 2 ? 0 : cl + 1; cs ^= 1; }
        if (kt + 1 < nk) { ktile25(kt, cl, cs, std::true_type{}, std::false_type{}); cl = cl == 2 ? 0 : cl + 1; cs ^= 1; ++kt; }
        if (kt < nk) ktile25(kt, cl, cs, std::false_type{}, std::false_type{});
    } else {
#pragma unroll
    for (int t = 0; t < NST - 1; ++t)
        if (t < nk) {
#pragma unroll
            for (int pc = 0; pc < NP; ++pc) stage_piece(pc, (unsigned)t * 128u, t);
        }
    int cur = 0;
    int kt = 0;
    for (; kt + NST - 1 < nk; ++kt) { ktile(kt, cur, std::true_type{}); cur = cur + 1 == NST ? 0 : cur + 1; }
    for (; kt < nk; ++kt) { ktile(kt, cur, std::false_type{}); cur = cur + 1 == NST ? 0 : cur + 1; }
    }

    // ---- epilogue.  Lane (g,i) holds C[m = .. + i][n = .. + 4g + r]: storing from that layout gives 32-B row segments and
    // uncoalesced residual reads.  Instead the f32 accumulator tile goes through the (now idle) staging LDS -- one ds_write_b128
    // per 16x16 tile, 16-B chunks XOR-swizzled with the row so both the writes and the row-major reads are conflict free -- and
    // the epilogue runs row-major: 32 threads per row, 16 B per thread, every global access a full 512-B (f32) / 256-B (bf16) run.
    __syncthreads();                                       // all waves finished reading the operand images
    float* sC = reinterpret_cast<float*>(smem);            // [EP_ROWS][BN] f32 inside the (now idle) staging buffers
    constexpr int ROWB_C = BN * 4;                          // bytes per staged row
    constexpr int CPR = BN / 4;                             // 16-B chunks per row (32 / 64)
    constexpr int LDS_BYTES = NST * (TILE_A + TILE_B);
    constexpr int EP_ROWS = (LDS_BYTES / ROWB_C) < BM ? (LDS_BYTES / ROWB_C) / (16 * TM) * (16 * TM) : BM;   // rows per pass: whole wave-row bands
    constexpr int NPASS = BM / EP_ROWS;
    static_assert(EP_ROWS >= 16 * TM && BM % EP_ROWS == 0, "epilogue staging");
    const long coff = zb * p.c_zb + zg * p.c_zg;
    TO* C = reinterpret_cast<TO*>(p.C) + coff;
    TO* Cpre = p.Cpre ? reinterpret_cast<TO*>(p.Cpre) + coff : nullptr;
    const TS* Gin = p.gelu_in ? reinterpret_cast<const TS*>(p.gelu_in) + (zb * p.g_zb + zg * p.c_zg) : nullptr;
    const float alpha = p.alpha * (p.sa ? *p.sa : 1.f) * (p.sb ? *p.sb : 1.f);
    const float* R = p.resid ? p.resid + coff : nullptr;
    // What the epilogue does is a launch-time constant.  EPI = NT_GEN reads it from the arguments (any combination); the four flavours the
    // transformer layers use are compiled as straight-line code (the generic loop spends more issue slots on uniform branches than on the
    // data: with two waves per SIMD and the matrix pipe idle, the epilogue of a 256 x 256 tile is VALU-issue bound).
    constexpr bool GEN = EPI == NT_GEN;
    const bool f_resid = GEN ? (R != nullptr) : (EPI == NT_RESID);                    // + f32 residual
    const bool f_pre = GEN ? (Cpre != nullptr && !(p.act & 2)) : false;                // second output: the pre-activation
    const bool f_act3 = GEN ? ((p.act & 3) == 3) : (EPI == NT_GELU_D);                 // GELU out, gelu' to the second output
    const bool f_gelu = GEN ? ((p.act & 3) == 1) : false;                              // GELU out only
    const bool f_gin = GEN ? (Gin != nullptr) : (EPI == NT_MUL_D);                     // multiply by gelu'(side input)
    const bool f_gin_d = GEN ? ((p.act & 4) != 0) : true;                              // ... which already is the derivative
    const bool f_acc = GEN ? (p.accumulate != 0) : false;
    const int ch = tid % CPR, rr = tid / CPR;              // this thread's 16-B column chunk (fixed) and row within an iteration
    constexpr int RPI = 64 * NW / CPR;                      // rows per iteration of the store loop
    const int n = n0 + 4 * ch;
    f32x4 bv = {0.f, 0.f, 0.f, 0.f};
    if (n < p.N && p.bias) bv = ld4(p.bias + zg * p.bias_zg + n);
    constexpr int NIT = EP_ROWS / RPI;                      // rows per thread and pass (<= 16)
    static_assert(EP_ROWS % RPI == 0 && NIT <= 16, "epilogue rows per thread");
    const bool interior = m0 + BM <= p.M && n0 + BN <= p.N; // no bounds checks inside (all but the last row / column of tiles)
    // Side inputs of a pass (f32 residual, gelu' for the dgrad, or C itself when accumulating) are requested BEFORE the accumulators are
    // staged: their HBM/L2 latency then runs under the LDS writes and the barrier instead of in front of every store (the fragment
    // registers of the main loop are dead by now).  One flavour per launch; the rare combinations load inside the store loop.
    // Requests in flight per thread.  vmcnt retires in issue order, so with a rolling prefetch every wait for a side value also waits for
    // the STORES issued before it (their write acknowledgements), and the loop runs at "depth" accesses per memory round trip.  The gelu'
    // side input takes two registers per row: all of a pass's rows are requested up front, every load is older than every store and the
    // loop never waits on a store.  The f32 residual takes four (16 x 4 registers on top of the accumulators would spill): depth 8.
    constexpr int PD = (EPI == NT_MUL_D) ? NIT : (NIT > 8 ? 8 : NIT);
    constexpr bool EARLY = (TNW == 4);                      // ... and no registers to spare while they are
    const bool pre_r = f_resid, pre_g = !pre_r && f_gin && sizeof(TS) == 2, pre_c = !pre_r && !pre_g && f_acc && sizeof(TO) == 4;
    const bool any_side = pre_r || pre_c || pre_g;
    // Addresses: a wave-uniform 64-bit base (the tile's first row, SGPRs) + a 32-bit per-thread BYTE offset that advances by a uniform
    // step per row iteration: the global_load/store "saddr + voffset" form, one v_add per access.  (long)m * ld + n per access costs two
    // quarter-rate 32-bit multiplies and a 64-bit multiply-add per address, which made the address arithmetic the largest part of the
    // loop.  The host checks that a tile's offsets fit 32 bits.
    char* const Cb = reinterpret_cast<char*>(C + (long)m0 * p.ldc);
    char* const Pb = Cpre ? reinterpret_cast<char*>(Cpre + (long)m0 * p.ld_pre) : nullptr;
    const char* const Gb = Gin ? reinterpret_cast<const char*>(Gin + (long)m0 * p.ld_gelu) : nullptr;
    const char* const Rb = R ? reinterpret_cast<const char*>(R + (long)m0 * p.ld_resid) : nullptr;
    const unsigned s_c = RPI * (unsigned)p.ldc * sizeof(TO), s_p = RPI * (unsigned)p.ld_pre * sizeof(TO);
    const unsigned s_g = RPI * (unsigned)p.ld_gelu * sizeof(TS), s_r = RPI * (unsigned)p.ld_resid * 4u;
    auto run_pass = [&](int row_lo, auto full_tag) __attribute__((always_inline)) {
        constexpr bool FULL = decltype(full_tag)::value;
        const unsigned row = (unsigned)(row_lo + rr);        // (offsets depend on the pass: nothing for the compiler to hoist and keep live)
        const unsigned o_c = (row * (unsigned)p.ldc + (unsigned)n) * (unsigned)sizeof(TO), o_p = (row * (unsigned)p.ld_pre + (unsigned)n) * (unsigned)sizeof(TO);
        const unsigned o_g = (row * (unsigned)p.ld_gelu + (unsigned)n) * (unsigned)sizeof(TS), o_r = (row * (unsigned)p.ld_resid + (unsigned)n) * 4u;
        f32x4 side[PD];                                     // (gelu' side input: two packed words in .x/.y)
        auto side_load = [&](int it) __attribute__((always_inline)) -> f32x4 {
            const int m = m0 + row_lo + rr + it * RPI;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (FULL || (n < p.N && m < p.M)) {
                if (pre_r) v = ld4(reinterpret_cast<const float*>(Rb + (o_r + it * s_r)));
                else if (pre_c) { if constexpr (sizeof(TO) == 4) v = ld4(reinterpret_cast<const float*>(Cb + (o_c + it * s_c))); }
                else if (pre_g) {
                    const uint2 w = *reinterpret_cast<const uint2*>(Gb + (o_g + it * s_g));
                    v[0] = __uint_as_float(w.x);
                    v[1] = __uint_as_float(w.y);
                }
            }
            return v;
        };
        auto side_loads = [&]() __attribute__((always_inline)) {
            if (!any_side) return;
#pragma unroll
            for (int it = 0; it < PD; ++it) side[it] = side_load(it);
        };
        if constexpr (EARLY) side_loads();
        if (wm * 16 * TM >= row_lo && wm * 16 * TM < row_lo + EP_ROWS) {
#pragma unroll
            for (int tm = 0; tm < TM; ++tm) {
                const int r = wm * 16 * TM + tm * 16 + i - row_lo;
#pragma unroll
                for (int tn = 0; tn < TNW; ++tn) {
                    const int cc = wn * 4 * TNW + tn * 4 + g;
                    *reinterpret_cast<f32x4*>(reinterpret_cast<char*>(sC) + r * ROWB_C + ((cc ^ (r & 31)) << 4)) = acc[tn][tm];
                }
            }
        }
        if constexpr (!EARLY) side_loads();                 // staged accumulators are dead: the requests fly across the barrier
        __syncthreads();
        if (FULL || n < p.N) {
            auto staged = [&](int it) __attribute__((always_inline)) -> f32x4 {
                const int r = rr + it * RPI;
                return *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(sC) + r * ROWB_C + ((ch ^ (r & 31)) << 4));
            };
            f32x4 v_next = staged(0);                           // the staged row is read one iteration ahead of its use
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int r = rr + it * RPI;
                const int m = m0 + row_lo + r;
                const f32x4 sv = side[it % PD];
                if constexpr (PD < NIT) { if (it + PD < NIT && any_side) side[it % PD] = side_load(it + PD); }
                f32x4 v = v_next;
                if (it + 1 < NIT) v_next = staged(it + 1);
                if (FULL || m < p.M) {
                    v = v * alpha + bv;
                    if (f_pre) st4(reinterpret_cast<TO*>(Pb + (o_p + it * s_p)), v);
                    if (f_act3) {                               // GELU out, gelu' to C_pre
                        f32x4 d, y4;
                        gelu_both4_t<TS>(v, y4, d);
                        v = y4;
                        if (GEN ? Cpre != nullptr : true) st4(reinterpret_cast<TO*>(Pb + (o_p + it * s_p)), d);
                    } else if (f_gelu) { v[0] = gelu_t<TS>(v[0]); v[1] = gelu_t<TS>(v[1]); v[2] = gelu_t<TS>(v[2]); v[3] = gelu_t<TS>(v[3]); }
                    if (f_gin) {
                        f32x4 u;
                        if (pre_g) {
                            const uint32_t w0 = __float_as_uint(sv[0]), w1 = __float_as_uint(sv[1]);
                            u = f32x4{bf16_bits_to_f32(w0 & 0xffffu), bf16_bits_to_f32(w0 >> 16), bf16_bits_to_f32(w1 & 0xffffu), bf16_bits_to_f32(w1 >> 16)};
                        }
                        else u = ld4(reinterpret_cast<const TS*>(Gb + (o_g + it * s_g)));
                        if (f_gin_d) v *= u;                    // the side input already is gelu'(pre-activation)
                        else { v[0] *= gelu_grad_t<TS>(u[0]); v[1] *= gelu_grad_t<TS>(u[1]); v[2] *= gelu_grad_t<TS>(u[2]); v[3] *= gelu_grad_t<TS>(u[3]); }
                    }
                    if (pre_r) v += sv;
                    if (f_acc) {
                        if (pre_c) v += sv;
                        else v += ld4(reinterpret_cast<const TO*>(Cb + (o_c + it * s_c)));
                    }
                    st4(reinterpret_cast<TO*>(Cb + (o_c + it * s_c)), v);
                }
            }
        }
    };
    if constexpr (GEN) {
#pragma unroll 1
        for (int pass = 0; pass < NPASS; ++pass) {          // (one copy: the generic epilogue is large enough)
            if (pass) __syncthreads();                      // the previous pass has been stored
            run_pass(pass * EP_ROWS, std::false_type{});
        }
    } else {
        // passes unrolled: inside a loop the waitcnt pass merges the pending-load state at the header and protects the first reuse of a
        // side register with s_waitcnt vmcnt(0) -- which also waits for every STORE of the previous pass to be acknowledged
        if (interior) {
#pragma unroll
            for (int pass = 0; pass < NPASS; ++pass) {
                if (pass) __syncthreads();
                run_pass(pass * EP_ROWS, std::true_type{});
            }
        } else {
#pragma unroll
            for (int pass = 0; pass < NPASS; ++pass) {
                if (pass) __syncthreads();
                run_pass(pass * EP_ROWS, std::false_type{});
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
struct GemmTN {
    const char* A; const char* B; float* S;   // S: slabs [nsplit][N1][N2] fp32
    float* bias_part;       // optional column sums of A (the bias gradient): [nsplit][N1] written by the t2 == 0 tiles, or -- bias_spread --
                            // [nsplit][tiles_2][N1]: tile (t1, t2) sums the K-tiles with kt % tiles_2 == t2, so the work is shared by a tile row
    int bias_spread;
    int N1, N2;
    long lda, ldb;          // row strides (elements) of the token-major operands
    int rows_per_batch;     // T: tokens per batch entry (reduction axis = nbatch * T)
    long a_zb, b_zb;        // batch strides (elements)
    int chunk_rows;         // tokens per split (multiple of 64)
    int chunks_per_batch;
    int tiles_1, tiles_2;
};

// LDS image of one TN operand tile: [64 tokens][128 features] in natural order, 16-B chunks XOR-swizzled per row so the
// token rows one half-wave touches in a single transposed read fall into different bank windows:
//   bf16 (ds_read_b64_tr_b16, 8 rows x 32 B, 64 banks): chunk ^ ((row & 7) << 1)  -> 8 distinct 32-B windows of 256 B
//   f32  (ds_read_b32, 2 rows x 64 B, 32 banks)       : chunk ^ (((row >> 2) & 1) << 2) -> the two rows 64 B apart
// The image is linear per wave instruction, so it is filled by LDS-DMA with the swizzle applied to the source chunk.
template <typename T> struct TNTile {
    static constexpr int ES = ET<T>::ES, ROWB = 128 * ES, CPR = ROWB / 16;
    static TAV_DEV int sw(int row, int chunk) { return ES == 2 ? (chunk ^ ((row & 7) << 1)) : (chunk ^ (((row >> 2) & 1) << 2)); }
};
template <typename T> TAV_DEV uint4 tn_frag(const char* tile, int krow0, int col0, int lane);
template <> TAV_DEV uint4 tn_frag<bf16>(const char* tile, int krow0, int col0, int lane) {
    using TT = TNTile<bf16>;
    const int g = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3;
    const int r0 = krow0 + 4 * g + q, r1 = r0 + 16;
    const int cb = (col0 + 4 * p) * 2;                         // byte column of this lane's 4 elements
    const char* a0 = tile + r0 * TT::ROWB + (TT::sw(r0, cb >> 4) << 4) + (cb & 15);
    const char* a1 = tile + r1 * TT::ROWB + (TT::sw(r1, cb >> 4) << 4) + (cb & 15);
    const uint2 lo = lds_read_tr16(a0), hi = lds_read_tr16(a1);
    return make_uint4(lo.x, lo.y, hi.x, hi.y);
}
template <> TAV_DEV uint4 tn_frag<float>(const char* tile, int krow0, int col0, int lane) {
    using TT = TNTile<float>;
    const int g = lane >> 4, i = lane & 15;
    const int cb = (col0 + i) * 4;
    uint4 r;
    uint32_t* rr = reinterpret_cast<uint32_t*>(&r);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int row = krow0 + 4 * g + t;
        rr[t] = *reinterpret_cast<const uint32_t*>(tile + row * TT::ROWB + (TT::sw(row, cb >> 4) << 4) + (cb & 15));
    }
    return r;
}

// K-tile and ring depth (64 tokens, two buffers, for both dtypes).  A deeper ring of shorter tiles at the same LDS budget (32 tokens x 4 buffers,
// three tiles in flight) was tried on the theory that a workgroup's K-tile period is one DMA round trip: it is not -- that variant pays
// twice the barriers and ran 17 % slower (profiles/r02_experiments.md).
// Bias gradients (column sums of dY) on the matrix pipe: one extra MFMA per 16-column dY fragment with an all-ones first operand gives the
// column sums of that fragment's K-step in every accumulator row -- the dY fragments are in registers anyway, so the sums cost no LDS reads
// (rounds 1-3 read 32 two-byte LDS values per thread and K-tile: 16-33 us of every layer's launch).  f32 accumulation of exact products.
template <typename T> TAV_DEV uint4 ones_frag();
template <> TAV_DEV uint4 ones_frag<bf16>() { return make_uint4(0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u); }
template <> TAV_DEV uint4 ones_frag<float>() { return make_uint4(0x3f800000u, 0x3f800000u, 0x3f800000u, 0x3f800000u); }

template <typename T> struct TNShape { static constexpr int KT = 64, NST = 2; };

template <typename T>
TAV_DEV void gemm_tn_body(const GemmTN& p, const int tile, const int split) {
    using TT = TNTile<T>;
    constexpr int ES = ET<T>::ES, PK = ET<T>::PK, KSTEP = ET<T>::KSTEP;
    constexpr int BT = 128, KT = TNShape<T>::KT, NST = TNShape<T>::NST;
    constexpr int ROWB = TT::ROWB, CPR = TT::CPR;           // 256 B / 16 chunks (bf16), 512 B / 32 chunks (f32)
    constexpr int TILE_BYTES = KT * ROWB;
    constexpr int RPI = 64 / CPR;                           // token rows per wave instruction (4 / 2)
    constexpr int WROWS = KT / 4;                           // token rows of a K-tile staged by one wave
    constexpr int NINST = WROWS / RPI;                      // DMA instructions per wave per operand per K-tile
    static_assert(KT % KSTEP == 0 && WROWS % RPI == 0 && NINST >= 1, "TN tile shape");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* sA = smem;                      // [NST][KT][ROWB]  dY  (n1 along the row)
    char* sB = smem + NST * TILE_BYTES;   // [NST][KT][ROWB]  X   (n2 along the row)

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // (scalar: the w2 tests are branches, not masks)
    const int g = lane >> 4, i = lane & 15;
    const int w1 = wave >> 1, w2 = wave & 1;

    // consecutive tiles (same XCD, same L2) walk the SHORTER tile axis fastest: the panel of the other operand is reused at
    // once and the working set of re-read panels is min(tiles_1, tiles_2) x ~1 MB instead of the max (dW2: 24 -> 6 panels)
    int t1, t2;
    if (p.tiles_1 >= p.tiles_2) { t1 = tile / p.tiles_2; t2 = tile - t1 * p.tiles_2; }
    else { t2 = tile / p.tiles_1; t1 = tile - t2 * p.tiles_1; }
    const int n1_0 = t1 * BT, n2_0 = t2 * BT;
    const int zb = split / p.chunks_per_batch, ck = split - zb * p.chunks_per_batch;
    const int row_begin = ck * p.chunk_rows;
    int row_end = row_begin + p.chunk_rows; row_end = row_end < p.rows_per_batch ? row_end : p.rows_per_batch;

    const char* Ab = p.A + zb * p.a_zb * ES;
    const char* Bb = p.B + zb * p.b_zb * ES;

    // DMA geometry: wave w stages token rows [WROWS*w, +WROWS) of each K-tile; instruction j covers RPI rows; lane -> (row, slot)
    const int lrow = lane / CPR, lslot = lane % CPR;
    // Feature columns past N1/N2: the source chunk is clamped to chunk 0 (valid memory); those outputs are never stored.
    // Token rows past the split end would pollute the sums, so a ragged last K-tile is staged by ordinary loads with
    // zero fill instead of DMA (block-uniform branch, at most once per workgroup).
    const int a_cmax = (p.N1 - n1_0) * ES / 16, b_cmax = (p.N2 - n2_0) * ES / 16;   // valid chunks in this tile (may exceed CPR)

    f32x4 acc[4][4];  // [t1][t2]
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    // The column sums read 32 two-byte LDS values per thread and K-tile: on the t2 == 0 tiles alone they made those tiles (and with them the
    // launch) 7-30 % longer; spread over the tile row every tile pays 1/tiles_2 of it.
    const bool do_bias = p.bias_part != nullptr && (p.bias_spread || t2 == 0);
    const int bias_mod = p.bias_spread ? p.tiles_2 : 1, bias_rem = p.bias_spread ? t2 : 0;
    // the two waves that share a dY block (w2 = 0 / 1) take two of its four 16-column fragments each
    f32x4 bacc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    const uint4 ones = ones_frag<T>();

    const int nrows = row_end - row_begin;
    const int nk = (nrows + KT - 1) / KT;
    const unsigned ldsA = __builtin_amdgcn_readfirstlane(lds_addr(sA) + wave * WROWS * ROWB);
    const unsigned ldsB = __builtin_amdgcn_readfirstlane(lds_addr(sB) + wave * WROWS * ROWB);
    // per-lane byte offsets of the wave's NINST source chunks in K-tile 0 (relative to the wave-uniform bases below); a K-tile
    // later is one scalar stride further, so staging costs one v_add_u32 per DMA instruction
    const char* Ab0 = Ab + ((long)row_begin * p.lda + n1_0) * ES;
    const char* Bb0 = Bb + ((long)row_begin * p.ldb + n2_0) * ES;
    unsigned offA[NINST], offB[NINST];
#pragma unroll
    for (int j = 0; j < NINST; ++j) {
        const int trow = wave * WROWS + j * RPI + lrow;            // row inside the K-tile
        int ca = TT::sw(trow, lslot); ca = ca < a_cmax ? ca : 0;
        int cb = TT::sw(trow, lslot); cb = cb < b_cmax ? cb : 0;
        offA[j] = (unsigned)(trow * p.lda * ES + ca * 16);
        offB[j] = (unsigned)(trow * p.ldb * ES + cb * 16);
    }
    const unsigned strideA = (unsigned)(KT * p.lda * ES), strideB = (unsigned)(KT * p.ldb * ES);
    // A whole K-tile goes by LDS-DMA: exactly 2 * NINST vector-memory instructions per wave (the counted waits below rely on it).  The
    // ragged tile -- always the LAST one -- goes through registers and is complete when stage_ragged() returns.
    auto stage = [&](int kt, int buf) {
        const unsigned ka = kt * strideA, kb = kt * strideB;
#pragma unroll
        for (int j = 0; j < NINST; ++j) {
            glds16_m0(Ab0 + ka, offA[j], ldsA + buf * TILE_BYTES + j * 1024);      // (K offset on the scalar base, no M0 save / restore: common.h)
            glds16_m0(Bb0 + kb, offB[j], ldsB + buf * TILE_BYTES + j * 1024);
        }
    };
    auto stage_ragged = [&](int kt, int buf) {                  // ordinary loads, zero fill
        const int base_row = row_begin + kt * KT + wave * WROWS;
#pragma unroll 1
        for (int j = 0; j < NINST; ++j) {
            const int r = j * RPI + lrow;
            const int trow = wave * WROWS + r;
            const int ca = TT::sw(trow, lslot), cb = TT::sw(trow, lslot);
            const bool ok = (kt * KT + trow) < nrows;
            uint4 va = make_uint4(0, 0, 0, 0), vb = va;
            if (ok && ca < a_cmax) va = *reinterpret_cast<const uint4*>(Ab + ((long)(base_row + r) * p.lda + n1_0) * ES + ca * 16);
            if (ok && cb < b_cmax) vb = *reinterpret_cast<const uint4*>(Bb + ((long)(base_row + r) * p.ldb + n2_0) * ES + cb * 16);
            *reinterpret_cast<uint4*>(sA + buf * TILE_BYTES + trow * ROWB + lslot * 16) = va;
            *reinterpret_cast<uint4*>(sB + buf * TILE_BYTES + trow * ROWB + lslot * 16) = vb;
        }
    };
    // bias_cnt: K-tiles until the next one whose column sums this tile takes (kt % bias_mod == bias_rem without the division)
    int bias_cnt = bias_rem;
    auto compute = [&](int cur) {
        const char* cA = sA + cur * TILE_BYTES;
        const char* cB = sB + cur * TILE_BYTES;
        const bool bias_now = do_bias && bias_cnt == 0;
        bias_cnt = bias_cnt == 0 ? bias_mod - 1 : bias_cnt - 1;
        // bf16: both k-steps' fragments (64 registers) are requested before the K-tile's first MFMA; f32 (four k-steps): one at a time
        constexpr int NS = KT / KSTEP, G = ES == 2 ? NS : 1;
#pragma unroll
        for (int s0 = 0; s0 < NS; s0 += G) {
            uint4 f1[G][4], f2[G][4];
#pragma unroll
            for (int s = 0; s < G; ++s)
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    f1[s][t] = tn_frag<T>(cA, (s0 + s) * KSTEP, w1 * 64 + t * 16, lane);
                    f2[s][t] = tn_frag<T>(cB, (s0 + s) * KSTEP, w2 * 64 + t * 16, lane);
                }
#pragma unroll
            for (int s = 0; s < G; ++s) {
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b) mma16<T>(f2[s][b], f1[s][a], acc[a][b]);   // rows(regs) = n2, cols(lanes) = n1
                if (bias_now) {                                  // (block-uniform; w2 wave-uniform)
                    if (w2 == 0) { mma16<T>(ones, f1[s][0], bacc[0]); mma16<T>(ones, f1[s][1], bacc[1]); }
                    else { mma16<T>(ones, f1[s][2], bacc[0]); mma16<T>(ones, f1[s][3], bacc[1]); }
                }
            }
        }
    };

    // NST-deep ring: while tile kt is multiplied, tiles kt+1 .. kt+NST-2 are in flight and tile kt+NST-1 is issued right after the
    // barrier (its buffer held tile kt-1, which every wave has finished).  vmcnt retires in issue order: tile kt has landed once at
    // most (NST-2) younger tiles x 2*NINST instructions are outstanding; the last NST-2 tiles (fewer in flight, possibly the ragged
    // one) wait for everything.  Whether the last tile is ragged is decided here, once: the steady loop stages whole tiles only.
    const int nd = nrows / KT;                                  // whole K-tiles: 0 .. nd-1 go by DMA, tile nd (if nk > nd) is the ragged one
#pragma unroll
    for (int t = 0; t < NST - 1; ++t)
        if (t < nk) { if (t < nd) stage(t, t); else stage_ragged(t, t); }
    int cur = 0, kt = 0;
    for (; kt + NST - 1 < nd; ++kt) {
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NST - 2) * 2 * NINST) : "memory");
        __syncthreads();
        stage(kt + NST - 1, cur == 0 ? NST - 1 : cur - 1);
        compute(cur);
        cur = cur + 1 == NST ? 0 : cur + 1;
    }
    if (kt + NST - 1 < nk) {                                    // the ragged tile's turn to be staged
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NST - 2) * 2 * NINST) : "memory");
        __syncthreads();
        stage_ragged(kt + NST - 1, cur == 0 ? NST - 1 : cur - 1);
        compute(cur);
        cur = cur + 1 == NST ? 0 : cur + 1;
        ++kt;
    }
    for (; kt < nk; ++kt) {
        wait_vmcnt0();
        __syncthreads();
        compute(cur);
        cur = cur + 1 == NST ? 0 : cur + 1;
    }
    __syncthreads();

    if (do_bias && g == 0) {                                 // every accumulator row holds the sums: lanes 0-15 (row 0) write them
        const long slot = p.bias_spread ? (long)split * p.tiles_2 + t2 : split;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int n1 = n1_0 + w1 * 64 + (2 * w2 + j) * 16 + i;
            if (n1 < p.N1) p.bias_part[slot * p.N1 + n1] = bacc[j][0];
        }
    }
    float* S = p.S + (long)split * p.N1 * p.N2;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int n1 = n1_0 + w1 * 64 + a * 16 + i;
        if (n1 >= p.N1) continue;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int n2 = n2_0 + w2 * 64 + b * 16 + 4 * g;
            if (n2 >= p.N2) continue;
            st4(S + (long)n1 * p.N2 + n2, acc[a][b]);
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256, 2) void gemm_tn_kernel(const GemmTN p) {
    gemm_tn_body<T>(p, xcd_remap(blockIdx.x, p.tiles_1 * p.tiles_2), blockIdx.y);
}

// Up to TN_GROUP_MAX weight gradients that share the token axis (one transformer layer: dWqkv, dWo, dW1, dW2) in ONE launch,
// each tile summing over ALL tokens: the layer's 432 tiles fill the chip on their own, so nothing is split over tokens -- no f32
// slabs, no reduce kernels, a quarter of the launches.  S / bias_part of each problem point at the final dW / db.
constexpr int TN_GROUP_MAX = 4;
struct GemmTNGroup {
    GemmTN p[TN_GROUP_MAX];
    int tile_end[TN_GROUP_MAX];     // prefix sums of tiles_1 * tiles_2
    int n;
};
template <typename T>
__global__ __launch_bounds__(256, 2) void gemm_tn_grouped_kernel(const GemmTNGroup grp) {
    const int t = xcd_remap(blockIdx.x, grp.tile_end[grp.n - 1]);
    int g = 0;
#pragma unroll
    for (int k = 0; k < TN_GROUP_MAX - 1; ++k) g += (k < grp.n - 1 && t >= grp.tile_end[k]) ? 1 : 0;
    const int first = g == 0 ? 0 : grp.tile_end[g - 1];
    gemm_tn_body<T>(grp.p[g], t - first, 0);
}

// ------------------------------------------------------------------------------------------------
// 256 x 256 weight-gradient tile (bf16): 8 waves as 4 (n1) x 2 (n2), each a 64 x 128 block = 4 x 8 accumulator tiles, one workgroup per
// CU.  128 FLOP per staged byte instead of 64: the 128-wide kernel is bound by the L2 -> LDS intake like its NT sibling.  The LDS image of
// a K-tile (64 tokens) is four [64][128-feature] sub-images in the layout of TNTile<bf16> (A half 0/1, B half 0/1, 16 KB each), so the
// transposed fragment reads are the same code; two stages = 128 KB.  A layer's four gradients are only 108 such tiles at width 768, so
// the token axis is split over blockIdx.y into f32 slabs (or straight into dW when one split suffices) and summed in fixed order.
template <typename T>
TAV_DEV void gemm_tn_big_body(const GemmTN& p, const int tile, const int split) {
    using TT = TNTile<T>;
    static_assert(ET<T>::ES == 2, "bf16 only");
    constexpr int ES = 2, KSTEP = ET<T>::KSTEP, KT = 64, ROWB = TT::ROWB;
    constexpr int SUB = KT * ROWB;                          // one [64][128] sub-image: 16 KB
    constexpr int STAGE = 4 * SUB;                          // A0 A1 B0 B1
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // (scalar: the w2 tests are branches, not masks)
    const int g = lane >> 4, i = lane & 15;
    const int w1 = wave >> 1, w2 = wave & 1;                // n1 block of 64 (0..3), n2 block of 128 (0..1)

    int t1, t2;
    if (p.tiles_1 >= p.tiles_2) { t1 = tile / p.tiles_2; t2 = tile - t1 * p.tiles_2; }
    else { t2 = tile / p.tiles_1; t1 = tile - t2 * p.tiles_1; }
    const int n1_0 = t1 * 256, n2_0 = t2 * 256;
    const int row_begin = split * p.chunk_rows;
    int row_end = row_begin + p.chunk_rows; row_end = row_end < p.rows_per_batch ? row_end : p.rows_per_batch;
    const int nrows = row_end - row_begin;
    const int nk = nrows > 0 ? (nrows + KT - 1) / KT : 0;

    // DMA geometry: wave w stages token rows [8w, 8w+8) of each sub-image, 4 rows (x 256 B) per instruction
    const int lrow = lane >> 4, lslot = lane & 15;
    const int a_cmax = (p.N1 - n1_0) * ES / 16, b_cmax = (p.N2 - n2_0) * ES / 16;   // valid 16-B chunks from the tile's first column
    const char* Ab0 = p.A + ((long)row_begin * p.lda + n1_0) * ES;
    const char* Bb0 = p.B + ((long)row_begin * p.ldb + n2_0) * ES;
    unsigned offA[2][2], offB[2][2];                        // [half][instruction]
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int trow = wave * 8 + j * 4 + lrow;
            int ca = 16 * h + TT::sw(trow, lslot); ca = ca < a_cmax ? ca : 0;      // columns past N1 / N2: any valid chunk (never stored)
            int cb = 16 * h + TT::sw(trow, lslot); cb = cb < b_cmax ? cb : 0;
            offA[h][j] = (unsigned)(trow * p.lda * ES + ca * 16);
            offB[h][j] = (unsigned)(trow * p.ldb * ES + cb * 16);
        }
    const unsigned strideA = (unsigned)(KT * p.lda * ES), strideB = (unsigned)(KT * p.ldb * ES);
    const unsigned lds0 = __builtin_amdgcn_readfirstlane(lds_addr(smem) + wave * 8 * ROWB);
    // LDS: FIVE 32 KB images (two [64][128] sub-images each) -- three dY slots and two X slots (the NT kernel's ring, see R25 there):
    // dY(kt+2) is issued while K-step 0 of tile kt is multiplied, X(kt+2) behind the barrier inside its K-step 1, which ends the reads of
    // X(kt)'s slot.  The sub-images are ordered [operand][half][slot]:
    // the ring slots of the half a wave reads lie SUB apart, so slot, K-step and 16-row offsets of a fragment read all fit the 16-bit offset
    // field of ds_read (dY: at most 2 * 16 KB + 12 KB).
    constexpr int NSA = 3, NSB = 2;
    constexpr int HALF_A = NSA * SUB, HALF_B = NSB * SUB;   // distance of an operand's halves 0 / 1
    constexpr int OFF_B = 2 * HALF_A;                       // X images behind the dY images
    // ragged last K-tile of one operand: ordinary loads, zero fill (block-uniform condition at the call sites)
    auto stage_ragged = [&](int kt, int slot, bool is_b) {
#pragma unroll 1
        for (int e = 0; e < 4; ++e) {
            const int h = e >> 1, j = e & 1;
            const int trow = wave * 8 + j * 4 + lrow;
            const int c = 16 * h + TT::sw(trow, lslot);
            const bool ok = (kt * KT + trow) < nrows;
            const long grow = (long)row_begin + kt * KT + trow;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (!is_b) { if (ok && c < a_cmax) v = *reinterpret_cast<const uint4*>(p.A + (grow * p.lda + n1_0) * ES + c * 16); }
            else { if (ok && c < b_cmax) v = *reinterpret_cast<const uint4*>(p.B + (grow * p.ldb + n2_0) * ES + c * 16); }
            *reinterpret_cast<uint4*>(smem + (is_b ? OFF_B + h * HALF_B : h * HALF_A) + slot * SUB + trow * ROWB + lslot * 16) = v;
        }
    };
    // piece pc (0..3 = [half][instruction]) of an operand's K-tile image by LDS-DMA
    auto piece_a = [&](int pc, unsigned ka, int slot) { glds16_m0(Ab0 + ka, offA[pc >> 1][pc & 1], lds0 + (pc >> 1) * HALF_A + slot * SUB + (pc & 1) * 1024); };
    auto piece_b = [&](int pc, unsigned kb, int slot) { glds16_m0(Bb0 + kb, offB[pc >> 1][pc & 1], lds0 + OFF_B + (pc >> 1) * HALF_B + slot * SUB + (pc & 1) * 1024); };
    const bool last_ragged = nk > 0 && nk * KT > nrows;     // only the last K-tile can be short
    auto is_dma = [&](int kt) { return kt < nk && !(last_ragged && kt == nk - 1); };
    auto stage_a = [&](int kt, int slot) {                  // whole image, up front (prologue / ragged tile)
        if (is_dma(kt)) {
#pragma unroll
            for (int pc = 0; pc < 4; ++pc) piece_a(pc, (unsigned)kt * strideA, slot);
        } else stage_ragged(kt, slot, false);
    };
    auto stage_b = [&](int kt, int slot) {
        if (is_dma(kt)) {
#pragma unroll
            for (int pc = 0; pc < 4; ++pc) piece_b(pc, (unsigned)kt * strideB, slot);
        } else stage_ragged(kt, slot, true);
    };

    f32x4 acc[4][8];  // [n1 tile][n2 tile]
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 8; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    const bool do_bias = p.bias_part != nullptr && (p.bias_spread || t2 == 0);
    const int bias_mod = p.bias_spread ? p.tiles_2 : 1, bias_rem = p.bias_spread ? t2 : 0;
    f32x4 bacc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};      // (see ones_frag: w2 = 0 / 1 take two dY fragments each)
    const bf16x8_t ones = __builtin_bit_cast(bf16x8_t, ones_frag<T>());

    // The DMA pieces of later K-tiles (8 per wave and steady iteration) are issued between the MFMA groups: back to back right after the
    // barrier they cost every wave of the CU ~1000 cycles of issue time at the same moment, with nothing on the matrix pipe.  The steady
    // iteration kt issues dY(kt+2) in its K-step 0 and X(kt+2) in its K-step 1, behind its barrier (below); the prologue issues dY(0), X(0),
    // dY(1), X(1).  At every wait the youngest pieces belong to later tiles and may stay in flight.
    // One K-tile, compiled three times like the NT kernel's ktile25: steady <IB, IA> (tile kt+2 is whole, both its images go out by DMA),
    // penultimate <IB> and last <>; the two TAIL bodies issue no DMA, one of the tiles behind theirs may be the ragged last tile, staged
    // through registers right after their barrier.  The steady body decides nothing at run time but the bias MFMAs.  K-step 1's fragments
    // are requested while K-step 0 is multiplied: X fragment b right after the MFMA group that was the last reader of K-step 0's, the four
    // dY fragments (16 registers of their own) after the fourth group -- the second K-step starts with its reads landed or in flight.
    // bias_cnt: K-tiles until the next one whose column sums this tile takes (kt % bias_mod == bias_rem without the division).
    // Fragment addresses (tn_frag<bf16>'s, split into a lane part and a constant): the lane reads token row r = 4g + q (+ K-step, + 16) of
    // feature chunk (2c | p >> 1) ^ ((r & 7) << 1), c = the fragment's 16-column index in its sub-image.  The XOR term does not depend on the
    // K-step or the 16-row half (both multiples of 8 rows) but it does on c, so one lane address per fragment column -- 4 for dY, 8 for X,
    // constant for the whole kernel, the wave's half included -- and slot, K-step and row half are constants in the instruction.  The steady
    // body is compiled once per slot phase (3 dY x 2 X slots: period 6) for that; the two tail bodies take the slots at run time.
    lds_cchar* fa[4];
    lds_cchar* fb[8];
    {
        const int r = 4 * g + (i >> 2), pp = i & 3;
        lds_cchar* const l0 = (lds_cchar*)smem + r * ROWB + ((pp >> 1) << 4) + (pp & 1) * 8;
#pragma unroll
        for (int t = 0; t < 4; ++t) fa[t] = l0 + (w1 >> 1) * HALF_A + ((((w1 & 1) * 4 + t) ^ (r & 7)) << 5);
#pragma unroll
        for (int t = 0; t < 8; ++t) fb[t] = l0 + OFF_B + w2 * HALF_B + ((t ^ (r & 7)) << 5);
    }
    auto frag = [&](lds_cchar* base, int off) { return lds_read_tr16_pair(base + off, base + off + 16 * ROWB); };
    auto mma = [&](const bf16x8_t& a, const bf16x8_t& b, f32x4& c) { c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); };
    // K-step 0 of tile kt+1 under K-step 1 of tile kt: the steady body is entered with its tile's images landed, the workgroup past the
    // barrier that says so, and its K-step-0 fragments requested into f1 / f2 -- by the hand-in below for tile 0, by the steady body before
    // it otherwise, which waits and meets the barrier after MFMA group NEXT_AT of its K-step 1 and then requests X fragment b of the next
    // tile after group b (its registers are free from there on) and the dY fragments into f1 (dead since K-step 0's bias MFMAs).  The same
    // barrier frees the X slot of tile kt, so X(kt+2) goes out right behind it, a whole K-tile time before its own wait (issued in K-step 0
    // of body kt+1 it has half a K-tile and the wait stalls: 4-8 % slower than no overlap at all, profiles/tn_ladder.txt section 2).  The
    // penultimate and last bodies begin with their own wait, barrier and reads as before; the last steady body's requests for the
    // penultimate tile are made again there (24 reads per workgroup) so that no fragment register is live into the tail bodies.
    constexpr int NEXT_AT = 1;
    bf16x8_t f1[4], f2[8], g1[4];
    int bias_cnt = bias_rem;
    auto ktile = [&](int kt, auto issue_b, auto issue_a, auto tail, auto slot_a, auto slot_b) __attribute__((always_inline)) {
        constexpr bool IB = decltype(issue_b)::value, IA = decltype(issue_a)::value, TAIL = decltype(tail)::value;
        const int ca = slot_a, cb = slot_b;                     // (std::integral_constant in the steady body)
        const int na = ca == 0 ? 2 : ca - 1, nb = cb ^ 1;      // slots of dY(kt + 2), X(kt + 1)
        const int oa = ca * SUB, ob = cb * SUB;
        if constexpr (!IA) {
            if constexpr (IB) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");      // dY(kt+1) and X(kt+1) were issued after tile kt's: they may fly
            else wait_vmcnt0();
            __syncthreads();
        }
        if constexpr (TAIL) {                                   // (block-uniform; at most once per operand and workgroup)
            if (last_ragged && kt + 1 == nk - 1) stage_ragged(kt + 1, nb, true);
            if (last_ragged && kt + 2 == nk - 1) stage_ragged(kt + 2, na, false);
        }
        const unsigned ka = (unsigned)(kt + 2) * strideA, kb = (unsigned)(kt + 2) * strideB;
        const bool bias_now = do_bias && bias_cnt == 0;
        if constexpr (!IA) {
#pragma unroll
            for (int t = 0; t < 4; ++t) f1[t] = frag(fa[t], oa);
#pragma unroll
            for (int t = 0; t < 8; ++t) f2[t] = frag(fb[t], ob);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
#pragma unroll
            for (int a = 0; a < 4; ++a) mma(f2[b], f1[a], acc[a][b]);       // rows(regs) = n2, cols(lanes) = n1
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (IA) { if (b >= 4) piece_a(b - 4, ka, na); }
            f2[b] = frag(fb[b], ob + KSTEP * ROWB);
            if (b == 3) {
#pragma unroll
                for (int t = 0; t < 4; ++t) g1[t] = frag(fa[t], oa + KSTEP * ROWB);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if (bias_now) {
            if (w2 == 0) { mma(ones, f1[0], bacc[0]); mma(ones, f1[1], bacc[1]); }
            else { mma(ones, f1[2], bacc[0]); mma(ones, f1[3], bacc[1]); }
        }
#pragma unroll
        for (int b = 0; b < 8; ++b) {
#pragma unroll
            for (int a = 0; a < 4; ++a) mma(f2[b], g1[a], acc[a][b]);
            if constexpr (IA) if (b >= NEXT_AT) {
                __builtin_amdgcn_sched_barrier(0);
                if (b == NEXT_AT) {
                    // Tile kt+1's images: this wave's DMA pieces in flight are, oldest first, dY(kt+1) (K-step 0 of body kt-1, or the
                    // prologue), X(kt+1) (K-step 1 of body kt-1, or the prologue) and dY(kt+2) (K-step 0 of this body) -- vmcnt retires in
                    // order, the four youngest may fly.
                    asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
                    // Ring invariant at this barrier, B(kt).  __syncthreads() waits for the wave's own LDS reads (lgkmcnt(0)) first, so every
                    // read a wave issued before B(kt) has returned when any wave is past it.  Every read of tile kt's slots is issued
                    // before B(kt) -- K-step 0's behind B(kt-1) (or in the hand-in), K-step 1's in K-step 0 of this body -- and behind
                    // B(kt) a wave reads only tile kt+1's slots until B(kt+1).  A slot is refilled only behind the barrier that ends its
                    // tile's reads: X(kt+2) into X(kt)'s slot right behind B(kt), below; dY(kt+3) into dY(kt)'s slot in K-step 0 of body
                    // kt+1, behind B(kt) as well; a ragged tile's stores behind a tail body's own barrier, which follows B(kt).  What this
                    // body issued before B(kt), dY(kt+2) into dY(kt-1)'s slot, lay behind B(kt-1) in the same way.
                    __syncthreads();
                    constexpr int pa = ((decltype(slot_a)::value + 1) % 3) * SUB, pb = (decltype(slot_b)::value ^ 1) * SUB;
#pragma unroll
                    for (int t = 0; t < 4; ++t) f1[t] = frag(fa[t], pa);
#pragma unroll
                    for (int t = 0; t <= NEXT_AT; ++t) f2[t] = frag(fb[t], pb);
                } else {
                    if (b - NEXT_AT - 1 < 4) piece_b(b - NEXT_AT - 1, kb, cb);
                    f2[b] = frag(fb[b], (decltype(slot_b)::value ^ 1) * SUB);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (bias_now) {
            if (w2 == 0) { mma(ones, g1[0], bacc[0]); mma(ones, g1[1], bacc[1]); }
            else { mma(ones, g1[2], bacc[0]); mma(ones, g1[3], bacc[1]); }
        }
        bias_cnt = bias_cnt == 0 ? bias_mod - 1 : bias_cnt - 1;
    };
    const int nd = last_ragged ? nk - 1 : nk;               // whole K-tiles: 0 .. nd-1 go by DMA
    if (nk > 0) { stage_a(0, 0); stage_b(0, 0); if (nk > 1) stage_a(1, 1); if (nd > 1) stage_b(1, 1); }
    const int ns = nd - 2;                                  // steady tiles: 0 .. ns-1 (tile kt + 2 is whole); tile kt in slots kt % 3 (dY), kt % 2 (X)
    int kt = 0;
    if (ns > 0) {                                           // dY(0), X(0), dY(1), X(1) went out by DMA in that order: the steady loop's hand-in
        asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 4; ++t) f1[t] = frag(fa[t], 0);
#pragma unroll
        for (int t = 0; t < 8; ++t) f2[t] = frag(fb[t], 0);
    }
    if (ns > 0) {
        const auto steady = [&](auto sa, auto sb) __attribute__((always_inline)) { ktile(kt, std::true_type{}, std::true_type{}, std::false_type{}, sa, sb); return ++kt == ns; };
        using std::integral_constant;
        for (;;) {
            if (steady(integral_constant<int, 0>{}, integral_constant<int, 0>{})) break;
            if (steady(integral_constant<int, 1>{}, integral_constant<int, 1>{})) break;
            if (steady(integral_constant<int, 2>{}, integral_constant<int, 0>{})) break;
            if (steady(integral_constant<int, 0>{}, integral_constant<int, 1>{})) break;
            if (steady(integral_constant<int, 1>{}, integral_constant<int, 0>{})) break;
            if (steady(integral_constant<int, 2>{}, integral_constant<int, 1>{})) break;
        }
    }
    if (kt + 1 < nd) { ktile(kt, std::true_type{}, std::false_type{}, std::true_type{}, kt % 3, kt & 1); ++kt; }
    for (; kt < nk; ++kt) ktile(kt, std::false_type{}, std::false_type{}, std::true_type{}, kt % 3, kt & 1);
    __syncthreads();

    if (do_bias && g == 0) {
        const long slot = p.bias_spread ? (long)split * p.tiles_2 + t2 : split;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int n1 = n1_0 + w1 * 64 + (2 * w2 + j) * 16 + i;
            if (n1 < p.N1) p.bias_part[slot * p.N1 + n1] = bacc[j][0];
        }
    }
    float* S = p.S + (long)split * p.N1 * p.N2;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int n1 = n1_0 + w1 * 64 + a * 16 + i;
        if (n1 >= p.N1) continue;
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const int n2 = n2_0 + w2 * 128 + b * 16 + 4 * g;
            if (n2 >= p.N2) continue;
            st4(S + (long)n1 * p.N2 + n2, acc[a][b]);
        }
    }
}

template <typename T>
__global__ __launch_bounds__(512, 1) __attribute__((amdgpu_waves_per_eu(2, 2))) void gemm_tn_grouped_big_kernel(const GemmTNGroup grp) {
    const int t = xcd_remap(blockIdx.x, grp.tile_end[grp.n - 1]);
    int g = 0;
#pragma unroll
    for (int k = 0; k < TN_GROUP_MAX - 1; ++k) g += (k < grp.n - 1 && t >= grp.tile_end[k]) ? 1 : 0;
    const int first = g == 0 ? 0 : grp.tile_end[g - 1];
    gemm_tn_big_body<T>(grp.p[g], t - first, blockIdx.y);
}

// dW_k = sum_s slab_k[s], db_k = sum_s bias_part_k[s] for the problems of one grouped launch (fixed order: bitwise reproducible)
struct TNGroupReduce {
    const float* slabs[TN_GROUP_MAX]; float* out[TN_GROUP_MAX]; const float* bias_part[TN_GROUP_MAX]; float* dbias[TN_GROUP_MAX];
    long n4[TN_GROUP_MAX];          // N1 * N2 / 4 per problem
    long end4[TN_GROUP_MAX];        // prefix sums of n4
    int N1[TN_GROUP_MAX];
    int nbias[TN_GROUP_MAX];       // bias partial slots per problem (splits x tiles sharing the sums)
    int n, nsplit;
};
__global__ void tn_group_reduce_kernel(const TNGroupReduce r) {
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= r.end4[r.n - 1]) return;
    int k = 0;
#pragma unroll
    for (int q = 0; q < TN_GROUP_MAX - 1; ++q) k += (q < r.n - 1 && gid >= r.end4[q]) ? 1 : 0;
    const long local = gid - (k == 0 ? 0 : r.end4[k - 1]);
    const float* S = r.slabs[k];
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    for (int s2 = 0; s2 < r.nsplit; ++s2) v += ld4(S + ((long)s2 * r.n4[k] + local) * 4);
    st4(r.out[k] + local * 4, v);
    if (r.dbias[k] && local < r.N1[k]) {                     // the first N1 threads of a problem also finish its bias gradient
        float b = 0.f;
        for (int s2 = 0; s2 < r.nbias[k]; ++s2) b += r.bias_part[k][(long)s2 * r.N1[k] + local];
        r.dbias[k][local] = b;
    }
}
// the bias gradients alone (unsplit launches: the tiles wrote dW themselves); grid covers the N1 of all problems
__global__ void tn_group_bias_reduce_kernel(const TNGroupReduce r, int total_n1) {
    int gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total_n1) return;
    int k = 0;
    while (k < r.n - 1 && gid >= r.N1[k]) { gid -= r.N1[k]; ++k; }
    if (!r.dbias[k]) return;
    float b = 0.f;
    for (int s2 = 0; s2 < r.nbias[k]; ++s2) b += r.bias_part[k][(long)s2 * r.N1[k] + gid];
    r.dbias[k][gid] = b;
}

// out[n1][perm(n2)] (+)= sum_s S[s][n1][n2];  perm(n2) = (n2 % inner) * outer + n2 / inner  (outer = 1: identity).
// Used with inner = C_in, outer = kernel width to hand conv wgrads back in nn.Conv1d's [co][ci][k] order.
__global__ void splitk_reduce_kernel(const float* __restrict__ S, float* __restrict__ out, int nsplit, long n_elems, int N2,
                                     int inner, int outer, int accumulate, float scale, const float* __restrict__ bias_part,
                                     float* __restrict__ dbias, int N1) {
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (dbias && gid < N1) {          // the first N1 threads also finish the fused bias gradient (one launch fewer)
        float b = 0.f;
        for (int s = 0; s < nsplit; ++s) b += bias_part[(long)s * N1 + gid];
        b *= scale;
        dbias[gid] = accumulate ? dbias[gid] + b : b;
    }
    const long idx4 = gid * 4;
    if (idx4 >= n_elems) return;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < nsplit; ++s) v += ld4(S + (long)s * n_elems + idx4);
    v *= scale;
    if (outer == 1) {
        if (accumulate) v += ld4(out + idx4);
        st4(out + idx4, v);
    } else {
        const long n1 = idx4 / N2; const int n2 = (int)(idx4 - n1 * N2);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int q = n2 + e;
            const long o = n1 * N2 + (long)(q % inner) * outer + q / inner;
            out[o] = accumulate ? out[o] + v[e] : v[e];
        }
    }
}

__global__ void bias_reduce_kernel(const float* __restrict__ part, float* __restrict__ out, int nsplit, int N1, int accumulate, float scale) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N1) return;
    float s = 0.f;
    for (int k = 0; k < nsplit; ++k) s += part[(long)k * N1 + n];
    s *= scale;
    out[n] = accumulate ? out[n] + s : s;
}

// column sums (bias gradients): out[n] (+)= sum_m X[m][n], two deterministic stages.
template <typename T>
__global__ void colsum_partial_kernel(const T* __restrict__ X, float* __restrict__ part, int M, int N, long ld, int rows_per_block) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    const int r_begin = blockIdx.y * rows_per_block;
    int r_end = r_begin + rows_per_block; r_end = r_end < M ? r_end : M;
    if (n >= N) return;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;            // four independent chains: the loads of 4 rows are in flight together
    int r = r_begin;
    for (; r + 3 < r_end; r += 4) {
        s0 += ET<T>::ld(X + (long)r * ld + n); s1 += ET<T>::ld(X + (long)(r + 1) * ld + n);
        s2 += ET<T>::ld(X + (long)(r + 2) * ld + n); s3 += ET<T>::ld(X + (long)(r + 3) * ld + n);
    }
    for (; r < r_end; ++r) s0 += ET<T>::ld(X + (long)r * ld + n);
    part[(long)blockIdx.y * N + n] = (s0 + s1) + (s2 + s3);
}
__global__ void colsum_final_kernel(const float* __restrict__ part, float* __restrict__ out, int nparts, int N, int accumulate) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;            // up to 256 partial rows: four loads in flight instead of a serial chain
    int k = 0;
    for (; k + 3 < nparts; k += 4) {
        s0 += part[(long)k * N + n]; s1 += part[(long)(k + 1) * N + n]; s2 += part[(long)(k + 2) * N + n]; s3 += part[(long)(k + 3) * N + n];
    }
    for (; k < nparts; ++k) s0 += part[(long)k * N + n];
    const float s = (s0 + s1) + (s2 + s3);
    out[n] = accumulate ? out[n] + s : s;
}

}  // namespace tav

using namespace tav;

// ================================================================================================ host: enqueue only
// Every decision -- argument checks, tile plan, kernel and launch geometry, workspace layout -- is a pure function of gemm_plan.h.
static_assert(NT_GEN == plan::EPI_GEN && NT_PLAIN == plan::EPI_PLAIN && NT_RESID == plan::EPI_RESID && NT_GELU_D == plan::EPI_GELU_D &&
              NT_MUL_D == plan::EPI_MUL_D && TN_GROUP_MAX == plan::TN_PROBLEMS_MAX, "gemm_plan.h mirrors these");

// the kernels of plan::nt_keys, in its order
template <int DTYPE> struct NtElem;
template <> struct NtElem<TAV_F32> { using type = float; };
template <> struct NtElem<TAV_BF16> { using type = bf16; };
template <> struct NtElem<TAV_FP8> { using type = fp8; };
using NtKernel = void (*)(const GemmNT);
#define TAV_NT_KERNEL(IN, OUT, TM, NST, NW, TNW, EPI) gemm_nt_kernel<NtElem<TAV_##IN>::type, NtElem<TAV_##OUT>::type, TM, NST, NW, TNW, NT_##EPI>,
static const NtKernel nt_kernels[] = {TAV_NT_KERNELS(TAV_NT_KERNEL)};
#undef TAV_NT_KERNEL
static_assert(sizeof(nt_kernels) / sizeof(nt_kernels[0]) == plan::nt_num_keys, "one kernel per key");

extern "C" int tav_gemm_nt_schedule(const tav_gemm_nt_args* a, int32_t* tile, int32_t* rows_first, int32_t* tile_rest) {
    if (!tile || !rows_first || !tile_rest) return TAV_ERR_NULL;
    const int rc = plan::nt_validate(a, false);
    if (rc != 0) return rc;
    int tm, rb, tr;
    plan::nt_plan(a, &tm, &rb, &tr);
    *tile = tm; *rows_first = rb; *tile_rest = rb < a->M ? tr : 0;
    return 0;
}

static int nt_enqueue(const tav_gemm_nt_args* a, GemmNT p, int tm, hipStream_t stream) {
    const plan::NtLaunch L = plan::nt_launch(a, p.M, tm);
    const int k = plan::nt_key_index(L.key);
    if (k < 0) return TAV_ERR_DTYPE;                         // no such kernel (nt_launch returns only keys of the list: unreachable)
    p.tiles_m = L.tiles_m; p.tiles_n = L.tiles_n;
    hipLaunchKernelGGL(nt_kernels[k], dim3(L.grid_x, L.grid_y), dim3(L.block), L.lds, stream, p);
    return 0;
}

extern "C" int tav_gemm_nt(const tav_gemm_nt_args* a, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    { const int rc = plan::nt_validate(a, true); if (rc != 0) return rc; }
    GemmNT p;
    p.A = (const char*)a->A; p.B = (const char*)a->B; p.C = (char*)a->C; p.Cpre = (char*)a->C_pre; p.bias = a->bias;
    p.gelu_in = (const char*)a->gelu_in; p.resid = a->resid;
    p.M = (int)a->M; p.N = (int)a->N; p.K = (int)a->K;
    p.lda = a->lda; p.ldb = a->ldb; p.ldc = a->ldc; p.ld_pre = a->ld_pre; p.ld_gelu = a->ld_gelu_in; p.ld_resid = a->ld_resid;
    p.nzg = a->nzg > 0 ? a->nzg : 1;
    p.a_zb = a->a_zb; p.a_zg = a->a_zg; p.b_zb = a->b_zb; p.b_zg = a->b_zg; p.c_zb = a->c_zb; p.c_zg = a->c_zg; p.bias_zg = a->bias_zg;
    p.g_zb = a->gelu_zb ? a->gelu_zb : a->c_zb;
    p.act = a->act; p.accumulate = a->accumulate; p.alpha = a->alpha;
    p.sa = a->in_dtype == TAV_FP8 ? a->a_dequant : nullptr; p.sb = a->in_dtype == TAV_FP8 ? a->b_dequant : nullptr;
    int tm, rows_big, tm_rest;
    plan::nt_plan(a, &tm, &rows_big, &tm_rest);
    if (rows_big < p.M) {
        // mixed schedule: whole rounds of 256 x 256 tiles over the leading rows, then the 128-wide tile over the rest (same stream, disjoint rows)
        const plan::NtSplit s = plan::nt_split(a, rows_big);
        GemmNT q = p;
        q.M = s.M_rest;
        q.A = p.A + s.a_bytes; q.C = p.C + s.c_bytes;
        if (p.Cpre) q.Cpre = p.Cpre + s.pre_bytes;
        if (p.gelu_in) q.gelu_in = p.gelu_in + s.gelu_bytes;
        if (p.resid) q.resid = p.resid + s.resid_elems;
        p.M = rows_big;
        int rc = nt_enqueue(a, p, 16, stream);
        if (rc == 0) rc = nt_enqueue(a, q, tm_rest, stream);
        if (rc != 0) return rc;
    } else {
        const int rc = nt_enqueue(a, p, tm, stream);
        if (rc != 0) return rc;
    }
    return (int)hipGetLastError();
}

extern "C" int tav_gemm_tn_splits(int64_t n1, int64_t n2, int64_t rows_per_batch, int64_t nbatch, int32_t* chunk_rows, int32_t* nsplit) {
    if (!chunk_rows || !nsplit || n1 <= 0 || n2 <= 0 || rows_per_batch <= 0 || nbatch <= 0) return TAV_ERR_SHAPE;
    plan::tn_splits(n1, n2, rows_per_batch, nbatch, chunk_rows, nsplit);
    return 0;
}

// Kernel arguments of a grouped launch from its layout; `ws` is the workspace the layout's offsets refer to.  use_ws as in tn_group_layout:
// without it the tiles write out and dbias themselves (bias_spread = 0) and `red` is filled but not needed.
static void tn_group_fill(const tav_gemm_tn_problem* probs, int nprob, long rows, const plan::TnGroupPlan& P, const plan::TnGroupLayout& L,
                          bool use_ws, float* ws, GemmTNGroup* grp, TNGroupReduce* red) {
    for (int k = 0; k < TN_GROUP_MAX; ++k) {
        const tav_gemm_tn_problem& a = probs[k < nprob ? k : nprob - 1];
        float* const bias_ws = L.bias_off[k] >= 0 ? ws + L.bias_off[k] : nullptr;
        GemmTN& p = grp->p[k];
        p.A = (const char*)a.A; p.B = (const char*)a.B; p.N1 = (int)a.N1; p.N2 = (int)a.N2; p.lda = a.lda; p.ldb = a.ldb;
        p.rows_per_batch = (int)rows; p.a_zb = 0; p.b_zb = 0; p.chunk_rows = (int)P.chunk; p.chunks_per_batch = P.nsplit;
        p.tiles_1 = L.tiles_1[k]; p.tiles_2 = L.tiles_2[k];
        p.S = L.slab_off[k] >= 0 ? ws + L.slab_off[k] : a.out;
        p.bias_part = use_ws ? bias_ws : a.dbias; p.bias_spread = use_ws ? 1 : 0;
        grp->tile_end[k] = L.tile_end[k];
        red->slabs[k] = p.S; red->out[k] = a.out; red->dbias[k] = a.dbias; red->N1[k] = (int)a.N1; red->n4[k] = L.n4[k];
        red->nbias[k] = L.nbias[k]; red->bias_part[k] = bias_ws; red->end4[k] = L.end4[k];
    }
    grp->n = nprob; red->n = nprob; red->nsplit = P.nsplit;
}

extern "C" int tav_gemm_tn_grouped(const tav_gemm_tn_problem* probs, int32_t nprob, int64_t rows, int32_t dtype, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!probs) return TAV_ERR_NULL;
    if (nprob <= 0 || nprob > TN_GROUP_MAX || rows <= 0) return TAV_ERR_SHAPE;
    if (dtype != TAV_BF16 && dtype != TAV_F32) return TAV_ERR_DTYPE;
    { const int rc = plan::tn_validate_group(probs, nprob, rows, dtype); if (rc != 0) return rc; }
    const plan::TnGroupPlan P = plan::tn_plain_plan(rows);
    const plan::TnGroupLayout L = plan::tn_group_layout(probs, nprob, P, false);
    GemmTNGroup grp;
    TNGroupReduce red;                                                  // (not used: nothing to reduce)
    tn_group_fill(probs, nprob, rows, P, L, false, nullptr, &grp, &red);
    dim3 grid(L.total), block(256);
    if (dtype == TAV_BF16) hipLaunchKernelGGL((gemm_tn_grouped_kernel<bf16>), grid, block, 4 * 64 * 256, stream, grp);
    else hipLaunchKernelGGL((gemm_tn_grouped_kernel<float>), grid, block, 4 * 64 * 512, stream, grp);
    return (int)hipGetLastError();
}

extern "C" int64_t tav_gemm_tn_grouped_ws_bytes(const tav_gemm_tn_problem* probs, int32_t nprob, int64_t rows, int32_t dtype, int32_t flags) {
    if (!probs || nprob <= 0 || nprob > TN_GROUP_MAX || rows <= 0) return 0;
    return plan::tn_big_plan(probs, nprob, rows, dtype, flags).ws_floats * 4;
}

extern "C" int tav_gemm_tn_grouped_ws(const tav_gemm_tn_problem* probs, int32_t nprob, int64_t rows, int32_t dtype, void* workspace,
                                      int64_t workspace_bytes, int32_t flags, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!probs) return TAV_ERR_NULL;
    if (nprob <= 0 || nprob > TN_GROUP_MAX || rows <= 0) return TAV_ERR_SHAPE;
    if (dtype != TAV_BF16 && dtype != TAV_F32) return TAV_ERR_DTYPE;
    const plan::TnGroupPlan P = plan::tn_big_plan(probs, nprob, rows, dtype, flags);
    if (P.ws_floats > 0 && (!workspace || workspace_bytes < P.ws_floats * 4)) return tav_gemm_tn_grouped(probs, nprob, rows, dtype, stream_);   // no room: the workspace-free form
    // Preserved, not designed: the empty split is refused BEFORE the problems are looked at (a NULL operand in the same call reports
    // TAV_ERR_SHAPE), and a call that took the fallback above is never asked.
    if (plan::tn_has_empty_split(P, rows)) return TAV_ERR_SHAPE;
    { const int rc = plan::tn_validate_group(probs, nprob, rows, dtype); if (rc != 0) return rc; }
    const plan::TnGroupLayout L = plan::tn_group_layout(probs, nprob, P, true);
    GemmTNGroup grp;
    TNGroupReduce red;
    tn_group_fill(probs, nprob, rows, P, L, true, (float*)workspace, &grp, &red);
    if (P.big) hipLaunchKernelGGL((gemm_tn_grouped_big_kernel<bf16>), dim3(L.total, P.nsplit), dim3(512), 5 * 2 * 64 * 256, stream, grp);
    else if (dtype == TAV_BF16) hipLaunchKernelGGL((gemm_tn_grouped_kernel<bf16>), dim3(L.total), dim3(256), 4 * 64 * 256, stream, grp);
    else hipLaunchKernelGGL((gemm_tn_grouped_kernel<float>), dim3(L.total), dim3(256), 4 * 64 * 512, stream, grp);
    if (P.nsplit > 1) hipLaunchKernelGGL(tn_group_reduce_kernel, dim3((unsigned)((L.end4[TN_GROUP_MAX - 1] + 255) / 256)), dim3(256), 0, stream, red);
    else if (L.any_bias) hipLaunchKernelGGL(tn_group_bias_reduce_kernel, dim3((unsigned)((L.total_n1 + 255) / 256)), dim3(256), 0, stream, red, L.total_n1);
    return (int)hipGetLastError();
}

extern "C" int tav_gemm_tn(const tav_gemm_tn_args* a, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!a || !a->slabs) return TAV_ERR_NULL;
    { const int rc = plan::tn_validate_problem(a->A, a->B, a->out, a->N1, a->N2, a->lda, a->ldb, a->a_zb, a->b_zb, a->rows_per_batch, a->nbatch, a->dtype);
      if (rc != 0) return rc; }
    if (a->chunk_rows <= 0 || a->chunk_rows % 64) return TAV_ERR_SHAPE;
    GemmTN p;
    p.A = (const char*)a->A; p.B = (const char*)a->B; p.S = a->slabs;
    p.bias_part = a->dbias ? a->bias_partials : nullptr; p.bias_spread = 0;
    if (a->dbias && !a->bias_partials) return TAV_ERR_NULL;
    p.N1 = (int)a->N1; p.N2 = (int)a->N2; p.lda = a->lda; p.ldb = a->ldb;
    p.rows_per_batch = (int)a->rows_per_batch; p.a_zb = a->a_zb; p.b_zb = a->b_zb;
    p.chunk_rows = a->chunk_rows;
    p.chunks_per_batch = (int)((a->rows_per_batch + a->chunk_rows - 1) / a->chunk_rows);
    const int nsplit = p.chunks_per_batch * (int)a->nbatch;
    if (nsplit != a->nsplit) return TAV_ERR_SHAPE;
    p.tiles_1 = (p.N1 + 127) / 128; p.tiles_2 = (p.N2 + 127) / 128;
    const int inner = a->perm_inner > 0 ? a->perm_inner : p.N2, outer = a->perm_outer > 0 ? a->perm_outer : 1;
    if (outer > 1 && inner * outer != p.N2) return TAV_ERR_SHAPE;       // checked before anything is launched
    dim3 grid(p.tiles_1 * p.tiles_2, nsplit), block(256);
    if (a->dtype == TAV_BF16) {
        const size_t lds = 4 * 64 * 256;
        hipLaunchKernelGGL((gemm_tn_kernel<bf16>), grid, block, lds, stream, p);
    } else {
        const size_t lds = 4 * 64 * 512;
        hipLaunchKernelGGL((gemm_tn_kernel<float>), grid, block, lds, stream, p);
    }
    int e = (int)hipGetLastError();
    if (e) return e;
    const long n_elems = (long)p.N1 * p.N2;
    const long nthreads = (n_elems + 3) / 4;
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)((nthreads + 255) / 256)), dim3(256), 0, stream, a->slabs, a->out, nsplit,
                       n_elems, p.N2, inner, outer, a->accumulate, a->scale == 0.f ? 1.f : a->scale, (const float*)a->bias_partials, a->dbias, p.N1);
    return (int)hipGetLastError();
}

extern "C" int tav_colsum(const void* x, int32_t dtype, int64_t M, int64_t N, int64_t ld, float* partials, int32_t nparts, float* out,
                          int32_t accumulate, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!x || !partials || !out) return TAV_ERR_NULL;
    if (M <= 0 || N <= 0 || nparts <= 0) return TAV_ERR_SHAPE;
    const int rows_per_block = (int)((M + nparts - 1) / nparts);
    dim3 grid((unsigned)((N + 255) / 256), nparts), block(256);
    if (dtype == TAV_BF16) hipLaunchKernelGGL((colsum_partial_kernel<bf16>), grid, block, 0, stream, (const bf16*)x, partials, (int)M, (int)N, (long)ld, rows_per_block);
    else if (dtype == TAV_F32) hipLaunchKernelGGL((colsum_partial_kernel<float>), grid, block, 0, stream, (const float*)x, partials, (int)M, (int)N, (long)ld, rows_per_block);
    else return TAV_ERR_DTYPE;
    hipLaunchKernelGGL(colsum_final_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream, partials, out, nparts, (int)N, accumulate);
    return (int)hipGetLastError();
}
