"""A fixed list of calls through tav_amd.ops, once each, no timing, nothing printed: the launches a change of the host code must leave as they are.

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python tools/launch_list.py --family gemm|ops     (GPU box; a run of its own, no counters)
    python tools/launch_list.py --compare OUT_PARENT OUT_NEW                                                  (anywhere)

--compare reads the kernel-trace CSVs of two such runs and compares, line for line and in launch order, (kernel name with its template
arguments, grid, workgroup size, LDS bytes) of every libtavhip kernel (zero_pad_rows_kernel and namespace tav); exit status 1 when they differ;
--lines OUT prints those lines.
Family ops: every other op of ops.py at the smallest shapes on each side of the geometry caps that are cheap to run (LayerNorm rows 16 / 17
and 8192 / 8193, embedding rows 65536 / 65537, conv0 chunks around 512 steps, SpecAugment parts around 32 rows, every dtype an op accepts,
the streaming and the tiled fp8 quantisation in their current-scaling and delayed forms, the state roll, the fp8 weight gradient's split-K
reduce, deferred LayerNorm parameter reduces of 1, 3 and 70 items, one and two resizes of a clip); the caps at 131072 and above stay in the CPU sweep
(tests/host/entry_plan_check.cpp).  Family gemm: every
epilogue flavour x {bf16 -> bf16, bf16 -> f32, f32, fp8 -> bf16, fp8 -> f32}; tile hints 0 / 2 / 3 / 4 / 8 / 16 / 17; ring hints; grids under
and over one workgroup per CU; the mixed schedule (M = 46885, N = K = 768); batched nzb / nzg; gemm_tn with and without bias and column
permutation; grouped weight gradients with flags 0 / 1 / 2 and one to three splits; the workspace-free fallback; column sums."""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rows(d):
    files = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))
    assert files, f"no kernel trace under {d}"
    out = []
    for f in files:
        with open(f) as fh:
            recs = [r for r in csv.DictReader(fh) if "tav::" in r["Kernel_Name"] or "zero_pad_rows_kernel" in r["Kernel_Name"]]
        recs.sort(key=lambda r: int(r["Start_Timestamp"]))
        cols = [c for c in (recs[0] if recs else {}) if c.startswith(("Grid_Size", "Workgroup_Size", "LDS_Block_Size"))]
        assert not recs or len(cols) >= 3, cols
        out += [(r["Kernel_Name"],) + tuple(f"{c}={r[c]}" for c in cols) for r in recs]
    return out


def compare(dir_a, dir_b):
    a, b = rows(dir_a), rows(dir_b)
    diff = [(k, x, y) for k, (x, y) in enumerate(zip(a, b)) if x != y]
    print(f"launches: {len(a)} / {len(b)}; distinct kernels {len({x[0] for x in a})} / {len({x[0] for x in b})}; differing lines {len(diff)}")
    for k, x, y in diff[:10]:
        print(f"  #{k}: {x}\n   vs  {y}")
    same = len(a) == len(b) and not diff
    print("LAUNCH SEQUENCE", "IDENTICAL" if same else "DIFFERENT")
    return 0 if same else 1


def gemm_calls():
    sys.path[:0] = [ROOT]
    import torch

    import tav_amd  # noqa: F401
    from tav_amd import ops
    dev = "cuda"
    bf, f32, f8 = torch.bfloat16, torch.float32, torch.float8_e4m3fn

    def t(*shape, dtype=bf):
        if dtype == f8:
            return torch.zeros(*shape, dtype=torch.uint8, device=dev).view(f8)
        return torch.zeros(*shape, dtype=dtype, device=dev)

    one = torch.ones(1, dtype=f32, device=dev)

    def nt(in_dt, out_dt, M, N, K, flavour="plain", tile_m=0, **kw):
        a, b = t(M, K, dtype=in_dt), t(N, K, dtype=in_dt)
        side = bf if in_dt == f8 else in_dt
        if in_dt == f8:
            kw.update(a_dequant=one, b_dequant=one)
        if flavour == "resid":
            kw.update(resid=t(M, N, dtype=f32), bias=t(N, dtype=f32))
        elif flavour == "gelu_d":
            kw.update(want_pre=True, act=3, bias=t(N, dtype=f32))
        elif flavour == "mul_d":
            kw.update(gelu_in=t(M, N, dtype=side), act=4)
        elif flavour == "generic":
            kw.update(resid=t(M, N, dtype=f32), act=1, accumulate=True, out=t(M, N, dtype=out_dt))
        ops.gemm_nt(a, b, out_dtype=out_dt, tile_m=tile_m, **kw)

    pairs_of = {"bf16->bf16": (bf, bf), "bf16->f32": (bf, f32), "f32": (f32, f32), "fp8->bf16": (f8, bf), "fp8->f32": (f8, f32)}
    for in_dt, out_dt in pairs_of.values():                                    # 25: every flavour asked of every type pair
        for flavour in ("plain", "resid", "gelu_d", "mul_d", "generic"):
            nt(in_dt, out_dt, 300, 384, 256, flavour)
    for hint in (2, 3, 4, 8, 16, 17):                                          # tile hints (0 above)
        nt(bf, bf, 333, 384, 256, tile_m=hint)
        nt(bf, f32, 333, 384, 256, "resid", tile_m=hint)
    for hint in (2, 3, 16):
        nt(f32, f32, 333, 384, 256, tile_m=hint)
    for hint in (4, 16):
        nt(f8, bf, 700, 384, 1024, "gelu_d", tile_m=hint)
        nt(f8, f32, 700, 384, 1024, "resid", tile_m=hint)
    for ring in (2, 3, 4):                                                     # ring hints, alone and with a forced tile
        nt(bf, bf, 333, 384, 256, "gelu_d", tile_m=ring << 5)
        nt(bf, f32, 333, 384, 256, "resid", tile_m=3 | (ring << 5))
    nt(bf, bf, 4096, 3072, 768)                                                # over one workgroup per CU: ring depth 2, the big tile
    nt(bf, f32, 4096, 768, 768, "resid")
    nt(bf, bf, 46885, 768, 768)                                                # the mixed schedule: two launches
    nt(bf, f32, 46885, 768, 768, "resid")
    nt(bf, bf, 46885, 768, 768, tile_m=17)
    for dt_ in (bf, f32):                                                      # batched: z = zb * nzg + zg
        M, N, K, nzb, nzg = 70, 132, 128, 2, 3
        a, b, out = t(nzb * nzg * M, K, dtype=dt_), t(nzg * N, K, dtype=dt_), t(nzb * nzg * M, N, dtype=dt_)
        ops.gemm_nt(a, b, out=out, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, nzb=nzb, nzg=nzg, a_zb=nzg * M * K, a_zg=M * K, b_zg=N * K, c_zb=nzg * M * N,
                    c_zg=M * N)

    for dt_ in (bf, f32):                                                      # weight gradients
        a, b = t(1000, 256, dtype=dt_), t(1000, 384, dtype=dt_)
        ops.gemm_tn(a, b)
        ops.gemm_tn(a, b, want_bias=True)
        a3, b3 = t(3 * 249, 136, dtype=dt_), t(3 * 249, 264, dtype=dt_)
        ops.gemm_tn(a3, b3, N1=136, N2=264, lda=136, ldb=264, rows_per_batch=249, nbatch=3, a_zb=249 * 136, b_zb=249 * 264, perm_inner=88, perm_outer=3,
                    want_bias=True)
        ops.colsum(t(1000, 384, dtype=dt_))
    ragged, layer = [(384, 136), (136, 264), (256, 512), (520, 128)], [(2304, 768), (768, 768), (3072, 768), (768, 3072)]

    def grouped(shapes, rows, dt_, flags, bias=True):
        ops.gemm_tn_grouped([(t(rows, n1, dtype=dt_), t(rows, n2, dtype=dt_)) for n1, n2 in shapes], want_bias=bias, flags=flags)

    for flags in (0, 1, 2, 1 | (1 << 8), 1 | (2 << 8), 1 | (3 << 8)):
        grouped(ragged, 5000, bf, flags)
    grouped(ragged, 777, f32, 0)
    grouped(ragged[:2], 777, bf, 0, bias=False)
    grouped(layer, 12288, bf, 0)                                               # the library's own choice of the 256-wide form with splits
    for dt_, flags in ((bf, 1 | (2 << 8)), (f32, 0)):                           # a workspace too small: the fallback, and the direct call
        prs = [(t(777, n1, dtype=dt_), t(777, n2, dtype=dt_)) for n1, n2 in ragged]
        probs, keep = (ops.L.GemmTNProblem * 4)(), []
        for k, (a, b) in enumerate(prs):
            dW, db = t(a.shape[1], b.shape[1], dtype=f32), t(a.shape[1], dtype=f32)
            keep += [dW, db]
            probs[k].A, probs[k].B, probs[k].out, probs[k].dbias = ops.ptr(a), ops.ptr(b), ops.ptr(dW), ops.ptr(db)
            probs[k].N1, probs[k].N2, probs[k].lda, probs[k].ldb = a.shape[1], b.shape[1], a.stride(0), b.stride(0)
        ops.check(ops.lib().tav_gemm_tn_grouped_ws(probs, 4, 777, ops.dt(prs[0][0]), None, 0, flags, ops.stream()), "gemm_tn_grouped_ws")
        ops.check(ops.lib().tav_gemm_tn_grouped(probs, 4, 777, ops.dt(prs[0][0]), ops.stream()), "gemm_tn_grouped")
    torch.cuda.synchronize()


def op_calls():
    sys.path[:0] = [ROOT]
    import torch

    import tav_amd  # noqa: F401
    from tav_amd import ops
    dev = "cuda"
    bf, f32 = torch.bfloat16, torch.float32

    def t(*shape, dtype=f32):
        return torch.zeros(*shape, dtype=dtype, device=dev)

    def ids(*shape, hi=3, dtype=torch.int64):
        return (torch.arange(int(torch.tensor(shape).prod()), device=dev) % hi).to(dtype).view(*shape)

    for dt_ in (bf, f32):                                                          # attention: every mask mode, both directions, plain and length-aware
        for S in (128, 129, 200):
            B, nh = 2, 2
            qkv = t(B * S, 3 * nh * 64, dtype=dt_)
            q, k, v = qkv[:, :128], qkv[:, 128:256], qkv[:, 256:]
            for mode in (0, 1, 2):
                km = t(B, S) if mode else None
                for pre in (False, True):
                    for lens in (None, ids(B, hi=S, dtype=torch.int32) + 1):
                        o, lse, corr = ops.attn_fwd(q, k, v, B, S, nh, key_mask=km, mask_mode=mode, q_prescaled=pre, seq_lens=lens)
                        ops.attn_bwd(q, k, v, o, t(B * S, nh * 64, dtype=dt_), lse, corr if mode == 2 else None, B, S, nh, key_mask=km, mask_mode=mode,
                                     q_prescaled=pre, seq_lens=lens)
            o, lse, _ = ops.attn_fwd(q, k, v, B, S, nh)
            ops.attn_probs(q, k, lse, B, S, nh, head_scale=t(nh))
            ops.head_scale(o, o, t(B, nh), -1.0, B, S, nh)
    for rows_ in (1, 16, 17, 8192, 8193):                                          # LayerNorm: the block count on both sides of its clamp and cap
        for W in (64, 768, 1024):
            g, b = t(W), t(W)
            for xdt in (f32, bf):
                x = t(rows_, W, dtype=xdt)
                for lp in (None, bf):
                    _, _, mean, rstd = ops.ln_fwd(x, g, b, 1e-5, lp_dtype=lp)
                    for dydt in (f32, bf):
                        ops.ln_bwd(t(rows_, W, dtype=dydt), x, g, b, mean, rstd, lp_dtype=lp)
            ops.ln_bwd(t(rows_, W), t(rows_, W), g, b, t(rows_), t(rows_), param_grads=False, act=1)
    for dt_ in (bf, f32):                                                          # group norm, GELU backward, the audio front-end
        for B, T, Cc in ((1, 1, 64), (2, 63, 256), (2, 64, 512), (3, 65, 320), (2, 1000, 512)):
            x, g, b = t(B, T, Cc, dtype=dt_), t(Cc), t(Cc)
            y, stats = ops.gn_gelu_fwd(x, g, b, 1e-5)
            ops.gn_gelu_bwd(x, y, g, b, stats)
            ops.gelu_bwd(x.view(-1, Cc), y.view(-1, Cc))
        for T_out in (1, 127, 128, 129, 511, 512, 513, 1025):
            wave, w = t(2, 5 * T_out + 5), t(512, 1, 10)
            y = ops.conv0_fwd(wave, w, t(512), T_out, 5, dt_)
            ops.conv0_bwd_w(wave, y, 10, 5, True)
        ops.col2im_1d(t(2, 19, 3 * 64, dtype=dt_), 2, 40, 19, 64, 3, 2, pre_act=t(2, 40, 64, dtype=dt_))
        ops.group_pad(t(2 * 50, 768), 2, 50, 768, 16, 64, 63, dt_)
        for H, Cg, K in ((768, 48, 128), (64, 16, 8), (4096, 32, 2), (4112, 16, 2)):          # 36864, 1024, 131072 rows (the cap of 512 parts), 65792
            v, g = t(H, Cg, K) + 1.0, t(K)
            w, wf, norms = ops.weight_norm_fwd(v, g, dt_)
            ops.weight_norm_bwd(v, g, norms, t(H // Cg, Cg, K * Cg))
        if dt_ == bf:
            ops.group_pad(t(2 * 50, 768, dtype=bf), 2, 50, 768, 16, 64, 63, bf)
        ops.cast_weight(t(70, 100), dt_)                                           # casts and data movement
        ops.cast_conv_weight(t(16, 8, 3), dt_, conv_stride=2)
        ops.zero_pad_rows(t(2, 12, 64, dtype=dt_), 2, 8, 64, 2)
        for src in (f32, bf):
            ops.cast2d(t(33, 64, dtype=src), dt_)
        ops.transpose2d(t(3 * 40, 72, dtype=dt_), 40, 72, 3)
        ops.add_f32(t(64, 64), t(64, 64), lp_dtype=dt_)
        ops.patchify(t(2, 4, 3, 32, 32), ids(2, 3, hi=8, dtype=torch.int32), dt_)
        ops.mean_pool_bwd(t(2, 768), 2, 9, lp_dtype=dt_)
        ops.mean_pool_bwd(t(2, 768), 2, 9, lp_dtype=dt_, seq_lens=ids(2, hi=9, dtype=torch.int32))
        for rows_, cols in ((8, 64), (333, 100), (700, 768)):                       # fp8: the streaming form, the tiles, the transposed copy
            x = t(rows_, cols, dtype=dt_)
            ops.fp8_quantize(x)
            ops.fp8_quantize(x, want_t=True)
    sts = ops.Fp8States(dev, n=16)                                                 # delayed scaling: the first call of a site calibrates, the second is
    for dt_ in (bf, f32):                                                          # tav_fp8_quantize_delayed -- streaming, tiles, transposed copy
        for rows_, cols, want_t in ((8, 64, False), (333, 100, False), (700, 768, False), (700, 768, True)):
            for _ in range(2):
                ops.fp8_quantize(t(rows_, cols, dtype=dt_), want_t=want_t, state=(sts, (dt_, rows_, cols, want_t)))
    ops.fp8_roll_all()                                                             # tav_fp8_roll_states
    ops.wgrad_fp8(ops.fp8_quantize(t(700, 256, dtype=bf), want_t=True), ops.fp8_quantize(t(700, 384, dtype=bf), want_t=True))     # tav_splitk_reduce

    class DeferredLn(torch.autograd.Function):                                     # a LayerNorm backward inside an autograd pass defers its parameter
        @staticmethod                                                              # reduce: tav_ln_param_reduce_multi when the pass ends (ops.ln_flush)
        def forward(ctx, x, g, b):
            ctx.save_for_backward(x, g, b)
            return x.clone()

        @staticmethod
        def backward(ctx, dy):
            x, g, b = ctx.saved_tensors
            dx, _, dg, db = ops.ln_bwd(dy.contiguous(), x, g, b, t(x.shape[0]), t(x.shape[0]))
            return dx, dg, db

    for nln, W in ((1, 768), (3, 64), (70, 256)):                                  # one item, a few, and more than one launch's 64
        x = t(40, W).requires_grad_()
        y = x
        for _ in range(nln):
            y = DeferredLn.apply(y, t(W).requires_grad_(), t(W).requires_grad_())
        y.sum().backward()
    ops.ln_flush()
    e = [(t(70, 100), t(70, 100, dtype=bf), t(100, 70, dtype=bf)), (t(64, 64), t(64, 64, dtype=bf), None)]
    descs, tiles = ops.make_cast_descs(e, dev)
    ops.cast_weights_multi(descs, 2, blocks_per_tensor=tiles)
    ops.zeros_f32((5000,), dev)
    ops.zeros_f32((4096 * 256 + 1,), dev)
    for rows_ in (1, 255, 256, 257, 65536, 65537):                                 # the embedding sum: parts on both sides of the cap of 256
        ops.embed_add_fwd(t(rows_, 64), ids(rows_), t(3, 64))
        ops.embed_add_bwd(t(rows_, 64), ids(rows_), 3)
    for S in (1, 64, 65, 512):
        ops.text_embed_fwd(ids(2, S, hi=50), t(50, 768), t(520, 768), t(1, 768), t(768), t(768), 1e-5, 1, lp_dtype=bf)
    ops.scatter_add_rows(t(100, 768), ids(100, hi=50), 50)
    ops.gather_rows(t(50, 768), ids(30, hi=50, dtype=torch.int32))
    m = ids(2, 16, hi=2, dtype=torch.uint8)
    ops.mask_to_index(m, 0, 8)
    ops.ragged_lens(m, 8, 8, 4)
    for W in (64, 768, 772):
        ops.mean_pool_fwd(t(2 * 9, W), 2, 9)
        ops.mean_pool_fwd(t(2 * 9, W), 2, 9, seq_lens=ids(2, hi=9, dtype=torch.int32))
    ops.head_fwd(t(4, 3072), t(7, 3072), t(7))
    ops.head_bwd(t(4, 3072), t(7, 3072), t(4, 7))
    ops.tanh_bwd(ops.tanh_fwd(t(4, 768)), t(4, 768))
    logits, target = t(4, 7), ids(4, hi=7)
    loss, _ = ops.cross_entropy(logits, target)
    ops.step_stats(logits=logits, target=target, cm=torch.zeros(49, dtype=torch.int64, device=dev), loss=loss, acc=ops.loop_acc_new(dev))
    seed = torch.ones(1, dtype=torch.int64, device=dev)
    for sd in (7, seed):
        y, mk = ops.dropout_fwd(t(4, 3072), 0.1, sd, 0)
        ops.dropout_bwd(y, mk, 0.1)
        ops.specaug_draw(None, 3, 200, 0.05, 10, 2, sd, ops.SPECAUG_TAG_TIME, device=dev)
    for B, T in ((1, 1), (1, 31), (1, 32), (1, 33), (3, 200)):                      # SpecAugment: parts on both sides of 32 rows
        tm, fm = ids(B, T, hi=2, dtype=torch.uint8), ids(B, 768, hi=2, dtype=torch.uint8)
        ops.specaug_fwd(t(B * T, 768), tm, fm, t(768), B, T)
        ops.specaug_bwd(t(B * T, 768), tm, fm, B, T)
        ops.specaug_bwd(t(B * T, 768), None, fm, B, T, want_dembed=False)
    for src in (torch.zeros(6, 40, 50, 3, dtype=torch.uint8, device=dev), t(3, 6, 40, 50)):     # clip transform: both sources, one and two resizes
        for mid in (None, (36, 44)):
            for hw in ((8, 32), (9, 33), (224, 224)):
                ops.video_clip_transform(src, None, ops.clip_xform(src, [0, 2, 5], mid=mid, out_hw=hw, crop=(2, 3, 30, 40)))
    for sr in (16000, 44100, 48000, 8000):                                         # resampler: identity, the compact table in LDS, up-sampling
        tab = ops.audio_resample_table(sr, 16000, dev)
        for pcm in (t(2, 5000), torch.zeros(5000, 2, dtype=torch.int16, device=dev)):
            ops.audio_resample(pcm, tab)
    torch.cuda.synchronize()


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) == 3 and sys.argv[1] == "--lines":
        print("\n".join(" ".join(r) for r in rows(sys.argv[2])))
        sys.exit(0)
    if len(sys.argv) == 3 and sys.argv[1] == "--family" and sys.argv[2] in ("gemm", "ops"):
        gemm_calls() if sys.argv[2] == "gemm" else op_calls()
        sys.exit(0)
    sys.exit(__doc__)
