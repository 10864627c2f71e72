"""A fixed list of GEMM calls through tav_amd.ops, once each, no timing: the launches a change of the GEMM host code must leave as they are.

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python tools/gemm_launch_list.py        (GPU box; a run of its own, no counters)
    python tools/gemm_launch_list.py --compare OUT_PARENT OUT_NEW                                   (anywhere)

--compare reads the kernel-trace CSVs of two such runs and compares, line for line and in launch order, (kernel name with its template
arguments, grid, workgroup size, LDS bytes) of every libtavhip kernel (namespace tav); exit status 1 when they differ.  Covered: every
epilogue flavour x {bf16 -> bf16, bf16 -> f32, f32, fp8 -> bf16, fp8 -> f32}; tile hints 0 / 2 / 3 / 4 / 8 / 16 / 17; ring hints; grids under
and over one workgroup per CU; the mixed schedule (M = 46885, N = K = 768); batched nzb / nzg; gemm_tn with and without bias and column
permutation; grouped weight gradients with flags 0 / 1 / 2 and one to three splits; the workspace-free fallback; column sums."""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def compare(dir_a, dir_b):
    def rows(d):
        files = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))
        assert files, f"no kernel trace under {d}"
        out = []
        for f in files:
            with open(f) as fh:
                recs = [r for r in csv.DictReader(fh) if "tav::" in r["Kernel_Name"]]
            recs.sort(key=lambda r: int(r["Start_Timestamp"]))
            cols = [c for c in (recs[0] if recs else {}) if c.startswith(("Grid_Size", "Workgroup_Size", "LDS_Block_Size"))]
            assert not recs or len(cols) >= 3, cols
            out += [(r["Kernel_Name"],) + tuple(f"{c}={r[c]}" for c in cols) for r in recs]
        return out
    a, b = rows(dir_a), rows(dir_b)
    diff = [(k, x, y) for k, (x, y) in enumerate(zip(a, b)) if x != y]
    print(f"launches: {len(a)} / {len(b)}; distinct kernels {len({x[0] for x in a})} / {len({x[0] for x in b})}; differing lines {len(diff)}")
    for k, x, y in diff[:10]:
        print(f"  #{k}: {x}\n   vs  {y}")
    same = len(a) == len(b) and not diff
    print("LAUNCH SEQUENCE", "IDENTICAL" if same else "DIFFERENT")
    return 0 if same else 1


def main():
    sys.path[:0] = [ROOT]
    import ctypes as C

    import torch

    import tav_amd  # noqa: F401
    from tav_amd import ops
    dev = "cuda"
    bf, f32, f8 = torch.bfloat16, torch.float32, torch.float8_e4m3fn
    n = 0

    def t(*shape, dtype=bf):
        if dtype == f8:
            return torch.zeros(*shape, dtype=torch.uint8, device=dev).view(f8)
        return torch.zeros(*shape, dtype=dtype, device=dev)

    one = torch.ones(1, dtype=f32, device=dev)

    def nt(in_dt, out_dt, M, N, K, flavour="plain", tile_m=0, **kw):
        nonlocal n
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
        n += 1

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
        n += 1

    for dt_ in (bf, f32):                                                      # weight gradients
        a, b = t(1000, 256, dtype=dt_), t(1000, 384, dtype=dt_)
        ops.gemm_tn(a, b)
        ops.gemm_tn(a, b, want_bias=True)
        a3, b3 = t(3 * 249, 136, dtype=dt_), t(3 * 249, 264, dtype=dt_)
        ops.gemm_tn(a3, b3, N1=136, N2=264, lda=136, ldb=264, rows_per_batch=249, nbatch=3, a_zb=249 * 136, b_zb=249 * 264, perm_inner=88, perm_outer=3,
                    want_bias=True)
        ops.colsum(t(1000, 384, dtype=dt_))
        n += 4
    ragged, layer = [(384, 136), (136, 264), (256, 512), (520, 128)], [(2304, 768), (768, 768), (3072, 768), (768, 3072)]

    def grouped(shapes, rows, dt_, flags, bias=True):
        nonlocal n
        ops.gemm_tn_grouped([(t(rows, n1, dtype=dt_), t(rows, n2, dtype=dt_)) for n1, n2 in shapes], want_bias=bias, flags=flags)
        n += 1

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
        n += 2
    torch.cuda.synchronize()
    print(f"{n} GEMM calls issued")


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    main()
