#!/usr/bin/env python3
"""The host decisions of the GEMM entry points as a table (tests/golden/gemm_plan_golden.json), taken from a built libtavhip.so through
ctypes.  No call here launches anything: the planners are host arithmetic, and every case put on a launching entry point carries an
argument fault that is refused before the launch.

    python tests/make_gemm_plan_golden.py --lib <libtavhip.so of the commit to record> --commit <its hash>

tests/test_gemm_plan_host.py replays table(lib) against the library of the tree and demands equality on every row; the axes below are also
the sweep of tests/host/gemm_plan_check.cpp (same order), whose lines are compared with the same table."""
import base64
import ctypes as C
import itertools
import json
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "gemm_plan_golden.json")
F32, BF16, FP8 = 0, 1, 2

# ---- tav_gemm_nt_schedule: full cross product, in this nesting order (outermost first)
NT_DTYPES = [(BF16, BF16), (BF16, F32), (F32, BF16), (F32, F32), (FP8, BF16), (FP8, F32)]      # (F32, BF16) is refused: in the table as a code
NT_NZB = [1, 3]
NT_M = [1, 7, 128, 255, 256, 257, 1000, 4096, 11712, 23424, 46848, 46885, 255968]
NT_N = [4, 128, 132, 256, 768, 2304, 3072]
NT_KBYTES = [1, 2, 6, 12, 36, 37, 48]                       # K * element size / 128
NT_HINTS = [0, 2, 3, 4, 8, 16, 17]
NT_BITS = range(32)                                         # bit 0 resid, 1 accumulate, 2 act = 1, 3 gelu_in, 4 C_pre
NT_BLOCK = len(NT_HINTS) * 32                               # results per (dtypes, nzb, M, N, K)

# ---- tav_gemm_tn_splits
TN_N = [4, 128, 136, 512, 768, 1536, 2304, 3072]
TN_ROWS = [1, 63, 64, 255, 256, 257, 1464, 7999, 11712, 46848]
TN_NBATCH = [1, 8, 32]

# ---- tav_gemm_tn_grouped_ws_bytes
WS_SHAPES = {"layer": [(2304, 768), (768, 768), (3072, 768), (768, 3072)], "ragged": [(384, 136), (136, 264), (256, 512), (520, 128)]}
WS_ROWS = [100, 777, 2047, 2048, 5856, 12287, 12288, 46848]
WS_FLAGS = [0, 1, 2, 1 | (1 << 8), 1 | (2 << 8), 1 | (3 << 8), 1 | (4 << 8)]

PTR = 0x1000                                                # stands for a device pointer: tested for NULL-ness, never read on the host


def _structs():
    from tav_amd import _lib
    return _lib


def nt_args(in_dt, out_dt, nzb, M, N, kbytes, hint, bits):
    L = _structs()
    es = {F32: 4, BF16: 2, FP8: 1}[in_dt]
    g = L.GemmNTArgs()
    g.A = g.B = g.C = PTR
    g.M, g.N, g.K = M, N, kbytes * 128 // es
    g.lda = g.ldb = g.K
    g.ldc = g.ld_pre = g.ld_gelu_in = g.ld_resid = N
    g.in_dtype, g.out_dtype, g.nzb, g.nzg, g.tile_m_hint, g.alpha = in_dt, out_dt, nzb, 1, hint, 1.0
    g.resid = PTR if bits & 1 else None
    g.accumulate = 1 if bits & 2 else 0
    g.act = 1 if bits & 4 else 0
    g.gelu_in = PTR if bits & 8 else None
    g.C_pre = PTR if bits & 16 else None
    return g


def nt_schedule_rows(h):
    """One 'rc,tile,rows_first,tile_rest' per case, in axis order."""
    t, r, tr = C.c_int32(), C.c_int32(), C.c_int32()
    rows = []
    for (i, o), nzb, M, N, kb in itertools.product(NT_DTYPES, NT_NZB, NT_M, NT_N, NT_KBYTES):
        for hint in NT_HINTS:
            for bits in NT_BITS:
                t.value = r.value = tr.value = 0
                rc = h.tav_gemm_nt_schedule(C.byref(nt_args(i, o, nzb, M, N, kb, hint, bits)), C.byref(t), C.byref(r), C.byref(tr))
                rows.append(f"{rc},{t.value},{r.value},{tr.value}")
    return rows


def pack(rows):
    codes = sorted(set(rows))
    assert len(codes) < 65536
    idx = {c: k for k, c in enumerate(codes)}
    arr = np.array([idx[x] for x in rows], dtype="<u2")
    return {"codes": codes, "count": len(rows), "index_u16_zlib_b64": base64.b64encode(zlib.compress(arr.tobytes(), 9)).decode()}


def unpack(p):
    arr = np.frombuffer(zlib.decompress(base64.b64decode(p["index_u16_zlib_b64"])), dtype="<u2")
    assert len(arr) == p["count"]
    return [p["codes"][k] for k in arr]


def nt_case_of_row(k):
    """The arguments of row k of the schedule table (for a failure message)."""
    axes = list(itertools.product(NT_DTYPES, NT_NZB, NT_M, NT_N, NT_KBYTES, NT_HINTS, NT_BITS))
    (i, o), nzb, M, N, kb, hint, bits = axes[k]
    return dict(in_dtype=i, out_dtype=o, nzb=nzb, M=M, N=N, kbytes=kb, hint=hint, bits=bits)


def tn_splits_rows(h):
    cr, ns = C.c_int32(), C.c_int32()
    rows = []
    for n1, n2, rpb, nb in itertools.product(TN_N, TN_N, TN_ROWS, TN_NBATCH):
        rc = h.tav_gemm_tn_splits(n1, n2, rpb, nb, C.byref(cr), C.byref(ns))
        rows.append([rc, cr.value, ns.value])
    return rows


def problems(shapes, bias=True, **edit):
    L = _structs()
    probs = (L.GemmTNProblem * max(len(shapes), 1))()
    for k, (n1, n2) in enumerate(shapes):
        probs[k].A = probs[k].B = probs[k].out = PTR
        probs[k].dbias = PTR if bias else None
        probs[k].N1, probs[k].N2, probs[k].lda, probs[k].ldb = n1, n2, n1, n2
    for key, v in edit.items():                             # e.g. A1=None: field A of problem 1
        setattr(probs[int(key[-1])], key[:-1], v)
    return probs


def ws_bytes_rows(h):
    rows = []
    for name, n, r, dt, fl, bias in itertools.product(WS_SHAPES, (1, 2, 3, 4), WS_ROWS, (BF16, F32), WS_FLAGS, (True, False)):
        rows.append(h.tav_gemm_tn_grouped_ws_bytes(problems(WS_SHAPES[name][:n], bias), n, r, dt, fl))
    return rows


# ---- return codes of the launching entry points: INVALID arguments only.  Each case names its faults; the code of the parent commit was
# read for every one of them: the fault is met by a test that returns before hipLaunchKernelGGL.  (A workspace too small sends
# tav_gemm_tn_grouped_ws to tav_gemm_tn_grouped: wherever that matters the case says which of the two answers.)
def _nt(**kw):
    g = nt_args(BF16, BF16, 1, 256, 256, 2, 0, 0)           # valid by itself: K = 128, lda = ldb = 128, ldc = 256
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def _tn(**kw):
    L = _structs()
    g = L.GemmTNArgs()
    g.A = g.B = g.slabs = g.out = PTR
    g.N1 = g.N2 = g.lda = g.ldb = 128
    g.rows_per_batch, g.nbatch, g.chunk_rows, g.nsplit, g.dtype, g.scale = 256, 1, 256, 1, BF16, 1.0
    for k, v in kw.items():
        setattr(g, k, v)
    return g


BIG_WS = 1 << 40                                            # "workspace_bytes" of a workspace that is never touched
RAGGED = WS_SHAPES["ragged"]


def invalid_cases(h):
    """[(entry point, case name, thunk -> rc)]"""
    nt = lambda **kw: (lambda: h.tav_gemm_nt(C.byref(_nt(**kw)), None))
    tn = lambda **kw: (lambda: h.tav_gemm_tn(C.byref(_tn(**kw)), None))
    grp = lambda shapes=RAGGED, n=4, rows=777, dt=BF16, bias=True, **e: (lambda: h.tav_gemm_tn_grouped(problems(shapes, bias, **e), n, rows, dt, None))
    gws = lambda shapes=RAGGED, n=4, rows=777, dt=BF16, ws=PTR, nbytes=BIG_WS, flags=0, bias=True, **e: (
        lambda: h.tav_gemm_tn_grouped_ws(problems(shapes, bias, **e), n, rows, dt, ws, nbytes, flags, None))
    cs = lambda x=PTR, dt=BF16, M=100, N=64, ld=64, part=PTR, nparts=4, out=PTR: (lambda: h.tav_colsum(x, dt, M, N, ld, part, nparts, out, 0, None))
    cases = [
        ("tav_gemm_nt", "args NULL", lambda: h.tav_gemm_nt(None, None)),
        ("tav_gemm_nt", "A NULL", nt(A=None)), ("tav_gemm_nt", "B NULL", nt(B=None)), ("tav_gemm_nt", "C NULL", nt(C=None)),
        ("tav_gemm_nt", "M 0", nt(M=0)), ("tav_gemm_nt", "N 0", nt(N=0)), ("tav_gemm_nt", "K 0", nt(K=0)), ("tav_gemm_nt", "M negative", nt(M=-5)),
        ("tav_gemm_nt", "in_dtype 7", nt(in_dtype=7)), ("tav_gemm_nt", "out_dtype 5", nt(out_dtype=5)), ("tav_gemm_nt", "f32 in, bf16 out", nt(in_dtype=F32, K=32, lda=32, ldb=32)),
        ("tav_gemm_nt", "K 100: no whole K-tile", nt(K=100)), ("tav_gemm_nt", "fp8 K 64", nt(in_dtype=FP8, K=64, lda=64, ldb=64)),
        ("tav_gemm_nt", "A slice past 32-bit staging offsets", nt(M=255968, lda=16384)), ("tav_gemm_nt", "B slice past 32-bit staging offsets", nt(N=2304, ldc=2304, ldb=1 << 20)),
        ("tav_gemm_nt", "N 130", nt(N=130)), ("tav_gemm_nt", "ldc past the epilogue's 32-bit offsets", nt(ldc=1 << 22)),
        ("tav_gemm_nt", "ld_resid past the offsets, resid given", nt(resid=PTR, ld_resid=1 << 22)),
        ("tav_gemm_nt", "lda 129", nt(lda=129)), ("tav_gemm_nt", "ldb 132", nt(ldb=132)), ("tav_gemm_nt", "ldc 258", nt(ldc=258)),
        ("tav_gemm_nt", "a_zb 1", nt(a_zb=1)), ("tav_gemm_nt", "b_zg 4", nt(b_zg=4)), ("tav_gemm_nt", "c_zb 2", nt(c_zb=2)), ("tav_gemm_nt", "gelu_zb 2", nt(gelu_zb=2)),
        ("tav_gemm_nt", "A NULL x M 0", nt(A=None, M=0)), ("tav_gemm_nt", "in_dtype 7 x lda 129", nt(in_dtype=7, lda=129)),
        ("tav_gemm_nt", "M 0 x in_dtype 7", nt(M=0, in_dtype=7)), ("tav_gemm_nt", "K 100 x lda 129", nt(K=100, lda=129)), ("tav_gemm_nt", "N 130 x ldc 258", nt(N=130, ldc=258)),
        ("tav_gemm_nt", "out_dtype 5 x K 100", nt(out_dtype=5, K=100)),

        ("tav_gemm_tn", "args NULL", lambda: h.tav_gemm_tn(None, None)),
        ("tav_gemm_tn", "A NULL", tn(A=None)), ("tav_gemm_tn", "B NULL", tn(B=None)), ("tav_gemm_tn", "slabs NULL", tn(slabs=None)), ("tav_gemm_tn", "out NULL", tn(out=None)),
        ("tav_gemm_tn", "N1 0", tn(N1=0)), ("tav_gemm_tn", "N2 0", tn(N2=0)), ("tav_gemm_tn", "rows 0", tn(rows_per_batch=0)), ("tav_gemm_tn", "nbatch 0", tn(nbatch=0)),
        ("tav_gemm_tn", "dtype fp8", tn(dtype=FP8)), ("tav_gemm_tn", "N1 132 (bf16)", tn(N1=132)), ("tav_gemm_tn", "N2 132 (bf16)", tn(N2=132)), ("tav_gemm_tn", "N2 6 (f32)", tn(dtype=F32, N2=6)),
        ("tav_gemm_tn", "lda 132", tn(lda=132)), ("tav_gemm_tn", "ldb 132", tn(ldb=132)), ("tav_gemm_tn", "a_zb 4", tn(a_zb=4)), ("tav_gemm_tn", "b_zb 4", tn(b_zb=4)),
        ("tav_gemm_tn", "chunk_rows 0", tn(chunk_rows=0)), ("tav_gemm_tn", "chunk_rows 100", tn(chunk_rows=100)),
        ("tav_gemm_tn", "rows past 32-bit staging offsets", tn(lda=1 << 24)), ("tav_gemm_tn", "dbias without bias_partials", tn(dbias=PTR)),
        ("tav_gemm_tn", "nsplit 2 of 1", tn(nsplit=2)), ("tav_gemm_tn", "perm_outer 3 does not divide N2", tn(perm_outer=3)), ("tav_gemm_tn", "perm 40 x 3 != N2", tn(perm_inner=40, perm_outer=3)),
        ("tav_gemm_tn", "A NULL x N1 0", tn(A=None, N1=0)), ("tav_gemm_tn", "dtype 9 x lda 132", tn(dtype=9, lda=132)), ("tav_gemm_tn", "dtype 9 x N1 0", tn(dtype=9, N1=0)),
        ("tav_gemm_tn", "dtype 9 x N1 132", tn(dtype=9, N1=132)), ("tav_gemm_tn", "a_zb 4 x staging offsets", tn(a_zb=4, ldb=1 << 24)),
        ("tav_gemm_tn", "chunk_rows 100 x dbias without partials", tn(chunk_rows=100, dbias=PTR)), ("tav_gemm_tn", "dbias without partials x nsplit 2 of 1", tn(dbias=PTR, nsplit=2)),
        ("tav_gemm_tn", "dbias without partials x perm_outer 3", tn(dbias=PTR, perm_outer=3)), ("tav_gemm_tn", "lda 132 x chunk_rows 100", tn(lda=132, chunk_rows=100)),

        ("tav_gemm_tn_grouped", "problems NULL", lambda: h.tav_gemm_tn_grouped(None, 4, 777, BF16, None)),
        ("tav_gemm_tn_grouped", "0 problems", grp(n=0)), ("tav_gemm_tn_grouped", "5 problems", grp(n=5)), ("tav_gemm_tn_grouped", "rows 0", grp(rows=0)),
        ("tav_gemm_tn_grouped", "dtype fp8", grp(dt=FP8)), ("tav_gemm_tn_grouped", "A NULL (0)", grp(A0=None)), ("tav_gemm_tn_grouped", "B NULL (3)", grp(B3=None)),
        ("tav_gemm_tn_grouped", "out NULL (2)", grp(out2=None)), ("tav_gemm_tn_grouped", "N1 0 (1)", grp(N11=0)), ("tav_gemm_tn_grouped", "N1 132 (1)", grp(N11=132)),
        ("tav_gemm_tn_grouped", "N2 6 (f32, 0)", grp(dt=F32, N20=6)), ("tav_gemm_tn_grouped", "lda 388 (0)", grp(lda0=388)), ("tav_gemm_tn_grouped", "ldb 132 (3)", grp(ldb3=132)),
        ("tav_gemm_tn_grouped", "staging offsets (2)", grp(lda2=1 << 24)),
        ("tav_gemm_tn_grouped", "lda 388 (0) x A NULL (1)", grp(lda0=388, A1=None)), ("tav_gemm_tn_grouped", "A NULL (0) x lda 140 (1): problems in order", grp(A0=None, lda1=140)),
        ("tav_gemm_tn_grouped", "dtype 9 x A NULL (0)", grp(dt=9, A0=None)), ("tav_gemm_tn_grouped", "5 problems x dtype 9", grp(n=5, dt=9)),
        ("tav_gemm_tn_grouped", "A NULL (0) x N1 0 (0)", grp(A0=None, N10=0)), ("tav_gemm_tn_grouped", "N1 132 (0) x lda 388 (0)", grp(N10=132, lda0=388)),
        ("tav_gemm_tn_grouped", "lda 388 (0) x staging offsets (0)", grp(lda0=388, ldb0=1 << 24)), ("tav_gemm_tn_grouped", "2 problems: A NULL (1); A NULL (3) is not looked at", grp(n=2, A3=None, A1=None)),

        ("tav_gemm_tn_grouped_ws", "problems NULL", lambda: h.tav_gemm_tn_grouped_ws(None, 4, 777, BF16, PTR, BIG_WS, 0, None)),
        ("tav_gemm_tn_grouped_ws", "0 problems", gws(n=0)), ("tav_gemm_tn_grouped_ws", "5 problems", gws(n=5)), ("tav_gemm_tn_grouped_ws", "rows 0", gws(rows=0)),
        ("tav_gemm_tn_grouped_ws", "dtype fp8", gws(dt=FP8)), ("tav_gemm_tn_grouped_ws", "A NULL (0)", gws(A0=None)), ("tav_gemm_tn_grouped_ws", "out NULL (3)", gws(out3=None)),
        ("tav_gemm_tn_grouped_ws", "N2 0 (1)", gws(N21=0)), ("tav_gemm_tn_grouped_ws", "N1 132 (1)", gws(N11=132)), ("tav_gemm_tn_grouped_ws", "lda 388 (0)", gws(lda0=388)),
        ("tav_gemm_tn_grouped_ws", "staging offsets (2)", gws(ldb2=1 << 24)), ("tav_gemm_tn_grouped_ws", "A NULL (0), flags 1", gws(A0=None, flags=1)),
        ("tav_gemm_tn_grouped_ws", "lda 388 (0), flags 1 | 2 splits, rows 5000", gws(lda0=388, flags=1 | (2 << 8), rows=5000)),
        ("tav_gemm_tn_grouped_ws", "empty split: 3 splits of 100 rows", gws(rows=100, flags=1 | (3 << 8))),
        ("tav_gemm_tn_grouped_ws", "empty split: 4 splits of 130 rows, no bias", gws(rows=130, flags=1 | (4 << 8), bias=False)),
        ("tav_gemm_tn_grouped_ws", "empty split x A NULL (0): the split answers", gws(rows=100, flags=1 | (3 << 8), A0=None)),
        ("tav_gemm_tn_grouped_ws", "empty split x A NULL (0) without workspace: tav_gemm_tn_grouped answers", gws(rows=100, flags=1 | (3 << 8), A0=None, ws=None, nbytes=0)),
        ("tav_gemm_tn_grouped_ws", "empty split x lda 388 (0), workspace 4 bytes short", gws(rows=100, flags=1 | (3 << 8), lda0=388, nbytes=4)),
        ("tav_gemm_tn_grouped_ws", "A NULL (2) without workspace", gws(A2=None, ws=None, nbytes=0)), ("tav_gemm_tn_grouped_ws", "dtype 9 x empty split", gws(dt=9, rows=100, flags=1 | (3 << 8))),
        ("tav_gemm_tn_grouped_ws", "A NULL (0) x N1 0 (0), no bias, no workspace needed", gws(A0=None, N10=0, bias=False, ws=None, nbytes=0)),

        ("tav_colsum", "x NULL", cs(x=None)), ("tav_colsum", "partials NULL", cs(part=None)), ("tav_colsum", "out NULL", cs(out=None)),
        ("tav_colsum", "M 0", cs(M=0)), ("tav_colsum", "N 0", cs(N=0)), ("tav_colsum", "nparts 0", cs(nparts=0)), ("tav_colsum", "dtype fp8", cs(dt=FP8)),
        ("tav_colsum", "x NULL x M 0", cs(x=None, M=0)), ("tav_colsum", "M 0 x dtype fp8", cs(M=0, dt=FP8)),
    ]
    return cases


def invalid_rows(h):
    rows = []
    for entry, name, thunk in invalid_cases(h):
        rc = thunk()
        assert rc in (-1, -2, -3, -4), f"{entry} [{name}] returned {rc}: not an argument fault -- it must not be in this table"
        rows.append([entry, name, rc])
    return rows


def table(h):
    return {"nt_schedule": pack(nt_schedule_rows(h)), "tn_splits": tn_splits_rows(h), "tn_grouped_ws_bytes": ws_bytes_rows(h), "invalid_arguments": invalid_rows(h)}


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True)
    ap.add_argument("--commit", required=True)
    ap.add_argument("--out", default=GOLDEN)
    a = ap.parse_args()
    os.environ["TAV_LIB"] = os.path.abspath(a.lib)
    sys.path.insert(0, os.path.dirname(HERE))
    import tav_amd  # noqa: F401
    from tav_amd import _lib
    doc = {"recorded_from_commit": a.commit, "made_by": "tests/make_gemm_plan_golden.py"}
    doc.update(table(_lib.lib()))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(a.out, os.path.getsize(a.out), "bytes;", doc["nt_schedule"]["count"], "schedule rows,", len(doc["nt_schedule"]["codes"]), "distinct")
