"""The ends of the weight-gradient (TN) K loops.

The 256-wide body runs a steady K-tile body while two more whole tiles follow, then a penultimate and a last body; the 128-wide body a steady
loop over whole tiles, one iteration that stages the ragged tile and a drain.  Those pieces can only go wrong where the loop begins and ends,
so the shapes here are the smallest that reach each of them: 1 to 6 K-tiles of 64 rows, with and without a ragged last tile, widths with edge
tiles on either axis, every launch form, with and without bias gradients.

Operands are bf16 integers from {-2 .. 2}: with at most 3 x 321 rows every sum is an integer far below 2^24, so dW and db are exact in f32
whatever the order of summation, the expected values are exact CPU sums and the comparison is ==.  Every case runs under the guard bands
of tests/guarded.py, twice from the same inputs with bit-equal outputs.
"""
import functools

import pytest
import torch

import guarded

pytestmark = pytest.mark.gpu

ROWS = (1, 63, 64, 65, 128, 129, 192, 193, 256, 257, 321)
WIDTHS = ((256, 256), (264, 256), (256, 520), (768, 264))
# (name, kind, argument): grouped launches by `flags` (tavhip.h: bit 0 the 256-wide form, bits 8.. an explicit split count, bit 1 the 128-wide
# form with its bias partials spread over the tile row), the workspace-free grouped call (128-wide, no spreading), tav_gemm_tn by batch count
PATHS = (("big", "grouped", 1), ("big.s1", "grouped", 1 | 1 << 8), ("big.s2", "grouped", 1 | 2 << 8), ("big.s3", "grouped", 1 | 3 << 8),
         ("small.spread", "grouped", 2), ("small.plain", "plain", None), ("single.nb1", "single", 1), ("single.nb3", "single", 3))


@functools.lru_cache(maxsize=None)
def _problem(rows, n1, n2):
    """(a, b, dW, db) on the CPU: the bf16 operands and their exact sums (every value and every sum an integer f32 holds exactly)."""
    gen = torch.Generator().manual_seed(7919 * rows + 31 * n1 + n2)
    a = torch.randint(-2, 3, (rows, n1), generator=gen).to(torch.bfloat16)
    b = torch.randint(-2, 3, (rows, n2), generator=gen).to(torch.bfloat16)
    dW, db = a.double().t() @ b.double(), a.double().sum(0)
    assert dW.abs().max() < 2 ** 24
    return a, b, dW.float(), db.float()


def _empty_split(rows, nsplit):
    return (nsplit - 1) * (((rows + nsplit - 1) // nsplit + 63) // 64 * 64) >= rows      # (the library refuses it)


def _launch(kind, arg, a, b, rows, want_bias):
    """-> [(dW, db | None), ...] of one launch; a, b: [nbatch * rows, N] on the GPU."""
    from tav_amd import ops
    n1, n2 = a.shape[1], b.shape[1]
    if kind == "grouped":                                   # two problems per launch: (a, b) and, behind it in the tile list, (b, a)
        return ops.gemm_tn_grouped([(a, b), (b, a)], want_bias=want_bias, flags=arg)
    if kind == "plain":
        g = guarded.current()
        pairs, outs = [(a, b), (b, a)], []
        probs = (ops.L.GemmTNProblem * 2)()
        for pr, (x, y) in zip(probs, pairs):
            dW = g.empty((x.shape[1], y.shape[1]), dtype=torch.float32, device=x.device)
            db = g.empty((x.shape[1],), dtype=torch.float32, device=x.device) if want_bias else None
            pr.A, pr.B, pr.out, pr.dbias = ops.ptr(x), ops.ptr(y), ops.ptr(dW), ops.ptr(db)
            pr.N1, pr.N2, pr.lda, pr.ldb = x.shape[1], y.shape[1], x.stride(0), y.stride(0)
            outs.append((dW, db))
        ops.check(ops.lib().tav_gemm_tn_grouped(probs, 2, rows, ops.dt(a), ops.stream()), "gemm_tn_grouped")
        return outs
    r = ops.gemm_tn(a, b, N1=n1, N2=n2, lda=n1, ldb=n2, rows_per_batch=rows, nbatch=arg, a_zb=rows * n1, b_zb=rows * n2, want_bias=want_bias)
    return [r if want_bias else (r, None)]


@pytest.mark.parametrize("widths", WIDTHS, ids=lambda w: f"{w[0]}x{w[1]}")
@pytest.mark.parametrize("path", PATHS, ids=lambda p: p[0])
def test_tn_loop_ends_exact(gpu, path, widths):
    name, kind, arg = path
    n1, n2 = widths
    nbatch = arg if kind == "single" else 1
    nsplit = (arg >> 8) if kind == "grouped" else 0
    ran = 0
    for rows in ROWS:
        if nsplit > 1 and _empty_split(rows, nsplit):
            continue
        a_cpu, b_cpu, dW, db = _problem(rows * nbatch, n1, n2)
        want = [(dW, db), (dW.t(), b_cpu.double().sum(0).float())]
        for want_bias in (True, False):
            tag = f"{name} {n1}x{n2} rows {rows} bias {int(want_bias)}"
            with guarded.active() as g:
                a, b = guarded.guarded_input(a_cpu.to(gpu)), guarded.guarded_input(b_cpu.to(gpu))
                first = _launch(kind, arg, a, b, rows, want_bias)
                again = _launch(kind, arg, a, b, rows, want_bias)
                g.verify()
                first = [(w.cpu(), None if d is None else d.cpu()) for w, d in first]
                again = [(w.cpu(), None if d is None else d.cpu()) for w, d in again]
            for k, ((w, d), (w2, d2), (rw, rd)) in enumerate(zip(first, again, want)):
                assert torch.equal(w, rw), f"{tag}: dW of problem {k} differs from the exact sums in {int((w != rw).sum())} elements"
                assert torch.equal(w.view(torch.int32), w2.view(torch.int32)), f"{tag}: dW of problem {k} differs between two runs"
                assert (d is None) == (not want_bias)
                if want_bias:
                    assert torch.equal(d, rd), f"{tag}: db of problem {k} differs from the exact sums in {int((d != rd).sum())} elements"
                    assert torch.equal(d.view(torch.int32), d2.view(torch.int32)), f"{tag}: db of problem {k} differs between two runs"
            ran += 1
    assert ran >= 8                                         # (three splits leave only 129, 192, 257 and 321 rows without an empty split)
