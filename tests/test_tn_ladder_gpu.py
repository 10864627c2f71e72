"""The 256-wide weight-gradient (TN) K loop beyond its slot period.

The steady K-tile body of gemm_tn_big_body is compiled once per ring-slot phase (three dY slots x two X slots: period 6), requests the next
tile's first fragments behind a barrier in the middle of the current tile and hands over to the penultimate body.  All of that goes wrong
only at 7 and more K-tiles per workgroup -- tests/test_tn_loop_edges_gpu.py stops at 6 -- so the rows here are 7 .. 14 whole K-tiles of 64
tokens, and the same plus a ragged tail of 1, 63 and 33 tokens: every slot phase is run twice and the steady -> penultimate hand-over happens
at each phase.  Grouped launches through tav_gemm_tn_grouped_ws (ops.gemm_tn_grouped), forced 256-wide (flags bit 0) with explicit split
counts 1, 2 and 3 (flags bits 8-11), one to four problems of N1, N2 in {256, 512}, with and without bias gradients, bf16.

Operands are integers from {-2 .. 2}: with at most 14 * 64 + 63 = 959 tokens every sum has |sum| <= 3836 < 2^24, so f32 accumulates exactly
whatever the order and the expected dW and db are int64 sums made on the host; the comparison is bit for bit.  Inputs, outputs and the
workspace lie under the guard bands of tests/guarded.py, and every case runs twice from the same inputs with equal bits.
"""
import functools

import pytest
import torch

import guarded

pytestmark = pytest.mark.gpu

KT = 64
NTILES = tuple(range(7, 15))
TAILS = (0, 1, 63, 33)
SPLITS = (1, 2, 3)
WIDE = 512                                                   # the pools' width; a problem's operands are column windows of the pools
# problem sets of one grouped launch: (N1, N2, first column of the dY window, first column of the X window)
PROBLEM_SETS = (((256, 256, 256, 0),),
                ((512, 256, 0, 256), (256, 512, 0, 0)),
                ((256, 512, 256, 0), (512, 512, 0, 0), (256, 256, 0, 256)),
                ((512, 512, 0, 0), (256, 256, 256, 256), (512, 256, 0, 0), (256, 512, 0, 0)))
MAX_ROWS = NTILES[-1] * KT + max(TAILS)


@functools.lru_cache(maxsize=None)
def _pools():
    """(dY pool, X pool) as int64 [MAX_ROWS, WIDE] on the CPU, values from {-2 .. 2}."""
    gen = torch.Generator().manual_seed(20250607)
    return (torch.randint(-2, 3, (MAX_ROWS, WIDE), generator=gen), torch.randint(-2, 3, (MAX_ROWS, WIDE), generator=gen))


@functools.lru_cache(maxsize=None)
def _reference():
    """{rows: (dW [WIDE, WIDE], db [WIDE])} as f32 holding exact int64 sums over the pools' first `rows` rows, for every row count of the
    file; summed once, in ascending order of rows, each step adding the product of the new rows only."""
    a, b = _pools()
    out, dW, db, done = {}, torch.zeros(WIDE, WIDE, dtype=torch.int64), torch.zeros(WIDE, dtype=torch.int64), 0
    for rows in sorted({n * KT + t for n in NTILES for t in TAILS}):
        dW = dW + a[done:rows].t() @ b[done:rows]
        db = db + a[done:rows].sum(0)
        done = rows
        assert int(dW.abs().max()) < 2 ** 24 and int(db.abs().max()) < 2 ** 24       # f32 holds every sum
        out[rows] = (dW.float(), db.float())
    return out


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("want_bias", (True, False), ids=("bias", "nobias"))
@pytest.mark.parametrize("nsplit", SPLITS, ids=lambda s: f"x{s}")
@pytest.mark.parametrize("ntiles", NTILES, ids=lambda n: f"kt{n}")
def test_tn_ladder_exact(gpu, ntiles, nsplit, want_bias):
    from tav_amd import ops
    a_pool, b_pool = _pools()
    ref = _reference()
    flags = 1 | nsplit << 8
    for ti, tail in enumerate(TAILS):
        rows = ntiles * KT + tail
        pset = PROBLEM_SETS[(ntiles + ti + nsplit) % len(PROBLEM_SETS)]
        ref_dW, ref_db = ref[rows]
        tag = f"{ntiles} K-tiles + {tail} rows, {nsplit} split(s), bias {int(want_bias)}, {len(pset)} problem(s)"
        with guarded.active() as g:
            pairs = [(guarded.guarded_input(a_pool[:rows, ca:ca + n1].to(torch.bfloat16).contiguous().to(gpu)),
                      guarded.guarded_input(b_pool[:rows, cb:cb + n2].to(torch.bfloat16).contiguous().to(gpu))) for n1, n2, ca, cb in pset]
            first = ops.gemm_tn_grouped(pairs, want_bias=want_bias, flags=flags)
            again = ops.gemm_tn_grouped(pairs, want_bias=want_bias, flags=flags)
            g.verify()
            first = [(w.cpu(), None if d is None else d.cpu()) for w, d in first]
            again = [(w.cpu(), None if d is None else d.cpu()) for w, d in again]
        assert len(first) == len(pset)
        for k, ((n1, n2, ca, cb), (w, d), (w2, d2)) in enumerate(zip(pset, first, again)):
            rw, rd = ref_dW[ca:ca + n1, cb:cb + n2], ref_db[ca:ca + n1]
            assert w.shape == rw.shape and w.dtype == torch.float32
            wrong = int((_bits(w) != _bits(rw)).sum())
            assert wrong == 0, f"{tag}: dW of problem {k} ({n1}x{n2}) differs from the exact sums in {wrong} elements"
            assert torch.equal(_bits(w), _bits(w2)), f"{tag}: dW of problem {k} differs between two runs"
            assert (d is None) == (not want_bias)
            if want_bias:
                wrong = int((_bits(d) != _bits(rd)).sum())
                assert wrong == 0, f"{tag}: db of problem {k} differs from the exact sums in {wrong} elements"
                assert torch.equal(_bits(d), _bits(d2)), f"{tag}: db of problem {k} differs between two runs"
