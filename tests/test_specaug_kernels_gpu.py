"""GPU: the SpecAugment kernels (csrc/specaug.hip) against their host model (tests/specaug_ref.py).

tav_specaug_draw / _dev: mask bytes and span counts bit-equal to the model; tav_specaug_fwd and the dx of tav_specaug_bwd: bit-equal (they
are selects); dembed: within the any-order f32 summation bound gamma_{k-1} * sum|dy| of the float64 sum per column (k = masked rows,
u = 2^-24, gamma_n = n u / (1 - n u)), bitwise equal between two launches, exact zeros for k = 0.

Every test runs inside the guard-band allocator (tests/guarded.py): outputs start as 0xFF, operands sit in watched buffers, and verify()
reports any store outside a tensor or into an operand."""
import functools

import numpy as np
import pytest
import torch

import guarded
import specaug_ref as R
import tav_amd  # noqa: F401
from tav_amd import ops

pytestmark = pytest.mark.gpu
SEEDS = [12345, (1 << 63) + 5, (1 << 64) - 17]


def _g(t):
    return t if t is None or guarded.current() is None else guarded.guarded_input(t)


def under_guard(fn):
    @functools.wraps(fn)
    def run(*args, **kw):
        with guarded.active() as g:
            fn(*args, **kw)
            assert g.allocs
            g.verify()
    return run


def _i64(v):
    return v - (1 << 64) if v >= (1 << 63) else v


def _check_draw(valid, B, L, prob, length, min_masks, seed, tag):
    want_m, want_n, _ = R.draw(valid, B, L, prob, length, min_masks, seed, tag)
    v = None if valid is None else _g(torch.from_numpy(valid).cuda())                     # bool [B, L]: one byte per element
    m0, n0 = ops.specaug_draw(v, B, L, prob, length, min_masks, seed, tag, device="cuda", want_nspans=True)
    word = _g(torch.tensor([_i64(seed)], dtype=torch.int64, device="cuda"))
    m1, n1 = ops.specaug_draw(v, B, L, prob, length, min_masks, word, tag, want_nspans=True)
    m2 = ops.specaug_draw(v, B, L, prob, length, min_masks, seed, tag, device="cuda")      # without the span counts
    where = f"L={L} length={length} prob={prob} seed={seed:#x} valid={'none' if valid is None else 'lens'}"
    assert m0.dtype == torch.uint8 and m0.shape == (B, L) and n0.dtype == torch.int32
    assert np.array_equal(n0.cpu().numpy(), want_n), (where, n0.tolist(), want_n.tolist())
    assert np.array_equal(m0.cpu().numpy(), want_m), where
    assert torch.equal(m0, m1) and torch.equal(n0, n1) and torch.equal(m0, m2), where
    return want_m, want_n


@pytest.mark.parametrize("L", [10, 11, 49, 257, 600])
@under_guard
def test_draw_equals_host_model(gpu, L):
    """length 10 at L = 10 (exactly one start), 11 (two), 49 (the tiny preset), 257 (past one 256-thread stride), 600 (several); rows of
    length L, 10, 9 and 0 -- the last two cannot hold a span and stay empty; the same without a validity mask."""
    B = 4
    lens = np.array([L, 10, 9, 0])
    valid = np.arange(L)[None, :] < lens[:, None]
    for seed in SEEDS:
        m, n = _check_draw(valid, B, L, 0.05, 10, 2, seed, R.TAG_TIME)
        assert n[1] == 1 and m[1, :10].all() and not m[1, 10:].any()
        assert n[2] == 0 and n[3] == 0 and not m[2:].any()
        assert 1 <= n[0] <= min(L - 9, L // 10) and not (m.astype(bool) & ~valid).any()
        m, n = _check_draw(None, B, L, 0.05, 10, 2, seed, R.TAG_TIME)
        assert len(set(n.tolist())) == 1 and n[0] >= 1
    if L >= 257:                                                        # many spans: one selection pass each
        m, n = _check_draw(valid, B, L, 0.9, 10, 2, SEEDS[1], R.TAG_TIME)
        assert n[0] >= 20


@under_guard
def test_draw_feature_axis(gpu):
    """L = 64, spans of 4 channels, prob 0.2, min_masks 1, no validity mask: the feature-axis call; its tag draws another stream."""
    for seed in SEEDS:
        m, n = _check_draw(None, 4, 64, 0.2, 4, 1, seed, R.TAG_FEATURE)
        assert n[0] in (3, 4) and len(set(n.tolist())) == 1
        mt, _ = _check_draw(None, 4, 64, 0.2, 4, 1, seed, R.TAG_TIME)
        assert not np.array_equal(m, mt)


def _masks(kind, B, T, H, gen):
    tm = fm = None
    if kind in ("both", "time"):
        tm = torch.rand(B, T, generator=gen) < 0.3
        tm[0, 0] = True
    if kind in ("both", "feature"):
        fm = torch.rand(B, H, generator=gen) < 0.3
        fm[B - 1, H - 1] = True
    if kind == "all-time":
        tm = torch.ones(B, T, dtype=torch.bool)
    return tm, fm


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("H", [4, 64, 1024])
@pytest.mark.parametrize("T", [1, 49])
@under_guard
def test_fwd_and_bwd_equal_host_model(gpu, T, H):
    B = 3
    gen = torch.Generator().manual_seed(1000 * T + H)
    x, dy, embed = torch.randn(B * T, H, generator=gen), torch.randn(B * T, H, generator=gen), torch.rand(H, generator=gen)
    u = 2.0 ** -24
    for kind in ("both", "time", "feature", "neither", "all-time"):
        tm, fm = _masks(kind, B, T, H, gen)
        tmn, fmn = (None if tm is None else tm.numpy()), (None if fm is None else fm.numpy())
        # masks as bool (the model's frame mask) and as uint8 (what specaug_draw returns)
        tmd = None if tm is None else _g(tm.cuda() if kind != "time" else tm.to(torch.uint8).cuda())
        fmd = None if fm is None else _g(fm.cuda() if kind != "feature" else fm.to(torch.uint8).cuda())
        xd, dyd, ed = _g(x.cuda()), _g(dy.cuda()), _g(embed.cuda())
        y = ops.specaug_fwd(xd, tmd, fmd, ed, B, T)
        want_y = torch.from_numpy(R.fwd(x.numpy(), tmn, fmn, embed.numpy(), B, T)).float()
        assert torch.equal(_bits(y.cpu()), _bits(want_y)), (kind, T, H)
        dx, de = ops.specaug_bwd(dyd, tmd, fmd, B, T)
        dx2, de2 = ops.specaug_bwd(dyd, tmd, fmd, B, T)
        dx3, none = ops.specaug_bwd(dyd, tmd, fmd, B, T, want_dembed=False)
        want_dx, want_de, k = R.bwd(dy.numpy(), tmn, fmn, B, T)
        want_dx = torch.from_numpy(want_dx).float()
        # (+0.0 where the model has it: a masked element is a stored zero, never -0.0 or a product)
        assert torch.equal(_bits(dx.cpu()), _bits(want_dx)), (kind, T, H)
        assert torch.equal(_bits(dx), _bits(dx2)) and torch.equal(_bits(dx), _bits(dx3)) and none is None
        assert torch.equal(_bits(de), _bits(de2)), (kind, T, H)
        de = de.cpu().double().numpy()
        assert k == (0 if tm is None else int(tm.sum())) and (kind != "all-time" or k == B * T)
        if k == 0:
            assert not de.any() and not np.signbit(de).any()
        else:
            tmr = tmn.reshape(B * T) != 0
            absdy = np.abs(dy.numpy().astype(np.float64))
            if fmn is not None:
                absdy = np.where(np.repeat(fmn.reshape(B, 1, H), T, axis=1).reshape(B * T, H), 0.0, absdy)
            bound = ((k - 1) * u / (1 - (k - 1) * u)) * absdy[tmr].sum(axis=0)
            err = np.abs(de - want_de)
            print(f"dembed {kind} T={T} H={H} k={k}: max err {err.max():.3e}, min slack {(bound - err).min():.3e}")
            assert (err <= bound).all(), (kind, T, H, k, float(err.max()))
