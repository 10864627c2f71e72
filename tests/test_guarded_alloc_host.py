"""CPU: the guard-band allocator of tests/guarded.py does what the GPU kernel tests rely on (no GPU, no library)."""
import types

import pytest
import torch

import guarded

# every dtype multi-modal-emotion_amd/ops.py allocates
DTYPES = [torch.float32, torch.bfloat16, torch.float8_e4m3fn, torch.uint8, torch.int32, torch.int64]


def _fake_module():
    cleared = []
    m = types.SimpleNamespace(torch=torch, clear_workspaces=lambda: cleared.append(1))
    return m, cleared


def _blank_ok(t):
    if t.dtype in (torch.float32, torch.bfloat16, torch.float8_e4m3fn):
        return bool(torch.isnan(t.float()).all())
    return bool((t == (255 if t.dtype == torch.uint8 else -1)).all())


def _alloc_of(g, t):
    (a,) = [a for a in g.allocs if a.raw.data_ptr() <= t.data_ptr() < a.raw.data_ptr() + a.raw.numel()]
    return a


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_allocators_match_torch_and_start_blank(dtype):
    m, cleared = _fake_module()
    with guarded.active([m]) as g:
        assert cleared == [1]
        src = torch.empty(6, 10, dtype=dtype)[:, :8]                    # a strided tensor: empty_like makes it dense, as torch does
        perm = torch.empty(4, 6, 8, dtype=dtype).permute(1, 0, 2)       # dense but permuted: empty_like keeps the strides
        made = [(m.torch.empty(5, 12, dtype=dtype), torch.empty(5, 12, dtype=dtype)),
                (m.torch.empty((3, 5, 12), dtype=dtype, device="cpu"), torch.empty((3, 5, 12), dtype=dtype)),
                (m.torch.empty(7, dtype=dtype), torch.empty(7, dtype=dtype)),
                (m.torch.empty(0, dtype=dtype), torch.empty(0, dtype=dtype)),
                (m.torch.empty_like(src), torch.empty_like(src)),
                (m.torch.empty_like(perm), torch.empty_like(perm)),
                (m.torch.empty_strided((5, 8), (12, 1), dtype=dtype), torch.empty_strided((5, 8), (12, 1), dtype=dtype)),
                (m.torch.zeros(4, 4, dtype=dtype), torch.zeros(4, 4, dtype=dtype))]
        for got, want in made:
            assert got.dtype == want.dtype and got.shape == want.shape and got.stride() == want.stride() and got.device == want.device
            assert got.numel() == 0 or got.data_ptr() % 256 == 0
            a = _alloc_of(g, got) if got.numel() else None
            if a is not None:
                pitch = (got.stride(-2) if got.dim() >= 2 else 1) * dtype.itemsize
                assert a.lead >= max(64 * 1024, 256 * pitch) and a.raw.numel() - a.lead - a.span >= max(64 * 1024, 256 * pitch)
        for got, _ in made[:-1]:
            assert _blank_ok(got)
        z = made[-1][0]
        assert bool((z.float() == 0).all())
        assert m.torch.float32 is torch.float32 and m.torch.Tensor is torch.Tensor        # everything else is torch's own
        g.verify()                                                                        # a clean run reports nothing
        z.fill_(1)
        made[0][0].fill_(1)                                                                # writing the bodies is what kernels do
        g.verify()
    assert m.torch is torch and cleared == [1, 1]


def test_zeros_of_a_strided_output_keeps_gaps_blank():
    g = guarded.Guard()
    t = g.empty_strided((4, 6), (8, 1), dtype=torch.float32)
    t.zero_()
    g.verify()
    gap = t.as_strided((3, 2), (8, 1), 6)
    assert _blank_ok(gap)


def _violation(g):
    with pytest.raises(guarded.GuardError) as e:
        g.verify()
    return str(e.value)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.uint8, torch.int64], ids=str)
def test_one_element_before_and_after_an_output(dtype):
    for where, word in ((-1, "leading guard"), (5 * 12, "trailing guard")):
        g = guarded.Guard()
        other = g.empty(3, 3, dtype=dtype)
        t = g.empty(5, 12, dtype=dtype)
        t.fill_(1)
        t.as_strided((1,), (1,), t.storage_offset() + where).fill_(1)
        msg = _violation(g)
        assert word in msg and "(5, 12)" in msg and str(dtype) in msg and "output" in msg and "(3, 3)" not in msg
        assert __file__.rsplit(".", 1)[0] in msg                                       # the call site
        assert f"first bad byte {dtype.itemsize if where < 0 else 0} " in msg
        del other


def test_write_into_the_row_gap_of_a_strided_output():
    g = guarded.Guard()
    t = g.empty_strided((5, 8), (12, 1), dtype=torch.bfloat16)
    t.fill_(1)
    g.verify()
    t.as_strided((1,), (1,), t.storage_offset() + 8).fill_(1)       # column 8 of row 0: the first gap element
    msg = _violation(g)
    assert "row gap" in msg and "offset 16 " in msg


def test_inputs_are_copied_bitwise_and_watched():
    src = torch.randn(5, 8)
    src[1, 2] = float("nan")
    for dtype in (torch.float32, torch.bfloat16, torch.int64):
        x = src.to(dtype)
        g = guarded.Guard()
        v = g.input(x)
        w = g.input(x, pitch_extra=4)
        assert v.is_contiguous() and w.stride() == (12, 1) and v.dtype == dtype
        bits = {4: torch.int32, 2: torch.int16, 8: torch.int64}[dtype.itemsize]
        assert torch.equal(v.view(bits), x.view(bits)) and torch.equal(w.contiguous().view(bits), x.view(bits))
        assert _blank_ok(w.as_strided((4, 4), (12, 1), w.storage_offset() + 8))
        g.verify()
        w.as_strided((1,), (1,), w.storage_offset() + 12 + 9).fill_(3)                  # the gap after row 1
        msg = _violation(g)
        assert "row gap" in msg and "input" in msg and "strides (12, 1)" in msg and "input body" not in msg
        g = guarded.Guard()
        v = g.input(x)
        w = g.input(x, pitch_extra=4)
        v[2, 3] = 7                                                                     # a store into a `const` operand
        msg = _violation(g)
        assert "input body changed" in msg and "strides (8, 1)" in msg and "strides (12, 1)" not in msg
        assert f"offset {(2 * 8 + 3) * dtype.itemsize} " in msg
        g = guarded.Guard()
        v = g.input(x)
        v.as_strided((1,), (1,), v.storage_offset() - 1).fill_(1)
        assert "leading guard" in _violation(g)
        g = guarded.Guard()
        v = g.input(x)
        v.as_strided((1,), (1,), v.storage_offset() + 40).fill_(1)
        assert "trailing guard" in _violation(g)


def test_three_d_input_pitch_and_nesting():
    x = torch.randn(2, 3, 4)
    m, _ = _fake_module()
    assert guarded.current() is None
    with guarded.active([m]) as g:
        assert guarded.current() is g
        w = guarded.guarded_input(x, pitch_extra=4)
        assert w.stride() == (24, 8, 1) and torch.equal(w, x)
        g.verify()
    assert guarded.current() is None
    with pytest.raises(RuntimeError):
        guarded.guarded_input(x)


def test_context_restores_modules_after_an_exception():
    m, cleared = _fake_module()
    with pytest.raises(ZeroDivisionError):
        with guarded.active([m]):
            assert m.torch is not torch
            1 / 0
    assert m.torch is torch and cleared == [1, 1] and guarded.current() is None
