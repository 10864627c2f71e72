"""-m gpu: every libtavhip kernel against a plain PyTorch reference of the same op (tests/kernel_checks.py), each case inside the guard-band
allocator of tests/guarded.py: outputs and scratch start as 0xFF (NaN) with watched bands around them, operands sit in watched 0xFF buffers."""
import pytest

pytestmark = pytest.mark.gpu


def _cases():
    import kernel_checks
    return kernel_checks.all_checks()


@pytest.mark.parametrize("idx", range(len(_cases())))
def test_kernel_check(gpu, idx):
    import guarded
    cases = _cases()
    with guarded.active() as g:
        for name, err, tol, ok in cases[idx]():
            assert ok, f"{name}: rel err {err:.3e} > tol {tol:.1e}"
        assert g.allocs, "the case allocated nothing under guard"
        g.verify()


def test_guard_bites(gpu):
    """The guard really is in the kernels' way: an output allocated by ops.py is all NaN before the launch and all finite after it, scratch
    comes from the guard at the size the host formula asked for, and nothing guarded is left behind."""
    import torch

    import guarded
    import kernel_checks as kc
    from tav_amd import ops
    with guarded.active() as g:
        a = kc._rnd(130, 64, dtype=torch.bfloat16, seed=1)
        b = kc._rnd(132, 64, dtype=torch.bfloat16, seed=2)
        out = ops.torch.empty(130, 132, dtype=torch.bfloat16, device=a.device)
        assert out.data_ptr() % 256 == 0 and bool(torch.isnan(out.float()).all())
        got = ops.gemm_nt(a, b, out=out)
        assert got.data_ptr() == out.data_ptr() and bool(torch.isfinite(out.float()).all())
        n_before = len(g.allocs)
        fresh = ops.gemm_nt(a, b)                                   # allocated inside ops.gemm_nt
        assert len(g.allocs) == n_before + 1 and g.allocs[-1].site.rsplit(":", 1)[0].endswith("ops.py")
        assert torch.equal(fresh, out)
        part = ops.workspace("guard_probe", 1000, a.device)
        assert part.numel() == 1000 and bool(torch.isnan(part).all())
        g.verify()
    assert ops.torch is torch and not ops._ws
