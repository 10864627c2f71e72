"""Guard-band allocator for the kernel tests.

While a guard is active, the name `torch` inside tav_amd.ops and tav_amd.engine is a proxy whose empty / empty_like / empty_strided / zeros
place every tensor in the middle of a buffer filled with byte 0xFF.  0xFF bytes read as NaN in f32, bf16 and e4m3, as -1 in int32 / int64
and as 255 in uint8, so

  * an output element the kernel never writes is NaN (or an impossible index) instead of whatever the allocator's last tenant left there,
  * a store before / after the tensor, or into the gap between the rows of a strided one, lands in memory the test owns and verify() reports it
    with the allocation's call site, shape, dtype, side and byte offset,
  * guarded_input() puts an operand into such a buffer too (optionally with a wider row pitch): a read past the logical tensor that reaches the
    result yields NaN, and verify() checks that operands and their surroundings are bit for bit what they were.

Nothing here launches a kernel of its own or changes one: it only decides where tensors live.  Works on CPU tensors as well (tests/
test_guarded_alloc_host.py tests the tester).
"""
import contextlib
import sys

import torch as _torch

FILL = 0xFF
GUARD_ROWS = 256             # the tallest tile in the library
GUARD_MIN = 64 * 1024
GUARD_MIN_FLAT = 1 << 20     # 1-D tensors are mostly scratch slabs whose row structure only the kernel knows: a generous flat band
ALIGN = 256

_SAME_SIZE_INT = {1: _torch.uint8, 2: _torch.int16, 4: _torch.int32, 8: _torch.int64}
_HERE = __file__.rsplit(".", 1)[0]


class GuardError(AssertionError):
    pass


def _up(n, m):
    return (n + m - 1) // m * m


def _span_elems(shape, strides):
    if any(s == 0 for s in shape):
        return 0
    return 1 + sum((s - 1) * st for s, st in zip(shape, strides))


def _call_site():
    """file:line of the allocation: the innermost frame inside the package (ops.py / engine.py), else the first frame outside this module."""
    f = sys._getframe(1)
    outside = None
    while f is not None:
        fn = f.f_code.co_filename
        if not fn.startswith(_HERE):
            if outside is None:
                outside = f"{fn}:{f.f_lineno}"
            if fn.endswith(("ops.py", "engine.py")):
                return f"{fn}:{f.f_lineno}"
        f = f.f_back
    return outside or "?"


class _Alloc:
    __slots__ = ("raw", "lead", "span", "shape", "strides", "dtype", "site", "kind", "snapshot", "dense")

    def describe(self):
        return f"{self.kind} {tuple(self.shape)} strides {tuple(self.strides)} {self.dtype} allocated at {self.site}"

    def element_bytes(self):
        """uint8 [span]: 1 where a byte belongs to an element of the tensor, 0 in the gaps between its rows."""
        cover = _torch.zeros(self.span, dtype=_torch.uint8, device=self.raw.device)
        if self.span:
            cover.view(_SAME_SIZE_INT[self.dtype.itemsize]).as_strided(self.shape, self.strides).fill_(-1 if self.dtype.itemsize > 1 else 255)
        return cover.ne(0)


class Guard:
    """One guarded region of a test: hands out tensors and checks their surroundings afterwards."""

    def __init__(self):
        self.allocs = []

    # ------------------------------------------------------------------------------------------ allocation
    def _place(self, shape, strides, dtype, device, kind, site):
        shape, strides = tuple(int(s) for s in shape), tuple(int(s) for s in strides)
        item = dtype.itemsize
        span = _span_elems(shape, strides) * item
        if len(shape) >= 2:
            guard = max(GUARD_MIN, GUARD_ROWS * max(strides[-2], shape[-1]) * item)
        else:
            guard = GUARD_MIN_FLAT
        guard = _up(guard, ALIGN)
        raw = _torch.empty(ALIGN + guard + _up(span, ALIGN) + guard, dtype=_torch.uint8, device=device)
        raw.fill_(FILL)
        a = _Alloc()
        a.raw, a.lead, a.span = raw, (-raw.data_ptr()) % ALIGN + guard, span
        a.shape, a.strides, a.dtype, a.site, a.kind, a.snapshot = shape, strides, dtype, site, kind, None
        a.dense = span == item * _prod(shape)
        self.allocs.append(a)
        t = raw[a.lead:a.lead + span].view(dtype).as_strided(shape, strides)
        assert t.data_ptr() % ALIGN == 0 or span == 0
        return a, t

    def _like_meta(self, fn, args, kw):
        """Shape, strides and dtype exactly as torch's own `fn` would choose them (asked of the meta device), placed under guard."""
        kw = dict(kw)
        device = kw.pop("device", None)
        if device is None:
            device = args[0].device if args and isinstance(args[0], _torch.Tensor) else _torch.empty(0).device
        meta = fn(*args, device="meta", **kw)
        return self._place(meta.shape, meta.stride(), meta.dtype, device, "output", _call_site())[1]

    def empty(self, *args, **kw):
        return self._like_meta(_torch.empty, args, kw)

    def empty_like(self, *args, **kw):
        return self._like_meta(_torch.empty_like, args, kw)

    def empty_strided(self, *args, **kw):
        return self._like_meta(_torch.empty_strided, args, kw)

    def zeros(self, *args, **kw):
        return self._like_meta(_torch.zeros, args, kw).zero_()          # (the elements only: gaps and guards stay 0xFF)

    def input(self, t, pitch_extra=0):
        """A bitwise copy of `t` inside a 0xFF buffer; pitch_extra > 0 widens the row pitch by that many elements (0xFF between the rows)."""
        shape = tuple(t.shape)
        strides = list(_torch.empty(shape, device="meta").stride())
        if pitch_extra and len(shape) >= 2:
            pitch = shape[-1] + int(pitch_extra)
            strides[-2] = pitch
            for d in range(len(shape) - 3, -1, -1):
                strides[d] = strides[d + 1] * shape[d + 1]
        a, v = self._place(shape, strides, t.dtype, t.device, "input", _call_site())
        if v.numel():
            v.view(_SAME_SIZE_INT[t.dtype.itemsize]).copy_(t.contiguous().view(_SAME_SIZE_INT[t.dtype.itemsize]).view(shape))
        a.snapshot = a.raw.clone()
        return v

    # ------------------------------------------------------------------------------------------ checking
    def verify(self):
        """Every guard byte of every allocation still 0xFF, every gap of a strided output still 0xFF, every input buffer bit for bit unchanged."""
        if any(a.raw.is_cuda for a in self.allocs):
            _torch.cuda.synchronize()
        flags = []
        for a in self.allocs:
            if a.snapshot is not None:
                flags.append(a.raw.ne(a.snapshot).any())
            else:
                bad = a.raw[:a.lead].ne(FILL).any() | a.raw[a.lead + a.span:].ne(FILL).any()
                if not a.dense:
                    bad = bad | (a.raw[a.lead:a.lead + a.span].ne(FILL) & ~a.element_bytes()).any()
                flags.append(bad)
        if not flags:
            return
        by_dev = {}
        for i, f in enumerate(flags):
            by_dev.setdefault(f.device, []).append((i, f))
        hit = []
        for items in by_dev.values():
            vals = _torch.stack([f for _, f in items]).tolist()
            hit += [i for (i, _), v in zip(items, vals) if v]
        if not hit:
            return
        msgs = []
        for i in sorted(hit):
            msgs += self._explain(self.allocs[i])
        raise GuardError(f"{len(msgs)} guard violation(s):\n  " + "\n  ".join(msgs[:20]))

    @staticmethod
    def _first(mask):
        return int(mask.nonzero()[0].item()) if bool(mask.any()) else None

    def _explain(self, a):
        raw, lo, hi = a.raw, a.lead, a.lead + a.span
        want = a.snapshot if a.snapshot is not None else _torch.full_like(raw, FILL)
        diff = raw.ne(want)
        out = []
        k = self._first(diff[:lo])
        if k is not None:
            out.append(f"{a.describe()}: leading guard changed, first bad byte {lo - k} before the tensor")
        k = self._first(diff[hi:])
        if k is not None:
            out.append(f"{a.describe()}: trailing guard changed, first bad byte {k} past the tensor's end")
        if a.span and (a.snapshot is not None or not a.dense):
            elem = a.element_bytes()
            k = self._first(diff[lo:hi] & ~elem)
            if k is not None:
                out.append(f"{a.describe()}: row gap changed, first bad byte at offset {k} of the tensor")
            if a.snapshot is not None:
                k = self._first(diff[lo:hi] & elem)
                if k is not None:
                    out.append(f"{a.describe()}: input body changed, first bad byte at offset {k} of the tensor")
        return out


def _prod(shape):
    n = 1
    for s in shape:
        n *= s
    return n


class _TorchProxy:
    """Stands in for the module `torch` inside the patched modules: everything is torch's own, except the four allocators."""

    def __init__(self, guard):
        object.__setattr__(self, "_guard", guard)
        for name in ("empty", "empty_like", "empty_strided", "zeros"):
            object.__setattr__(self, name, getattr(guard, name))

    def __getattr__(self, name):
        return getattr(_torch, name)

    def __setattr__(self, name, value):
        raise AttributeError("the guarded torch proxy is read-only")


_active = []


def current():
    """The innermost active Guard, or None."""
    return _active[-1] if _active else None


def guarded_input(t, pitch_extra=0):
    g = current()
    if g is None:
        raise RuntimeError("guarded_input() outside guarded.active()")
    return g.input(t, pitch_extra)


def _default_modules():
    import tav_amd.engine
    import tav_amd.ops
    return [tav_amd.ops, tav_amd.engine]


@contextlib.contextmanager
def active(modules=None):
    """with active() as g: ...; g.verify().  Patches `torch` in tav_amd.ops / tav_amd.engine (or the given modules) for the duration and drops
    the cached ops.workspace() buffers on entry and on exit, so scratch is reallocated under guard at exactly the size its host formula asks
    for and no guarded buffer outlives the region."""
    modules = _default_modules() if modules is None else list(modules)
    g = Guard()
    proxy = _TorchProxy(g)
    saved = [m.torch for m in modules]
    clear = [m.clear_workspaces for m in modules if hasattr(m, "clear_workspaces")]
    for c in clear:
        c()
    for m in modules:
        m.torch = proxy
    _active.append(g)
    try:
        yield g
    finally:
        _active.pop()
        for m, t in zip(modules, saved):
            m.torch = t
        for c in clear:
            c()
        g.allocs = []
