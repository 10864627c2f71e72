"""fp64 model with per-element bounds of the dense 3-D convolution entry points (include/tavhip_conv.h, csrc/conv3d.hip), in the manner of
gemm_ref.py (whose number formats, GELU terms and DCDF it reuses).  numpy only: shared by tests/test_conv3d_gpu.py and by
tests/test_conv3d_host.py, which tests this tester on the CPU (against torch in float64 and against six mutants).

Tensors here are in torch's layouts (NCDHW activations, [Cout][Cin][3][3][3] weights, [O][C D H W] for the flattened Linear); the GPU test
converts to and from the kernels' padded channels-last layout.

Bounds per output element, u = 2^-24, S = sum |a||b| over the products of the element in fp64, KM = products of one MFMA (bf16 32, f32 4):

  convolution      E_acc = D * 2u * S with D = KM + 1 + ceil(27 Cin_p / KM), Cin_p = ceil(Cin / 16) 16: the chain of gemm_ref.py for the
                   reduction the kernel runs, K pad included.  The input gradient is the same kernel with Cout in Cin's place.
  weight gradient  the reduction runs over voxels, not over 27 Cin_p: L = the voxels the longest slab sums, counted in whole 32-wide patch rows
                   as the kernel stages them, and D = KM + 1 + ceil(L / KM) + nslabs (one more addition per slab in the slab sum).  db rides
                   the same MFMA chain against a fragment of ones: the same D on sum |dz|.
  bias, GELU       as gemm_ref.nt_ref: one rounding for the bias add, E' = 1.13 E + |z| dcdf + u |y| for gelu, 0.8 E + dcdf + 3u + u |g| for gelu'.
  store            f32: u |v|; bf16: half a bf16 ulp at |v| + E.
  dz = dy g        one product of two stored values, rounded once: the store term alone (+ u |v|), and 2^-126 absolute: gelu' underflows for
                   z << 0 and the device may flush a product below the smallest normal number to zero.
  flat linear      f32 fma chains: a thread adds ceil(ceil(S / nparts) / 256) C products, then 6 butterfly steps, 3 adds over the waves, nparts
                   partials and the bias: D u S.  Backward: dx (O + 1) u S + store, dw (B + 1) u S, db (B + 1) u sum |dy|.
  sigmoid          expf 2 ulp, 1 + e, the division: 8u y;  dx = dy (y (1 - y)): three roundings, 4u |dx|.

Exact integer operands (values in -7 .. 7): every partial sum in any order is an integer below 2^24 as long as terms * 49 + 7 < 2^24, so
f32 results equal fp64 bit for bit and bf16 results its round-to-nearest-even.

chain(): the whole VisualClassification step (convs, GELU, flatten + Linear, sigmoid, class-weighted cross entropy, and back) in two modes.
"exact" is float64 throughout.  "chained" rounds where include/tavhip_conv.h says the kernels round (the packed input and weight operands, y
and g, dX, dZ, the flat linear's dx -- to bf16 under "bf16", to f32 under "f32") and does its sums in float32, so its distance from "exact" is
the error the number formats themselves cost on this input: the yardstick e_chain of the model test.
"""
import math

import numpy as np

from gemm_ref import DCDF, GELU_D1, GELU_D2, MFMA_K, U, F, _rnd, _store, bf16_rne, gelu, gelu_d, int_tensor, ratio, round_to  # noqa: F401

TAPS = [(kd, kh, kw) for kd in range(3) for kh in range(3) for kw in range(3)]
TW = 32


def cp(C):
    return (C + 15) // 16 * 16


def chain_len(Cin, dtype):
    km = MFMA_K[dtype]
    return km + 1 + -(-27 * cp(Cin) // km)


# ---------------------------------------------------------------------------------------------- layouts
def to_cl(x, C=None):
    """NCDHW -> padded channels-last [B, D, H, W, Cp] (float64)."""
    B, Cn, D, H, W = x.shape
    out = np.zeros((B, D, H, W, cp(Cn)))
    out[..., :Cn] = np.moveaxis(x, 1, -1)
    return out


def from_cl(x, C):
    """Padded channels-last -> (NCDHW of the first C channels, the pad channels)."""
    return np.moveaxis(x[..., :C], -1, 1), x[..., C:]


# ---------------------------------------------------------------------------------------------- the arithmetic, fp64 (or float32 for chain())
def _window(xp, k, od, oh, ow):
    return xp[:, :, k[0]:k[0] + od, k[1]:k[1] + oh, k[2]:k[2] + ow]


def conv(x, w, pad=0, skip_tap=None, edge=False):
    """z[b, o, d, h, w] = sum x[b, c, d + kd - pad, ...] w[o, c, kd, kh, kw], zeros outside x (edge: the mutant that repeats the edge)."""
    xp = np.pad(x, ((0, 0), (0, 0)) + ((pad, pad),) * 3, mode="edge" if edge else "constant") if pad else x
    od, oh, ow = (s - 2 for s in xp.shape[2:])
    z = np.zeros((x.shape[0], w.shape[0], od, oh, ow), dtype=x.dtype)
    for t, k in enumerate(TAPS):
        if t != skip_tap:
            z += np.einsum("bcdhw,oc->bodhw", _window(xp, k, od, oh, ow), w[:, :, k[0], k[1], k[2]])
    return z


def conv_dgrad(dz, w):
    """The scatter form, written independently of conv(): dx[b, c, d + kd, h + kh, w + kw] += dz[b, o, d, h, w] w[o, c, kd, kh, kw]."""
    B, _, od, oh, ow = dz.shape
    dx = np.zeros((B, w.shape[1], od + 2, oh + 2, ow + 2), dtype=dz.dtype)
    for k in TAPS:
        dx[:, :, k[0]:k[0] + od, k[1]:k[1] + oh, k[2]:k[2] + ow] += np.einsum("bodhw,oc->bcdhw", dz, w[:, :, k[0], k[1], k[2]])
    return dx


def flip_t(w):
    """The input gradient's operand in torch layout: [Cin][Cout][3][3][3], taps reversed."""
    return np.ascontiguousarray(np.transpose(w, (1, 0, 2, 3, 4))[:, :, ::-1, ::-1, ::-1])


def conv_wgrad(x, dz):
    od, oh, ow = dz.shape[2:]
    dw = np.zeros((dz.shape[1], x.shape[1], 3, 3, 3), dtype=x.dtype)
    for k in TAPS:
        dw[:, :, k[0], k[1], k[2]] = np.einsum("bcdhw,bodhw->oc", _window(x, k, od, oh, ow), dz)
    return dw, dz.sum(axis=(0, 2, 3, 4))


# ---------------------------------------------------------------------------------------------- inputs
def inputs(B, Cin, Cout, D, H, W, dtype, seed, O=7):
    """Spread magnitudes: x by channel (period 7) and by column (period 5), weights, bias and dy by output channel (period 11) -- all coprime
    to the tile edges 16 and 32 and to the patch heights; everything rounded to what its buffer holds."""
    rng = np.random.default_rng(seed)
    xs = (2.0 ** (np.arange(Cin) % 7 - 3.0))[None, :, None, None, None] * (2.0 ** (np.arange(W) % 5 - 2.0))[None, None, None, None, :]
    cs = 2.0 ** (np.arange(Cout) % 11 - 5.0)
    x = round_to(rng.standard_normal((B, Cin, D, H, W)) * xs, dtype)[0]
    w = round_to(0.1 * rng.standard_normal((Cout, Cin, 3, 3, 3)) * cs[:, None, None, None, None], dtype)[0]
    b = (rng.standard_normal(Cout) * cs).astype(F).astype(np.float64)
    dy = round_to(rng.standard_normal((B, Cout, D - 2, H - 2, W - 2)) * cs[None, :, None, None, None], dtype)[0]
    return dict(x=x, w=w, b=b, dy=dy, dtype=dtype, Cin=Cin, Cout=Cout)


def int_inputs(B, Cin, Cout, D, H, W, seed):
    x, w = int_tensor((B, Cin, D, H, W), seed), int_tensor((Cout, Cin, 3, 3, 3), seed + 1)
    b, dy = int_tensor((Cout,), seed + 2), int_tensor((B, Cout, D - 2, H - 2, W - 2), seed + 3)
    assert 27 * Cin * 49 + 7 < 2 ** 24 and 27 * Cout * 49 < 2 ** 24 and dy[0, 0].size * B * 49 < 2 ** 24
    return dict(x=x, w=w, b=b, dy=dy, Cin=Cin, Cout=Cout)


# ---------------------------------------------------------------------------------------------- references with bounds
def forward_ref(x, w, b, dtype, gelu_on=True, pad=0):
    """-> dict(y, y_bound[, g, g_bound]) of tav_conv3d_fwd; x, w as the operand dtype holds them; b f32 or None."""
    z, S = conv(x, w, pad), conv(np.abs(x), np.abs(w), pad)
    err = chain_len(x.shape[1], dtype) * 2 * U * S
    if b is not None:
        bb = b[None, :, None, None, None]
        z = z + bb
        err = err + U * (S + np.abs(bb) + err)
    if not gelu_on:
        return dict(y=z, y_bound=_store(z, err, dtype))
    y, g, dc = gelu(z), gelu_d(z), DCDF[dtype]
    return dict(y=y, y_bound=_store(y, GELU_D1 * err + np.abs(z) * dc + U * np.abs(y), dtype),
                g=g, g_bound=_store(g, GELU_D2 * err + dc + 3 * U + U * np.abs(g), dtype))


def dgrad_ref(dz, w, dtype):
    dx, S = conv_dgrad(dz, w), conv_dgrad(np.abs(dz), np.abs(w))
    return dict(dx=dx, dx_bound=_store(dx, chain_len(w.shape[0], dtype) * 2 * U * S, dtype))


def dz_ref(dy, g, dtype):
    v = dy * g
    return dict(dz=v, dz_bound=_store(v, U * np.abs(v), dtype) + 2.0 ** -126)      # (gelu' underflows for z << 0: a product below the smallest normal may be flushed)


def wgrad_chain(B, od, oh, ow, th, nslabs, dtype):
    """D of the weight gradient: the longest slab's voxels in whole patch rows, MFMA by MFMA, plus the slab sum."""
    patches = B * od * -(-oh // th) * -(-ow // TW)
    per_slab = -(-patches // max(1, min(nslabs, patches)))
    km = MFMA_K[dtype]
    return km + 1 + -(-per_slab * th * TW // km) + nslabs


def wgrad_ref(x, dz, dtype, th, nslabs):
    dw, db = conv_wgrad(x, dz)
    Sw, Sb = conv_wgrad(np.abs(x), np.abs(dz))
    D = wgrad_chain(dz.shape[0], *dz.shape[2:], th, nslabs, dtype)
    return dict(dw=dw, dw_bound=_rnd(dw, D * 2 * U * Sw), db=db, db_bound=_rnd(db, D * 2 * U * Sb))


def flat_ref(x, w, b, nparts, dx_dtype="f32", dy=None):
    """x NCDHW (as stored), w [O, C S] f32 values, b [O] -> out and, with dy [B, O], the backward."""
    B, Cn = x.shape[:2]
    S = x[0, 0].size
    xf = x.reshape(B, -1)
    out, Sab = xf @ w.T, np.abs(xf) @ np.abs(w).T
    D = -(-(-(-S // nparts)) // 256) * Cn + 6 + 3 + nparts + 1
    err = D * U * Sab
    if b is not None:
        out = out + b[None, :]
        err = err + U * (np.abs(out) + err)
    res = dict(out=out, out_bound=_rnd(out, err))
    if dy is not None:
        O = w.shape[0]
        dx, Sx = dy @ w, np.abs(dy) @ np.abs(w)
        dw, Sw = dy.T @ xf, np.abs(dy).T @ np.abs(xf)
        res.update(dx=dx.reshape(x.shape), dx_bound=_store(dx, (O + 1) * U * Sx, dx_dtype).reshape(x.shape), dw=dw, dw_bound=_rnd(dw, (B + 1) * U * Sw),
                   db=dy.sum(0), db_bound=(B + 1) * U * np.abs(dy).sum(0) + U)
    return res


def sigmoid_ref(x, dy):
    y = 1.0 / (1.0 + np.exp(-x))
    yk = y.astype(F).astype(np.float64)                  # the backward reads the stored y: exact inputs
    dx = dy * yk * (1.0 - yk)
    return dict(y=y, y_bound=8 * U * y + 2.0 ** -149, dx=dx, dx_bound=4 * U * np.abs(dx) + 2.0 ** -149)


def check(got, ref, names):
    """-> {name: worst |got - ref| / bound} (gemm_ref.ratio: a zero bound demands equality, non-finite is infinitely wrong)."""
    return {n: ratio(got[n], ref[n], ref[n + "_bound"]) for n in names}


def passed(res):
    return all(v <= 1.0 for v in res.values())


# ---------------------------------------------------------------------------------------------- the tester tested: a stand-in kernel with mutants
MUTANTS = {1: "dropped_tap", 2: "unflipped_dgrad_weight", 3: "swapped_ci_co", 4: "missing_halo_zero", 5: "channels_last_flatten_order", 6: "missing_bias"}


def simulate(x, dtype, flat_w, flat_b, mut=0):
    """What correct kernels would store (fp64 arithmetic, each output rounded once to its buffer's type), or one mutant of them.
    x = inputs(...) with Cin == Cout (mutant 3 swaps them).  -> dict(y, g, dz, dx, dw, db, out)."""
    rt = lambda a: round_to(a, dtype)[0]                                    # noqa: E731
    w = np.ascontiguousarray(np.transpose(x["w"], (1, 0, 2, 3, 4))) if mut == 3 else x["w"]
    z = conv(x["x"], w, 0, skip_tap=13 if mut == 1 else None)
    if mut != 6:
        z = z + x["b"][None, :, None, None, None]
    y, g = rt(gelu(z)), rt(gelu_d(z))
    dz = rt(x["dy"] * g)
    if mut == 2:
        dx = conv(dz, np.ascontiguousarray(np.transpose(x["w"], (1, 0, 2, 3, 4))), 2)
    else:
        dx = conv(dz, flip_t(x["w"]), 2, edge=(mut == 4))
    dw, db = conv_wgrad(x["x"], dz)
    yf = np.moveaxis(y, 1, -1).reshape(y.shape[0], -1) if mut == 5 else y.reshape(y.shape[0], -1)
    return dict(y=y, g=g, dz=dz, dx=rt(dx), dw=dw.astype(F).astype(np.float64), db=db.astype(F).astype(np.float64),
                out=(yf @ flat_w.T + flat_b[None, :]).astype(F).astype(np.float64))


def verdict(x, dtype, k, flat_w, flat_b, th=4, nslabs=2):
    """Every check the GPU test makes, on the outputs k of (a stand-in for) the kernels; later stages are fed k's own earlier outputs."""
    f = forward_ref(x["x"], x["w"], x["b"], dtype)
    res = check(k, f, ("y", "g"))
    res.update(check(k, dz_ref(x["dy"], k["g"], dtype), ("dz",)))
    res.update(check(k, dgrad_ref(k["dz"], x["w"], dtype), ("dx",)))
    res.update(check(k, wgrad_ref(x["x"], k["dz"], dtype, th, nslabs), ("dw", "db")))
    res.update(check(k, flat_ref(k["y"], flat_w, flat_b, 1), ("out",)))
    return res


# ---------------------------------------------------------------------------------------------- the whole step, exact and chained
def weighted_ce(logits, target, cw):
    """torch.nn.CrossEntropyLoss(weight=cw) on [B, O] logits: (loss, dlogits)."""
    m = logits - logits.max(1, keepdims=True)
    logp = m - np.log(np.exp(m).sum(1, keepdims=True))
    wt = cw[target]
    loss = -(wt * logp[np.arange(len(target)), target]).sum() / wt.sum()
    d = np.exp(logp) * wt[:, None]
    d[np.arange(len(target)), target] -= wt
    return loss, d / wt.sum()


def chain(x, convs, out_w, out_b, target, cw, dtype, mode):
    """x NCDHW float values, convs = [(w, b), ...] torch layouts, out_w [O, F], out_b [O].  mode "exact": float64; "chained": operands and
    stored activations rounded to `dtype` where the kernels round, sums in float32.  -> dict(logits, loss, grads=[...] in parameter order
    in_layer.weight, in_layer.bias, hidden..., out_layer.weight, out_layer.bias)."""
    ch = mode == "chained"
    rt = (lambda a: round_to(a, dtype)[0]) if ch else (lambda a: np.asarray(a, dtype=np.float64))        # noqa: E731
    ar = (lambda a: np.asarray(a, dtype=F)) if ch else (lambda a: np.asarray(a, dtype=np.float64))      # noqa: E731  (the working type of sums)
    act, saved = rt(x), []
    for w, b in convs:
        wq = rt(w)
        z = conv(ar(act), ar(wq), 0).astype(np.float64) + np.asarray(b, dtype=np.float64)[None, :, None, None, None]
        if ch:
            z = z.astype(F).astype(np.float64)
        y, g = rt(gelu(z)), rt(gelu_d(z))
        saved.append((act, wq, g))
        act = y
    B = act.shape[0]
    xf = act.reshape(B, -1)
    lin = (ar(xf) @ ar(out_w).T).astype(np.float64) + out_b[None, :]
    sig = 1.0 / (1.0 + np.exp(-lin))
    if ch:
        sig = sig.astype(F).astype(np.float64)
    loss, dsig = weighted_ce(ar(sig), target, ar(cw))              # (chained: the loss kernel works and stores in f32)
    loss, dsig = float(loss), dsig.astype(np.float64)
    dlin = dsig * sig * (1.0 - sig)
    if ch:
        dlin = dlin.astype(F).astype(np.float64)
    g_out_w, g_out_b = (ar(dlin).T @ ar(xf)).astype(np.float64), dlin.sum(0)
    d = rt((ar(dlin) @ ar(out_w)).astype(np.float64)).reshape(act.shape)
    grads = []
    for k in range(len(convs) - 1, -1, -1):
        xin, wq, g = saved[k]
        dz = rt(d * g)
        dw, db = conv_wgrad(ar(xin), ar(dz))
        grads = [dw.astype(np.float64), db.astype(np.float64)] + grads
        if k > 0:
            d = rt(conv_dgrad(ar(dz), ar(wq)).astype(np.float64))
    return dict(logits=sig, loss=float(loss), grads=grads + [g_out_w, g_out_b])


def rel_max(got, ref):
    """Tensor-wise error relative to the tensor's largest magnitude."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(got - ref).max() / max(float(np.abs(ref).max()), 1e-300))
