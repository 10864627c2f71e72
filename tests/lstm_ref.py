"""fp64 restatement of the LSTM recurrence kernels (csrc/lstm.hip, include/tavhip_rnn.h) with per-element bounds, and of the log-sigmoid
(numpy only: shared by tests/test_lstm_host.py, which tests this tester on the CPU, and tests/test_lstm_gpu.py).

Everything is carried padded: Hp = ceil(H / 64) 64, gate q's unit u is row q Hp + u of W_hh [4 Hp, Hp] (PyTorch's order i, f, g, o), pads zero.
A value with its error bound is a V(v, e): v the fp64 value of exact inputs, e >= |what the kernel may hold - v|.

Bounds, u = 2^-24, in the vocabulary of front_ref / norm_ref.  A sum or difference: the operands' errors and u (|result| + error); a product
likewise (so a multiply-add is charged two roundings and the bound holds whether or not it is contracted; the kernel's explicit fmaf rounds
once).  Division is correctly rounded (hipcc's default): u.  expf 6u and tanhf 10u relative (front_ref's figures for the device library)
plus 2^-126 for a flushed result; the error of their argument goes through the function on the interval [z - e, z + e].  Stores: f32 nothing
more, bf16 half an ulp at |v| + e.  The chains, from csrc/lstm.hip:

  forward product   lstm_fwd_kernel: acc from 0 over k0 = 0, KSTEP, ... of mma16: one chain of Hp products per element (bf16: Hp / 32 MFMAs of 32
                    exact products; f32: Hp / 4 MFMAs of 4 rounded products).  Charged gamma(Hp + 2) times sum |w| |h|, gamma(D) = D u / (1 - D u):
                    Hp links and one each for the rounding of an f32 product and for the order inside an MFMA.
  z                 acc + (xproj + b_hh): two additions.
  gates             s(z) = 1 / (1 + expf(-z)): expf, one addition, one division.  tanhf for g and for tanh(c).
  c, h              c = fmaf(f, c, i g), h = o tanhf(c); h is stored in the operand dtype and THAT value is what the next step multiplies.
  backward product  lstm_bwd_kernel: one chain of 4 Hp products of the STORED dZ_t with W_hh^T: gamma(4 Hp + 2) times sum |w| |dz|.
  gate derivatives  d = dy + dh; tc = tanhf(c_t); zo = d tc (o (1 - o)); dc = fmaf(d o, 1 - tc tc, carry); zi = dc g (i (1 - i));
                    zf = dc c_{t-1} (f (1 - f)); zg = dc i (1 - g g); carry' = dc f.

Two modes.  STEP-FED: step t of the reference is fed the kernel's own h_{t-1}, c_{t-1} (backward: its saved gates and cells, its stored dZ_{t+1}
and its traced carry), all with error 0, so every bound is a one-step bound, tight at any T and any weight scale.  CHAINED: the reference runs
alone and every error is propagated through all steps; with PyTorch-scale weights that bound is vacuous, so chained cases draw W_hh from
U(-1/H, 1/H), where the recurrence contracts (chained_cap() states the condition the host test asserts).

MUTANTS of the reference, each of which the test inputs must catch in both modes (tests/test_lstm_host.py).
"""
import numpy as np

from gemm_ref import F, U, bf16_half_ulp, bf16_rne

EXP_REL, TANH_REL = 6 * U, 10 * U
TINY = 2.0 ** -126
MUTANTS = {1: "gate_order_ifog", 2: "h_from_previous_c", 3: "backward_time_reversed", 4: "b_hh_dropped", 5: "pad_column_leaks", 6: "last_step_skipped"}
CHAINED_CAP = {"f32": 1e-4, "bf16": 1e-3}


def hp_of(H):
    return (H + 63) // 64 * 64


def gamma(D):
    return D * U / (1.0 - D * U)


def rnd(x, dtype):
    """x rounded to the storage dtype ("f32" / "bf16"; None: not at all), as float64."""
    if dtype is None:
        return np.asarray(x, np.float64)
    return bf16_rne(x) if dtype == "bf16" else np.asarray(x, np.float64).astype(F).astype(np.float64)


def store_err(v, e, dtype):
    return e + bf16_half_ulp(np.abs(v) + e) if dtype == "bf16" else e


class V:
    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, np.float64)
        self.e = np.zeros_like(self.v) + e


def add(a, b):
    v = a.v + b.v
    e = a.e + b.e
    return V(v, e + U * (np.abs(v) + e))


def mul(a, b):
    v = a.v * b.v
    e = a.e * np.abs(b.v) + b.e * np.abs(a.v) + a.e * b.e
    return V(v, e + U * (np.abs(v) + e))


def one_minus(a):
    v = 1.0 - a.v
    return V(v, a.e + U * (np.abs(v) + a.e))


def neg(a):
    return V(-a.v, a.e)


def vexp(a):
    v = np.exp(a.v)
    e = v * (np.expm1(a.e) + EXP_REL * np.exp(a.e)) + TINY
    return V(v, e)


def vtanh(a):
    v = np.tanh(a.v)
    lo = np.maximum(np.abs(a.v) - a.e, 0.0)
    slope = 1.0 - np.tanh(lo) ** 2
    return V(v, slope * a.e + TANH_REL * (np.abs(v) + slope * a.e) + TINY)


def vsigmoid(z):
    ex = vexp(neg(z))
    d = add(V(np.ones_like(ex.v)), ex)
    v = 1.0 / d.v
    lo = np.maximum(d.v - d.e, 1.0)
    e = d.e / (d.v * lo)
    return V(v, e + U * (v + e))


def matvec(x, W, links):
    """x [B, K] (a V) times W [N, K]^T: one chain of `links` per element."""
    v = x.v @ W.T
    mag = np.abs(x.v) @ np.abs(W).T
    e = x.e @ np.abs(W).T
    return V(v, e + gamma(links) * (mag + e))


# ------------------------------------------------------------------------------------------------ padding
def pad_gate_rows(w, H):
    """[4 H, ...] -> [4 Hp, ...], each gate block padded with zero rows."""
    Hp = hp_of(H)
    w = np.asarray(w, np.float64)
    out = np.zeros((4 * Hp,) + w.shape[1:])
    for q in range(4):
        out[q * Hp:q * Hp + H] = w[q * H:(q + 1) * H]
    return out


def unpad_gate_rows(w, H):
    Hp = w.shape[0] // 4
    return np.concatenate([w[q * Hp:q * Hp + H] for q in range(4)], 0)


def pad_cols(w, H):
    w = np.asarray(w, np.float64)
    out = np.zeros(w.shape[:-1] + (hp_of(H),))
    out[..., :H] = w[..., :H]
    return out


# ------------------------------------------------------------------------------------------------ one step each way
def fwd_step(W, b_hh, xp_t, hprev, cprev, dtype, mut=0, H=None):
    """W [4 Hp, Hp], b_hh [4 Hp] or None, xp_t [B, 4 Hp] (exact values), hprev / cprev V [B, Hp] -> dict of V: i f g o c h (h as stored)."""
    Hp = W.shape[1]
    acc = matvec(hprev, W, Hp + 2)
    zin = V(xp_t) if (b_hh is None or mut == 4) else add(V(xp_t), V(np.broadcast_to(b_hh, xp_t.shape)))
    z = add(acc, zin)
    if mut == 5 and H is not None and H < Hp:
        leak = np.zeros(4 * Hp)
        for q in range(4):
            leak[q * Hp + H:(q + 1) * Hp] = 1.0
        z = V(z.v + leak, z.e)
    blocks = [V(z.v[:, q * Hp:(q + 1) * Hp], z.e[:, q * Hp:(q + 1) * Hp]) for q in range(4)]
    if mut == 1:
        blocks[2], blocks[3] = blocks[3], blocks[2]
    i, f, g, o = vsigmoid(blocks[0]), vsigmoid(blocks[1]), vtanh(blocks[2]), vsigmoid(blocks[3])
    c = add(mul(f, cprev), mul(i, g))
    h = mul(o, vtanh(cprev if mut == 2 else c))
    return dict(i=i, f=f, g=g, o=o, c=c, h=V(h.v, store_err(h.v, h.e, dtype)))       # (the centre stays the unrounded value)


def bwd_step(W, gates, ct, cprev, dy_t, dh, dc_in, dtype):
    """gates: dict of V i f g o; ct, cprev, dh (dY excluded), dc_in: V [B, Hp]; dy_t exact -> (dz V [B, 4 Hp] as stored, carry V)."""
    i, f, g, o = gates["i"], gates["f"], gates["g"], gates["o"]
    d = add(V(dy_t), dh)
    tc = vtanh(ct)
    zo = mul(mul(d, tc), mul(o, one_minus(o)))
    dc = add(mul(mul(d, o), one_minus(mul(tc, tc))), dc_in)
    zi = mul(mul(dc, g), mul(i, one_minus(i)))
    zf = mul(mul(dc, cprev), mul(f, one_minus(f)))
    zg = mul(mul(dc, i), one_minus(mul(g, g)))
    carry = mul(dc, f)
    v = np.concatenate([zi.v, zf.v, zg.v, zo.v], 1)
    e = np.concatenate([zi.e, zf.e, zg.e, zo.e], 1)
    return V(v, store_err(v, e, dtype)), carry


# ------------------------------------------------------------------------------------------------ whole passes
def _zeros(B, Hp):
    return V(np.zeros((B, Hp)))


def forward(W, b_hh, xproj, h0=None, c0=None, dtype=None, fed=None, mut=0, H=None):
    """xproj [T, B, 4 Hp] -> dict of lists over t of V: i f g o c h, plus h_init / c_init.  fed: the kernel's dict(y [T + 1, B, Hp], cells
    [T + 1, B, Hp]) for the STEP-FED mode; None for CHAINED (dtype None: plain fp64, no rounding anywhere)."""
    T, B = xproj.shape[:2]
    Hp = W.shape[1]
    h = V(h0, store_err(np.asarray(h0, np.float64), 0.0, dtype)) if h0 is not None else _zeros(B, Hp)
    c = V(c0) if c0 is not None else _zeros(B, Hp)
    out = dict(i=[], f=[], g=[], o=[], c=[], h=[], h_init=h, c_init=c)
    steps = T - 1 if mut == 6 else T
    for t in range(T):
        if fed is not None:
            h, c = V(fed["y"][t]), V(fed["cells"][t])
        if t < steps:
            s = fwd_step(W, b_hh, xproj[t], h, c, dtype, mut, H)
        h, c = s["h"], s["c"]
        for k in "ifgoch":
            out[k].append(s[k])
    return out


def backward(W, fwd, dy, dh_T=None, dc_T=None, dtype=None, fed=None, mut=0):
    """dy [T, B, Hp] -> dict(dz: list of V [B, 4 Hp], carry: list of V, dh0, dc0).  fed: the kernel's dict(gates [T, B, 4, Hp], cells, dz
    [T, B, 4 Hp], trace [T, B, Hp]) for the STEP-FED mode."""
    T, B = dy.shape[:2]
    Hp = W.shape[1]
    dzs, carries = [None] * T, [None] * T
    dh = V(dh_T) if dh_T is not None else _zeros(B, Hp)
    dc = V(dc_T) if dc_T is not None else _zeros(B, Hp)
    for t in range(T - 1, -1, -1):
        if fed is not None:
            gates = {k: V(fed["gates"][t][:, q]) for q, k in enumerate("ifgo")}
            ct, cp = V(fed["cells"][t + 1]), V(fed["cells"][t])
            if t < T - 1:
                dh = matvec(V(fed["dz"][t + 1]), W.T, 4 * Hp + 2)
                dc = V(fed["trace"][t + 1])
        else:
            gates = {k: fwd[k][t] for k in "ifgo"}
            ct, cp = fwd["c"][t], (fwd["c"][t - 1] if t else fwd["c_init"])
        dz, carry = bwd_step(W, gates, ct, cp, dy[T - 1 - t] if mut == 3 else dy[t], dh, dc, dtype)
        dzs[t], carries[t] = dz, carry
        if fed is None:
            dh, dc = matvec(dz, W.T, 4 * Hp + 2), carry
    last = V(fed["dz"][0]) if fed is not None else dzs[0]
    return dict(dz=dzs, carry=carries, dh0=matvec(last, W.T, 4 * Hp + 2), dc0=V(fed["trace"][0]) if fed is not None else carries[0])


def simulate(W, b_hh, xproj, h0, c0, dy, dh_T, dc_T, dtype):
    """What a correct kernel could leave: the chained fp64 values rounded where the kernel stores -> (fwd dict, bwd dict) of arrays shaped as
    the kernel's outputs (y, gates, cells; dz, trace, dh0, dc0).  The stand-in for the device in the host tests."""
    T, B = xproj.shape[:2]
    Hp = W.shape[1]
    h = rnd(h0, dtype) if h0 is not None else np.zeros((B, Hp))
    c = rnd(c0, "f32") if c0 is not None else np.zeros((B, Hp))
    y, cells, gates = [h], [c], []
    for t in range(T):
        s = fwd_step(W, b_hh, xproj[t], V(h), V(c), None)
        h, c = rnd(s["h"].v, dtype), rnd(s["c"].v, "f32")
        y.append(h)
        cells.append(c)
        gates.append(np.stack([rnd(s[k].v, "f32") for k in "ifgo"], 1))
    fk = dict(y=np.stack(y), cells=np.stack(cells), gates=np.stack(gates))
    dz, trace = [None] * T, [None] * T
    dh = np.asarray(dh_T, np.float64) if dh_T is not None else np.zeros((B, Hp))
    dc = np.asarray(dc_T, np.float64) if dc_T is not None else np.zeros((B, Hp))
    for t in range(T - 1, -1, -1):
        g = {k: V(fk["gates"][t][:, q]) for q, k in enumerate("ifgo")}
        z, carry = bwd_step(W, g, V(fk["cells"][t + 1]), V(fk["cells"][t]), dy[t], V(dh), V(dc), None)
        dz[t], trace[t] = rnd(z.v, dtype), rnd(carry.v, "f32")
        dh, dc = rnd(dz[t] @ W, "f32"), trace[t]
    bk = dict(dz=np.stack(dz), trace=np.stack(trace), dh0=dh, dc0=dc)
    return fk, bk


# ------------------------------------------------------------------------------------------------ comparing
def worst(got, want):
    """max |got - v| / e over the elements (0 / 0 = 0; anything / 0 = inf), for reporting and asserting in one figure."""
    err = np.abs(np.asarray(got, np.float64) - want.v)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / want.e)
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max()) if r.size else 0.0


def check_forward(fk, ref, H):
    """-> {name: worst ratio} of a kernel's forward outputs against forward()'s bounds, and whether the pads are exactly zero."""
    T = len(ref["h"])
    Hp = fk["y"].shape[-1]
    res = {"h": max(worst(fk["y"][t + 1], ref["h"][t]) for t in range(T)), "c": max(worst(fk["cells"][t + 1], ref["c"][t]) for t in range(T))}
    for q, k in enumerate("ifgo"):
        res[k] = max(worst(fk["gates"][t][:, q], ref[k][t]) for t in range(T))
    res["h_init"] = worst(fk["y"][0], ref["h_init"])
    res["c_init"] = worst(fk["cells"][0], ref["c_init"])
    res["pads_zero"] = bool((fk["y"][..., H:] == 0).all() and (fk["cells"][..., H:] == 0).all()) if H < Hp else True
    return res


def check_backward(bk, ref, H):
    T = len(ref["dz"])
    Hp = bk["trace"].shape[-1]
    res = {"dz": max(worst(bk["dz"][t], ref["dz"][t]) for t in range(T)), "trace": max(worst(bk["trace"][t], ref["carry"][t]) for t in range(T)),
           "dh0": worst(bk["dh0"], ref["dh0"]), "dc0": worst(bk["dc0"], ref["dc0"])}
    pads = bk["dz"].reshape(T, -1, 4, Hp)[..., H:]
    res["pads_zero"] = bool((pads == 0).all() and (bk["dh0"][..., H:] == 0).all() and (bk["dc0"][..., H:] == 0).all()) if H < Hp else True
    return res


def passed(res):
    return all((v is True) if isinstance(v, bool) else (v <= 1.0) for v in res.values())


# ------------------------------------------------------------------------------------------------ inputs
def inputs(H, T, B, dtype, seed, scale="torch", with_state=True):
    """Padded operands, rounded to their storage types: W [4 Hp, Hp], b_hh [4 Hp], xproj [T, B, 4 Hp], h0, c0, dy [T, B, Hp], dh_T, dc_T.
    scale "torch": U(-1/sqrt(H), 1/sqrt(H)), PyTorch's initial scale; "contract": W_hh from U(-1/H, 1/H) and the projection and the states
    at a fifth of their size, so that |h| stays below 1/4: the bf16 store of h alone is half an ulp, 2^-10 there and 2^-9 from 1/2 on, which
    is the whole of the chained cap (1e-3)."""
    rng = np.random.default_rng(seed)
    k = 1.0 / np.sqrt(H)
    kw = k if scale == "torch" else 1.0 / H
    amp = 1.0 if scale == "torch" else 0.2
    W = pad_cols(pad_gate_rows(rng.uniform(-kw, kw, (4 * H, H)), H), H)
    b = pad_gate_rows(rng.uniform(-k, k, (4 * H,)), H)
    xp = np.stack([np.stack([pad_gate_rows(rng.standard_normal(4 * H) * 0.6 * amp, H) for _ in range(B)]) for _ in range(T)])
    dy = pad_cols(rng.standard_normal((T, B, H)), H)
    st = [pad_cols(rng.standard_normal((B, H)) * s, H) for s in (0.5 * amp, 0.8 * amp, 1.0, 1.0)] if with_state else [None] * 4
    r32 = lambda a: None if a is None else rnd(a, "f32")      # noqa: E731
    return dict(W=rnd(W, dtype), b=r32(b), xp=rnd(xp, dtype), dy=rnd(dy, dtype), h0=r32(st[0]), c0=r32(st[1]), dh_T=r32(st[2]), dc_T=r32(st[3]), H=H)


def chained_last_h_bound(H, T, dtype, seed=0, B=2):
    x = inputs(H, T, B, dtype, seed, scale="contract")
    ref = forward(x["W"], x["b"], x["xp"], x["h0"], x["c0"], dtype)
    return float(ref["h"][-1].e.max())


# ------------------------------------------------------------------------------------------------ a whole layer in plain fp64 (against torch.nn.LSTM)
def layer_forward(x, W_ih, W_hh, b_ih, b_hh, h0=None, c0=None):
    """x [B, T, E]; PyTorch-shaped parameters ([4 H, E], [4 H, H], [4 H]) -> (out [B, T, H], h_T, c_T, saved)."""
    H = W_hh.shape[1]
    Wp = pad_cols(pad_gate_rows(W_hh, H), H)
    xproj = np.einsum("bte,ne->tbn", x, W_ih) + b_ih
    xp = np.stack([np.stack([pad_gate_rows(r, H) for r in xt]) for xt in xproj])
    f = forward(Wp, pad_gate_rows(b_hh, H), xp, None if h0 is None else pad_cols(h0, H), None if c0 is None else pad_cols(c0, H))
    out = np.stack([s.v[:, :H] for s in f["h"]], 1)
    return out, f["h"][-1].v[:, :H], f["c"][-1].v[:, :H], (f, Wp, x, W_ih, H)


def layer_backward(saved, dout, dh_T=None, dc_T=None):
    """-> dict of dx, dW_ih, dW_hh, db_ih, db_hh, dh0, dc0 (un-padded, PyTorch's shapes)."""
    f, Wp, x, W_ih, H = saved
    dy = pad_cols(np.transpose(dout, (1, 0, 2)), H)
    b = backward(Wp, f, dy, None if dh_T is None else pad_cols(dh_T, H), None if dc_T is None else pad_cols(dc_T, H))
    dz = np.stack([unpad_gate_rows(z.v.T, H).T for z in b["dz"]])                 # [T, B, 4 H]
    hprev = np.stack([f["h_init"].v[:, :H]] + [s.v[:, :H] for s in f["h"][:-1]])  # [T, B, H]
    return dict(dx=np.einsum("tbn,ne->bte", dz, W_ih), dW_ih=np.einsum("tbn,bte->ne", dz, x), dW_hh=np.einsum("tbn,tbh->nh", dz, hprev),
                db_ih=dz.sum((0, 1)), db_hh=dz.sum((0, 1)), dh0=b["dh0"].v[:, :H], dc0=b["dc0"].v[:, :H])


# ------------------------------------------------------------------------------------------------ log-sigmoid
def logsigmoid_bounds(x, dy=None):
    """y = min(x, 0) - log1p(exp(-|x|)) with its bound; with dy also dx = dy s(-x)."""
    x = np.asarray(x, np.float64)
    e = vexp(V(-np.abs(x)))
    l = np.log1p(e.v)
    le = e.e / (1.0 + np.maximum(e.v - e.e, 0.0)) + 6 * U * l + TINY          # log1pf: 3 ulp as logf
    y = add(V(np.minimum(x, 0.0)), V(-l, le))
    if dy is None:
        return y
    d = add(V(np.ones_like(x)), e)
    num = V(np.where(x >= 0, e.v, 1.0), np.where(x >= 0, e.e, 0.0))
    q = num.v / d.v
    qe = num.e / np.maximum(d.v - d.e, 1.0) + q * d.e / np.maximum(d.v - d.e, 1.0)
    return y, mul(V(dy), V(q, qe + U * (q + qe)))
