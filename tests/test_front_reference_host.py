"""CPU test of the tester behind the front-end, pooling, head, loss and index checks (tests/front_ref.py): an f32 emulation of the kernels'
arithmetic with their real summation structure -- chunks, time groups and the partial-block reduce of the conv0 weight gradient, the four-chain
column sums, row groups of the pools, lanes and wave_sum of the head, the 256-thread tree of the cross entropy, the scan of the position ids --
stays inside every per-element bound of the fp64 reference in both dtypes and in forward and reversed order; it equals every exact case bit
for bit; forty-one wrong kernels, each a one-line mutation of it, are rejected in every dtype they apply to.  Run with -s to see every ratio."""
import numpy as np
import pytest

import front_ref as R

DTYPES = ("bf16", "f32")
INF = float("inf")


def _judge(e, ref, names, exact=False, dtof=None):
    """name -> err / bound, or for an exact case 0 | inf: the emulation's output equals the one right answer as its dtype holds it."""
    dtof = dtof or {}
    if exact:
        return {n: 0.0 if R.equal(e[n], R.held(ref[n], dtof.get(n, "f32"))) else INF for n in names}
    return R.ratios(e, ref, names)


# ------------------------------------------------------------------------------------------------ one runner per family
def conv0_fwd(dt, mut=None, rev=False, exact=False, shape=(2, 129, 12, 10, 5), extra=7, bias=True):
    p = R.conv0_inputs(*shape, extra=extra, exact=exact)
    return _judge(R.emu_conv0_fwd(p, bias, dt, rev, mut), R.conv0_ref_fwd(p, bias, dt), ("y",), exact, {"y": dt})


def conv0_bwd(dt, mut=None, rev=False, exact=False, shape=(3, 513, 8, 3, 2), accumulate=True):
    p = R.conv0_inputs(*shape, dydt=dt, exact=exact)
    return _judge(R.emu_conv0_bwd_w(p, accumulate, rev, mut), R.conv0_ref_bwd_w(p, accumulate), ("dw", "dbias"), exact)


def wn_fwd(dt, mut=None, rev=False, exact=False, shape=(64, 8, 5)):
    p = R.wn_inputs(*shape, exact=exact)
    return _judge(R.emu_wn_fwd(p, dt, rev, mut), R.wn_ref_fwd(p, dt), ("norms", "w", "w_flip"), exact, {"w": dt, "w_flip": dt})


def wn_bwd(dt, mut=None, rev=False, exact=False, shape=(64, 8, 5), accumulate=True, chained=False):
    p = R.wn_inputs(*shape, exact=exact)
    ref = R.wn_ref_fwd(p, "f32")
    if chained:
        nv, n32 = ref["_norms"], R.emu_wn_fwd(p, "f32", rev)["norms"]
    else:
        nv, n32 = R.fed(ref["norms"])
    return _judge(R.emu_wn_bwd(p, n32, accumulate, rev, mut), R.wn_ref_bwd(p, nv, accumulate), ("dv", "dg"), exact)


def group_pad(dt, mut=None, rev=False, exact=True, shape=(2, 5, 16, 2, 3, 2)):
    B, T, H, G, pl, pr = shape
    x = R.gp_inputs(B, T, H, "f32")
    return {"xg": 0.0 if R.equal(R.emu_group_pad(x, G, pl, pr, dt, mut), R.gp_ref(x, G, pl, pr, dt)) else INF}


def col2im(dt, mut=None, rev=False, exact=False, shape=(2, 7, 8, 3, 2), extra=3, pre=True):
    p = R.c2i_inputs(*shape, extra, dt, exact=exact)
    return _judge(R.emu_col2im(p, pre, rev, mut), R.c2i_ref(p, pre), ("dx",), exact, {"dx": dt})


def gelu(dt, mut=None, rev=False, exact=False, n=1028):
    p = R.gelu_inputs(n, dt)
    return _judge(R.emu_gelu(p, mut), R.gelu_ref(p), ("y", "dx"))


def tanh(dt, mut=None, rev=False, exact=False, n=1028):
    p = R.tanh_inputs(n)
    return _judge(R.emu_tanh(p, mut), R.tanh_ref(p), ("y", "dx"))


def colsum(dt, mut=None, rev=False, exact=False, shape=(1000, 257), nparts=None, accumulate=True, ld=None):
    p = R.colsum_inputs(*shape, dt, exact=exact)
    nparts = nparts or R.colsum_nparts(shape[0])
    return _judge(R.emu_colsum(p, nparts, accumulate, rev, mut, ld), R.colsum_ref(p, nparts, accumulate), ("out",), exact)


def pool(dt, mut=None, rev=False, exact=False, shape=(3, 77, 68), lens=None):
    p = R.pool_inputs(*shape, exact=exact)
    e, ref = R.emu_pool(p, lens, rev, mut), R.pool_ref(p, lens)
    return _judge(e, ref, ("y", "dx_f32") + (("dx_lp",) if dt == "bf16" else ()), exact, {"dx_lp": "bf16"})


def head(dt, mut=None, rev=False, exact=False, shape=(5, 65, 7), bias=True, accumulate=True):
    p = R.head_inputs(*shape, exact=exact)
    return _judge(R.emu_head(p, bias, accumulate, rev, mut), R.head_ref(p, bias, accumulate), ("y", "dx", "dW", "db"), exact)


def ce(dt, mut=None, rev=False, exact=False, shape=(257, 7), weighted=True, grad_scale=3.0):
    p = R.ce_inputs(*shape)
    return _judge(R.emu_ce(p, weighted, grad_scale, rev, mut), R.ce_ref(p, weighted, grad_scale), ("loss", "dlogits"))


def _eq(e, ref, names):
    return {n: 0.0 if R.equal(e[n], ref[n]) else INF for n in names}


def text(dt, mut=None, rev=False, exact=True, shape=(5, 65, 1)):
    p = R.text_inputs(*shape)
    return _eq(R.emu_text(p, mut), R.text_ref(p), ("pos_ids", "pre"))


def embed(dt, mut=None, rev=False, exact=True, shape=(257, 4, 8), accumulate=True):
    p = R.embed_inputs(*shape)
    return _eq(R.emu_embed(p, accumulate, rev, mut), R.embed_ref(p, accumulate), ("out", "dtable"))


def scatter(dt, mut=None, rev=False, exact=True, shape=(1025, 4)):
    p = R.scatter_inputs(*shape)
    return _eq(R.emu_scatter(p, rev, mut), R.scatter_ref(p), ("dtable",))


# ------------------------------------------------------------------------------------------------ the inputs
def test_inputs_and_constructions_are_what_the_checks_promise():
    assert R.exact_ok()
    p = R.conv0_inputs(3, 129, 12, 10, 5, dydt="bf16")
    assert np.array_equal(p["dy"], R.bf16_rne(p["dy"])) and np.array_equal(p["wave"], R.f32(p["wave"])) and p["T_in"] == 128 * 5 + 10
    rms = np.sqrt((p["w"] ** 2).mean(1))
    assert rms.max() / rms.min() > 16                                              # channels spread over 2^-3 .. 2^3
    tap = np.sqrt((R.conv0_inputs(1, 1, 512, 10, 5)["w"] ** 2 / R.ch_scale(512)[:, None] ** 2).mean(0))
    assert tap.max() / tap.min() > 8                                               # taps over 2^-2 .. 2^2
    assert np.abs(p["wave"][2]).mean() / np.abs(p["wave"][0]).mean() > 100          # rows cycle through scales and offsets
    q = R.conv0_inputs(3, 513, 8, 3, 2, exact=True)
    assert all(np.array_equal(q[k], np.rint(q[k])) and np.abs(q[k]).max() <= 7 for k in ("wave", "dy", "bias"))
    assert set(np.abs(q["w"]).ravel()) <= {1.0, 2.0, 4.0}
    w = R.wn_inputs(64, 8, 5, exact=True)
    assert ((w["v"] != 0).sum((0, 1)) == 1).all() and np.array_equal(np.log2(R.wn_ref_fwd(w, "f32")["norms"]) % 1, np.zeros(5))
    assert R.wn_blocks(8, 4) == (1, 32) and R.wn_blocks(260, 4) == (5, 208) and R.wn_blocks(1024, 256) == (512, 512)
    g = R.gelu_inputs(1028, "bf16")
    assert g["x"].min() == -40 and g["x"].max() == 40 and np.signbit(g["x"][-3]) and g["x"][-3] == 0 and (np.diff(g["x"][:1024]) >= 0).all()
    c = R.ce_inputs(600, 7)
    assert c["z"].max() > 2.9e4 and c["z"].min() < -2.9e4 and c["peak"].sum() > 40 and (c["t"] >= 0).all() and (c["t"] < 7).all()
    ref = R.ce_ref(c, False, 1.0)
    lo = R.ce_ref(dict(c, z=c["z"][c["peak"]], t=c["t"][c["peak"]], B=int(c["peak"].sum())), False, 1.0)["loss"][0]
    assert 0 < lo < 1e-24 and np.isfinite(ref["loss"]).all()                       # the rows whose loss is ~ e^-60
    assert c["cw"].max() / c["cw"].min() == 64
    t = R.text_inputs(5, 65, 1)
    assert (t["ids"][3] == 1).all() and t["ids"][0, 0] == 1 and t["ids"][2, -1] == 1 and t["ids"][1, 0] == 1 and (t["ids"][4] != 1).all()
    s = R.scatter_inputs(4096, 4)
    assert sorted(np.bincount(s["idx"])[:4]) == [1, 16, 17, 1024]
    assert R.d4(8) == 4 and R.d4(7) == 6 and R.d4(1) == 3


# ------------------------------------------------------------------------------------------------ emulation inside the bounds
BOUNDED = [
    ("conv0_fwd", conv0_fwd, [dict(), dict(shape=(1, 1, 4, 1, 1), extra=0, bias=False), dict(shape=(3, 257, 1028, 16, 8), extra=0), dict(shape=(1, 127, 512, 3, 2))]),
    ("conv0_bwd", conv0_bwd, [dict(), dict(shape=(1, 1, 8, 1, 1), accumulate=False), dict(shape=(5, 1025, 64, 10, 5)), dict(shape=(1, 3, 520, 3, 2))]),
    ("wn_fwd", wn_fwd, [dict(), dict(shape=(8, 4, 3)), dict(shape=(260, 4, 1)), dict(shape=(256, 64, 128))]),
    ("wn_bwd", wn_bwd, [dict(), dict(chained=True), dict(shape=(260, 4, 1), accumulate=False), dict(shape=(256, 64, 128), chained=True)]),
    ("col2im", col2im, [dict(), dict(pre=False), dict(shape=(1, 5, 4, 10, 5), extra=0), dict(shape=(2, 6, 4, 3, 1)), dict(shape=(2, 6, 4, 2, 2))]),
    ("gelu", gelu, [dict(), dict(n=4), dict(n=1020)]),
    ("tanh", tanh, [dict()]),
    ("colsum", colsum, [dict(), dict(shape=(1, 1), accumulate=False), dict(shape=(4097, 255), nparts=256), dict(shape=(17, 768), nparts=1), dict(shape=(15, 4), nparts=256)]),
    ("pool", pool, [dict(), dict(shape=(1, 1, 4)), dict(shape=(3, 17, 768), lens=(0, 1, 22)), dict(shape=(3, 16, 68), lens=(16, 15, 0))]),
    ("head", head, [dict(), dict(shape=(1, 1, 1), bias=False, accumulate=False), dict(shape=(5, 3072, 7)), dict(shape=(1, 63, 256))]),
    ("ce", ce, [dict(), dict(shape=(1, 1), weighted=False, grad_scale=1.0), dict(shape=(600, 64), grad_scale=0.125), dict(shape=(255, 2), weighted=False)]),
]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("fam", BOUNDED, ids=[b[0] for b in BOUNDED])
def test_emulation_is_inside_every_bound(fam, dt):
    name, run, cases = fam
    worst = {}
    for kw in cases:
        for rev in (False, True):
            for k, v in run(dt, rev=rev, **kw).items():
                worst[k] = max(worst.get(k, 0.0), v)
    print(f"{name} emulation[{dt}] worst err / bound:", {k: round(v, 3) for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, worst


EXACT = [
    ("conv0_fwd", conv0_fwd, [dict(), dict(shape=(3, 257, 1028, 16, 8), extra=0), dict(bias=False)]),
    ("conv0_bwd", conv0_bwd, [dict(), dict(shape=(5, 2050, 8, 10, 5)), dict(shape=(1, 3, 520, 3, 2), accumulate=False)]),
    ("wn_fwd", wn_fwd, [dict(), dict(shape=(260, 4, 1)), dict(shape=(256, 64, 128))]),
    ("wn_bwd", wn_bwd, [dict(), dict(shape=(260, 4, 1), accumulate=False)]),
    ("col2im", col2im, [dict(), dict(pre=False), dict(shape=(1, 5, 4, 10, 5), extra=0)]),
    ("colsum", colsum, [dict(), dict(shape=(4097, 255), nparts=256), dict(shape=(17, 768), nparts=1, accumulate=False)]),
    ("pool", pool, [dict(shape=(3, 64, 68)), dict(shape=(3, 77, 68), lens=(64, 0, 1)), dict(shape=(1, 16, 4), lens=(21,))]),
    ("head", head, [dict(), dict(shape=(5, 3072, 7)), dict(shape=(1, 63, 256), bias=False, accumulate=False)]),
    ("group_pad", group_pad, [dict(), dict(shape=(1, 1, 8, 2, 0, 0)), dict(shape=(2, 49, 256, 4, 63, 64))]),
    ("text", text, [dict(), dict(shape=(5, 64, 0)), dict(shape=(5, 513, 1)), dict(shape=(4, 1024, -1)), dict(shape=(5, 63, 1))]),
    ("embed", embed, [dict(), dict(shape=(1, 4, 1), accumulate=False), dict(shape=(65536 + 300, 4, 3))]),
    ("scatter", scatter, [dict(), dict(shape=(1, 4)), dict(shape=(17, 132)), dict(shape=(4096, 4))]),
]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("fam", EXACT, ids=[b[0] for b in EXACT])
def test_emulation_equals_every_exact_case(fam, dt):
    name, run, cases = fam
    for kw in cases:
        for rev in (False, True):
            r = run(dt, rev=rev, exact=True, **kw)
            assert max(r.values()) == 0.0, (name, kw, rev, r)


def test_copies_have_one_right_answer():
    rng = np.random.default_rng(0)
    table = R.ints(rng, (9, 8))
    idx = np.array([0, 8, 3, -2, 11, 3], dtype=np.int32)
    assert np.array_equal(R.gather_ref(table, idx), table[[0, 8, 3, 0, 8, 3]])
    video = rng.standard_normal((2, 4, 3, 32, 48))
    keep = np.array([[0, 5, 11], [7, 100, -1]], dtype=np.int32)
    out = R.patchify_ref(video, keep)
    tok = 7                                                                        # (tt, hh, ww) = (1, 0, 1) of a 2 x 2 x 3 grid
    assert out.shape == (6, 1536) and out[3, (1 * 2 + 1) * 256 + 5 * 16 + 2] == video[1, 2 * (tok // 6) + 1, 1, 5, 16 * 1 + 2]
    assert np.array_equal(out[4], R.patchify_ref(video, np.array([[0], [11]], dtype=np.int32))[1])                              # clamped high
    m = np.array([[1, 0, 1, 1, 0], [0, 0, 0, 0, 0]], dtype=np.uint8)
    ki, cnt = R.mask_to_index_ref(m, 1, 4)
    assert ki.tolist() == [[0, 2, 3, 3], [0, 0, 0, 0]] and cnt.tolist() == [3, 0]
    ki, cnt = R.mask_to_index_ref(m, 0, 1)
    assert ki.tolist() == [[1], [0]] and cnt.tolist() == [2, 5]


# ------------------------------------------------------------------------------------------------ wrong kernels
# number -> (runner, the arguments of the bounded problem that must reject it | None, those of the exact case | None, dtypes it applies to)
BOTH = DTYPES
AT = {
    1: (conv0_fwd, dict(), dict(), BOTH), 2: (conv0_fwd, dict(), dict(), BOTH), 3: (conv0_fwd, dict(), dict(), BOTH),
    4: (conv0_fwd, dict(), None, ("bf16",)),
    5: (conv0_bwd, dict(), dict(), BOTH), 6: (conv0_bwd, dict(), dict(), BOTH), 7: (conv0_bwd, dict(), dict(), BOTH), 8: (conv0_bwd, dict(), dict(), BOTH),
    9: (conv0_bwd, dict(), dict(), BOTH), 10: (conv0_bwd, dict(), dict(), BOTH),
    11: (conv0_bwd, dict(shape=(1, 3, 520, 3, 2)), dict(shape=(1, 3, 520, 3, 2)), BOTH),
    12: (wn_fwd, dict(), dict(), BOTH), 13: (wn_fwd, dict(), dict(), BOTH), 14: (wn_fwd, dict(), dict(), BOTH), 15: (wn_fwd, dict(), dict(), BOTH),
    16: (wn_bwd, dict(), dict(), BOTH), 17: (wn_bwd, dict(), dict(), BOTH), 18: (wn_fwd, dict(), dict(), BOTH),
    19: (group_pad, None, dict(), BOTH), 20: (group_pad, None, dict(), BOTH),
    21: (col2im, dict(), dict(), BOTH), 22: (col2im, dict(), None, BOTH),
    23: (colsum, dict(nparts=7), dict(nparts=7), BOTH), 24: (colsum, dict(ld=265), dict(ld=265), BOTH),
    25: (pool, dict(), dict(shape=(3, 77, 68), lens=(64, 8, 1)), BOTH), 26: (pool, dict(lens=(5, 77, 30)), dict(shape=(3, 64, 68), lens=(16, 64, 1)), BOTH),
    27: (pool, dict(lens=(5, 77, 30)), dict(shape=(3, 64, 68), lens=(16, 64, 1)), BOTH),
    28: (head, dict(), dict(), BOTH), 29: (head, dict(), dict(), BOTH), 30: (head, dict(), dict(), BOTH),
    31: (ce, dict(), None, BOTH), 32: (ce, dict(), None, BOTH), 33: (ce, dict(), None, BOTH), 34: (ce, dict(), None, BOTH), 35: (ce, dict(), None, BOTH),
    36: (tanh, dict(), None, BOTH),
    37: (text, None, dict(), BOTH), 38: (text, None, dict(), BOTH), 39: (embed, None, dict(), BOTH), 40: (scatter, None, dict(), BOTH),
    41: (gelu, dict(), None, BOTH),
}


def test_the_mutant_table_is_complete():
    assert sorted(AT) == sorted(R.MUTANTS) == list(range(1, 42))


@pytest.mark.parametrize("num,dt", [(n, d) for n in sorted(AT) for d in AT[n][3]])
def test_wrong_kernels_are_rejected(num, dt):
    run, bounded, exact, _ = AT[num]
    mut = R.MUTANTS[num]
    msg, hit = f"mutant {num:2d} {mut:34s} [{dt}]", False
    if bounded is not None:
        assert max(run(dt, **bounded).values()) <= 1.0                           # (the unmutated emulation passes the same problem)
        name, r = max(run(dt, mut=mut, **bounded).items(), key=lambda kv: kv[1])
        msg += f" bound: {name} {r:.3g}"
        hit |= r > 1.0
    if exact is not None:
        assert max(run(dt, exact=True, **exact).values()) == 0.0
        bad = [n for n, v in run(dt, mut=mut, exact=True, **exact).items() if v]
        msg += f"  exact: {'rejected by ' + ', '.join(bad) if bad else 'equal'}"
        hit |= bool(bad)
    print(msg)
    assert hit, msg
