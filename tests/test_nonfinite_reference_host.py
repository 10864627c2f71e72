"""CPU test of the tester behind nonfinite_checks() (tests/nonfinite_ref.py): for the problems, sites and patterns of every family the GPU checks
run (the same generators of nonfinite_ref.py; options that do not move the sets -- the split count of a weight gradient, the hint's tile where two
hints share a site -- are taken once), built from the fp64 references alone, the set N of non-finite outputs is the structural set one expects (an A row gives an output row, a B row a column, one quantiser input
one byte, ...), N and U are both non-empty so no case is vacuous, and the verdict accepts the reference itself and REJECTS two wrong kernels:
one that launders (N replaced by clamped finite values, what v_med3 does) and one that spreads (one more row of U is NaN)."""
import numpy as np
import pytest

import gemm_ref as GR
import nonfinite_ref as NF


def _judge(name, ref_clean, ref_poisoned, bound, sets, want_n, want_c=False):
    """The three checks of one output tensor; prints |N|, |U|, |C| and the two rejections."""
    n, u, c = NF.counts(sets)
    assert np.array_equal(sets["N"], want_n), f"{name}: N is not the structural set ({n} vs {int(want_n.sum())} elements)"
    assert n > 0 and u > 0, f"{name}: vacuous (|N|={n}, |U|={u})"
    assert (c > 0) == want_c, f"{name}: |C|={c}"
    assert NF.accepted(NF.verdict(name, ref_clean, ref_poisoned, ref_poisoned, bound, sets)), f"{name}: the reference itself fails"
    laundered = NF.verdict(name, ref_clean, NF.launder(ref_poisoned, sets), ref_poisoned, bound, sets)
    spreading = NF.verdict(name, ref_clean, NF.spread(ref_poisoned, sets), ref_poisoned, bound, sets)
    assert not laundered[0][3] and laundered[1][3], f"{name}: the laundering mutant must fail on N alone"
    assert not spreading[1][3] and spreading[0][3], f"{name}: the spreading mutant must fail on U alone"
    print(f"{name}: |N|={n} |U|={u} |C|={c}; laundering mutant rejected ({laundered[0][1]:.0f} finite in N), "
          f"spreading mutant rejected ({spreading[1][1]:.0f} changed in U)")


def test_patterns_are_exact_and_of_the_right_class():
    for dt, width in (("f32", 32), ("bf16", 16)):
        vals = [NF.value(i, dt) for i in range(NF.NPAT)]
        assert all(np.isnan(v) for v in vals[:3]) and vals[3] == np.inf and vals[4] == -np.inf
        for i in range(NF.NPAT):
            assert NF.signed_bits(i, dt) % (1 << width) == NF.bits(i, dt)
            assert NF.bits(i + NF.NPAT, dt) == NF.bits(i, dt)
    assert NF.bits(1, "f32") == 0xFFFFFFFF and NF.bits(1, "bf16") == 0xFFFF          # the guard allocator's fill
    assert NF.bits(2, "f32") == 0x7F800001 and NF.bits(2, "bf16") == 0x7F81          # signalling
    a = np.arange(6.0).reshape(2, 3)
    b = NF.plant(a, (1, 2), 4)
    assert b[1, 2] == -np.inf and a[1, 2] == 5.0 and np.array_equal(a.ravel()[:5], b.ravel()[:5])


def test_classify_verdict_and_widen():
    clean = np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]])
    pois = np.array([[np.nan, np.inf, 3.0], [4.0, 5.5, 6.0]])
    s = NF.classify(clean, pois)
    assert NF.counts(s) == (2, 3, 1) and s["C"][1, 1]
    bound = np.full((2, 3), 0.25)
    assert NF.accepted(NF.verdict("t", clean, pois, pois, bound, s))
    assert NF.accepted(NF.verdict("t", clean, np.array([[np.inf, np.nan, 3.0], [4.0, 5.7, 6.0]]), pois, bound, s))       # the class, not the kind
    assert not NF.accepted(NF.verdict("t", clean, np.array([[np.nan, np.inf, 3.0], [4.0, 5.9, 6.0]]), pois, bound, s))   # C outside its bound
    assert not NF.accepted(NF.verdict("t", clean, np.array([[np.nan, np.inf, 3.0], [4.0, 5.5, 6.0 + 2 ** -40]]), pois, bound, s))
    assert not NF.accepted(NF.verdict("t", np.array([[1.0, 2.0, 0.0], [4.0, 5.0, 6.0]]), np.array([[np.nan, np.inf, -0.0], [4.0, 5.5, 6.0]]), pois, bound, s))
    w = NF.widen(s, np.array([[False, False, True], [False, False, False]]), "the element next to the poison, read by the same 8-byte load")
    assert NF.counts(w) == (3, 2, 1) and (w["N"] >= s["N"]).all()
    nb = NF.usable_bound(np.array([np.nan, 1.0, np.inf]), np.array([2.0, 2.0, 2.0]))
    assert np.array_equal(nb, [2.0, 1.0, 2.0])


def test_e4m3_model():
    b = np.arange(256, dtype=np.uint8)
    v = NF.e4m3_decode(b)
    assert np.isnan(v[0x7F]) and np.isnan(v[0xFF]) and int(np.isnan(v).sum()) == 2
    assert v[0x7E] == 448.0 and v[0xFE] == -448.0 and v[0x01] == 2.0 ** -9 and v[0x08] == 2.0 ** -6 and v[0x38] == 1.0
    fin = ~np.isnan(v)
    assert np.array_equal(GR.e4m3_rne(v[fin]), v[fin])                               # every finite byte is a fixed point of the rounding
    x = np.array([1e10, -1e10, 1e-32, 0.0, np.nan, np.inf, -np.inf, 1.0])
    big = float(np.float32(448.0) / np.float32(1e-30))
    with np.errstate(over="ignore"):
        assert np.isinf(np.float32(1e10) * np.float32(big))
    q = NF.e4m3_quantize(x, big)
    assert q[0] == 448.0 and q[1] == -448.0 and q[3] == 0.0 and np.isnan(q[4:7]).all() and q[7] == 448.0
    assert NF.finite_amax(x) == np.float32(1e10)
    assert np.array_equal(NF.amax_scales(np.array([1.0, np.nan, -7.0])), np.array([64.0, 2.0 ** -6, 7.0], dtype=np.float32))
    assert np.array_equal(NF.amax_scales(np.array([1.0, np.inf, -7.0])), np.array([1.0, 1.0, 0.0], dtype=np.float32))
    assert np.array_equal(NF.amax_scales(np.zeros(4)), np.array([1.0, 1.0, 0.0], dtype=np.float32))


@pytest.mark.parametrize("dn", ["f32", "bf16"])
def test_fp8_quantiser_cases(dn):
    launch = 0
    for rows, cols0 in NF.FP8_SHAPES:
        for cols in (cols0, cols0 - 4):
            x = NF.fp8_inputs(rows, cols, dn)
            scale = float(np.float32(448.0) / np.float32(float(NF.finite_amax(x)) * 0.5))
            for site in NF.fp8_sites(rows, cols):
                pat = launch % NF.NPAT
                launch += 1
                xp, rc, rp, sets, want = NF.fp8_quantize_case(rows, cols, dn, site, pat, scale)
                assert int((np.abs(rc) == 448.0).sum()) > 0                          # the scale saturates part of the range
                _judge(f"fp8.quantize[{dn},{rows}x{cols},{NF.NAMES[pat]}@{site}]", rc, rp, None, sets, want)
                amax = NF.finite_amax(xp)
                assert np.isfinite(amax) and amax == np.abs(np.where(np.isfinite(xp), xp, 0.0)).max()
    assert launch >= NF.NPAT


@pytest.mark.parametrize("shape", [(130, 132, 128, 4), (257, 260, 256, 16)])
def test_fp8_gemm_cases(shape):
    M, N, K, hint = shape
    x = GR.nt_inputs(M, N, K, "fp8", seed=9100 + M + N + K)
    rc = GR.nt_ref(x, bias=True, out_dtype="f32")
    for tensor, index, kind in NF.fp8_nt_sites(M, N, K, hint):
        rp, sets = NF.fp8_nt_case(x, rc, tensor, index)
        _judge(f"fp8.gemm_nt[M{M},N{N},K{K},{tensor}{index}]", rc["out"], rp["out"], rp["out_bound"], sets, NF.fp8_expect((M, N), tensor, index))


def test_fp8_wgrad_cases():
    T, N1, N2 = 333, 132, 256
    p = NF.fp8_wgrad_problem(T, N1, N2)
    assert p["at"].shape == (N1, 1024) and not p["at"][:, T:].any() and not p["bt"][:, T:].any()
    rc = NF.fp8_wgrad_ref(p)
    for tensor, index in NF.fp8_wgrad_sites(T, N1, N2):
        assert index[1] < T
        rp, sets = NF.fp8_wgrad_case(p, rc, tensor, index)
        _judge(f"fp8.wgrad[T{T},{tensor}{index}]", rc["out"], rp["out"], rp["out_bound"], sets, NF.fp8_expect((N1, N2), tensor, index))


@pytest.mark.parametrize("dn,hint", [("f32", 0), ("bf16", 0), ("bf16", 8), ("bf16", 16)])
def test_gemm_nt_cases(dn, hint):
    M, N, K = NF.NT_SHAPE
    x = GR.nt_inputs(M, N, K, dn, seed=7 * M + 3 * N + K)
    launch, used, tensors = 0, set(), set()
    for name in NF.nt_flavours(dn):
        rc = GR.nt_ref(x, **GR.FLAVOURS[name])
        for tensor, index, kind in NF.nt_sites(dn, hint, name):
            pat = launch % NF.NPAT
            launch += 1
            used.add(pat)
            tensors.add(tensor.split("_")[0])
            rp, sets, pre_sets = NF.nt_case(x, rc, name, tensor, index, pat)
            want = NF.nt_expect(tensor, index, kind)
            tag = f"gemm_nt[{dn},tm{hint},{name},{NF.NAMES[pat]}@{tensor}{index}]"
            _judge(tag, rc["out"], rp["out"], rp["out_bound"], sets, want)
            if pre_sets is not None:
                if kind == "elem":                                                   # the side tensors enter after C_pre is taken
                    assert NF.counts(pre_sets)[0] == 0 and NF.counts(pre_sets)[2] == 0
                else:
                    _judge(tag + ".pre", rc["pre"], rp["pre"], rp["pre_bound"], pre_sets, want)
    assert used == set(range(NF.NPAT)), "every pattern is used in the family"
    assert tensors == {"a", "b", "bias", "resid", "gin", "cprev"}


@pytest.mark.parametrize("dn", ["f32", "bf16"])
@pytest.mark.parametrize("T", [130, 747])
def test_gemm_tn_cases(dn, T):
    """tav_gemm_tn and the grouped forms (problem 1 of the grouped launch has the same widths)."""
    N1, N2 = NF.TN_WIDTHS
    x = GR.tn_inputs(T, N1, N2, dn, seed=T + 3 * N1 + 5 * N2)
    launch = 0
    for kw in (dict(), dict(scale=0.37), dict(perm=(88, 3))):
        rc = GR.tn_ref(x, nsplit=3, **kw)
        for tensor, index in NF.tn_sites(T, N1, N2):
            assert index[0] < T
            pat = launch % NF.NPAT
            launch += 1
            rp, sets, bsets = NF.tn_case(x, rc, tensor, index, pat, nsplit=3, **kw)
            want, want_b = NF.tn_expect(N1, N2, tensor, index, kw.get("perm", (0, 0)))
            tag = f"gemm_tn[{dn},T{T},{kw},{NF.NAMES[pat]}@{tensor}{index}]"
            _judge(tag, rc["out"], rp["out"], rp["out_bound"], sets, want)
            if tensor == "a":
                _judge(tag + ".dbias", rc["dbias"], rp["dbias"], rp["dbias_bound"], bsets, want_b)
            else:
                assert NF.counts(bsets) == (0, N1, 0), "a B element reaches nothing of dbias"


def test_sumsq_and_adamw_cases():
    import step_end_ref as SR
    sizes = SR.SIZE_LISTS[NF.STEP_SIZES]
    n = sum(sizes)
    p0, g0, m0, v0 = NF.adamw_state(SR)
    sites = NF.step_sites(sizes)
    assert sites[0] == 0 and sites[-1] == n - 1 and sizes[0] < sites[1] < n - 1
    for pat in range(NF.NPAT):
        s = NF.sumsq_ref(NF.plant(g0, sites[1], pat))
        assert np.isnan(s) if pat < 3 else s == np.inf
        for site in sites:
            rc, rp, sets = NF.adamw_case(p0, g0, m0, v0, 2, SR.f32(SR.LR), SR.WD, SR.CLIP_STEP2, site, pat, SR.ref_step)
            want = np.zeros(n, dtype=bool)
            want[site] = True
            for k in "pmv":
                _judge(f"adamw[{NF.NAMES[pat]}@{site}].{k}", rc[k], rp[k], rp[k + "_bound"], sets[k], want)
    rc, rp, sets = NF.adamw_case(p0, g0, m0, v0, 2, SR.f32(SR.LR), SR.WD, SR.CLIP_STEP2, None, 0, SR.ref_step)
    for k in "pmv":                                                   # a NaN clip coefficient: every element, the one case without a U
        assert NF.counts(sets[k]) == (n, 0, 0)
        assert not NF.accepted(NF.verdict(k, rc[k], NF.launder(rp[k], sets[k]), rp[k], rp[k + "_bound"], sets[k]))
    print(f"adamw[NaN clip coefficient]: |N|={n} |U|=0 |C|=0; laundering mutant rejected")


def test_cross_entropy_cases():
    import front_ref as FR
    for B, C, weighted, gs in ((3, 7, True, 1.0), (257, 7, False, 0.125)):
        p = FR.ce_inputs(B, C)
        rc = FR.ce_ref(p, weighted, gs)
        sites = NF.ce_sites(p)
        assert {w for _, _, w in sites} == {"target", "off"} and all(p["t"][r] != c for r, c, w in sites if w == "off")
        for row, col, where in sites:
            for pat in range(NF.NPAT):
                rp, lsets, dsets = NF.ce_case(p, rc, FR.ce_ref, weighted, gs, row, col, pat)
                tag = f"ce[B{B},C{C},{NF.NAMES[pat]}@({row},{col}) {where}]"
                rowmask = np.zeros((B, C), dtype=bool)
                rowmask[row] = True
                if pat < 4:                                           # NaN and +Inf: the row's dlogits and the shared loss
                    _judge(tag + ".dlogits", rc["dlogits"], rp["dlogits"], rp["dlogits_b"], dsets, rowmask)
                    assert NF.counts(lsets) == (1, 0, 0)
                else:                                                 # -Inf: softmax gives it probability 0, the row stays finite but changes
                    assert NF.counts(dsets)[0] == 0 and np.array_equal(dsets["C"].any(1), rowmask.any(1)) and np.isfinite(rp["dlogits_b"][dsets["C"]]).all()
                    assert NF.counts(lsets) == ((1, 0, 0) if where == "target" else (0, 0, 1))       # -log 0 at the target
                    print(f"{tag}: dlogits |N|=%d |U|=%d |C|=%d, loss |N|=%d |U|=%d |C|=%d" % (NF.counts(dsets) + NF.counts(lsets)))


@pytest.mark.parametrize("xdt", ["f32", "bf16"])
@pytest.mark.parametrize("act", [0, 1])
def test_layernorm_cases(xdt, act):
    import norm_ref as NR
    rows, W = NF.LN_SHAPE
    p = NR.ln_inputs(rows, W, xdt, xdt)
    for launch, (lp, (tensor, index)) in enumerate((lp_, s_) for lp_ in (False, True) for s_ in NF.ln_sites(rows, W)):
        pat = (launch + act) % NF.NPAT
        c = NF.ln_case(NR, p, tensor, index, pat, act, lp=lp)
        want = NF.ln_expect(rows, W, tensor, index, act)
        tag = f"ln[{xdt},act{act},lp{int(lp)},{NF.NAMES[pat]}@{tensor}{index}]"
        for side, names in (("fwd", NR.LN_FWD_OUT), ("bwd", NR.LN_BWD_OUT)):
            if side == "fwd" and tensor in ("dy", "add"):
                continue                                             # the forward reads neither
            for n in names:
                sets = c[side + "_sets"][n]
                assert np.array_equal(sets["N"], want[n]), f"{tag}.{n}: N is not the structural set {NF.counts(sets)} vs {int(want[n].sum())}"
                assert NF.counts(sets)[2] == 0
                if want[n].any() and not want[n].all():
                    _judge(f"{tag}.{n}", c[side + "_clean"][n], c[side][n], c[side][n + "_b"], sets, want[n])
                else:
                    print(f"{tag}.{n}: |N|=%d |U|=%d |C|=%d" % NF.counts(sets))


@pytest.mark.parametrize("dn", ["f32", "bf16"])
@pytest.mark.parametrize("S", NF.ATTN_S)
def test_attention_cases(dn, S):
    import attn_ref as AR
    cfg, used, with_c = 0, set(), 0
    for mode in (0, 1, 2):
        for pre in (False, True):
            x = AR.make_inputs(2, S, 3, dn, seed=11, **AR.bound_config(S, mode, pre, None))
            plain, full = NF.attn_plain(AR, x), AR.attn_ref(x)
            for n in AR.FWD_OUT + AR.BWD_OUT:                         # the plain model IS attn_ref's on clean operands
                assert np.allclose(plain[n], full[n], rtol=1e-9, atol=1e-12), n
            for i in range(len(NF.ATTN_SITES)):
                site = NF.attn_site(S, mode, cfg, i)
                if site is None:
                    continue
                tensor, index = site
                pat = NF.attn_pattern(tensor, cfg + i, mode, pre)
                used.add(pat)
                xp, rc, rp, sets = NF.attn_case(AR, x, tensor, index, pat)
                tag = f"attn[{dn},S{S},mode{mode},pre{int(pre)},{NF.NAMES[pat]}@{tensor}{index}]"
                if "o_bound" in rp:                                   # -Inf in the pre-softmax mask: probability 0 for that key, all of the entry changes
                    with_c += 1
                    for n in AR.FWD_OUT + AR.BWD_OUT:
                        if n != "corr":
                            assert NF.counts(sets[n])[0] == 0 and sets[n]["C"][index[0]].any() and not sets[n]["C"][1 - index[0]].any(), (tag, n)
                            assert np.isfinite(rp[n + "_bound"]).all()
                            bound = rp[n + "_bound"]
                            assert NF.accepted(NF.verdict(n, rc[n], rp[n], rp[n], bound, sets[n])), (tag, n)
                            stale = np.where(sets[n]["C"], rc[n], rp[n])          # a kernel that ignores the -Inf: the clean values on C
                            off = NF.verdict(n, rc[n], stale, rp[n], bound, sets[n])
                            assert not off[2][3] and off[0][3] and off[1][3], f"{tag}.{n}: the clean values must leave the bound on C"
                            assert not NF.verdict(n, rc[n], NF.spread(rp[n], sets[n]), rp[n], bound, sets[n])[1][3], (tag, n)
                    print(f"{tag}: " + ", ".join(f"{n} |N|=%d |U|=%d |C|=%d" % NF.counts(sets[n]) for n in ("o", "lse", "dq", "dk", "dv")) +
                          "; the clean values and a spread row rejected on every output")
                    continue
                want = NF.attn_expect(x, tensor, index)
                for n in AR.FWD_OUT + AR.BWD_OUT:
                    assert np.array_equal(sets[n]["N"], want[n]), f"{tag}.{n}: N {NF.counts(sets[n])} is not the structural set ({int(want[n].sum())})"
                    assert NF.counts(sets[n])[2] == 0, f"{tag}.{n}: C"
                for n in AR.FWD_OUT + AR.BWD_OUT:
                    if want[n].any() and not want[n].all():
                        _judge(f"{tag}.{n}", rc[n], rp[n], None, sets[n], want[n])
            cfg += 1
    assert used == set(range(NF.NPAT))
    assert with_c == 1, "one configuration per (dtype, S) takes the -Inf pre-softmax mask element"
    print(f"cases with a C set (a -Inf pre-softmax mask element): {with_c}")


def test_cast_and_dropout_cases():
    rng = np.random.default_rng(5)
    w = rng.standard_normal((65, 127)).astype(np.float32).astype(np.float64)
    keep = rng.random((65, 127)) >= 0.3
    keep[0, 0], keep[64, 126] = False, True
    for k, site in enumerate(((0, 0), (64, 126), (32, 64))):
        for pat in (k, k + 3):
            want = np.zeros(w.shape, dtype=bool)
            want[site] = True
            for dn, scale in (("bf16", None), ("f32", None), ("bf16", 0.18033688)):
                rc, rp = NF.cast_ref(w, dn, scale), NF.cast_ref(NF.plant(w, site, pat), dn, scale)
                assert np.array_equal(rc, GR.round_to(w if scale is None else (w.astype(np.float32) * np.float32(scale)).astype(np.float64), dn)[0])
                _judge(f"cast[{dn},scale {scale},{NF.NAMES[pat % NF.NPAT]}@{site}]", rc, rp, None, NF.classify(rc, rp), want)
            rc, rp = NF.dropout_ref(w, keep, 0.3), NF.dropout_ref(NF.plant(w, site, pat), keep, 0.3)
            sets = NF.classify(rc, rp)
            if keep[site]:
                _judge(f"dropout[kept,{NF.NAMES[pat % NF.NPAT]}@{site}]", rc, rp, None, sets, want)
            else:                                                     # a dropped poison is exactly 0: nothing at all changes
                assert NF.counts(sets) == (0, w.size, 0) and rp[site] == 0.0
                print(f"dropout[dropped,{NF.NAMES[pat % NF.NPAT]}@{site}]: |N|=0 |U|={w.size} |C|=0")
    assert keep[0, 0] != keep[64, 126] or keep[0, 0] != keep[32, 64], "kept and dropped sites both occur"
