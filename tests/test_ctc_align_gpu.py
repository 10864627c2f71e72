"""GPU: tav_ctc_align and tav_ctc_log_softmax (csrc/ctc_align.hip) against their host model (tests/ctc_align_ref.py), CTCAligner against
the oracle's wav2vec2 plus the head in torch, and get_times / align_batch end to end.

The kernel tests run inside the guard-band allocator (tests/guarded.py): emissions sit in a watched buffer with a padded row pitch (0xFF =
NaN between the rows and in the frames past a row's own length), every output is the middle row of a three-row 0xFF tensor whose
neighbours must stay 0xFF, and verify() reports any store outside a tensor or into an operand.

Trellis: bit for bit (f32 add and max are correctly rounded on both sides, the recurrence has one order).  path_token, seg, span: element
for element.  path_prob: within the documented expf error plus one rounding of the fp64 exp (ctc_align_ref.prob_bounds).  seg_score: the
f64 mean of the kernel's own path_prob, rounded once, bit for bit."""
import functools

import numpy as np
import pytest
import torch

import ctc_align_ref as R
import guarded
import tav_amd  # noqa: F401
from oracle import tav_oracle as O
from tav_amd import config as cfgmod
from tav_amd import ops, runtime, synthetic
from tav_amd.models.aligner import CTCAligner
from tav_amd.run_scripts import get_times as GT

pytestmark = pytest.mark.gpu


def _emission(rng, T, V, kind):
    if kind == "int":
        return -rng.integers(0, 4, size=(T, V)).astype(np.float32)
    x = rng.standard_normal((T, V)) * 2.0
    em = (x - np.log(np.exp(x).sum(1, keepdims=True))).astype(np.float32)
    if kind == "inf":                                          # impossible labels: -inf log-probabilities
        em[rng.random((T, V)) < 0.15] = -np.inf
    return em


@functools.lru_cache(maxsize=None)
def _thresholds():
    """From tav_ctc_align_plan: the largest N one thread per column covers at the smallest block build, the largest N with one column per
    thread, and the stage length at 32 labels."""
    small = max(n for n in range(1, 600) if ops.ctc_align_plan(8, n, 32)["block"] <= 256)
    one = max(n for n in range(1, 2049) if ops.ctc_align_plan(8, n, 32)["tokens_per_thread"] == 1)
    assert ops.ctc_align_plan(8, small + 1, 32)["block"] == 320 and ops.ctc_align_plan(8, one + 1, 32)["tokens_per_thread"] == 2
    return small, one, ops.ctc_align_plan(8, 8, 32)["frames_per_stage"]


def _edge(name):
    """(T, N, V, blank, kind of emission) of an edge case."""
    small, one, stage = _thresholds()
    table = {
        "t1n1": (1, 1, 4, 0, "ls"), "n_eq_t": (20, 20, 8, 0, "ls"), "t_eq_n_minus_1": (19, 20, 8, 0, "ls"),
        "n63": (90, 63, 32, 0, "ls"), "n64": (90, 64, 32, 0, "int"), "n65": (90, 65, 32, 0, "ls"), "n128": (150, 128, 29, 0, "ls"), "n129": (150, 129, 29, 0, "int"),
        "n_small_block": (small + 40, small, 32, 0, "ls"), "n_small_block_plus_1": (small + 40, small + 1, 32, 0, "int"),
        "n_one_per_thread": (one + 60, one, 32, 0, "ls"), "n_two_per_thread": (one + 60, one + 1, 32, 0, "int"),
        "t_stage": (stage, 10, 32, 0, "ls"), "t_stage_plus_1": (stage + 1, 10, 32, 0, "int"), "t_two_stages_plus_3": (2 * stage + 3, 70, 32, 0, "ls"),
        "words_in_workspace": (1200, 1100, 32, 0, "ls"), "three_per_thread": (2100, 2048, 29, 0, "int"),
        "blank_3": (50, 7, 29, 3, "ls"), "blank_3_int": (60, 9, 8, 3, "int"), "minus_inf": (80, 12, 8, 0, "inf"), "wide_v": (40, 9, 128, 0, "ls"),
    }
    return table[name]


EDGES = ["t1n1", "n_eq_t", "t_eq_n_minus_1", "n63", "n64", "n65", "n128", "n129", "n_small_block", "n_small_block_plus_1", "n_one_per_thread",
         "n_two_per_thread", "t_stage", "t_stage_plus_1", "t_two_stages_plus_3", "words_in_workspace", "three_per_thread", "blank_3", "blank_3_int",
         "minus_inf", "wide_v"]


def _edge_inputs(name):
    T, N, V, blank, kind = _edge(name)
    rng = np.random.default_rng(sum(map(ord, name)))
    return _emission(rng, T, V, kind), rng.integers(0, V, size=N).astype(np.int32), V, blank


def _launch(g, ems, toks, V, blank=0, Tmax=None, Nmax=None, want_trellis=True):
    """One launch over the rows `ems` / `toks` under guard -> (CtcAlignment of host arrays, the three-row device tensors)."""
    B = len(ems)
    Tmax = max([len(e) for e in ems] + [1]) if Tmax is None else Tmax
    Nmax = max([len(t) for t in toks] + [1]) if Nmax is None else Nmax
    host = np.full((B, Tmax, V), np.nan, np.float32)
    tok = np.full((B, Nmax), 7777, np.int32)                   # past a row's own tokens: an id no row may use
    for b, (e, t) in enumerate(zip(ems, toks)):
        host[b, :len(e)] = e
        tok[b, :len(t)] = t
    emission = guarded.guarded_input(torch.from_numpy(host).cuda(), pitch_extra=(-V) % 4 + 4)
    assert emission.stride(1) % 4 == 0 and emission.stride(1) > V
    tokens = guarded.guarded_input(torch.from_numpy(tok).cuda())
    n_frames = guarded.guarded_input(torch.tensor([len(e) for e in ems], dtype=torch.int32).cuda())
    n_tokens = guarded.guarded_input(torch.tensor([len(t) for t in toks], dtype=torch.int32).cuda())
    i32, f32 = torch.int32, torch.float32
    three = [g.empty((3, B, Tmax), dtype=i32, device="cuda"), g.empty((3, B, Tmax), dtype=f32, device="cuda"), g.empty((3, B, Nmax, 2), dtype=i32, device="cuda"),
             g.empty((3, B, Nmax), dtype=f32, device="cuda"), g.empty((3, B, 4), dtype=i32, device="cuda"),
             g.empty((3, B, Tmax + 1, Nmax + 1), dtype=f32, device="cuda") if want_trellis else None]
    out = ops.CtcAlignment(*[None if t is None else t[1] for t in three])
    got = ops.ctc_align(emission, tokens, n_frames, n_tokens, V=V, blank_id=blank, out=out)
    assert got is out
    return ops.CtcAlignment(*[None if t is None else t.cpu().numpy() for t in out]), three


def _untouched(three):
    for t in three:
        if t is not None:
            raw = t.view(torch.int32) if t.dtype != torch.int32 else t
            assert bool((raw[0] == -1).all()) and bool((raw[2] == -1).all())


def _check_row(got, b, em, tok, V, blank, name):
    """Row b of a launch against the host model of that utterance alone."""
    Tmax, Nmax = got.path_token.shape[1], got.seg.shape[1]
    T, N = len(em), len(tok)
    want = R.align(em, tok, V=V, blank=blank, Tmax=Tmax, Nmax=Nmax)
    if got.trellis is not None:
        tr = got.trellis[b].view(np.int32)
        assert np.array_equal(tr[:T + 1, :N + 1], want["trellis"].view(np.int32)), name
        rest = np.ones(tr.shape, bool)
        rest[:T + 1, :N + 1] = False
        assert (tr[rest] == -1).all(), f"{name}: the trellis outside t <= T_b, j <= N_b was written"
    assert np.array_equal(got.path_token[b], want["path_token"]), name
    assert np.array_equal(got.seg[b], want["seg"]), name
    assert got.span[b].tolist() == want["span"].tolist(), name
    p64, margin = R.prob_bounds(em, want["column"])
    err = np.abs(got.path_prob[b].astype(np.float64) - p64)
    on = want["column"] >= 0
    worst = float((err[on] / margin[on]).max()) if on.any() else 0.0
    print(f"{name} row {b}: T {T} N {N} points {int(want['span'][2])} status {int(want['span'][3])} worst |path_prob - exp64| / margin = {worst:.3f}")
    assert (err <= margin).all(), name
    assert np.array_equal(got.path_prob[b][~on].view(np.int32), np.zeros(int((~on).sum()), np.int32))          # +0.0 off the path
    assert np.array_equal(got.seg_score[b].view(np.int32), R.seg_scores(got.path_prob[b], got.seg[b]).view(np.int32)), name
    return want


@pytest.mark.parametrize("name", [c[0] for c in R.CASES])
def test_recorded_cases(gpu, name):
    em, tok = R.case_inputs(name)
    with guarded.active() as g:
        got, three = _launch(g, [em], [tok], em.shape[1])
        want = _check_row(got, 0, em, tok, em.shape[1], 0, name)
        _untouched(three)
        g.verify()
    rec = np.load(R.GOLDEN)                                     # and against the reference's own path, directly
    assert bool(want["failed"]) == bool(rec[name + ".failed"])
    frames = rec[name + ".path_frame"]
    assert np.array_equal(got.path_token[0][frames], rec[name + ".path_token"]) and int((got.path_token[0] >= 0).sum()) == len(frames)


@pytest.mark.parametrize("name", EDGES)
def test_edges(gpu, name):
    em, tok, V, blank = _edge_inputs(name)
    T, N = len(em), len(tok)
    plan = ops.ctc_align_plan(max(T, 1), max(N, 1), V)
    if name in ("words_in_workspace", "three_per_thread"):     # the decision words do not fit LDS: they go through the workspace
        assert plan["ws_bytes_per_row"] > 0 and plan["bits_frames"] < T
    elif N <= 300:
        assert plan["ws_bytes_per_row"] == 0 and plan["bits_frames"] == T
    assert plan["tokens_per_thread"] == {"words_in_workspace": 2, "n_two_per_thread": 2, "three_per_thread": 3}.get(name, 1)
    with guarded.active() as g:
        got, three = _launch(g, [em], [tok], V, blank=blank, want_trellis=name != "three_per_thread")
        want = _check_row(got, 0, em, tok, V, blank, name)
        _untouched(three)
        assert g.allocs
        g.verify()
    assert bool(want["failed"]) == (name == "t_eq_n_minus_1") or name == "minus_inf"


def test_token_outside_the_vocabulary_is_clamped_and_reported(gpu):
    em, tok, V, blank = _edge_inputs("n65")
    wild = tok.copy()
    wild[[3, 40]] = [V + 5, -2]
    with guarded.active() as g:
        got, three = _launch(g, [em], [wild], V)
        ref, _ = _launch(g, [em], [np.clip(wild, 0, V - 1)], V)
        _check_row(got, 0, em, wild, V, 0, "wild tokens")
        _untouched(three)
        g.verify()
    assert got.span[0, 3] == 2 and ref.span[0, 3] == 0 and got.span[0, :3].tolist() == ref.span[0, :3].tolist()
    for a, b in zip(got[:4] + (got.trellis,), ref[:4] + (ref.trellis,)):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))


def test_ragged_batch_rows_equal_their_own_launch(gpu):
    """Five rows: different T_b and N_b, one that cannot align (T_b < N_b), one without tokens.  Every row equals the host model, equals
    its own B = 1 launch bit for bit, and the other rows do not notice the failing ones."""
    rng = np.random.default_rng(11)
    shapes = [(70, 9, "ls"), (33, 40, "ls"), (120, 66, "int"), (50, 0, "ls"), (97, 31, "ls")]
    V = 29
    ems = [_emission(rng, T, V, kind) for T, _, kind in shapes]
    toks = [rng.integers(1, V, size=N).astype(np.int32) for _, N, _ in shapes]
    with guarded.active() as g:
        got, three = _launch(g, ems, toks, V)
        wants = [_check_row(got, b, ems[b], toks[b], V, 0, "ragged") for b in range(5)]
        _untouched(three)
        assert [int(w["span"][3]) for w in wants] == [0, 1, 0, 1, 0]
        Tmax, Nmax = got.path_token.shape[1], got.seg.shape[1]
        for b in range(5):
            one, _ = _launch(g, [ems[b]], [toks[b]], V, Tmax=Tmax, Nmax=Nmax)
            for name, a, c in zip(ops.CtcAlignment._fields, got, one):
                assert np.array_equal(a[b].view(np.int32), c[0].view(np.int32)), (b, name)
        g.verify()


def test_two_launches_give_identical_bits(gpu):
    em, tok, V, blank = _edge_inputs("n129")
    e = torch.zeros(2, len(em), 32)
    e[:, :, :V] = torch.from_numpy(em)
    e, t = e.cuda(), torch.from_numpy(np.stack([tok, tok])).cuda()
    nf, nt = torch.full((2,), len(em), dtype=torch.int32).cuda(), torch.full((2,), len(tok), dtype=torch.int32).cuda()
    a = ops.ctc_align(e, t, nf, nt, V=V, want_trellis=True)
    b = ops.ctc_align(e, t, nf, nt, V=V, want_trellis=True)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
        assert torch.equal(x[0].view(torch.int32), x[1].view(torch.int32))           # and two workgroups of one launch
    assert int(a.span[0, 3]) == 0 and int(a.span[0, 2]) >= len(tok)


# ---------------------------------------------------------------------------------------------- log-softmax
@pytest.mark.parametrize("V", [1, 29, 32, 33, 64, 65])
def test_log_softmax_per_element(gpu, V):
    rng = np.random.default_rng(V)
    Rws = 7                                                    # two workgroups of four waves, the second one short
    x = (rng.standard_normal((Rws, V)) * 4.0).astype(np.float32)
    x[1] = -200.0
    x[1, V // 2] = 0.0                                         # one dominant logit: exactly 0.0 there
    x[2, 0] = -np.inf if V > 1 else x[2, 0]
    Y, bound = R.log_softmax_bounds(x)
    with guarded.active() as g:
        logits = guarded.guarded_input(torch.from_numpy(x).cuda(), pitch_extra=3)          # NaN pad columns
        three = g.empty((3, Rws, V + 5), dtype=torch.float32, device="cuda")
        out = ops.ctc_log_softmax(logits, out=three[1][:, :V])
        got = out.cpu().numpy()
        assert bool(torch.isnan(three[1][:, V:]).all()) and bool(torch.isnan(three[0]).all()) and bool(torch.isnan(three[2]).all())
        wide = guarded.guarded_input(torch.from_numpy(np.concatenate([x, np.full((Rws, 3), np.nan, np.float32)], 1)).cuda())
        alone = ops.ctc_log_softmax(wide, V=V)                 # a new output: pad columns unwritten (0xFF), the same bits
        assert np.array_equal(alone[:, :V].cpu().numpy().view(np.int32), got.view(np.int32)) and bool(torch.isnan(alone[:, V:]).all())
        g.verify()
    finite = np.isfinite(Y)
    err = np.abs(got.astype(np.float64)[finite] - Y[finite])
    print(f"V {V}: worst |kernel - fp64| / bound = {float((err / bound[finite]).max()):.3f}")
    assert (err <= bound[finite]).all()
    assert np.array_equal(np.isneginf(got), np.isneginf(Y))
    assert got[1, V // 2] == 0.0 and not np.signbit(got[1, V // 2])


# ---------------------------------------------------------------------------------------------- the model
def _rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


def _aligner(policy="fp32"):
    runtime.set_precision(policy)
    model = CTCAligner(cfgmod.preset("B-tiny"))
    synthetic.seeded_init_(model, 4)
    return model


@pytest.mark.parametrize("policy,tol", [("fp32", 1e-3), ("bf16", 1e-2)])
def test_aligner_logits_against_the_oracle(gpu, policy, tol):
    model = _aligner(policy)
    cfg = model.cfg
    torch.manual_seed(0)
    wave = torch.randn(2, 16000) * 0.1
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    with torch.no_grad():
        hidden = O.w2v2_model(sd, "wav2vec2", cfg["audio"], wave)
        want = hidden @ sd["lm_head.weight"].T + sd["lm_head.bias"]
    model.cuda()
    logits, lengths = model(wave.cuda())
    assert lengths is None and logits.shape == want.shape == (2, 49, 29) and logits.dtype == torch.float32 and not logits.requires_grad
    r = _rel(logits, want)
    print(f"CTCAligner[{policy}] logits rel err {r:.2e}")
    assert r < tol
    em = model.emission(wave.cuda())
    assert em.shape == (2, 49, 32)
    Y, bound = R.log_softmax_bounds(logits.reshape(-1, 29).cpu().numpy())
    assert (np.abs(em[..., :29].reshape(-1, 29).cpu().numpy().astype(np.float64) - Y) <= bound).all()
    runtime.set_precision("bf16")


def test_aligner_state_dict_keys_are_wav2vec2_for_ctc(gpu):
    from transformers import Wav2Vec2Config, Wav2Vec2ForCTC
    from tav_amd.models.tav import remap_reference_keys
    a = cfgmod.preset("B-tiny")["audio"]
    hf = Wav2Vec2ForCTC(Wav2Vec2Config(vocab_size=29, hidden_size=a["hidden"], num_hidden_layers=a["layers"], num_attention_heads=a["heads"],
                                       intermediate_size=a["inter"], feat_extract_norm="group", do_stable_layer_norm=False, conv_bias=False,
                                       conv_dim=tuple(a["conv_dim"]), conv_kernel=tuple(a["conv_kernel"]), conv_stride=tuple(a["conv_stride"]),
                                       num_conv_pos_embeddings=a["pos_k"], num_conv_pos_embedding_groups=a["pos_groups"]))
    want = remap_reference_keys(hf.state_dict())
    ours = CTCAligner(cfgmod.preset("B-tiny")).state_dict()
    assert set(ours) == set(want)
    for k in ours:
        assert tuple(ours[k].shape) == tuple(want[k].shape), k


# ---------------------------------------------------------------------------------------------- end to end
def test_get_times_and_align_batch_end_to_end(gpu):
    model = _aligner("fp32").cuda()
    torch.manual_seed(3)
    lengths, texts = [8000, 12345, 16000], ["hi", "a cat", "go on now"]
    waves = [(torch.randn(n) * 0.1).cuda() for n in lengths]
    want = []
    for w, text in zip(waves, texts):
        em = model.emission(w[None])[0, :, :29].cpu().numpy()            # the device's own emission bits, aligned on the host
        _, tokens = GT.transcript_tokens(text, GT.LABELS)
        a = R.align(em, tokens)
        assert not a["failed"]
        ratio = w.shape[0] / em.shape[0]
        want.append(((int(a["span"][0]) * ratio) / 16000, (int(a["span"][1]) * ratio) / 16000))
        got = GT.get_times(w[None].cpu(), text, model, GT.LABELS, 16000)
        assert got == want[-1], (text, got, want[-1])
        two = torch.stack([w, torch.zeros_like(w)])                      # channel 0 is the one aligned
        assert GT.get_times(two, text, model) == want[-1]
        # the four functions one by one, as the reference chains them
        emission = torch.from_numpy(em).cuda()
        tr = GT.get_trellis(emission, tokens)
        assert np.array_equal(tr.cpu().numpy().view(np.int32), a["trellis"].view(np.int32))
        path = GT.backtrack(tr, emission, tokens)
        assert [p.token_index for p in path] == a["path_token"][a["path_token"] >= 0].tolist() and path[0].time_index == a["span"][0]
        with pytest.raises(ValueError, match="does not belong"):
            GT.backtrack(tr[:-1], emission, tokens)
    times, status = GT.align_batch(waves, texts, model)
    assert times.dtype == torch.float64 and times.shape == (3, 2) and status.tolist() == [0, 0, 0]
    assert [tuple(r) for r in times.tolist()] == want
    long_text = "this transcript has many more letters than the first utterance has frames"
    with pytest.raises(ValueError, match="Failed to align") as info:
        GT.align_batch(waves, [long_text, texts[1], texts[2]], model)
    assert info.value.status.tolist() == [1, 0, 0] and [tuple(r) for r in info.value.times[1:].tolist()] == want[1:]
    assert bool(torch.isnan(info.value.times[0]).all())
    with pytest.raises(ValueError, match="Failed to align"):
        GT.get_times(waves[0][None], long_text, model)
    runtime.set_precision("bf16")
