"""CPU: the forced alignment's host side.

The numpy restatement (tests/ctc_align_ref.py) against the record of the reference's own get_trellis / backtrack (tests/golden/
ctc_align_golden.npz) bit for bit; csrc/align_plan.h alone under ASan + UBSan as a program of its own (tests/host_program.py);
include/tavhip_align.h against its row of _lib.ABIS type by type and the families kept apart (tests/abi_check.py); argument faults
through the built library; and the Python pieces of run_scripts/get_times.py that need no GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import abi_check
import ctc_align_ref as R
import tav_amd  # noqa: F401
from host_program import run_alone_under_sanitizers
from tav_amd import _lib
from tav_amd.run_scripts import get_times as GT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_NULL, ERR_SHAPE, ERR_ALIGN = -1, -2, -4


# ---------------------------------------------------------------------------------------------- the record
def test_restatement_equals_the_reference_record_bit_for_bit():
    rec = np.load(R.GOLDEN)
    on_path_ties = tied_maxima = failing = stored = 0
    for name, T, N, V, _ in R.CASES:
        em, tokens = R.case_inputs(name)
        assert em.shape == (T, V) and tokens.shape == (N,)
        assert np.array_equal(em.view(np.int32), rec[name + ".emission"].view(np.int32)) and np.array_equal(tokens, rec[name + ".tokens"])
        tr = R.trellis(em, tokens)
        path, t_start, failed = R.backtrack(tr, em, tokens)
        assert int(rec[name + ".failed"]) == int(failed), name
        if name + ".trellis" in rec:
            stored += 1
            assert np.array_equal(tr.view(np.int32), rec[name + ".trellis"].view(np.int32)), name
        assert [p[0] for p in path] == rec[name + ".path_token"].tolist() and [p[1] for p in path] == rec[name + ".path_frame"].tolist(), name
        a = R.align(em, tokens)
        if not failed:
            want, margin = R.prob_bounds(em, a["column"])
            frames = rec[name + ".path_frame"]
            assert (np.abs(rec[name + ".path_prob"].astype(np.float64) - want[frames]) <= margin[frames]).all(), name
            assert a["span"].tolist() == [path[0][1], t_start, len(path), 0]
            assert (a["seg"][:, 0] < a["seg"][:, 1]).all() and a["seg"][0, 0] == path[0][1] and a["seg"][-1, 1] == t_start
            assert (a["seg"][1:, 0] == a["seg"][:-1, 1]).all()
        else:
            assert a["span"].tolist() == [-1, -1, 0, 1] and (a["path_token"] == -1).all() and (a["seg"] == -1).all()
        n, tied = R.ties(em, tokens)
        on_path_ties, tied_maxima, failing = on_path_ties + n, tied_maxima + tied, failing + failed
    assert on_path_ties >= 1 and tied_maxima >= 1 and failing >= 1 and stored >= 4
    assert os.path.getsize(R.GOLDEN) < 200 * 1024


def test_restatement_edges():
    em = np.log(np.full((3, 4), 0.25, np.float32))
    assert R.align(em, [])["span"].tolist() == [-1, -1, 0, 1]                     # no tokens: the reference's loop never runs
    assert R.align(em[:0], [1])["span"].tolist() == [-1, -1, 0, 1]                # no frames
    a = R.align(em, [1, 9])                                                       # a token id outside [0, V): clamped, status bit 1
    b = R.align(em, [1, 3])
    assert a["span"].tolist() == (b["span"] | np.array([0, 0, 0, 2])).tolist() and np.array_equal(a["trellis"], b["trellis"])
    # uniform emissions: every frame costs the same, so the last column peaks at t = N, the smallest t that reaches it
    assert b["path_token"].tolist() == [0, 1, -1] and b["span"].tolist() == [0, 2, 2, 0] and b["seg"].tolist() == [[0, 1], [1, 2]]
    x = np.array([[0.0, -200.0, 3.0, 1.0]], np.float32)
    Y, bound = R.log_softmax_bounds(x)
    assert abs(Y[0, 2] + np.log1p(np.exp(-2.0) + np.exp(-3.0))) < 1e-12 and (bound > 0).all() and bound[0, 2] < 1e-6
    assert (bound <= 16 * R.U * (np.abs(Y) + 1)).all()                            # a few roundings of the element's own magnitude


# ---------------------------------------------------------------------------------------------- align_plan.h alone
def test_plan_header_alone_under_sanitizers(tmp_path):
    run_alone_under_sanitizers("align_plan_check.cpp", tmp_path)


# ---------------------------------------------------------------------------------------------- header against binding
def test_align_binding_matches_its_header_type_by_type(tmp_path):
    assert len(abi_check.check_binding(abi_check.abi("tavhip_align.h"), tmp_path)) == 5


def test_main_header_symbol_set_is_unchanged():
    """The alignment entry points live in their own header and table: include/tavhip.h declares exactly what _SIGS binds, as before, and
    none of the new names; the main ABI version did not move."""
    abi_check.check_families_apart()


# ---------------------------------------------------------------------------------------------- argument faults, nothing launches
def _args(**kw):
    a = _lib.CtcAlignArgs()
    for f in ("emission", "tokens", "n_frames", "n_tokens", "path_token", "path_prob", "seg", "seg_score", "span"):
        setattr(a, f, 64)                                     # only tested for NULL-ness before a fault is found
    a.B, a.Tmax, a.Nmax, a.V, a.ld, a.blank_id = 2, 100, 20, 29, 32, 0
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_invalid_arguments_are_refused_before_any_launch():
    h = _lib.lib()
    call = lambda **kw: h.tav_ctc_align(C.byref(_args(**kw)), None)          # noqa: E731
    assert h.tav_ctc_align(None, None) == ERR_NULL
    for f in ("emission", "tokens", "n_frames", "n_tokens", "path_token", "path_prob", "seg", "seg_score", "span"):
        assert call(**{f: None}) == ERR_NULL, f
    assert call(B=0) == ERR_SHAPE and call(B=-3) == ERR_SHAPE and call(B=65536) == ERR_SHAPE
    assert call(V=33) == ERR_SHAPE                                            # V > ld
    assert call(Tmax=4097) == ERR_SHAPE and call(Nmax=2049) == ERR_SHAPE and call(Tmax=0) == ERR_SHAPE and call(Nmax=0) == ERR_SHAPE
    assert call(V=129, ld=132) == ERR_SHAPE and call(blank_id=29) == ERR_SHAPE and call(blank_id=-1) == ERR_SHAPE
    assert call(ld=30) == ERR_ALIGN and call(ld=31) == ERR_ALIGN
    assert call(ld=30, Tmax=4097) == ERR_SHAPE and call(ld=30, span=None) == ERR_NULL      # pointers, then sizes, then strides
    assert call(Tmax=1200, Nmax=1100) == ERR_NULL                             # these sizes need the workspace
    assert call(Tmax=1200, Nmax=1100, workspace=64, workspace_bytes=8) == ERR_SHAPE
    p = _lib.AlignPlan()
    assert h.tav_ctc_align_plan(3000, 2048, 32, C.byref(p)) == 0 and p.block * p.tokens_per_thread >= 2049 and p.lds_bytes <= 160 * 1024
    assert p.ws_bytes_per_row == 3000 * (p.block // 64) * p.tokens_per_thread * 8 and p.bits_frames < 3000
    assert h.tav_ctc_align_ws_bytes(5, 3000, 2048, 32) == 5 * p.ws_bytes_per_row
    assert h.tav_ctc_align_plan(499, 60, 32, C.byref(p)) == 0 and (p.block, p.tokens_per_thread, p.ws_bytes_per_row, p.bits_frames) == (64, 1, 0, 499)
    assert h.tav_ctc_align_ws_bytes(32, 499, 60, 32) == 0
    assert h.tav_ctc_align_plan(4097, 60, 32, C.byref(p)) == ERR_SHAPE and h.tav_ctc_align_plan(499, 60, 32, None) == ERR_NULL
    assert h.tav_ctc_align_ws_bytes(0, 499, 60, 32) == ERR_SHAPE and h.tav_ctc_align_ws_bytes(1, 499, 2049, 32) == ERR_SHAPE
    ls = h.tav_ctc_log_softmax
    assert ls(None, 64, 4, 29, 32, 32, None) == ERR_NULL and ls(64, None, 4, 29, 32, 32, None) == ERR_NULL
    assert ls(64, 64, 0, 29, 32, 32, None) == ERR_SHAPE and ls(64, 64, 4, 0, 32, 32, None) == ERR_SHAPE
    assert ls(64, 64, 4, 33, 32, 36, None) == ERR_SHAPE and ls(64, 64, 4, 33, 36, 32, None) == ERR_SHAPE


# ---------------------------------------------------------------------------------------------- run_scripts/get_times.py without a GPU
def test_merge_repeats_transcript_and_seconds():
    P = GT.Point
    path = [P(0, 3, 0.5), P(0, 4, 0.25), P(1, 5, 1.0), P(2, 6, 0.5), P(2, 7, 0.5), P(2, 8, 0.125)]
    ratio, sr = 16000 / 49, 16000
    start, end = GT.merge_repeats(path, ratio, "A|B", sr)
    assert (start, end) == ((3 * ratio) / sr, (9 * ratio) / sr)                  # Python floats, the reference's order of operations
    # the segments themselves: consecutive equal token_index, score = mean
    seen = []
    orig = GT.Segment

    class Spy(orig):
        def __init__(self, *a):
            super().__init__(*a)
            seen.append(self)
    GT.Segment = Spy
    try:
        GT.merge_repeats(path, ratio, "A|B", sr)
    finally:
        GT.Segment = orig
    assert [(s.label, s.start, s.end, s.score, s.length) for s in seen] == [("A", 3, 5, 0.375, 2), ("|", 5, 6, 1.0, 1), ("B", 6, 9, 0.375, 3)]
    assert repr(seen[0]) == "A\t(0.38): [    3,     5)"
    assert GT.merge_repeats([P(0, 7, 1.0)], 2.0, "A", 4) == (3.5, 4.0)
    transcript, tokens = GT.transcript_tokens("hi there", GT.LABELS)
    assert transcript == "HI|THERE" and tokens == [8, 7, 1, 3, 8, 2, 10, 2]
    with pytest.raises(KeyError):
        GT.transcript_tokens("hi, there", GT.LABELS)
    assert len(GT.LABELS) == 29 and GT.LABELS[0] == "-" and GT.LABELS[1] == "|" and len(set(GT.LABELS)) == 29 and GT.SAMPLE_RATE == 16000
    with pytest.raises(ValueError, match="Failed to align"):
        GT._points([], [], [-1, -1, 0, 1])
    assert GT._points([-1, 0, 1], [0.0, 0.5, 0.25], [1, 3, 2, 0]) == [P(0, 1, 0.5), P(1, 2, 0.25)]


def test_root_shim_exposes_the_reference_names():
    import importlib.util
    spec = importlib.util.spec_from_file_location("root_get_times", os.path.join(ROOT, "run_scripts", "get_times.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for name in ("Point", "Segment", "get_trellis", "backtrack", "merge_repeats", "get_times", "align_batch"):
        assert getattr(mod, name) is getattr(GT, name)


def test_aligner_state_dict_keys_and_head_padding():
    import torch
    from tav_amd import config as cfgmod
    from tav_amd.models.aligner import CTCAligner
    m = CTCAligner(cfgmod.preset("B-tiny"))
    keys = set(m.state_dict())
    assert {"lm_head.weight", "lm_head.bias", "wav2vec2.feature_extractor.conv_layers.0.conv.weight", "wav2vec2.feature_projection.projection.weight",
            "wav2vec2.encoder.layers.1.attention.q_proj.weight", "wav2vec2.encoder.layer_norm.weight"} <= keys
    assert all(k.startswith(("wav2vec2.", "lm_head.")) for k in keys)
    assert m.lm_head.weight.shape == (29, 768) and m.vocab_padded == 32 and CTCAligner(cfgmod.preset("B-tiny"), vocab=32).vocab_padded == 32
    w, b = m._head_operands(torch.float32)
    assert w.shape == (32, 768) and torch.equal(w[:29], m.lm_head.weight.detach()) and not bool(w[29:].any()) and not bool(b[29:].any())
