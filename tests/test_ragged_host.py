"""CPU: the length-aware (per-row sequence length) entry points are exported and bound, and refuse bad arguments before
anything is launched; the engine refuses the paths that are not built for per-row lengths."""
import ctypes as C

import pytest
import torch

import tav_amd  # noqa: F401
from tav_amd import _lib, engine, ops, runtime, synthetic
from tav_amd import config as cfgmod
from tav_amd.models.tav import collate_batch, visual_true_counts
from tav_amd.utils.global_functions import arg_parse

NEW = ("tav_attn_fwd_len", "tav_attn_bwd_len", "tav_mean_pool_fwd_len", "tav_mean_pool_bwd_len")


def test_length_aware_symbols_are_exported_and_bound():
    h = _lib.lib()
    for n in NEW:
        assert hasattr(h, n), n
        assert n in _lib.declared_symbols(), n
    assert h.tav_version() == _lib.ABI_VERSION == 7


def _valid_args(bwd):
    """Host-valid attention arguments (fake, never dereferenced: validation returns before any launch)."""
    a = _lib.AttnArgs()
    a.q = a.k = a.v = a.o = a.lse = 4096
    a.B, a.S, a.nheads = 2, 100, 2
    a.ld_q = a.ld_k = a.ld_v = a.ld_o = 3 * 128
    a.dtype, a.mask_mode, a.scale = _lib.TAV_BF16, 0, 0.125
    if bwd:
        a.dout = a.dq = a.dk = a.dv = a.delta = 4096
        a.ld_do = a.ld_dq = a.ld_dk = a.ld_dv = 3 * 128
    return a


@pytest.mark.parametrize("name,bwd", [("tav_attn_fwd_len", False), ("tav_attn_bwd_len", True)])
def test_attention_len_argument_validation(name, bwd):
    fn = getattr(_lib.lib(), name)
    assert fn(C.byref(_lib.AttnArgs()), None, None) == -1                  # NULL operands: TAV_ERR_NULL
    assert fn(C.byref(_valid_args(bwd)), None, None) == -1                 # NULL seq_lens: TAV_ERR_NULL
    a = _valid_args(bwd)
    a.S = 0
    assert fn(C.byref(a), 4096, None) == -2                                # shapes checked as in the plain form
    a = _valid_args(bwd)
    a.mask_mode = 2                                                        # mode 2 without corr / o_soft / mask
    assert fn(C.byref(a), 4096, None) == -1
    a = _valid_args(bwd)
    a.dtype = 7
    assert fn(C.byref(a), 4096, None) == -3


def test_mean_pool_len_argument_validation():
    h = _lib.lib()
    assert h.tav_mean_pool_fwd_len(4096, 4096, None, 2, 10, 768, None) == -1
    assert h.tav_mean_pool_fwd_len(4096, 4096, 4096, 2, 10, 766, None) == -2
    assert h.tav_mean_pool_fwd_len(4096, 4096, 4096, 0, 10, 768, None) == -2
    assert h.tav_mean_pool_bwd_len(4096, 4096, None, 0, None, 2, 10, 768, None) == -1
    assert h.tav_mean_pool_bwd_len(4096, None, None, 0, 4096, 2, 10, 768, None) == -1
    assert h.tav_mean_pool_bwd_len(4096, 4096, None, 0, 4096, 2, 0, 768, None) == -2


def test_ops_reject_malformed_seq_lens():
    x = torch.zeros(4, 8)
    for bad in ([3, 4], torch.tensor([3, 4], dtype=torch.int64), torch.tensor([3, 4, 5], dtype=torch.int32)):
        with pytest.raises(ValueError, match="seq_lens"):
            ops._seq_lens(bad, 2, x.device)
    ok = torch.tensor([3, 4], dtype=torch.int32)
    assert ops._seq_lens(ok, 2, x.device) is ok


class _Pol:
    def __init__(self, fp8):
        self.fp8, self.f32, self.fp8_stacks = fp8, not fp8, ("video", "fusion") if fp8 else ()


class _Ctx:
    def __init__(self, fp8):
        self.pol = _Pol(fp8)


def test_layer_spec_carries_seq_lens_and_fp8_refuses_it():
    assert engine.LayerSpec(2, 16, 2, 1e-12, pre_ln=True).seq_lens is None
    sl = torch.tensor([16, 9], dtype=torch.int32)
    spec = engine.LayerSpec(2, 16, 2, 1e-12, pre_ln=True, branch="video", seq_lens=sl)
    assert spec.seq_lens is sl
    with pytest.raises(ValueError, match="fp8"):
        engine.encoder_layer(_Ctx(True), spec, torch.zeros(32, 128), None, None, [None] * 16)


def test_slow_path_options_refuse_seq_lens():
    sl = torch.tensor([16, 9], dtype=torch.int32)
    for kw in (dict(head_scale=torch.ones(2)), dict(probs_out=[])):
        spec = engine.LayerSpec(2, 16, 2, 1e-12, pre_ln=True, mask_mode=2, branch="fusion", seq_lens=sl, **kw)
        with pytest.raises(NotImplementedError, match="seq_lens"):
            engine.encoder_layer(_Ctx(False), spec, torch.zeros(32, 128), None, None, [None] * 16)


def test_visual_rows_switch_defaults_to_equal():
    assert runtime.visual_rows() == "equal"
    with pytest.raises(ValueError):
        runtime.set_visual_rows("jagged")
    assert runtime.visual_rows() == "equal"


def _items(B, frames=16, image=32):
    g = torch.Generator().manual_seed(0)
    return [([{"input_ids": torch.arange(8), "attention_mask": torch.ones(8)}, torch.randn(400 + 10 * b, generator=g),
              torch.randn(frames, 3, image, image, generator=g)], b % 7) for b in range(B)]


def test_collate_ragged_draws_per_token_and_keeps_rows_unequal():
    torch.manual_seed(0)
    B = 32
    (tx, au, vi), lab = collate_batch(_items(B, frames=16, image=224), "train", visual_rows="ragged")
    m = vi["attention_mask"]
    assert m.dtype == torch.bool and tuple(m.shape) == (B, 1568)
    p = m.float().mean().item()
    assert abs(p - 1 / 15) < 0.005, p                      # 50 176 Bernoulli(1/15) draws: std 0.0011
    counts = m.sum(1)
    assert len(set(counts.tolist())) > 1                   # rows keep their own counts (no equalising)
    torch.manual_seed(0)
    (tx2, au2, vi2), lab2 = collate_batch(_items(B, frames=16, image=224), "train")
    c2 = vi2["attention_mask"].sum(1)
    assert bool((c2 == c2[0]).all())                       # the default still equalises
    for a, b in ((tx, tx2), (au, au2)):
        assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    assert torch.equal(lab, lab2) and torch.equal(vi["visual_embeds"], vi2["visual_embeds"])
    with pytest.raises(ValueError):
        collate_batch(_items(2), "train", visual_rows="nope")


def test_make_batch_honours_per_row_counts():
    cfg = cfgmod.preset("B-tiny")
    (tx, au, vi), lab = synthetic.make_batch(cfg, 4, s_text=16, t_audio=800, n_visual_true=[3, 5, 4, 1])
    assert vi["attention_mask"].sum(1).tolist() == [3, 5, 4, 1]
    (_, _, vi2), _ = synthetic.make_batch(cfg, 4, s_text=16, t_audio=800, n_visual_true=4)
    assert vi2["attention_mask"].sum(1).tolist() == [4, 4, 4, 4]
    with pytest.raises(ValueError):
        synthetic.make_batch(cfg, 4, s_text=16, t_audio=800, n_visual_true=[3, 5])


def test_visual_true_counts_by_mode():
    m = torch.zeros(3, 32, dtype=torch.bool)
    m[0, :3], m[1, :5], m[2, :4] = True, True, True
    assert visual_true_counts(m, None) is None             # equal mode: the encoder counts (and checks) as before
    assert visual_true_counts(m, 4) == 4
    assert visual_true_counts(m, [4, 4, 4]) == 4
    with pytest.raises(ValueError, match="same number"):
        visual_true_counts(m, [3, 5, 4])
    runtime.set_visual_rows("ragged")
    try:
        assert visual_true_counts(m, None) == [3, 5, 4]
        assert visual_true_counts(m, [3, 5, 4]) == [3, 5, 4]
        assert visual_true_counts(m, torch.tensor([4, 4, 4])) == 4
    finally:
        runtime.set_visual_rows("equal")


def test_visual_rows_flag_parses():
    assert arg_parse("TAV", []).visual_rows == "equal"
    assert arg_parse("TAV", ["--visual-rows", "ragged"]).visual_rows == "ragged"
    with pytest.raises(SystemExit):
        arg_parse("TAV", ["--visual-rows", "jagged"])


def test_captured_data_parallel_step_refuses_ragged_rows():
    from tav_amd import ddp
    runtime.set_visual_rows("ragged")
    try:
        with pytest.raises(ValueError, match="ragged"):
            ddp.GraphedStep(None, None)
    finally:
        runtime.set_visual_rows("equal")
