"""GPU: tav_audio_resample (csrc/audio_resample.hip) against its host model (tests/audio_resample_ref.py).

Every case of the model stays within the per-element bound (ntap + C + 1) u S[i] of the fp64 chain, the row's tail is exactly 0.0 and the
mask exactly 1.0 / 0.0, for a row of exactly L_out elements and for a longer one; an impulse returns the f32 table's taps bit for bit; two
launches give identical bits; speech_features_device is the chain for host and for device PCM; the rows collate_batch_device fills from PCM
items equal speech_features_device on each item alone and nothing else of the batch moves.

The kernel tests run inside the guard-band allocator (tests/guarded.py): the sources sit in watched buffers with a padded pitch (0xFF between
the rows: a read past a channel's or a frame's end reaches the result as NaN or -1), the rows a launch fills start as 0xFF (an unwritten
element is NaN) and are the middle row of a three-row tensor whose neighbours must stay 0xFF, and verify() reports any store outside a
tensor or into an operand."""
import numpy as np
import pytest
import torch

import audio_resample_ref as R
import guarded
import tav_amd  # noqa: F401
from tav_amd import config as cfgmod
from tav_amd import ops, synthetic
from tav_amd.models import tav as M

pytestmark = pytest.mark.gpu


def _source(raw, pitch_extra):
    """The PCM as a device tensor inside a guarded buffer; 2-D sources get a padded pitch."""
    return guarded.guarded_input(torch.from_numpy(raw).cuda(), pitch_extra=pitch_extra if raw.ndim == 2 else 0)


def _rows(g, T_row):
    """The middle rows of two 0xFF [3, T_row] tensors: values and mask."""
    v = g.empty((3, T_row), dtype=torch.float32, device="cuda")
    m = g.empty((3, T_row), dtype=torch.float32, device="cuda")
    return v, m


def _neighbours_untouched(t):
    return bool(torch.isnan(t[0]).all()) and bool(torch.isnan(t[2]).all())


@pytest.mark.parametrize("case", list(R.CASES))
def test_every_case_stays_within_the_bound(gpu, case):
    c = R.CASES[case]
    want, bnd = R.reference(case)
    L_out = len(want)
    raw = R.source(case)
    with guarded.active() as g:
        table = ops.audio_resample_table(c["sr"])
        if case == "44k_seam":
            assert L_out == table.tile + 1
        for extra, k in ((0, 3), (37, 2)):
            src = _source(raw, pitch_extra=k)
            vals, mask = _rows(g, L_out + extra)
            out = ops.audio_resample(src, table, out=vals[1], mask=mask[1], layout=c["layout"])
            assert out.data_ptr() == vals[1].data_ptr()
            got, gm = vals[1].cpu().numpy(), mask[1].cpu().numpy()
            r = R.worst_ratio(got[:L_out], want, bnd)
            print(f"{case} T_row = L_out + {extra}: worst |kernel - fp64| / bound = {r:.3f}")
            assert r <= 1.0, (case, extra, r)
            assert np.array_equal(got[L_out:].view(np.int32), np.zeros(extra, np.int32))                 # the tail is +0.0
            assert np.array_equal(gm, np.concatenate([np.ones(L_out, np.float32), np.zeros(extra, np.float32)]))
            assert _neighbours_untouched(vals) and _neighbours_untouched(mask)
        # without a mask and without an out: a new tensor of L_out, the same bits
        alone = ops.audio_resample(_source(raw, pitch_extra=1), table, layout=c["layout"])
        assert alone.shape == (L_out,) and np.array_equal(alone.cpu().numpy().view(np.int32), got[:L_out].view(np.int32))
        assert g.allocs
        g.verify()


def test_identity_pair_is_exact(gpu):
    """16 kHz in: the mono result is the input bit for bit, the stereo result the f32 mean (a + b) * 0.5f."""
    with guarded.active() as g:
        table = ops.audio_resample_table(16000)
        mono = R.source("16k_mono_f32")
        got = ops.audio_resample(_source(mono, 0), table)
        assert np.array_equal(got.cpu().numpy().view(np.int32), mono.view(np.int32))
        st = R.source("16k_stereo_f32")
        got = ops.audio_resample(_source(st, 5), table, layout="CL")
        assert np.array_equal(got.cpu().numpy(), ((st[0] + st[1]).astype(np.float32) * np.float32(0.5)).astype(np.float32))
        i16 = R.source(dict(sr=16000, L=1000, C=1, dtype="i16", layout="L"))
        got = ops.audio_resample(_source(i16, 0), table)
        assert np.array_equal(got.cpu().numpy(), i16.astype(np.float32) / np.float32(32768.0))
        g.verify()


@pytest.mark.parametrize("sr", [44100, 8000])
def test_impulse_returns_the_table(gpu, sr):
    """A mono 2^-3 at one position: every output that sees it is 2^-3 * h[p][k] of the f32 table, bit for bit (a power of two scales exactly),
    and every other output is 0.0 -- at position 0, at L - 1 and mid-stream."""
    L = 1500
    h32, o, n, width = R.table32(sr)
    L_out = R.resampled_length(L, sr)
    i = np.arange(L_out)
    q, p = i // n, i % n
    with guarded.active() as g:
        table = ops.audio_resample_table(sr)
        for pos in (0, L - 1, 701):
            x = np.zeros(L, np.float32)
            x[pos] = 0.125
            k = pos + width - q * o                                # the tap of phase p that meets the impulse
            seen = (k >= 0) & (k < h32.shape[1])
            want = np.where(seen, h32[p, np.clip(k, 0, h32.shape[1] - 1)] * np.float32(0.125), np.float32(0)).astype(np.float32)
            want = (want + np.float32(0)).astype(np.float32)       # a tap that rounded to -0.0 gives +0.0: fmaf(-0.0, x, +0.0)
            assert np.count_nonzero(want) >= min(table.ntap, 12) // 2
            got = ops.audio_resample(_source(x, 0), table).cpu().numpy()
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), (sr, pos)
        g.verify()


def test_two_launches_give_identical_bits(gpu):
    c = R.CASES["44k_3s_stereo_i16"]
    src = torch.from_numpy(R.source("44k_3s_stereo_i16")).cuda()
    table = ops.audio_resample_table(c["sr"])
    a = ops.audio_resample(src, table)
    b = ops.audio_resample(src, table)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and not bool(torch.isnan(a).any())


def test_speech_features_device_is_the_chain(gpu):
    """The public entry: host PCM (shipped once, int16 as int16) and device PCM give the same bits, within the bound of the fp64 chain; `out`
    and `mask` rows are filled in full; numpy input and float64 input are taken."""
    for case in ("44k_stereo_i16", "48k_stereo_f32", "8k_mono_i16", "16k_stereo_f32"):
        c = R.CASES[case]
        want, bnd = R.reference(case)
        raw = R.source(case)
        host = M.speech_features_device(torch.from_numpy(raw), c["sr"])
        dev = M.speech_features_device(torch.from_numpy(raw).cuda(), c["sr"])
        arr = M.speech_features_device(raw, c["sr"])
        assert host.is_cuda and host.dim() == 1 and host.dtype == torch.float32 and host.shape == (len(want),)
        assert torch.equal(host.view(torch.int32), dev.view(torch.int32)) and torch.equal(host, arr)
        r = R.worst_ratio(host.cpu().numpy(), want, bnd)
        print(f"{case}: worst |speech_features_device - fp64| / bound = {r:.3f}")
        assert r <= 1.0
        rows = torch.full((2, len(want) + 9), float("nan"), device="cuda")
        got = M.speech_features_device(torch.from_numpy(raw), c["sr"], out=rows[0], mask=rows[1])
        assert got.data_ptr() == rows.data_ptr() and torch.equal(rows[0, :len(want)], host) and not bool(rows[0, len(want):].any())
        assert rows[1].tolist() == [1.0] * len(want) + [0.0] * 9
        if c["dtype"] == "f32":
            assert torch.equal(M.speech_features_device(torch.from_numpy(raw).double(), c["sr"]), host)
    with pytest.raises(ValueError, match="squeeze"):
        M.speech_features_device(torch.zeros(2, 2).cuda(), 44100)
    with pytest.raises(ValueError, match="empty waveform"):
        M.speech_features_device(torch.zeros(0).cuda(), 44100)


def _swap_audio(items, waves):
    return [([i[0], w, i[2]], lab) for (i, lab), w in zip(items, waves)]


def test_collate_batch_device_fills_the_rows(gpu):
    """Three items with 44.1 kHz stereo int16 PCM of unequal length: audio and its mask equal, bit for bit, the same batch collated from the
    waveforms speech_features_device returns item by item; under one seed the video clip, the video mask, the text and the labels are
    those of the finished-waveform call, with finished float clips and with decoded frames (the audio path draws nothing)."""
    cfg = cfgmod.preset("B-tiny")
    for raw_video, kw in ((None, {}), ((9, 40, 56), dict(size=32, num_frames=16))):
        items = synthetic.make_items(cfg, 3, raw_video=raw_video, seed=5, s_text=8, t_audio=3000, raw_audio=(44100, 2))
        waves = [M.speech_features_device(i[1]["pcm"], i[1]["sampling_rate"]) for (i, _) in items]
        lens = [R.resampled_length(len(i[1]["pcm"]), 44100) for (i, _) in items]
        assert [len(w) for w in waves] == lens and len(set(lens)) == 3
        torch.manual_seed(7)
        (t, a, v), lab = M.collate_batch_device(items, "train", n_visual_true=4, **kw)
        after = torch.get_rng_state()
        torch.manual_seed(7)
        (t2, a2, v2), lab2 = M.collate_batch_device(_swap_audio(items, [w.cpu() for w in waves]), "train", n_visual_true=4, **kw)
        assert torch.equal(after, torch.get_rng_state())
        T = max(lens)
        assert a["audio_features"].shape == (3, T) and a["audio_features"].dtype == torch.float32 and a["attention_mask"].shape == (3, T)
        assert torch.equal(a["audio_features"].view(torch.int32), a2["audio_features"].view(torch.int32))
        assert torch.equal(a["attention_mask"], a2["attention_mask"])
        for b in range(3):                                         # and against the rows written out by hand
            assert torch.equal(a["audio_features"][b, :lens[b]], waves[b]) and not bool(a["audio_features"][b, lens[b]:].any())
            assert a["attention_mask"][b].tolist() == [1.0] * lens[b] + [0.0] * (T - lens[b])
        assert torch.equal(v["visual_embeds"], v2["visual_embeds"]) and torch.equal(v["attention_mask"], v2["attention_mask"])
        assert torch.equal(t["input_ids"], t2["input_ids"]) and torch.equal(t["attention_mask"], t2["attention_mask"]) and torch.equal(lab, lab2)
    # mixed sampling rates and layouts in one batch
    mixed = _swap_audio(items, [{"pcm": torch.from_numpy(R.source(c)), "sampling_rate": R.CASES[c]["sr"]}
                                for c in ("48k_stereo_f32", "8k_mono_i16", "16k_mono_f32")])
    (_, am, _), _ = M.collate_batch_device(mixed, "val", n_visual_true=4, **kw)
    for b, c in enumerate(("48k_stereo_f32", "8k_mono_i16", "16k_mono_f32")):
        want, bnd = R.reference(c)
        assert R.worst_ratio(am["audio_features"][b, :len(want)].cpu().numpy(), want, bnd) <= 1.0
        assert int(am["attention_mask"][b].sum()) == len(want)
    with pytest.raises(ValueError, match="not both"):
        M.collate_batch_device([items[0], _swap_audio(items, [w.cpu() for w in waves])[1]], "train")
