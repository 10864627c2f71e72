"""GPU: tav_video_clip_transform (csrc/video_transform.hip) against its host model (tests/video_transform_ref.py).

Every case of the model, under all four flip combinations, both layouts and both source dtypes, stays within the per-element bound
16 u (v_raw a_c + |b_c|) of the fp64 chain; the exact cases are bit-equal to it; two launches give identical bits; the slabs of
collate_batch_device equal video_features_device on each item alone.

The kernel tests run inside the guard-band allocator (tests/guarded.py): the sources sit in watched buffers with a padded pitch (0xFF between
the rows: a read past a row's end or past the frame reaches the result as NaN or 255), outputs start as 0xFF (an unwritten element is NaN), the
slab a launch fills lies between two slabs that must stay untouched, and verify() reports any store outside a tensor or into an operand."""
import numpy as np
import pytest
import torch

import guarded
import tav_amd  # noqa: F401
import video_transform_ref as R
from tav_amd import config as cfgmod
from tav_amd import ops, synthetic
from tav_amd.models import tav as M

pytestmark = pytest.mark.gpu
RAW = dict(mean=(0.0, 0.0, 0.0), std=(1 / 255.0,) * 3)                # scale 1, shift 0


def _source(src_thwc, layout, dtype, pitch_extra):
    """The frames as a device tensor of the given layout and dtype inside a guarded buffer with a padded pitch."""
    t = torch.from_numpy(src_thwc)
    if layout == "CTHW":
        t = t.permute(3, 0, 1, 2).contiguous()
    return guarded.guarded_input(t.to(dtype).cuda(), pitch_extra=pitch_extra)


def _run_case(case, combos):
    c = R.REAL if case == "real" else R.CASES[case]
    want, bnd = R.reference(case)
    src = R.source(c)
    idx, crop, mid, out = R.plan(c)
    worst, k = 0.0, 0
    with guarded.active() as g:
        for layout, dtype in combos:
            for hf, vf in R.FLIPS:
                k += 1
                s = _source(src, layout, dtype, pitch_extra=1 + k % 5)
                x = ops.clip_xform(s, idx.tolist(), layout=layout, crop=crop, mid=mid, out_hw=out, hflip=hf, vflip=vf)
                got = ops.video_clip_transform(s, None, x)
                assert got.shape == (c["nf"], 3) + tuple(out) and got.dtype == torch.float32
                r = R.worst_ratio(got.cpu(), R.flipped(want, hf, vf), R.flipped(bnd, hf, vf))
                print(f"{case} {layout} {str(dtype)[6:]} hflip={hf} vflip={vf}: worst |kernel - fp64| / bound = {r:.3f}")
                worst = max(worst, r)
                assert r <= 1.0, (case, layout, dtype, hf, vf, r)
        assert g.allocs
        g.verify()
    return worst


@pytest.mark.parametrize("case", list(R.CASES))
def test_every_case_stays_within_the_bound(gpu, case):
    _run_case(case, [(lay, dt) for lay in ("THWC", "CTHW") for dt in (torch.uint8, torch.float32)])


def test_real_frame_size_stays_within_the_bound(gpu):
    """720 x 1280 frames, nf = 2, short side 288 (mid 288 x 512), out 224 x 224: seven workgroups across, the uint8 decoder layout and
    pytorchvideo's f32 CTHW."""
    _run_case("real", [("THWC", torch.uint8), ("CTHW", torch.float32)])


def test_exact_cases_are_bit_equal_and_launches_repeat(gpu):
    """scale 1, shift 0, 8 x 8 -> 16 x 16 -> 32 x 32: every weight is dyadic and every sum exact in f32, so the kernel returns the fp64 chain's
    values bit for bit; a second launch into another buffer returns the same bits; the slab written lies between two that stay 0xFF."""
    E = R.EXACT
    with guarded.active() as g:
        for seed in range(2):
            src = R.exact_source(seed)
            for layout, dtype in [("THWC", torch.uint8), ("CTHW", torch.uint8), ("CTHW", torch.float32), ("THWC", torch.float32)]:
                for hf, vf in R.FLIPS:
                    s = _source(src, layout, dtype, pitch_extra=3)
                    x = ops.clip_xform(s, range(E["nf"]), layout=layout, mid=E["mid"], out_hw=E["out"], hflip=hf, vflip=vf, **RAW)
                    assert [x.scale[c] for c in range(3)] == [1.0] * 3 and [x.shift[c] for c in range(3)] == [0.0] * 3
                    batch = g.empty((3, E["nf"], 3) + E["out"], dtype=torch.float32, device="cuda")
                    ops.video_clip_transform(s, batch[1], x)
                    again = ops.video_clip_transform(s, None, x)
                    want = R.exact_reference(src, hf, vf)
                    assert torch.equal(batch[1].cpu().double(), want), (seed, layout, dtype, hf, vf)
                    assert torch.equal(batch[1].view(torch.int32), again.view(torch.int32))
                    assert bool(torch.isnan(batch[0]).all()) and bool(torch.isnan(batch[2]).all())
        g.verify()


def test_two_launches_give_identical_bits(gpu):
    c = R.CASES["crop"]
    src = torch.from_numpy(R.source(c)).cuda()
    idx, crop, mid, out = R.plan(c)
    x = ops.clip_xform(src, idx.tolist(), crop=crop, mid=mid, out_hw=out, hflip=True, vflip=True)
    a = ops.video_clip_transform(src, None, x)
    b = ops.video_clip_transform(src, None, x)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and not bool(torch.isnan(a).any())


def test_video_features_device_is_the_chain(gpu):
    """The public entry: host uint8 frames (selected and shipped once), device frames, and pytorchvideo's f32 CTHW give the same bits, within the
    bound of the fp64 chain under the draws the seed gives; the validation form resizes once and draws once."""
    T, H, W, size, nf = 11, 368, 720, 64, 4
    frames = torch.from_numpy(np.random.default_rng(3).integers(0, 256, (T, H, W, 3), dtype=np.uint8))
    for speaker, check in [(None, "train"), (True, "train"), (False, "val"), (None, "val")]:
        torch.manual_seed(11)
        aug = M.draw_clip_augmentation(speaker, check)
        after = torch.get_rng_state()
        outs = []
        for f in (frames, frames.cuda(), frames.permute(3, 0, 1, 2).float().cuda()):
            torch.manual_seed(11)
            outs.append(M.video_features_device(f, speaker, check, num_frames=nf, size=size))
            assert torch.equal(torch.get_rng_state(), after)
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]) and outs[0].shape == (nf, 3, size, size)
        crop = (0, 0, H, W) if speaker is None else M.SPEAKER_CROPS[bool(speaker)]
        mid = None if check != "train" else R.short_side(crop[2], crop[3], aug["size"])
        idx = R.subsample(T, nf)
        want = R.chain64(frames.numpy(), idx, crop, mid, (size, size), aug["hflip"], aug["vflip"])
        bnd = R.bound(R.chain64(frames.numpy(), idx, crop, mid, (size, size), aug["hflip"], aug["vflip"], normalise=False))
        r = R.worst_ratio(outs[0].cpu(), want, bnd)
        print(f"speaker={speaker} {check} {aug}: worst |kernel - fp64| / bound = {r:.3f}")
        assert r <= 1.0


def _float_collate_as_before(batch, n_true):
    """collate_batch_device's float path as it stood before decoded items existed, restated: every tensor shipped once, clips stacked."""
    dev = torch.device("cuda")
    speech = [torch.as_tensor(i[1]).float().reshape(-1) for (i, _) in batch]
    lens = torch.tensor([len(s) for s in speech])
    audio = torch.nn.utils.rnn.pad_sequence([s.to(dev) for s in speech], batch_first=True)
    amask = (torch.arange(int(lens.max()), device=dev)[None, :] < lens.to(dev)[:, None]).float()
    video = torch.stack([i[2].float().to(dev) for (i, _) in batch])
    ntok = (video.shape[1] // 2) * (video.shape[3] // 16) * (video.shape[4] // 16)
    mask = M.sample_video_mask(len(batch), ntok, n_true, dev, None)
    ids = torch.stack([i[0]["input_ids"].reshape(-1) for (i, _) in batch]).long().to(dev)
    tmask = torch.stack([i[0]["attention_mask"].reshape(-1).float() for (i, _) in batch]).to(dev)
    return ids, tmask, audio, amask, video, mask, torch.tensor([float(lab) for (_, lab) in batch]).to(dev)


def test_collate_batch_device_fills_the_slabs(gpu):
    """Three decoded items (no speaker, left, right): each slab of visual_embeds equals video_features_device on that item alone, bit for bit,
    under the same seed; text, audio, mask and labels equal those of the call on float items; float items give what they always gave."""
    cfg = cfgmod.preset("B-tiny")
    size, nf = 64, 16
    items = synthetic.make_items(cfg, 3, raw_video=(21, 368, 720), seed=5, s_text=8, t_audio=2000, speakers=[None, True, False])
    torch.manual_seed(7)
    (t, a, v), lab = M.collate_batch_device(items, "train", n_visual_true=4, size=size, num_frames=nf)
    assert v["visual_embeds"].shape == (3, nf, 3, size, size) and v["visual_embeds"].dtype == torch.float32 and v["visual_embeds"].is_contiguous()
    torch.manual_seed(7)
    alone = [M.video_features_device(i[2]["frames"], i[2]["speaker"], "train", num_frames=nf, size=size) for (i, _) in items]
    for b in range(3):
        assert torch.equal(v["visual_embeds"][b].view(torch.int32), alone[b].view(torch.int32)), b
    assert not bool(torch.isnan(v["visual_embeds"]).any())
    assert not torch.equal(alone[1], alone[2])                                                  # the two speakers' crops differ
    floats = [([i[0], i[1], alone[b].cpu()], lab_) for b, (i, lab_) in enumerate(items)]
    torch.manual_seed(7)
    (t2, a2, v2), lab2 = M.collate_batch_device(floats, "train", n_visual_true=4)
    torch.manual_seed(7)
    ids, tmask, audio, amask, video, mask, labels = _float_collate_as_before(floats, 4)
    for got in ((t, a, v, lab), (t2, a2, v2, lab2)):
        gt, ga, gv, gl = got
        assert torch.equal(gt["input_ids"], ids) and torch.equal(gt["attention_mask"], tmask)
        assert torch.equal(ga["audio_features"], audio) and torch.equal(ga["attention_mask"], amask)
        assert torch.equal(gl, labels) and gv["attention_mask"].shape == mask.shape and gv["attention_mask"].sum(1).tolist() == [4, 4, 4]
    assert torch.equal(v2["visual_embeds"], video) and torch.equal(v2["attention_mask"], mask)
    # the decoded call drew its clips from the CPU generator only: the device-side mask draw is the float call's
    assert torch.equal(v["attention_mask"], v2["attention_mask"])
    # validation: one resize, no flips, one draw per speaker-less item
    torch.manual_seed(9)
    (_, _, vv), _ = M.collate_batch_device(items, "val", n_visual_true=4, size=size, num_frames=nf)
    torch.manual_seed(9)
    for b, (i, _) in enumerate(items):
        assert torch.equal(vv["visual_embeds"][b], M.video_features_device(i[2]["frames"], i[2]["speaker"], "val", num_frames=nf, size=size)), b
