"""Decoded frames to model input: can the host feed the training step, and what does the device path cost?  For T = 90 decoded uint8 frames
of 720 x 1280 and 480 x 720, check = "train" (subsample 16, normalise, short side 288, resize 224, both flips on):

  host chain    the reference's chain restated in f32 torch on the CPU (index_select, /255, normalise, F.interpolate twice, flip), with 1 and
                with 16 threads: ms per clip, host clock
  device path   models.tav.video_features_device on host frames: selecting 16 frames into pinned memory, the copy to the device and the
                kernel -- per clip (one clip, then a synchronise) and per batch of 32 (32 clips into one batch tensor, one synchronise)
  kernel alone  tav_video_clip_transform on frames already on the device, HIP events around a block of launches, against its byte floor:
                the 9.6 MB it writes plus the source bytes its taps touch, at the 6.29 TB/s a float4 copy reaches (8.0 TB/s is the spec)

All configurations live in one process, are warmed, and are timed in alternating blocks, `--rounds` times each; the spread (slowest block -
fastest block) stands next to each mean, and a difference below it is not one.  Without a GPU this fails: nothing here is a CPU estimate.

  python tools/gpu_video_transform_speed.py --out profiles/video_transform.txt
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEP_UTT_S = 425.0           # the training step (bench.py, preset B, global batch 32, bf16)
COPY_TBS = 6.29              # measured float4 copy rate of the part


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[720, 1280, 480, 720], help="H W pairs")
    ap.add_argument("--frames", type=int, default=90)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3, help="timed blocks per configuration")
    ap.add_argument("--host-clips", type=int, default=2, help="clips per timed block of the host chain")
    ap.add_argument("--kernel-launches", type=int, default=2000, help="launches per timed block of the kernel alone")
    ap.add_argument("--threads", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()

    import numpy as np
    import torch
    from torch.nn import functional as F

    import tav_amd  # noqa: F401
    from tav_amd import ops
    from tav_amd.models import tav as M

    if not torch.cuda.is_available():
        raise SystemExit("gpu_video_transform_speed measures on the GPU: none is visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    nf, size, short = 16, 224, 288
    mean = torch.tensor(ops.CLIP_MEAN)[:, None, None, None]
    std = torch.tensor(ops.CLIP_STD)[:, None, None, None]

    def host_chain(frames_thwc):
        """The reference's float chain on the CPU, f32 (what a user without the device path runs per clip)."""
        x = torch.index_select(frames_thwc, 0, M.subsample_indices(frames_thwc.shape[0], nf))
        x = x.permute(3, 0, 1, 2).float()                                 # only the 16 selected frames become f32 CTHW: the cheapest host order
        x = (x / 255.0 - mean) / std
        x = F.interpolate(x, size=M.short_side_size(x.shape[2], x.shape[3], short), mode="bilinear", align_corners=False)
        x = F.interpolate(x, size=(size, size), mode="bilinear", align_corners=False)
        return x.flip(-1).flip(-2).permute(1, 0, 2, 3).contiguous()

    class Cfg:
        def __init__(self, name, unit, per):
            self.name, self.unit, self.per, self.ms = name, unit, per, []

        def stats(self):
            m = sum(self.ms) / len(self.ms)
            return m, max(self.ms) - min(self.ms)

    lines, results = [], []
    sizes = list(zip(args.sizes[0::2], args.sizes[1::2]))
    for H, W in sizes:
        rng = np.random.default_rng(H)
        clips = [torch.from_numpy(rng.integers(0, 256, (args.frames, H, W, 3), dtype=np.uint8)) for _ in range(2)]
        aug = {"size": short, "hflip": True, "vflip": True}                   # given, not drawn: the same work in every block
        idx = M.subsample_indices(args.frames, nf)
        sel = clips[0].index_select(0, idx).to(dev)
        mid = M.short_side_size(H, W, short)
        x = ops.clip_xform(sel, range(nf), mid=mid, out_hw=(size, size), hflip=True, vflip=True)
        out1 = torch.empty(nf, 3, size, size, device=dev)
        batch = torch.empty(args.batch, nf, 3, size, size, device=dev)
        # the kernel and the host chain agree before anything is timed
        ref = host_chain(clips[0])
        got = M.video_features_device(clips[0], None, "train", augmentation=aug).cpu()
        err = float((got - ref).abs().max())
        if not err < 1e-3:
            raise RuntimeError(f"device path and host chain disagree at {H} x {W}: max abs diff {err}")

        def run_host(threads):
            def f():
                torch.set_num_threads(threads)
                t0 = time.perf_counter()
                for i in range(args.host_clips):
                    host_chain(clips[i % 2])
                return (time.perf_counter() - t0) / args.host_clips * 1e3
            return f

        def run_clip():
            n = 8
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(n):
                M.video_features_device(clips[i % 2], None, "train", out=out1, augmentation=aug)
                torch.cuda.synchronize()
            return (time.perf_counter() - t0) / n * 1e3

        def run_batch():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for b in range(args.batch):
                M.video_features_device(clips[b % 2], None, "train", out=batch[b], augmentation=aug)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        def run_kernel():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.kernel_launches):
                ops.video_clip_transform(sel, out1, x)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / args.kernel_launches

        cfgs = [(Cfg(f"host chain, {t} thread{'s' if t > 1 else ''}", "ms/clip", 1), run_host(t)) for t in args.threads]
        cfgs += [(Cfg("device path, one clip", "ms/clip", 1), run_clip), (Cfg(f"device path, batch of {args.batch}", "ms/batch", args.batch), run_batch),
                 (Cfg("kernel alone", "ms/launch", 1), run_kernel)]
        for c, f in cfgs:                                                    # warm every shape the timed window uses
            f()
        for _ in range(args.rounds):
            for c, f in cfgs:
                c.ms.append(f())
        torch.set_num_threads(max(args.threads))
        # bytes: what the kernel writes, and the source elements its taps touch (rows x columns of the integer coordinates, 3 channels)
        def touched(n_in, n_mid, n_out):
            o = np.arange(n_out)
            num = np.maximum((2 * o + 1) * n_mid - n_out, 0)
            j0 = num // (2 * n_out)
            j = np.unique(np.concatenate([j0, np.minimum(j0 + 1, n_mid - 1)]))
            num = np.maximum((2 * j + 1) * n_in - n_mid, 0)
            i0 = num // (2 * n_mid)
            return len(np.unique(np.concatenate([i0, np.minimum(i0 + 1, n_in - 1)])))
        rows, cols = touched(H, mid[0], size), touched(W, mid[1], size)
        src_bytes, dst_bytes = nf * rows * cols * 3, nf * 3 * size * size * 4
        floor_us = (src_bytes + dst_bytes) / (COPY_TBS * 1e12) * 1e6
        lines += [f"# {H} x {W} uint8 frames, T = {args.frames}: subsample {nf}, normalise, short side {short} -> {mid[0]} x {mid[1]}, resize {size} x {size}, "
                  f"both flips; {args.rounds} alternating blocks per line; device path and host chain agree to {err:.1e}",
                  f"# selected frames shipped per clip: {nf * H * W * 3 / 1e6:.1f} MB uint8 (the float clip is {dst_bytes / 1e6:.1f} MB); at {STEP_UTT_S:.0f} "
                  f"clips/s that is {nf * H * W * 3 * STEP_UTT_S / 1e9:.1f} GB/s over the host link against {dst_bytes * STEP_UTT_S / 1e9:.1f} GB/s",
                  f"{'configuration':<28} {'mean':>10} {'spread':>9} {'unit':>9} {'clips/s':>9} {'of step':>8}  blocks"]
        for c, _ in cfgs:
            m, sp = c.stats()
            rate = c.per / m * 1e3
            lines.append(f"{c.name:<28} {m:>10.3f} {sp:>9.3f} {c.unit:>9} {rate:>9.1f} {rate / STEP_UTT_S:>7.2f}x  " + " ".join(f"{v:.3f}" for v in c.ms))
            results.append(dict(H=H, W=W, configuration=c.name, mean_ms=round(m, 4), spread_ms=round(sp, 4), unit=c.unit, clips_per_s=round(rate, 1),
                                blocks_ms=[round(v, 4) for v in c.ms]))
        k_us = cfgs[-1][0].stats()[0] * 1e3
        lines += [f"# kernel alone: {k_us:.1f} us per launch; it writes {dst_bytes / 1e6:.2f} MB and its taps touch {rows} rows x {cols} columns of {nf} frames = "
                  f"{src_bytes / 1e6:.2f} MB of source; byte floor at {COPY_TBS} TB/s = {floor_us:.1f} us, so the kernel runs at {floor_us / k_us * 100:.0f}% of "
                  f"it ({(src_bytes + dst_bytes) / k_us / 1e6:.2f} TB/s of algorithmic bytes; HBM-bound, no FLOP bound applies; the launches of a block read one clip, which the Infinity Cache can hold)", ""]
        results.append(dict(H=H, W=W, kernel_us=round(k_us, 2), floor_us=round(floor_us, 2), src_bytes=src_bytes, dst_bytes=dst_bytes))
        del clips, sel, batch
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    print(json.dumps({"tool": "gpu_video_transform_speed", "results": results}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
