"""Decoded PCM to the 16 kHz batch rows: what does the host chain cost against the training step, and what does the device path cost?  For one
10 s stereo int16 utterance at 44.1 kHz and one at 48 kHz:

  host chain    the reference's speech_file_to_array_fn after the decoder, restated in f32 torch as torchaudio runs it (int16 -> f32 / 32768,
                F.pad(width, width + o), conv1d with the FULL [n, 1, 2 width + o] table at stride o, transpose + reshape, cut to L_out, the
                mean over the channels), with 1 and with 16 threads: ms per utterance, host clock
  device path   models.tav.speech_features_device on host PCM: the copy into pinned memory, the copy to the device (int16: 2 bytes per
                sample) and the kernel, writing a row of the batch and a row of its mask -- per utterance (one, then a synchronise) and per
                batch of 32 (32 utterances into one [32, T] pair, one synchronise)
  kernel alone  tav_audio_resample on PCM already on the device, HIP events around a block of launches, against its byte floor: the PCM it
                reads plus the two rows it writes, at the 6.29 TB/s a float4 copy reaches

All configurations live in one process, are warmed, and are timed in alternating blocks, `--rounds` times each; the spread (slowest block -
fastest block) stands next to each mean, and a difference below it is not one.  The device path and the host chain must agree before
anything is timed.  Without a GPU this fails: nothing here is a CPU estimate.

  python tools/gpu_audio_transform_speed.py --out profiles/audio_transform.txt
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
AGREE = 1e-4                 # f32 sums of at most 475 products of values below 1: 475 * 2^-24 = 2.8e-5 at the very worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rates", type=int, nargs="+", default=[44100, 48000])
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3, help="timed blocks per configuration")
    ap.add_argument("--host-utts", type=int, default=48, help="utterances per timed block of the host chain")
    ap.add_argument("--device-utts", type=int, default=1024, help="utterances per timed block of the device path, one at a time")
    ap.add_argument("--batches", type=int, default=32, help="batches per timed block of the device path in batches")
    ap.add_argument("--kernel-launches", type=int, default=20000, help="launches per timed block of the kernel alone")
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
        raise SystemExit("gpu_audio_transform_speed measures on the GPU: none is visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)

    class Cfg:
        def __init__(self, name, unit, per):
            self.name, self.unit, self.per, self.ms = name, unit, per, []

        def stats(self):
            m = sum(self.ms) / len(self.ms)
            return m, max(self.ms) - min(self.ms)

    lines = [f"# training step (bench.py, preset B, global batch 32, bf16): {STEP_UTT_S:.0f} utterances/s"]
    results = []
    for sr in args.rates:
        L = int(round(sr * args.seconds))
        rng = np.random.default_rng(sr)
        utts = [torch.from_numpy(rng.integers(-32768, 32768, (L, args.channels), dtype=np.int16)) for _ in range(2)]
        full, o, n, width = ops.sinc_resample_coefficients(sr)
        kernel = torch.from_numpy(full)[:, None, :]                       # [n, 1, 2 width + o], as torchaudio keeps it
        L_out = ops.resampled_length(L, sr)
        table = ops.audio_resample_table(sr, device=dev)

        def host_chain(pcm_lc):
            """torchaudio.load's scaling, Resample.forward, .squeeze(), the mean -- f32 on the CPU."""
            x = pcm_lc.t().float() / 32768.0                               # [C, L]
            x = F.pad(x, (width, width + o))
            y = F.conv1d(x[:, None], kernel, stride=o)                     # [C, n, frames]
            y = y.transpose(1, 2).reshape(x.shape[0], -1)[..., :L_out]
            return torch.mean(y.squeeze(), dim=0)

        ref = host_chain(utts[0])
        got = M.speech_features_device(utts[0], sr).cpu()
        err = float((got - ref).abs().max())
        if got.shape != ref.shape or not err < AGREE:
            raise RuntimeError(f"device path and host chain disagree at {sr} Hz: shapes {tuple(got.shape)} / {tuple(ref.shape)}, max abs diff {err}")

        row1, mrow1 = torch.empty(L_out, device=dev), torch.empty(L_out, device=dev)
        batch, bmask = torch.empty(args.batch, L_out, device=dev), torch.empty(args.batch, L_out, device=dev)
        on_dev = utts[0].to(dev)

        def run_host(threads):
            def f():
                torch.set_num_threads(threads)
                t0 = time.perf_counter()
                for i in range(args.host_utts):
                    host_chain(utts[i % 2])
                return (time.perf_counter() - t0) / args.host_utts * 1e3
            return f

        def run_one():
            k = args.device_utts
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(k):
                M.speech_features_device(utts[i % 2], sr, out=row1, mask=mrow1)
                torch.cuda.synchronize()
            return (time.perf_counter() - t0) / k * 1e3

        def run_batch():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.batches):
                for b in range(args.batch):
                    M.speech_features_device(utts[b % 2], sr, out=batch[b], mask=bmask[b])
                torch.cuda.synchronize()
            return (time.perf_counter() - t0) / args.batches * 1e3

        def run_kernel():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.kernel_launches):
                ops.audio_resample(on_dev, table, out=row1, mask=mrow1)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / args.kernel_launches

        cfgs = [(Cfg(f"host chain, {t} thread{'s' if t > 1 else ''}", "ms/utt", 1), run_host(t)) for t in args.threads]
        cfgs += [(Cfg("device path, one utterance", "ms/utt", 1), run_one), (Cfg(f"device path, batch of {args.batch}", "ms/batch", args.batch), run_batch),
                 (Cfg("kernel alone", "ms/launch", 1), run_kernel)]
        for c, f in cfgs:                                                   # warm every shape the timed window uses (a full block each)
            f()
        for _ in range(args.rounds):
            for c, f in cfgs:
                c.ms.append(f())
        torch.set_num_threads(max(args.threads))
        pcm_bytes, out_bytes = L * args.channels * 2, 2 * L_out * 4
        floor_us = (pcm_bytes + out_bytes) / (COPY_TBS * 1e12) * 1e6
        lines += [f"# {sr} Hz -> 16000 Hz, {args.seconds:g} s, {args.channels} channels int16 [L, C], L = {L}, L_out = {L_out}; o / n = {o} / {n}, "
                  f"{full.shape[1]} taps per phase in the host chain, {table.ntap} in the kernel; {args.rounds} alternating blocks per line "
                  f"({args.host_utts} / {args.device_utts} utterances, {args.batches} batches, {args.kernel_launches} launches per block); device "
                  f"path and host chain agree to {err:.1e}",
                  f"# shipped per utterance: {pcm_bytes / 1e6:.2f} MB int16 (f32 would be {2 * pcm_bytes / 1e6:.2f} MB; the finished waveform is "
                  f"{L_out * 4 / 1e6:.2f} MB); at {STEP_UTT_S:.0f} utterances/s that is {pcm_bytes * STEP_UTT_S / 1e9:.2f} GB/s over the host link",
                  f"{'configuration':<28} {'mean':>10} {'spread':>9} {'unit':>9} {'utts/s':>9} {'of step':>8}  blocks"]
        for c, _ in cfgs:
            m, sp = c.stats()
            rate = c.per / m * 1e3
            lines.append(f"{c.name:<28} {m:>10.3f} {sp:>9.3f} {c.unit:>9} {rate:>9.1f} {rate / STEP_UTT_S:>7.2f}x  " + " ".join(f"{v:.3f}" for v in c.ms))
            results.append(dict(sr=sr, configuration=c.name, mean_ms=round(m, 4), spread_ms=round(sp, 4), unit=c.unit, utts_per_s=round(rate, 1),
                                blocks_ms=[round(v, 4) for v in c.ms]))
        k_us = cfgs[-1][0].stats()[0] * 1e3
        one_us = cfgs[-3][0].stats()[0] * 1e3
        per_us = cfgs[-2][0].stats()[0] * 1e3 / args.batch
        lines += [f"# kernel alone: {k_us:.1f} us per launch for {pcm_bytes / 1e6:.2f} MB read + {out_bytes / 1e6:.2f} MB written; byte floor at {COPY_TBS} TB/s = "
                  f"{floor_us:.2f} us ({floor_us / k_us * 100:.0f}% of it); {L_out * table.ntap * 2 / k_us / 1e6:.2f} TFLOP/s of fma work",
                  f"# per utterance in a batch: {per_us:.1f} us, of which the kernel is {k_us:.1f} us and {pcm_bytes / 1e6:.2f} MB at 50 GB/s would be "
                  f"{pcm_bytes / 50e9 * 1e6:.1f} us; one at a time: {one_us:.1f} us", ""]
        results.append(dict(sr=sr, kernel_us=round(k_us, 2), floor_us=round(floor_us, 2), pcm_bytes=pcm_bytes, out_bytes=out_bytes))
        del utts, batch, bmask, on_dev
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    print(json.dumps({"tool": "gpu_audio_transform_speed", "results": results}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
