"""Measures the audio-only baseline on the GPU and writes profiles/audio_only.txt (a record, not a gate).

    python tools/gpu_audio_only_speed.py [--out profiles/audio_only.txt] [--batch 8]

At full preset-B depth (wav2vec2-base: 12 layers, 768 wide), bf16 policy, B = 8 seeded utterances of 3 to 8 s zero-padded to the longest of
their batch: the whole training step of Wav2Vec2ForSpeechClassification (forward, class-weighted cross entropy, backward, FusedAdamW, a
read of the loss, as train_model/audio_training.py runs it) in milliseconds and utterances per second; for scale, the same step of the
Hugging Face Wav2Vec2Model plus the same head in eager torch on the same GPU (bf16 autocast over f32 parameters, sdpa attention,
torch.optim.AdamW(fused=True); SpecAugment, dropouts inside the encoder and layerdrop off, as in this package's encoder); and the error
figures tests/test_audio_classifier_gpu.py prints.

Timing: four different batches in rotation (their padded lengths differ); every batch runs once as warm-up; then 5 blocks of 4 steps, one
per batch, under the host clock with a device synchronisation at both ends of a block; the record gives the median block [min .. max].

Every part runs in a child process of its own under its own time limit; the first part that fails, faults or runs out of time ends the
run, and the record says which."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

O, SECONDS, NBATCH = 7, (3.0, 8.0), 4
LIMITS = {"step": 300, "torch": 300, "errors": 300}


def _batches(B):
    import torch
    out = []
    for i in range(NBATCH):
        g = torch.Generator().manual_seed(100 + i)
        lens = [int((SECONDS[0] + (SECONDS[1] - SECONDS[0]) * float(torch.rand(1, generator=g))) * 16000) for _ in range(B)]
        wave = torch.zeros(B, max(lens))
        for b, L in enumerate(lens):
            wave[b, :L] = torch.randn(L, generator=g) * 0.1
        out.append((wave.cuda(), torch.randint(0, O, (B,), generator=g).cuda(), lens))
    return out


def _time(one, batches):
    import torch
    first = [one(w, lab) for (w, lab, _) in batches]
    torch.cuda.synchronize()
    ms = []
    for _ in range(5):
        t0 = time.perf_counter()
        for (w, lab, _) in batches:
            last = one(w, lab)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) / len(batches) * 1e3)
    return first[0], last, (statistics.median(ms), min(ms), max(ms))


def _report(name, B, batches, first, last, t):
    import torch
    secs = sum(sum(lens) for (_, _, lens) in batches) / 16000 / len(batches)
    print(f"  {name}: first loss {first:.5f}, last {last:.5f} (finite {first == first and last == last}); training step {t[0]:.1f} ms "
          f"[{t[1]:.1f} .. {t[2]:.1f}] = {B / t[0] * 1e3:.0f} utterances/s, {secs / t[0] * 1e3:.0f} s of audio per second; "
          f"peak memory {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")


def step_step(B):
    import torch

    import tav_amd  # noqa: F401
    from tav_amd import runtime
    from tav_amd.optim import FusedAdamW
    from tav_amd.SingleModels.models.audio import Wav2Vec2ForSpeechClassification
    from tav_amd.utils.global_functions import CrossEntropyLoss
    runtime.set_precision("bf16")
    torch.manual_seed(0)
    model = Wav2Vec2ForSpeechClassification({"output_dim": O}).cuda()          # config=None: preset B's audio block, training mode (dropout on)
    opt = FusedAdamW([p for p in model.parameters() if p.requires_grad], lr=1e-6, weight_decay=1e-4)
    crit = CrossEntropyLoss(weight=torch.linspace(0.6, 0.95, O).cuda())

    def one(wave, lab):
        loss = crit(model(wave), lab)
        opt.zero_grad()
        loss.backward()
        opt.step()
        return loss.item()
    batches = _batches(B)
    _report("this package, bf16 policy", B, batches, *_time(one, batches))


def step_torch(B):
    import torch
    from transformers import Wav2Vec2Config, Wav2Vec2Model
    torch.manual_seed(0)
    cfg = Wav2Vec2Config(apply_spec_augment=False, hidden_dropout=0.0, attention_dropout=0.0, activation_dropout=0.0, feat_proj_dropout=0.0,
                         layerdrop=0.0, attn_implementation="sdpa")            # the defaults are wav2vec2-base's geometry
    enc, head, drop = Wav2Vec2Model(cfg).cuda().train(), torch.nn.Linear(cfg.hidden_size, O).cuda(), torch.nn.Dropout(.5)
    params = [p for p in list(enc.parameters()) + list(head.parameters()) if p.requires_grad]
    opt = torch.optim.AdamW(params, lr=1e-6, weight_decay=1e-4, fused=True)
    weight = torch.linspace(0.6, 0.95, O).cuda()

    def one(wave, lab):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            logits = head(drop(torch.mean(enc(wave)[0], dim=1)))
        loss = torch.nn.functional.cross_entropy(logits.float(), lab, weight=weight)
        opt.zero_grad()
        loss.backward()
        opt.step()
        return loss.item()
    batches = _batches(B)
    _report("transformers Wav2Vec2Model + head, eager torch, bf16 autocast", B, batches, *_time(one, batches))


def step_errors():
    run = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_audio_classifier_gpu.py"), "-m", "gpu", "-q", "-s",
                          "-k", "golden or gradient or bf16"], capture_output=True, text=True, cwd=ROOT)
    keep = [ln for ln in run.stdout.splitlines() if " vs " in ln or " passed" in ln or " failed" in ln]
    print("\n".join("  " + ln.lstrip(".") for ln in keep))
    if run.returncode not in (0, 1):
        sys.exit(run.returncode)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "audio_only.txt"))
    ap.add_argument("--batch", default=8, type=int)
    ap.add_argument("--step", default=None, help="(internal) run one part in this process")
    args = ap.parse_args()
    if args.step:
        {"step": lambda: step_step(args.batch), "torch": lambda: step_torch(args.batch), "errors": step_errors}[args.step]()
        return
    import torch
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is no host form"
    lines = [f"Audio-only baseline on {torch.cuda.get_device_name(0)} (tools/gpu_audio_only_speed.py)", "",
             f"geometry: wav2vec2-base (preset B's audio block, 12 layers), mean over frames, dropout 0.5, Linear(768, {O}); B {args.batch}, "
             f"utterances of {SECONDS[0]:g} to {SECONDS[1]:g} s at 16 kHz, zero-padded to the longest of their batch",
             f"timing: {NBATCH} batches in rotation, each once as warm-up, then 5 blocks of {NBATCH} steps under the host clock (device synchronised at "
             "both ends), every step ending in a read of the loss; median block [min .. max]", ""]
    plan = [("step", "whole training step (forward, weighted cross entropy, backward, AdamW)"), ("torch", None),
            ("errors", "errors (tests/test_audio_classifier_gpu.py; gates 1e-3 fp32, 1e-2 bf16)")]
    for step, title in plan:
        if title:
            lines += [title + ":"]
        try:
            run = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step, "--batch", str(args.batch)], capture_output=True, text=True,
                                 timeout=LIMITS[step], cwd=ROOT)
        except subprocess.TimeoutExpired:
            lines += [f"  {step}: NOT MEASURED: ran past its limit of {LIMITS[step]} s; nothing after it was run"]
            break
        lines += [ln for ln in run.stdout.splitlines() if ln.strip()]
        if run.returncode != 0:
            lines += [f"  {step}: FAILED with exit status {run.returncode}; nothing after it was run", *("    " + ln for ln in run.stderr.splitlines()[-6:])]
            break
        if step == "torch":
            lines += [""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
