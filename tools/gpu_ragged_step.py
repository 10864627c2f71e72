"""Step time of ragged visual rows against equal rows: preset B, global batch 32, eager, bf16.

  equal : every row keeps 104 True video tokens (the reference's mean), runtime.set_visual_rows("equal")
  ragged: seeded reference-distribution masks (True w.p. 1/15 per token, models/tav.py:207-209 of the reference), set_visual_rows("ragged")

Both run the same step (forward + backward + clip + AdamW, check="val") on one GPU; prints one JSON line with ms per step for each.
usage: python tools/gpu_ragged_step.py [--steps 20] [--warmup 5] [--out FILE]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import tav_amd  # noqa: E402,F401
from tav_amd import config as C  # noqa: E402
from tav_amd import runtime, synthetic  # noqa: E402
from tav_amd.models.tav import PreFormer, TAVForMAE  # noqa: E402
from tav_amd.train_model.tav_train import TrainStep  # noqa: E402
from tav_amd.utils.global_functions import CrossEntropyLoss  # noqa: E402


def timed(stepper, inp, labels, n_true, steps, warmup):
    for _ in range(warmup):
        stepper.forward_backward(inp, labels, check="val", epoch=0, n_visual_true=n_true)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        stepper.forward_backward(inp, labels, check="val", epoch=0, n_visual_true=n_true)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    runtime.set_precision("bf16")
    cfg = C.preset("B")
    torch.manual_seed(0)
    pre, model = PreFormer(cfg).cuda(), TAVForMAE(dict(output_dim=7, dropout=0.5, learn_PosEmbeddings=True, num_layers=12), cfg).cuda()
    stepper = TrainStep(model, pre, CrossEntropyLoss(), lr=1e-6, weight_decay=1e-4, clip=1.0)
    inp, labels = synthetic.make_batch(cfg, a.batch, seed=1234, device="cuda")
    ntok = inp[2]["attention_mask"].shape[1]
    g = torch.Generator().manual_seed(1234)
    ragged = torch.randint(-13, 2, (a.batch, ntok), generator=g) > 0            # True w.p. 1/15 per token
    counts = ragged.sum(1).tolist()
    inp_r = [inp[0], inp[1], {"visual_embeds": inp[2]["visual_embeds"], "attention_mask": ragged.cuda()}]
    res = {}
    for mode, batch, n_true in (("equal", inp, 104), ("ragged", inp_r, counts), ("equal", inp, 104), ("ragged", inp_r, counts)):
        runtime.set_visual_rows(mode)
        res.setdefault(mode, []).append(timed(stepper, batch, labels, n_true, a.steps, a.warmup))
    runtime.set_visual_rows("equal")
    line = {"preset": "B", "batch": a.batch, "dtype": "bf16", "steps": a.steps, "warmup": a.warmup,
            "equal_ms_per_step": res["equal"], "ragged_ms_per_step": res["ragged"],
            "ragged_counts": {"min": min(counts), "max": max(counts), "mean": sum(counts) / len(counts)},
            "overhead_pct": 100.0 * (min(res["ragged"]) / min(res["equal"]) - 1.0)}
    print(json.dumps(line))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(line, indent=1) + "\n")


if __name__ == "__main__":
    main()
