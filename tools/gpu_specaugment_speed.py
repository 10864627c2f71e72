"""Cost of the SpecAugment sampler in the training loop: runtime.set_specaugment("torch") against "device", eager loop and graph loop, at
bench.py's preset and input shapes with check="train" (the step of tools/gpu_train_loop_speed.py).  All four configurations live in ONE process
and are timed in alternating blocks, `--rounds` times each, so that a drift of the machine hits them alike; the spread between the blocks of one
configuration is printed next to its mean -- a difference between two configurations below that spread is not a difference.

  python tools/gpu_specaugment_speed.py --global-batch 8 32 --steps 20 --rounds 3 --out profiles/specaugment_kernel.txt
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--global-batch", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--steps", type=int, default=20, help="steps per timed block")
    ap.add_argument("--rounds", type=int, default=3, help="timed blocks per configuration")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--preset", default="B")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()

    import torch
    import tav_amd  # noqa: F401
    from tav_amd import config as C
    from tav_amd import runtime, synthetic
    from tav_amd.models.tav import PreFormer, TAVForMAE
    from tav_amd.train_model import tav_train as T
    from tav_amd.train_model.graphed import GraphedSteps
    from tav_amd.utils.global_functions import CrossEntropyLoss, Metrics

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    work = torch.cuda.Stream()
    torch.cuda.set_stream(work)
    cfg = C.preset(args.preset)
    runtime.set_precision(args.dtype)
    lines = [f"# SpecAugment sampler in the training loop: preset {args.preset}, {args.dtype}, check=\"train\", mask_time_prob "
             f"{cfg['audio'].get('mask_time_prob', 0.05)}, {args.steps} steps per block, {args.rounds} blocks per configuration, alternating, one process",
             "# ms per step: mean over the blocks; spread = slowest block - fastest block of that configuration",
             f"{'batch':>5} {'loop':>6} {'sampler':>8} {'ms/step':>9} {'spread':>8} {'utt/s':>8}  blocks"]
    results = []

    class Run:
        def __init__(self, b, loop, mode, batches):
            self.b, self.loop, self.mode, self.batches, self.i, self.ms = b, loop, mode, batches, 0, []
            torch.manual_seed(0)
            self.pre, self.model = PreFormer(cfg), TAVForMAE(dict(output_dim=7, dropout=0.5, learn_PosEmbeddings=True, num_layers=12), cfg)
            synthetic.seeded_init_(self.pre, 1)
            synthetic.seeded_init_(self.model, 2)
            self.pre.to(dev)
            self.model.to(dev)
            self.crit, self.metric = CrossEntropyLoss(), Metrics(7)
            self.stepper = T.TrainStep(self.model, self.pre, self.crit, lr=1e-6, weight_decay=1e-4, clip=1.0)
            self.graphs = GraphedSteps(self.stepper) if loop == "graph" else None

        def step(self):
            inp, lab = self.batches[self.i % len(self.batches)]
            self.i += 1
            if self.graphs is not None:
                return self.graphs.step(inp, lab, 0, self.metric)
            loss = T.get_statistics(inp, lab, self.model, self.pre, self.crit, self.metric, check="train", epoch=0)
            v = loss.item()
            loss.backward()
            self.stepper.update()
            return v

        def block(self, n, timed):
            runtime.set_specaugment(self.mode)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            vs = [self.step() for _ in range(n)]
            torch.cuda.synchronize()
            if timed:
                self.ms.append((time.perf_counter() - t0) / n * 1e3)
            if not all(v == v and abs(v) != float("inf") for v in vs):
                raise RuntimeError(f"non-finite loss in {self.loop}/{self.mode} at batch {self.b}")

    try:
        for b in args.global_batch:
            batches = [synthetic.make_batch(cfg, b, seed=1234 + i, device=dev) for i in range(2)]
            runs = [Run(b, loop, mode, batches) for loop in ("eager", "graph") for mode in ("torch", "device")]
            for r in runs:
                r.block(args.warmup, False)
            for _ in range(args.rounds):
                for r in runs:
                    r.block(args.steps, True)
            for r in runs:
                mean = sum(r.ms) / len(r.ms)
                results.append(dict(batch=b, loop=r.loop, sampler=r.mode, ms_per_step=round(mean, 3), spread_ms=round(max(r.ms) - min(r.ms), 3),
                                    blocks_ms=[round(v, 3) for v in r.ms], replays=r.graphs.replays if r.graphs else 0))
                lines.append(f"{b:>5} {r.loop:>6} {r.mode:>8} {mean:>9.3f} {max(r.ms) - min(r.ms):>8.3f} {b / mean * 1e3:>8.1f}  "
                             + " ".join(f"{v:.3f}" for v in r.ms))
                if r.graphs is not None:
                    r.graphs.invalidate()
            del runs, batches
            torch.cuda.empty_cache()
    finally:
        runtime.set_specaugment("torch")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    print(json.dumps({"tool": "gpu_specaugment_speed", "results": results}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
