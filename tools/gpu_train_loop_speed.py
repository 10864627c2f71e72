"""Speed of the TRAINING LOOP's step machinery (train_model/tav_train.py not_grad_accum body: get_statistics with Metric, loss.item(), backward,
clip + AdamW, scheduler step), eager against graph mode (train_model/graphed.GraphedSteps), at bench.py's preset and input shapes with
check="train" (head dropout and SpecAugment on).  Batches are synthetic and resident on the device, cycled, so the loop -- not host-side data
generation -- is what is timed.  One mode per process (a graph pool next to an eager run's caches would distort the memory picture).

  python tools/gpu_train_loop_speed.py --global-batch 32 --mode graph --steps 30 --warmup 3 [--sync log]
prints one JSON line: ms per step and utterances per second over the timed steps.
--sync step (default): the loop reads the loss (and, through the host Metrics, predictions and labels) after every step, as the reference.
--sync log: train_tav_network(sync="log")'s step -- an on-device Metrics and one ops.step_stats launch per step; the accumulator is read once,
after the timed window, and last_loss / finite come from that read (no single step's loss is read in this mode: last_loss is the MEAN loss
of the timed steps, loss_sum their sum); a non-zero nonfinite count fails the run.
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
    ap.add_argument("--global-batch", type=int, default=32)
    ap.add_argument("--mode", choices=["eager", "graph"], required=True)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--preset", default="B")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--cycle", type=int, default=2, help="distinct device-resident batches, used in turn")
    ap.add_argument("--sync", default="step", choices=["step", "log"], help="per-step host reads (step) or device accumulator read once (log)")
    ap.add_argument("--specaugment", default="torch", choices=["torch", "device", "reference"], help="runtime.set_specaugment")
    args = ap.parse_args()

    import torch
    import tav_amd  # noqa: F401
    from tav_amd import config as C
    from tav_amd import ops, runtime, synthetic
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
    runtime.set_specaugment(args.specaugment)
    torch.manual_seed(0)
    pre, model = PreFormer(cfg), TAVForMAE(dict(output_dim=7, dropout=0.5, learn_PosEmbeddings=True, num_layers=12), cfg)
    synthetic.seeded_init_(pre, 1)
    synthetic.seeded_init_(model, 2)
    pre.to(dev)
    model.to(dev)
    b = args.global_batch
    batches = [synthetic.make_batch(cfg, b, seed=1234 + i, device=dev) for i in range(args.cycle)]      # bench.py's input shapes
    log_sync = args.sync == "log"
    crit, metric = CrossEntropyLoss(), Metrics(7, rank=dev, on_device=log_sync)
    sync = T.LogSync(metric, dev) if log_sync else None
    stepper = T.TrainStep(model, pre, crit, lr=1e-6, weight_decay=1e-4, clip=1.0)
    sched = T.CosineWarmRestarts(stepper.opt, T_0=2)
    n = args.warmup + args.steps
    graphs = GraphedSteps(stepper) if args.mode == "graph" else None

    def step(i):
        inp, lab = batches[i % len(batches)]
        if sync is not None:
            if graphs is not None:
                v = graphs.step(inp, lab, 0, metric, sync=sync)
            else:
                loss = T.recorded_loss(sync.train, inp, lab, model, pre, crit, metric, check="train", epoch=0)
                loss.backward()
                stepper.update()
                v = None
        elif graphs is not None:
            v = graphs.step(inp, lab, 0, metric)
        else:
            loss = T.get_statistics(inp, lab, model, pre, crit, metric, check="train", epoch=0)
            v = loss.item()
            loss.backward()
            stepper.update()
        sched.step(i / n)
        return v

    for i in range(args.warmup):
        step(i)
    if sync is not None:
        ops.loop_acc_reset(sync.train)           # (a fill: the timed window starts from an empty accumulator)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    losses = [step(args.warmup + i) for i in range(args.steps)]
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    ms = el / args.steps * 1e3
    extra = {}
    if sync is not None:
        r = T.LogSync.read(sync.train, "timed")                  # the one read, after the window
        assert r["steps"] == args.steps and r["rows"] == args.steps * b, r
        losses = [r["loss_sum"] / r["steps"]]
        extra = {"nonfinite": r["nonfinite"], "bad_rows": r["bad_rows"], "loss_sum": r["loss_sum"], "cm_total": int(metric.cm.sum().item())}
    out = {"tool": "gpu_train_loop_speed", "mode": args.mode, "preset": args.preset, "dtype": args.dtype, "global_batch": b, "check": "train",
           "specaugment": args.specaugment, "sync": args.sync,
           "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms, 3), "utt_per_s": round(b / (el / args.steps), 2),
           "last_loss": round(losses[-1], 5), "finite": all(v == v and abs(v) != float("inf") for v in losses),
           "peak_mem_gib": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}
    if graphs is not None:
        out.update(eager_steps=graphs.eager_steps, captures=graphs.captures, replays=graphs.replays)
        graphs.invalidate()
    out.update(extra)
    print(json.dumps(out), flush=True)
    if extra.get("nonfinite"):
        sys.exit(f"{extra['nonfinite']} of {args.steps} timed steps had a non-finite loss")


if __name__ == "__main__":
    main()
