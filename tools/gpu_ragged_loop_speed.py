"""Speed of the TRAINING LOOP's step on ragged video rows, eager against graph mode at a bucketed capacity, in the manner of
tools/gpu_train_loop_speed.py: preset B, bf16, check="train" (head dropout and SpecAugment on), bench.py's input shapes, the not_grad_accum
body (get_statistics with Metrics, loss.item(), backward, clip + AdamW, scheduler step).  The video masks come from
collate_batch(visual_rows="ragged") -- the reference's draw, True w.p. 1/15 per token -- a FRESH mask, hence fresh per-row counts, for every
step; the other tensors of the batch are device-resident and reused, so the loop, not host-side data generation, is what is timed.

Three loops per batch size, one after the other in one process:
  (i)   ragged, eager, bucket off          the loop ragged rows ran before graphs could take them: the baseline
  (ii)  ragged, graph mode, bucket 64      runtime.set_visual_rows("ragged", bucket=64) + GraphedSteps
  (iii) equal rows (104 per row), graph    the ceiling: no padded rows
Every step ends in loss.item(), so each step is timed on its own; a step that captured a graph is listed but kept out of the steady-state
mean (there are at most `max_graphs` of them per epoch).

  python tools/gpu_ragged_loop_speed.py [--batches 8 32] [--steps 30] [--warmup 3] [--bucket 64] [--out FILE]
prints one JSON line per loop and, with --out, writes the table."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bucket", type=int, default=64)
    ap.add_argument("--preset", default="B")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import tav_amd  # noqa: F401
    from tav_amd import config as C
    from tav_amd import runtime, synthetic
    from tav_amd.models.tav import PreFormer, TAVForMAE, collate_batch
    from tav_amd.train_model import tav_train as T
    from tav_amd.train_model.graphed import GraphedSteps
    from tav_amd.utils.global_functions import CrossEntropyLoss, Metrics

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    work = torch.cuda.Stream()
    torch.cuda.set_stream(work)
    cfg = C.preset(args.preset)
    runtime.set_precision("bf16")
    n = args.warmup + args.steps
    vc = cfg["video"]
    lines = []

    def reference_masks(b, count, seed):
        """`count` masks [b, ntok] as collate_batch(visual_rows="ragged") draws them (the items carry a clip of the preset's shape, nothing else)."""
        clip = torch.zeros(vc["frames"], 3, vc["image"], vc["image"])
        items = [([{"input_ids": torch.zeros(4, dtype=torch.int64), "attention_mask": torch.ones(4)}, torch.zeros(16), clip], 0) for _ in range(b)]
        torch.manual_seed(seed)
        return [collate_batch(items, "train", visual_rows="ragged")[0][2]["attention_mask"] for _ in range(count)]

    for b in args.batches:
        masks = reference_masks(b, n, 4321 + b)
        counts = [m.sum(1).tolist() for m in masks]
        for name, mode, bucket, graph in (("ragged eager, bucket off", "ragged", None, False), (f"ragged graph, bucket {args.bucket}", "ragged", args.bucket, True),
                                          ("equal rows graph", "equal", None, True)):
            runtime.set_visual_rows(mode, bucket=bucket)
            torch.manual_seed(0)
            pre, model = PreFormer(cfg), TAVForMAE(dict(output_dim=7, dropout=0.5, learn_PosEmbeddings=True, num_layers=12), cfg)
            pre.check_shapes = 2
            synthetic.seeded_init_(pre, 1)
            synthetic.seeded_init_(model, 2)
            pre.to(dev)
            model.to(dev)
            base = [synthetic.make_batch(cfg, b, seed=1234 + i, device=dev) for i in range(2)]      # bench.py's input shapes, equal rows (104)
            if mode == "ragged":
                batches = [([base[i % 2][0][0], base[i % 2][0][1], {"visual_embeds": base[i % 2][0][2]["visual_embeds"], "attention_mask": masks[i].to(dev)}],
                            base[i % 2][1]) for i in range(n)]
            else:
                batches = [base[i % 2] for i in range(n)]
            crit, metric = CrossEntropyLoss(), Metrics(7)
            stepper = T.TrainStep(model, pre, crit, lr=1e-6, weight_decay=1e-4, clip=1.0)
            sched = T.CosineWarmRestarts(stepper.opt, T_0=2)
            graphs = GraphedSteps(stepper) if graph else None
            caps_seen = {}

            def step(i):
                inp, lab = batches[i]
                if graphs is not None:
                    v = graphs.step(inp, lab, 0, metric)
                else:
                    loss = T.get_statistics(inp, lab, model, pre, crit, metric, check="train", epoch=0)
                    v = loss.item()
                    T.check_visual_rows(model)
                    loss.backward()
                    stepper.update()
                sched.step(i / n)
                return v

            torch.cuda.synchronize()
            times, captured, losses = [], [], []
            for i in range(n):
                c0 = graphs.captures if graphs is not None else 0
                t0 = time.perf_counter()
                losses.append(step(i))
                times.append((time.perf_counter() - t0) * 1e3)
                captured.append(graphs is not None and graphs.captures != c0)
                if bucket:
                    caps = runtime.visual_capacities(counts[i], masks[i].shape[1], bucket)
                    caps_seen[str(caps)] = caps_seen.get(str(caps), 0) + 1
            torch.cuda.synchronize()
            timed = [(t, c) for t, c in list(zip(times, captured))[args.warmup:]]
            steady = [t for t, c in timed if not c]
            out = {"tool": "gpu_ragged_loop_speed", "loop": name, "preset": args.preset, "dtype": "bf16", "global_batch": b, "check": "train",
                   "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(sum(steady) / len(steady), 3),
                   "ms_per_step_with_captures": round(sum(t for t, _ in timed) / len(timed), 3), "capture_steps_in_timed": sum(c for _, c in timed),
                   "utt_per_s": round(b / (sum(steady) / len(steady)) * 1e3, 2), "last_loss": round(losses[-1], 5),
                   "finite": all(v == v and abs(v) != float("inf") for v in losses), "peak_mem_gib": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}
            if mode == "ragged":
                flat = [c for row in counts for c in row]
                out["true_tokens_per_row"] = {"min": min(flat), "max": max(flat), "mean": round(sum(flat) / len(flat), 1)}
            if graphs is not None:
                out.update(eager_steps=graphs.eager_steps, captures=graphs.captures, replays=graphs.replays)
                graphs.invalidate()
            if bucket:
                out["capacities_seen"] = caps_seen
            print(json.dumps(out), flush=True)
            lines.append(out)
            del graphs, stepper, sched, batches, base, pre, model
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
    runtime.set_visual_rows("equal")
    if args.out:
        with open(args.out, "w") as f:
            f.write(f"{'b':>3}  {'loop':<28} {'ms/step':>9} {'utt/s':>8}  replays/captures/eager  capacities\n")
            for o in lines:
                f.write(f"{o['global_batch']:>3}  {o['loop']:<28} {o['ms_per_step']:>9.2f} {o['utt_per_s']:>8.1f}  "
                        f"{o.get('replays', '-')}/{o.get('captures', '-')}/{o.get('eager_steps', '-')}  {o.get('capacities_seen', '')}\n")
            f.write("\nRaw lines:\n" + "\n".join(json.dumps(o) for o in lines) + "\n")


if __name__ == "__main__":
    main()
