"""What do parameter groups cost the optimizer update?  On the parameter list of a preset (default B, the benchmarked trio) the two launches
FusedAdamW makes:

  one group     tav_adamw_chunked over the flat list, as TrainStep builds it by default
  four groups   tav_adamw_chunked_groups over optim.default_param_groups(encoder_lr_scale=0.1, no_decay_norm_bias=True): the same tensors in
                group order, {lr, weight_decay} per tensor through group_of and the device table
  one group, group order
                tav_adamw_chunked over the four groups' tensors in THEIR order: what of a difference between the first two lines is the
                order of the chunks (the groups put the ~750 no-decay vectors of the encoders last) and what is the kernel

Each optimizer takes one real step first (moments, pointer tables, chunk table, group table on the device); the timed launches are the C calls
alone on those tables, HIP events around a block of them, with the clip-coefficient pointer as in training.  The two are warmed and timed
in alternating blocks, `--rounds` times each; the spread (slowest block - fastest block) stands next to each mean, and a difference below it
is not one.  Bytes: four arrays read, three written, 4 bytes each.  Without a GPU this fails: nothing here is a CPU estimate.

  python tools/gpu_param_groups_speed.py --out profiles/param_groups.txt
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_TBS = 6.29              # measured float4 copy rate of the part


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="B")
    ap.add_argument("--rounds", type=int, default=5, help="timed blocks per launch")
    ap.add_argument("--launches", type=int, default=200, help="launches per timed block")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()

    import torch

    import tav_amd  # noqa: F401
    from tav_amd import config as C
    from tav_amd._lib import check, lib, ptr, stream
    from tav_amd.models.tav import PreFormer, TAVForMAE
    from tav_amd.optim import FusedAdamW, default_param_groups

    if not torch.cuda.is_available():
        raise SystemExit("gpu_param_groups_speed measures on the GPU: none is visible")
    torch.cuda.set_device(0)
    cfg = C.preset(args.preset)
    torch.manual_seed(0)
    pre = PreFormer(cfg).cuda()
    model = TAVForMAE(dict(output_dim=7, dropout=0.5, learn_PosEmbeddings=True, num_layers=12), cfg).cuda()
    lr, wd = 1e-6, 1e-4
    flat = default_param_groups(model, pre, lr, wd)
    groups = default_param_groups(model, pre, lr, wd, encoder_lr_scale=0.1, no_decay_norm_bias=True)
    for p in flat:
        p.grad = torch.randn_like(p) * 1e-3
    opts = {"one group": FusedAdamW(flat, lr=lr, weight_decay=wd), "four groups": FusedAdamW(groups, lr=lr, weight_decay=wd),
            "one group, group order": FusedAdamW([p for g in groups for p in g["params"]], lr=lr, weight_decay=wd)}
    for o in opts.values():
        o.clip_and_step(1.0)                     # a real step: moments, tables and the clip coefficient exist on the device afterwards
    torch.cuda.synchronize()
    L = lib()

    def launcher(o):
        tp, tg, tm, tv, ts = (t.dev for t in o._tables)
        n, d_c, nchunks = len(o.params), o._chunks[1], o._chunks[2]
        coef, b1, b2 = o._scal[1:2], o.betas[0], o.betas[1]
        if len(o.param_groups) > 1:
            return lambda: check(L.tav_adamw_chunked_groups(ptr(tp), ptr(tg), ptr(tm), ptr(tv), ptr(ts), ptr(d_c), n, nchunks, ptr(coef),
                                                            ptr(o._group_table.dev), ptr(o._hyper), len(o.param_groups), b1, b2, o.eps,
                                                            ptr(o._step_dev), ptr(o._scal[5:7]), stream()), "adamw_chunked_groups")
        return lambda: check(L.tav_adamw_chunked(ptr(tp), ptr(tg), ptr(tm), ptr(tv), ptr(ts), ptr(d_c), n, nchunks, ptr(coef), ptr(o._scal[4:5]), b1, b2,
                                                 o.eps, o.weight_decay, ptr(o._step_dev), ptr(o._scal[5:7]), stream()), "adamw_chunked")

    def block(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.launches):
            f()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.launches

    runs = {k: (launcher(o), []) for k, o in opts.items()}
    for f, _ in runs.values():
        block(f)                                 # warm-up: one full block each
    for _ in range(args.rounds):
        for f, ms in runs.values():
            ms.append(block(f))
    elems = sum(p.numel() for p in flat)
    nbytes = 7 * 4 * elems
    sizes = [len(g["params"]) for g in opts["four groups"].param_groups]
    lines = [f"# preset {args.preset}: {len(flat)} tensors, {elems / 1e6:.1f} M elements, {opts['one group']._chunks[2]} chunks; the four groups hold "
             f"{sizes} tensors (new decayed / new no-decay / pretrained decayed / pretrained no-decay)",
             f"# {args.rounds} alternating blocks of {args.launches} launches per line, HIP events around each block (tick kernel + update kernel per launch); "
             f"{nbytes / 1e9:.2f} GB moved per launch, byte floor at {COPY_TBS} TB/s = {nbytes / (COPY_TBS * 1e12) * 1e3:.3f} ms",
             f"{'launch':<24} {'mean ms':>9} {'spread':>8} {'TB/s':>7}  blocks"]
    res = []
    for k, (_, ms) in runs.items():
        m, sp = sum(ms) / len(ms), max(ms) - min(ms)
        lines.append(f"{k:<24} {m:>9.4f} {sp:>8.4f} {nbytes / (m * 1e-3) / 1e12:>7.2f}  " + " ".join(f"{v:.4f}" for v in ms))
        res.append(dict(launch=k, mean_ms=round(m, 5), spread_ms=round(sp, 5), blocks_ms=[round(v, 5) for v in ms]))
    d = res[1]["mean_ms"] - res[0]["mean_ms"]
    noise = max(res[0]["spread_ms"], res[1]["spread_ms"])
    lines.append(f"# four groups - one group = {d * 1e3:+.1f} us per launch ({d / res[0]['mean_ms'] * 100:+.2f}%); larger spread of the two lines {noise * 1e3:.1f} us: "
                 + ("within the spread" if abs(d) <= noise else "OUTSIDE the spread"))
    d2 = res[1]["mean_ms"] - res[2]["mean_ms"]
    noise2 = max(res[1]["spread_ms"], res[2]["spread_ms"])
    lines.append(f"# four groups - one group in group order (the kernels alone, same chunks in the same order) = {d2 * 1e3:+.1f} us per launch "
                 f"({d2 / res[2]['mean_ms'] * 100:+.2f}%); larger spread {noise2 * 1e3:.1f} us: " + ("within the spread" if abs(d2) <= noise2 else "OUTSIDE the spread"))
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    print(json.dumps({"tool": "gpu_param_groups_speed", "preset": args.preset, "results": res}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
