"""Measures the visual Conv3d baseline on the GPU and writes profiles/visual_conv3d.txt (a record, not a gate).

    python tools/gpu_conv3d_speed.py [--out profiles/visual_conv3d.txt] [--batch 8]

At the reference geometry -- [B, 3, 16, 224, 224] clips, --hidden_layers 32,32, B = 8 -- for both policies: every kernel of a training step
alone (device events, median of blocks of launches with their spread) next to its floor, the larger of its FLOPs over the dense bf16 MFMA
peak (the exact-f32 MFMA peak under fp32) and its bytes over the achievable HBM bandwidth; the whole training step (forward, weighted cross
entropy, backward, AdamW) with the loss, the finiteness of every gradient and the peak memory; torch's own F.conv3d forward + backward
(MIOpen) in bf16 on the same GPU and shapes as a yardstick; and the model-level errors of tests/test_conv3d_gpu.py's twin comparison.

Every step runs in a child process of its own under its own time limit; the first step that fails, faults or runs out of time ends the
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

PEAK_BF16, PEAK_F32, HBM = 2.5e15, 157.3e12, 6.3e12          # dense MFMA peaks (spec) and the achievable HBM rate, FLOP/s and bytes/s
CLIP, HIDDEN, O = (16, 224, 224), (32, 32), 7
LIMITS = {"kernels": 420, "step": 420, "torch": 300, "errors": 300}


def _blocks(fn, blocks=5, per_block=3):
    import torch
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(blocks):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(per_block):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / per_block)
    return statistics.median(ms), min(ms), max(ms)


def _line(name, t, flops, nbytes, peak):
    tf, tb = flops / peak * 1e3, nbytes / HBM * 1e3
    floor, by = (tf, "FLOPs") if tf >= tb else (tb, "bytes")
    rate = f"{flops / (t[0] * 1e-3) / 1e12:7.1f} TFLOP/s" if flops else f"{nbytes / (t[0] * 1e-3) / 1e12:7.2f} TB/s   "
    return f"  {name:22s} {t[0]:9.3f} ms [{t[1]:.3f} .. {t[2]:.3f}]  {rate}  floor {floor:7.3f} ms ({by}; {flops / 1e9:8.1f} GFLOP, {nbytes / 1e6:8.1f} MB)  x{t[0] / floor:6.1f} of the floor"


def step_kernels(policy, B):
    import torch

    import tav_amd  # noqa: F401
    from tav_amd import ops
    dt = torch.bfloat16 if policy == "bf16" else torch.float32
    es, peak = (2, PEAK_BF16) if policy == "bf16" else (4, PEAK_F32)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, 3, *CLIP, generator=g).cuda()
    shapes, acts, lines = [], [], []
    a = ops.conv3d_pack_input(x, dt)
    lines.append(_line("pack_input", _blocks(lambda: ops.conv3d_pack_input(x, dt)), 0, x.numel() * 4 + a.numel() * es, peak))
    cin = 3
    for cout in HIDDEN:
        w = (torch.randn(cout, cin, 3, 3, 3, generator=g) * (27 * cin) ** -0.5).cuda()
        w_op, w_flip = ops.conv3d_pack_weight(w, dt), ops.conv3d_pack_weight(w, dt, flip_transpose=True)
        bias = torch.zeros(ops.conv3d_cp(cout), device="cuda")
        y, gd = ops.conv3d_fwd(a, w_op, bias, cin, cout)
        vox = y.numel() // y.shape[-1]
        plan = ops.conv3d_plan(*a.shape[:4], cin, cout, dt)
        lines.append(f"  layer {cin} -> {cout}: plan tw {plan['tw']} th {plan['th']} block {plan['block']} lds {plan['lds_bytes']} grid {plan['patches']}; "
                     f"wgrad block {plan['wg_block']} lds {plan['wg_lds_bytes']} grid {plan['wg_nslabs']} x {plan['wg_groups']}")
        flops = 2.0 * vox * 27 * cin * cout                                          # the useful FLOPs (pad channels are the kernel's own cost)
        lines.append(_line(f"conv3d_fwd {cin}->{cout}", _blocks(lambda: ops.conv3d_fwd(a, w_op, bias, cin, cout)), flops, (a.numel() + 2 * y.numel()) * es, peak))
        dz = ops.conv3d_dz(y, gd)
        lines.append(_line(f"conv3d_dz {cout}", _blocks(lambda: ops.conv3d_dz(y, gd)), 0, 3 * y.numel() * es, peak))
        lines.append(_line(f"conv3d_wgrad {cin}->{cout}", _blocks(lambda: ops.conv3d_wgrad(a, dz, cin, cout)), flops, (a.numel() + dz.numel()) * es, peak))
        if cin != 3:
            lines.append(_line(f"conv3d_dgrad {cout}->{cin}", _blocks(lambda: ops.conv3d_dgrad(dz, w_flip, cin, cout)), flops, (a.numel() + dz.numel()) * es, peak))
        del gd, dz
        a, cin = y, cout
    S = a.numel() // a.shape[-1] // B
    wl = (torch.randn(O, cin * S, generator=g) * 1e-3).cuda()
    dy = torch.randn(B, O, generator=g).cuda()
    lines.append(_line("flat_linear_fwd", _blocks(lambda: ops.flat_linear_fwd(a, wl, None, cin)), 2.0 * B * O * cin * S, a.numel() * es + B * wl.numel() * 4, PEAK_F32))
    lines.append(_line("flat_linear_bwd", _blocks(lambda: ops.flat_linear_bwd(a, wl, dy, cin)), 4.0 * B * O * cin * S, 2 * a.numel() * es + 2 * wl.numel() * 4, PEAK_F32))
    print("\n".join(lines))


def _model(policy):
    import torch

    from tav_amd import runtime
    from tav_amd.SingleModels.models.visual import VisualClassification
    runtime.set_precision(policy)
    torch.manual_seed(0)
    return VisualClassification({"input_dim": 3, "output_dim": O, "hidden_layers": list(HIDDEN), "clip_shape": CLIP}).cuda()


def step_step(policy, B):
    import torch

    import tav_amd  # noqa: F401
    from tav_amd.optim import FusedAdamW
    from tav_amd.utils.global_functions import CrossEntropyLoss
    model = _model(policy)
    opt = FusedAdamW(list(model.parameters()), lr=1e-6, weight_decay=1e-4)
    crit = CrossEntropyLoss(weight=torch.linspace(0.6, 0.95, O))
    g = torch.Generator().manual_seed(1)
    x, lab = torch.randn(B, 1, 3, *CLIP, generator=g).cuda(), torch.randint(0, O, (B,), generator=g).cuda()

    def one():
        loss = crit(model(x), lab)
        opt.zero_grad()
        loss.backward()
        finite = all(bool(torch.isfinite(p.grad).all()) for p in model.parameters())
        opt.step()
        return float(loss), finite
    loss, finite = one()
    one()
    torch.cuda.synchronize()
    t0, n = time.perf_counter(), 4
    for _ in range(n):
        loss_n, finite_n = one()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / n * 1e3
    print(f"  {policy}: full-geometry smoke, B {B}: first loss {loss:.5f} (finite {loss == loss}), every gradient finite {finite and finite_n}; "
          f"training step {ms:.1f} ms (host clock around {n} steps, each ending in a read of the loss and of the gradients' finiteness); "
          f"peak memory {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")


def step_torch(B):
    import torch
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(0)
    total, lines, a, cin = 0.0, [], torch.randn(B, 3, *CLIP, generator=g).cuda().bfloat16(), 3
    for cout in HIDDEN:
        w = (torch.randn(cout, cin, 3, 3, 3, generator=g) * (27 * cin) ** -0.5).cuda().bfloat16().requires_grad_(True)
        b = torch.zeros(cout, device="cuda", dtype=torch.bfloat16, requires_grad=True)
        xin = a.detach().requires_grad_(cin != 3)

        def both():
            y = F.conv3d(xin, w, b)
            y.backward(y.detach())
        t = _blocks(both)
        total += t[0]
        lines.append(f"  torch F.conv3d {cin}->{cout} forward + backward (weight, bias{', input' if cin != 3 else ''}), bf16 NCDHW: {t[0]:9.3f} ms [{t[1]:.3f} .. {t[2]:.3f}]")
        with torch.no_grad():
            a = F.gelu(F.conv3d(xin, w, b))
        cin = cout
    print("\n".join(lines + [f"  torch, both layers: {total:.3f} ms"]))


def step_errors():
    run = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_conv3d_gpu.py"), "-q", "-s", "-k", "test_model_matches"],
                         capture_output=True, text=True, cwd=ROOT)
    keep = [ln for ln in run.stdout.splitlines() if ln.lstrip(".").startswith("model ") or " passed" in ln or " failed" in ln]
    print("\n".join("  " + ln.lstrip(".") for ln in keep))
    if run.returncode not in (0, 1):
        sys.exit(run.returncode)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "visual_conv3d.txt"))
    ap.add_argument("--batch", default=8, type=int)
    ap.add_argument("--step", default=None, help="(internal) run one step in this process")
    args = ap.parse_args()
    if args.step:
        name, _, policy = args.step.partition(":")
        {"kernels": lambda: step_kernels(policy, args.batch), "step": lambda: step_step(policy, args.batch), "torch": lambda: step_torch(args.batch),
         "errors": step_errors}[name]()
        return
    import torch
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is no host form"
    lines = [f"Visual Conv3d baseline on {torch.cuda.get_device_name(0)} (tools/gpu_conv3d_speed.py)", "",
             f"geometry: clips [B, 3, {', '.join(map(str, CLIP))}], hidden_layers {','.join(map(str, HIDDEN))}, B {args.batch}, output_dim {O}",
             f"floors: FLOPs over {PEAK_BF16 / 1e15:.1f} PFLOP/s (dense bf16 MFMA; fp32 policy and the f32 flat linear: {PEAK_F32 / 1e12:.1f} TFLOP/s), bytes over {HBM / 1e12:.1f} TB/s;",
             "kernel times: device events, median of 5 blocks of 3 launches [min .. max of the blocks], after 2 warm-up launches", ""]
    plan = [("kernels:bf16", "kernels, bf16 policy"), ("kernels:fp32", "kernels, fp32 policy"), ("step:bf16", "whole training step"), ("step:fp32", None),
            ("torch", "yardstick: torch's own convolution (MIOpen), same GPU, same shapes"), ("errors", "model against the float64 torch twin at clip (6, 12, 20), hidden 16,32, batch 3 (error, e_chain, ratio; the gate is 4)")]
    for step, title in plan:
        if title:
            lines += [title + ":"]
        try:
            run = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step, "--batch", str(args.batch)], capture_output=True, text=True,
                                 timeout=LIMITS[step.partition(":")[0]], cwd=ROOT)
        except subprocess.TimeoutExpired:
            lines += [f"  {step}: NOT MEASURED: ran past its limit of {LIMITS[step.partition(':')[0]]} s; nothing after it was run"]
            break
        lines += [ln for ln in run.stdout.splitlines() if ln.strip()]
        if run.returncode != 0:
            lines += [f"  {step}: FAILED with exit status {run.returncode}; nothing after it was run", *("    " + ln for ln in run.stderr.splitlines()[-6:])]
            break
        if title is None or step.startswith("kernels") or step in ("torch",):
            lines += [""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
