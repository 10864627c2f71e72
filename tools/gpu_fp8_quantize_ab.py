"""tav_fp8_quantize_delayed, two builds of the library in ONE process, alternating round by round (the second build: tools/ab_build.sh).
usage: python tools/gpu_fp8_quantize_ab.py path/to/other.so [rows cols ...]      default shapes: 46832 x 1024 and 46832 x 4096

bf16 input at the activation shapes the fp8 policy quantises in BASELINE config 5 (batch 16 x 2927 video tokens = 46 832 rows; hidden 1024, FFN
4096), the streaming kernel (q only) and the tiled kernel (q + qt).  Per round 20 back-to-back launches between two device events, 21 rounds per
build; prints microseconds per launch as median [min .. max] and quartiles, this build over the other, and whether q, qt and the state are the
same bits (finite inputs: they must be).  profiles/nonfinite_fp8_quantize.txt is one run of it against the parent of the NaN / Inf fix."""
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import tav_amd  # noqa: E402,F401
from tav_amd import ops  # noqa: E402

if len(sys.argv) < 2:
    sys.exit(__doc__)
this = ops.lib()
other = ctypes.CDLL(os.path.abspath(sys.argv[1]))
other.tav_fp8_quantize_delayed.argtypes = this.tav_fp8_quantize_delayed.argtypes
other.tav_fp8_quantize_delayed.restype = this.tav_fp8_quantize_delayed.restype
libs = {"other": other, "this": this}
dims = [int(a) for a in sys.argv[2:]] or [46832, 1024, 46832, 4096]
ROUNDS, N = 21, 20
print(f"# other = {sys.argv[1]}; {ROUNDS} rounds of {N} launches per build, alternating; us per launch, median [min .. max] (q1 / q3)")
for rows, cols in zip(dims[::2], dims[1::2]):
    g = torch.Generator(device="cpu").manual_seed(rows + cols)
    x = torch.randn(rows, cols, generator=g).cuda().to(torch.bfloat16)
    rows_pad = (rows + ops.FP8_KPAD - 1) // ops.FP8_KPAD * ops.FP8_KPAD
    amax = float(x.float().abs().max().item())

    def fresh_state():                                               # a scale that saturates the top of the range, as a tensor that outgrew its scale
        return torch.tensor([448.0 / amax * 1.5, amax / 448.0 / 1.5, amax / 1.5, 0.0], device="cuda")
    for form, want_t in (("stream", False), ("tiled ", True)):
        q = torch.empty(rows, cols, dtype=torch.uint8, device="cuda")
        qt = torch.empty(cols, rows_pad, dtype=torch.uint8, device="cuda") if want_t else None

        def launch(lib, state):
            rc = lib.tav_fp8_quantize_delayed(ops.ptr(x), ops.dt(x), rows, cols, x.stride(0), ops.ptr(state), ops.ptr(q), cols, ops.ptr(qt), rows_pad, rows_pad,
                                              ops.stream())
            assert rc == 0, rc
        outs = {}
        for k, lib in libs.items():                                  # warm-up, and the outputs of each build
            state = fresh_state()
            for _ in range(3):
                launch(lib, state)
            torch.cuda.synchronize()
            outs[k] = (q.clone(), None if qt is None else qt.clone(), state.clone())
        same = all(torch.equal(a, b) for a, b in zip(outs["other"], outs["this"]) if a is not None)
        times = {k: [] for k in libs}
        for r in range(ROUNDS):
            for k in (("other", "this") if r % 2 == 0 else ("this", "other")):
                state = fresh_state()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(N):
                    launch(libs[k], state)
                e1.record()
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1) / N * 1e3)
        line = f"{form} {rows} x {cols}"
        for k in ("other", "this"):
            t = sorted(times[k])
            line += f"   {k} {statistics.median(t):7.2f} [{t[0]:7.2f} .. {t[-1]:7.2f}] ({t[len(t) // 4]:.2f} / {t[3 * len(t) // 4]:.2f})"
        ratio = statistics.median(times["this"]) / statistics.median(times["other"])
        print(f"{line}   this / other {ratio:.4f}   bits {'equal' if same else 'DIFFER'}", flush=True)
