#!/usr/bin/env python3
"""The host decisions of the entry points outside gemm.hip as a table (tests/golden/entry_plan_golden.json), taken from a built libtavhip.so
through ctypes: (a) every size query of the ABI over arguments that bracket each clamp and cap, (b) the code every launching entry point
returns for INVALID arguments.  No call here launches anything: every case put on a launching entry point carries an argument fault that
the recorded commit refuses before its first launch (its code was read for each of them), and a case that comes back with anything but
-1..-4 stops the script.

    python tests/make_entry_plan_golden.py --lib <libtavhip.so of the commit to record> --commit <its hash>

tests/test_entry_plan_host.py replays table(lib) against the library of the tree; tests/host/entry_plan_check.cpp sweeps the same size
queries (same order) through csrc/entry_plan.h alone.  HAND holds what could not be recorded: faults the recorded commit answered only
after it had launched something, and which are now refused in front of the first launch with the same code."""
import ctypes as C
import itertools
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "entry_plan_golden.json")
HEADER = os.path.join(os.path.dirname(HERE), "multi-modal-emotion_amd", "csrc", "entry_plan.h")
F32, BF16, FP8, U8, I16 = 0, 1, 2, 3, 4
P = 0x1000                                                  # stands for a device pointer: tested for NULL-ness and alignment, never read


def header_constants():
    """{name: value} of every `constexpr int NAME = <number>` of csrc/entry_plan.h: the caps the axes below bracket."""
    out = {}
    for line in open(HEADER):
        if line.startswith("constexpr int "):
            out.update({k: int(v) for k, v in re.findall(r"(\w+) = (\d+)\s*[,;]", line)})
    return out


K = header_constants()


def around(x):
    return [x - 1, x, x + 1]


# ---- (a) size queries: name -> argument tuples, in this order
def query_axes():
    ln_rows, ln_cap = K["LN_BWD_ROWS"], K["LN_BWD_ROWS"] * K["LN_MAX_BLOCKS"]      # rows per block; rows at which ln_blocks reaches its cap
    emb_rows, emb_cap = K["EMB_PART_ROWS"], K["EMB_PART_ROWS"] * K["EMB_MAX_PARTS"]
    wn_rows, wn_cap = K["WN_PART_ROWS"], K["WN_PART_ROWS"] * K["WN_MAX_PARTS"]
    spec_cap = K["SPEC_ROWS"] * K["SPEC_MAX_PARTS"]
    amax_cap = K["FP8_AMAX_BLOCK_GROUPS"] * K["FP8_AMAX_MAX_PARTS"] * 4       # elements at which the amax partials reach their cap
    return {
        "tav_ln_bwd_partials": [(r,) for r in [0, 1] + around(ln_rows) + [46848] + around(ln_cap) + [1 << 40]],
        "tav_gn_workspace_floats": list(itertools.product([1, 4, 32], [64, 512, 768])),
        "tav_conv0_bwd_partials": [(b, t, 512, 10) for b in (1, 4) for t in [1] + around(K["C0_BT"]) + around(2 * K["C0_BT"]) + [49999]],
        "tav_weight_norm_partials": [(768, 48), (16, 16)] + [(r, 1) for r in [1] + around(wn_rows) + around(wn_cap) + [2 * wn_cap]],
        "tav_embed_add_bwd_parts": [(r,) for r in [1] + around(emb_rows) + around(emb_cap) + [1 << 40]],
        "tav_sumsq_partials": [(n,) for n in (1, 7, 300, 65535)],
        "tav_optim_chunk_elems": [()],
        "tav_optim_max_groups": [()],
        "tav_fp8_amax_partials": [(1, 4), (8, 1024), (9, 1024), (11712, 768)] + [(r, 4096) for r in around(amax_cap // 4096)] + [(1 << 30, 4096)],
        "tav_specaug_bwd_ws_bytes": [(r, h) for r in [0, 1] + around(K["SPEC_ROWS"]) + around(spec_cap) + [1 << 40] for h in (0, 4, 768)],
        "tav_audio_resample_tile": [(0, 1, 0), (1, 0, 0), (1, 1, -1)] + list(itertools.product([1, 2, 3, 7, 30, 31, 32, 147, 441], [1, 160, 320], [0, 6, 17, 100, 4000])),
    }


def query_rows(h):
    return {name: [int(getattr(h, name)(*a)) for a in axes] for name, axes in query_axes().items()}


# ---- (b) invalid arguments.  An entry: its arguments in call order (without the stream), valid as they stand; a struct argument is
# (ctypes class name, {field: value}).  A case edits them: "k=v, k=v" with k an argument or a field of the struct; "args=None" passes NULL.
ATT = dict(q=P, k=P, v=P, o=P, lse=P, B=2, S=128, nheads=2, ld_q=128, ld_k=128, ld_v=128, ld_o=128, ld_do=128, ld_dq=128, ld_dk=128, ld_dv=128,
           dtype=BF16, mask_mode=0, scale=0.125)
ATT_BWD = dict(ATT, dout=P, dq=P, dk=P, dv=P, delta=P)
ATT_CASES = ["args=None", "q=None", "k=None", "v=None", "o=None", "lse=None", "B=0", "S=0", "nheads=0", "B=1<<30", "dtype=FP8", "dtype=7", "mask_mode=3", "mask_mode=-1",
             "mask_mode=1", "mask_mode=2, key_mask=P", "mask_mode=2, key_mask=P, corr=P", "ld_q=132", "ld_k=132", "ld_v=132", "ld_o=130", "ld_q=64", "ld_o=64",
             "S=1<<20, ld_q=4096, ld_k=4096, ld_v=4096, ld_o=4096", "q=None, B=0", "B=0, dtype=7", "dtype=7, mask_mode=3", "mask_mode=3, ld_q=132",
             "mask_mode=1, ld_q=132", "ld_q=132, ld_k=64", "dtype=F32, ld_q=130"]
ATT_BWD_CASES = ATT_CASES + ["dout=None", "dq=None", "dk=None", "dv=None", "delta=None", "ld_do=132", "ld_dq=130", "ld_dk=130", "ld_dv=130", "ld_q=64, dout=None",
                             "dout=None, ld_do=132", "S=1<<20, ld_do=4096"]
LN = dict(x=P, x_dtype=F32, gamma=P, beta=P, y_f32=P, rows=8, W=64, ld_x=64, ld_y=64, eps=1e-5)
LN_BWD = dict(x=P, x_dtype=F32, gamma=P, dy=P, dy_dtype=F32, mean=P, rstd=P, dx_f32=P, rows=8, W=64, ld_x=64, ld_dy=64, ld_dx=64)
TXT = dict(ids=P, word=P, pos=P, type=P, gamma=P, beta=P, pre=P, pos_ids=P, y_f32=P, B=2, S=16, W=64, vocab=100, max_pos=64, pad_id=1, eps=1e-5)
CLIP = dict(src_dtype=U8, T=4, H=32, W=32, sT=3072, sH=96, sW=3, sC=1, nf=2, frame=(0, 1), crop_top=0, crop_left=0, crop_h=32, crop_w=32, mid_h=0, mid_w=0,
            out_h=16, out_w=16, scale=(1.0, 1.0, 1.0), shift=(0.0, 0.0, 0.0))
RES = dict(src_dtype=F32, C=1, L=1000, sC=0, sL=1, o=1, n=1, width=0, ntap=1, first_max=0, T_row=1000)
POOL = ["B=0", "S=0", "W=0", "W=6"]
DROP = ["n=0", "p=-0.1", "p=1.0", "x=None, n=0"]
ADAM = dict(params=P, grads=P, exp_avg=P, exp_avg_sq=P, sizes=P)
QUANT = ["x=None", "q=None", "rows=0", "cols=0", "cols=6", "ld=6", "ld_q=6", "qt=P, ld_qt=8, rows_pad=6", "qt=P, ld_qt=8, rows_pad=4", "qt=P, ld_qt=4, rows_pad=8",
         "qt=P, ld_qt=6, rows_pad=8", "dtype=FP8", "dtype=7", "x=None, rows=0", "cols=6, ld=6", "ld=6, dtype=7", "q=None, qt=P, ld_qt=8, rows_pad=8, dtype=7"]

ENTRIES = [
    ("tav_attn_fwd", dict(args=("AttnArgs", ATT)), ATT_CASES),
    ("tav_attn_bwd", dict(args=("AttnArgs", ATT_BWD)), ATT_BWD_CASES),
    ("tav_attn_fwd_len", dict(args=("AttnArgs", ATT), seq_lens=P), ATT_CASES + ["seq_lens=None", "B=0, seq_lens=None", "ld_q=132, seq_lens=None"]),
    ("tav_attn_bwd_len", dict(args=("AttnArgs", ATT_BWD), seq_lens=P), ATT_BWD_CASES + ["seq_lens=None", "dout=None, seq_lens=None", "ld_dq=130, seq_lens=None"]),
    ("tav_attn_probs", dict(args=("AttnArgs", ATT), probs=P, head_scale=None, hs_bstride=0),
     ["args=None", "q=None", "k=None", "lse=None", "probs=None", "B=0", "S=0", "nheads=0", "hs_bstride=-1", "dtype=FP8", "dtype=7", "mask_mode=3", "mask_mode=1", "ld_q=132",
      "ld_k=132", "dtype=F32, ld_k=130", "probs=None, B=0", "hs_bstride=-1, dtype=7", "dtype=7, mask_mode=3", "mask_mode=1, ld_q=132"]),
    ("tav_head_scale", dict(a=P, b=P, out=P, dtype=BF16, head_scale=None, hs_bstride=0, c0=1.0, B=2, S=8, nheads=2, lda=128, ldb=128, ldo=128),
     ["b=None", "out=None", "B=0", "S=0", "nheads=0", "hs_bstride=-1", "dtype=FP8", "dtype=7", "lda=2", "ldb=2", "ldo=2", "b=None, B=0", "B=0, dtype=7", "dtype=7, lda=2"]),
    ("tav_ln_fwd", dict(args=("LnArgs", LN)),
     ["args=None", "x=None", "gamma=None", "beta=None", "y_f32=None", "rows=0", "W=0", "W=1028", "W=66", "ld_x=66", "ld_y=2", "x_dtype=FP8", "x_dtype=7", "x=None, rows=0",
      "rows=0, ld_x=66", "ld_x=66, x_dtype=7"]),
    ("tav_ln_bwd", dict(args=("LnArgs", LN_BWD)),
     ["args=None", "x=None", "gamma=None", "dy=None", "mean=None", "rstd=None", "dx_f32=None", "act=1", "dgamma=P", "dbeta=P", "rows=0", "W=1028", "W=66", "ld_x=66", "ld_dy=66",
      "ld_dx=66", "defer_param_reduce=1", "x_dtype=7", "dy_dtype=FP8", "defer_param_reduce=1, ld_dx=66", "defer_param_reduce=1, x_dtype=7", "rows=0, dgamma=P",
      "rows=0, ld_x=66", "ld_x=66, dy_dtype=7"]),
    ("tav_gn_gelu_fwd", dict(x=P, y=P, dtype=BF16, gamma=P, beta=P, stats=P, workspace=P, B=2, T=100, C=64, eps=1e-5),
     ["x=None", "y=None", "gamma=None", "beta=None", "stats=None", "workspace=None", "B=0", "T=0", "C=0", "C=96", "dtype=FP8", "dtype=7", "x=None, B=0", "C=96, dtype=7"]),
    ("tav_gn_gelu_bwd", dict(x=P, dy=P, dx=P, dtype=BF16, gamma=P, beta=P, stats=P, workspace=P, dgamma=P, dbeta=P, B=2, T=100, C=64, accumulate=0),
     ["x=None", "dy=None", "dx=None", "gamma=None", "beta=None", "stats=None", "workspace=None", "dgamma=None", "dbeta=None", "B=0", "T=0", "C=96", "dtype=FP8", "dtype=7",
      "dy=None, T=0", "C=96, dtype=7"]),
    ("tav_gelu_fwd", dict(x=P, y=P, dtype=BF16, n=64), ["x=None", "y=None", "n=0", "n=6", "dtype=FP8", "dtype=7", "x=None, n=0", "n=6, dtype=7"]),
    ("tav_gelu_bwd", dict(x=P, dy=P, dx=P, dtype=BF16, n=64), ["x=None", "dy=None", "dx=None", "n=0", "n=6", "dtype=FP8", "dtype=7", "dx=None, n=6", "n=0, dtype=7"]),

    ("tav_cast_weight", dict(src=P, R=8, C=8, dst=P, ld_dst=0, dst_t=None, ld_dst_t=0, dst_dtype=BF16), ["src=None", "dst=None", "R=0", "C=0", "dst_dtype=FP8", "dst_dtype=7", "src=None, R=0", "R=0, dst_dtype=7"]),
    ("tav_cast_weights_multi", dict(descs=P, n=2, blocks_per_tensor=4), ["descs=None", "n=0", "n=65536", "blocks_per_tensor=0", "descs=None, n=0"]),
    ("tav_cast_conv_weight", dict(src=P, co=8, ci=4, k=3, dst=P, dst_t=None, dst_phase=None, conv_stride=0, dst_dtype=BF16),
     ["src=None", "dst=None", "co=0", "ci=0", "k=0", "dst_phase=P", "dst_phase=P, conv_stride=4", "dst_dtype=FP8", "dst_dtype=7", "src=None, co=0", "dst_phase=P, dst_dtype=7"]),
    ("tav_zero_pad_rows", dict(buf=P, dtype=BF16, B=2, T=8, C=8, pad=2), ["buf=None", "B=0", "T=0", "C=0", "C=6", "pad=0", "dtype=FP8", "dtype=7", "buf=None, B=0", "pad=0, dtype=7"]),
    ("tav_cast2d", dict(src=P, src_dtype=F32, ld_src=8, dst=P, dst_dtype=BF16, ld_dst=8, R=4, C=8),
     ["src=None", "dst=None", "R=0", "C=0", "C=6", "ld_src=6", "ld_dst=6", "src_dtype=FP8", "dst_dtype=7", "dst_dtype=U8", "src=None, R=0", "C=6, ld_src=6", "ld_src=6, src_dtype=7"]),
    ("tav_transpose2d", dict(src=P, dst=P, dtype=BF16, R=8, C=8, nbatch=2), ["src=None", "dst=None", "R=0", "C=0", "nbatch=0", "nbatch=65536", "dtype=FP8", "dtype=7", "nbatch=0, dtype=7"]),
    ("tav_add_f32", dict(a=P, b=P, y=P, y_lp=None, lp_dtype=0, n=64), ["a=None", "b=None", "y=None", "n=0", "n=6", "a=None, n=0"]),
    ("tav_fill_f32", dict(p=P, value=0.0, n=64), ["p=None", "n=0", "p=None, n=0"]),
    ("tav_embed_add_fwd", dict(x=P, ids=P, table=P, out=P, rows=8, W=64, ntable=3), ["x=None", "ids=None", "table=None", "out=None", "rows=0", "W=0", "W=6", "ntable=0", "x=None, W=6"]),
    ("tav_embed_add_bwd", dict(dy=P, ids=P, dtable=P, partials=P, rows=8, W=64, ntable=3, accumulate=0),
     ["dy=None", "ids=None", "dtable=None", "partials=None", "rows=0", "W=0", "ntable=0", "ntable=9", "partials=None, ntable=9"]),
    ("tav_text_embed_fwd", dict(args=("TextEmbedArgs", TXT)),
     ["args=None", "ids=None", "word=None", "pos=None", "type=None", "gamma=None", "beta=None", "pre=None", "pos_ids=None", "B=0", "S=0", "S=1025", "W=0", "W=6", "ids=None, B=0"]),
    ("tav_scatter_add_rows", dict(d=P, idx=P, dtable=P, rows=8, W=64, ntable=100),
     ["d=None", "idx=None", "dtable=None", "rows=0", "W=0", "W=6", "W=1028", "ntable=0", "rows=30000, W=768", "rows=38000, W=64", "d=None, rows=0"]),
    ("tav_gather_rows", dict(table=P, idx=P, out=P, rows=8, W=64, ntable=100), ["table=None", "idx=None", "out=None", "rows=0", "W=0", "W=6", "ntable=0", "out=None, W=6"]),
    ("tav_patchify", dict(video=P, keep_idx=P, patches=P, dtype=BF16, B=1, F=2, H=16, W=16, nkeep=1),
     ["video=None", "keep_idx=None", "patches=None", "B=0", "F=0", "F=3", "H=20", "W=20", "nkeep=0", "dtype=FP8", "dtype=7", "video=None, B=0", "F=3, dtype=7"]),
    ("tav_mask_to_index", dict(mask=P, keep_value=0, keep_idx=P, counts=None, B=2, n=16, nkeep=4), ["mask=None", "keep_idx=None", "B=0", "n=0", "nkeep=0", "nkeep=17", "mask=None, B=0"]),
    ("tav_ragged_lens", dict(mask=P, true_cnt=P, vid_lens=P, av_lens=P, status=P, B=2, ntok=16, cap_true=8, cap_keep=8, base=4),
     ["mask=None", "true_cnt=None", "vid_lens=None", "av_lens=None", "status=None", "B=0", "ntok=0", "cap_true=0", "cap_true=17", "cap_keep=0", "cap_keep=17", "base=-1",
      "ntok=1<<30", "base=1<<30", "status=None, B=0"]),
    ("tav_mean_pool_fwd", dict(x=P, y=P, B=2, S=8, W=64), ["x=None", "y=None", "x=None, B=0"] + POOL),
    ("tav_mean_pool_bwd", dict(dy=P, dx=P, dx_lp=None, lp_dtype=0, B=2, S=8, W=64), ["dy=None", "dx=None", "dy=None, W=6"] + POOL),
    ("tav_mean_pool_fwd_len", dict(x=P, y=P, seq_lens=P, B=2, S=8, W=64), ["x=None", "y=None", "seq_lens=None", "seq_lens=None, S=0"] + POOL),
    ("tav_mean_pool_bwd_len", dict(dy=P, dx=P, dx_lp=None, lp_dtype=0, seq_lens=P, B=2, S=8, W=64), ["dy=None", "dx=None", "seq_lens=None", "seq_lens=None, W=6"] + POOL),
    ("tav_head_fwd", dict(x=P, W=P, b=None, y=P, B=2, K=64, N=7), ["x=None", "W=None", "y=None", "B=0", "K=0", "N=0", "y=None, N=0"]),
    ("tav_head_bwd", dict(x=P, W=P, dy=P, dx=None, dW=P, db=None, B=2, K=64, N=7, accumulate=0), ["x=None", "W=None", "dy=None", "dW=None", "B=0", "K=0", "N=0", "N=257", "dW=None, N=257"]),
    ("tav_tanh_fwd", dict(x=P, y=P, n=8), ["x=None", "y=None", "n=0", "x=None, n=0"]),
    ("tav_tanh_bwd", dict(y=P, dy=P, dx=P, n=8), ["y=None", "dy=None", "dx=None", "n=0", "dx=None, n=0"]),
    ("tav_cross_entropy", dict(logits=P, target=P, class_weight=None, loss=P, dlogits=None, B=4, C=7, grad_scale=1.0),
     ["logits=None", "target=None", "loss=None", "B=0", "C=0", "C=65", "target=None, C=65"]),
    ("tav_step_stats", dict(logits=P, preds=None, target=P, cm=P, loss=None, status=None, acc=None, B=4, C=7),
     ["target=None", "logits=None", "preds=P", "cm=None", "B=0", "B=1<<31", "C=0", "C=65", "preds=P, C=65"]),
    ("tav_dropout_fwd", dict(x=P, y=P, mask=P, n=8, p=0.1, seed=1, offset=0), ["x=None", "y=None", "mask=None"] + DROP),
    ("tav_dropout_fwd_dev", dict(x=P, y=P, mask=P, n=8, p=0.1, seed_state=P, offset=0), ["x=None", "y=None", "mask=None", "seed_state=None"] + DROP),
    ("tav_dropout_bwd", dict(x=P, mask=P, dx=P, n=8, p=0.1), ["x=None", "mask=None", "dx=None"] + DROP),
    ("tav_sumsq_multi", dict(ptrs=P, sizes=P, ntensors=3, partials=P, out=P), ["ptrs=None", "sizes=None", "partials=None", "out=None", "ntensors=0", "ntensors=65536", "out=None, ntensors=0"]),
    ("tav_sumsq_chunked", dict(ptrs=P, sizes=P, chunk_prefix=P, ntensors=3, nchunks=5, partials=P, out=P),
     ["ptrs=None", "sizes=None", "chunk_prefix=None", "partials=None", "out=None", "ntensors=0", "nchunks=0", "out=None, nchunks=0"]),
    ("tav_sum_partials", dict(partials=P, n=5, out=P), ["partials=None", "out=None", "n=0", "out=None, n=0"]),
    ("tav_adamw_chunked", dict(ADAM, chunk_prefix=P, ntensors=3, nchunks=5, clip_coef=None, lr=P, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, step=P, bias_corr=P),
     ["params=None", "grads=None", "exp_avg=None", "exp_avg_sq=None", "sizes=None", "chunk_prefix=None", "lr=None", "step=None", "bias_corr=None", "ntensors=0", "nchunks=0",
      "lr=None, nchunks=0"]),
    ("tav_adamw_chunked_groups", dict(ADAM, chunk_prefix=P, ntensors=3, nchunks=5, clip_coef=None, group_of=P, hyper=P, ngroups=2, beta1=0.9, beta2=0.999, eps=1e-8, step=P, bias_corr=P),
     ["params=None", "grads=None", "exp_avg=None", "exp_avg_sq=None", "sizes=None", "chunk_prefix=None", "group_of=None", "hyper=None", "step=None", "bias_corr=None", "ntensors=0",
      "nchunks=0", "ngroups=0", "ngroups=%d" % (K["OPT_MAX_GROUPS"] + 1), "hyper=None, ngroups=0"]),
    ("tav_clip_coef", dict(sumsq=P, max_norm=1.0, coef_out=P, norm_out=None), ["sumsq=None", "coef_out=None"]),
    ("tav_adamw_multi", dict(ADAM, ntensors=3, clip_coef=None, lr=P, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, step=P, bias_corr=P),
     ["params=None", "grads=None", "exp_avg=None", "exp_avg_sq=None", "sizes=None", "lr=None", "step=None", "bias_corr=None", "ntensors=0", "ntensors=65536", "step=None, ntensors=0"]),

    ("tav_conv0_fwd", dict(wave=P, w=P, bias=None, y=P, y_dtype=BF16, B=1, T_in=100, T_out=19, C=8, K=10, stride=5),
     ["wave=None", "w=None", "y=None", "B=0", "T_in=0", "T_out=0", "C=0", "C=6", "K=0", "K=%d" % (K["C0_MAXK"] + 1), "stride=0", "stride=9", "T_in=99", "y_dtype=FP8", "y_dtype=7",
      "wave=None, C=6", "T_in=99, y_dtype=7"]),
    ("tav_conv0_bwd_w", dict(wave=P, dy=P, dy_dtype=BF16, dw=P, dbias=None, partials=P, B=1, T_in=100, T_out=19, C=8, K=10, stride=5, accumulate=0),
     ["wave=None", "dy=None", "dw=None", "partials=None", "B=0", "T_out=0", "C=12", "K=11", "stride=9", "dy_dtype=FP8", "dy_dtype=7", "dw=None, C=12", "K=11, dy_dtype=7"]),
    ("tav_col2im_1d", dict(dcol=P, dx=P, pre_act=None, dtype=BF16, B=1, T_in=100, T_out=19, C=8, K=10, stride=5),
     ["dcol=None", "dx=None", "B=0", "T_in=0", "T_out=0", "C=6", "K=0", "stride=0", "dtype=FP8", "dtype=7", "dx=None, C=6", "stride=0, dtype=7"]),
    ("tav_group_pad", dict(x=P, x_dtype=F32, xg=P, xg_dtype=BF16, B=1, T=8, H=64, G=4, pad_l=1, pad_r=1),
     ["x=None", "xg=None", "B=0", "T=0", "H=0", "G=0", "H=66", "G=32", "pad_l=-1", "pad_r=-1", "x_dtype=BF16, xg_dtype=F32", "x_dtype=7", "xg_dtype=FP8", "x=None, G=32", "pad_l=-1, x_dtype=7"]),
    ("tav_weight_norm_fwd", dict(v=P, g=P, norms=P, partials=P, w=P, w_flip=None, dtype=BF16, H=64, Cg=16, K=8),
     ["v=None", "g=None", "norms=None", "partials=None", "w=None", "H=0", "Cg=0", "K=0", "K=%d" % (K["WN_MAXK"] + 1), "H=60", "w=None, H=60"]),
    ("tav_weight_norm_bwd", dict(v=P, g=P, norms=P, dw_gemm=P, workspace=P, dv=P, dg=P, H=64, Cg=16, K=8, accumulate=0),
     ["v=None", "g=None", "norms=None", "dw_gemm=None", "workspace=None", "dv=None", "dg=None", "H=0", "K=%d" % (K["WN_MAXK"] + 1), "H=60", "dg=None, H=60"]),

    ("tav_fp8_amax", dict(x=P, dtype=BF16, rows=8, cols=64, ld=64, partials=P, scales=P),
     ["x=None", "partials=None", "scales=None", "rows=0", "cols=0", "cols=6", "ld=6", "dtype=FP8", "dtype=7", "x=None, rows=0", "cols=6, ld=6", "ld=6, dtype=7"]),
    ("tav_fp8_quantize", dict(x=P, dtype=BF16, rows=8, cols=64, ld=64, scales=P, q=P, ld_q=64, qt=None, ld_qt=0, rows_pad=0), QUANT + ["scales=None"]),
    ("tav_fp8_quantize_delayed", dict(x=P, dtype=BF16, rows=8, cols=64, ld=64, scales=P, q=P, ld_q=64, qt=None, ld_qt=0, rows_pad=0), QUANT + ["scales=None"]),
    ("tav_fp8_roll_states", dict(states=P, n=4), ["states=None", "n=0", "states=None, n=0"]),
    ("tav_splitk_reduce", dict(slabs=P, out=P, nsplit=2, n_elems=64, accumulate=0), ["slabs=None", "out=None", "nsplit=0", "n_elems=0", "n_elems=6", "out=None, nsplit=0"]),

    ("tav_specaug_draw", dict(valid=None, mask=P, nspans=None, B=2, L=100, prob=0.05, length=10, min_masks=2, seed=1, tag=0),
     ["mask=None", "B=0", "L=0", "length=0", "min_masks=-1", "prob=-0.1", "prob=1.5", "prob=float('nan')", "B=1<<31", "L=1<<31", "B=1<<21, L=1<<20", "L=100000, length=1, prob=1.0",
      "L=10000, min_masks=200", "mask=None, B=0"]),
    ("tav_specaug_draw_dev", dict(valid=None, mask=P, nspans=None, B=2, L=100, prob=0.05, length=10, min_masks=2, seed_state=P, tag=0),
     ["mask=None", "seed_state=None", "B=0", "length=0", "prob=1.5", "L=10000, min_masks=200", "seed_state=None, B=0"]),
    ("tav_specaug_fwd", dict(x=P, tmask=None, fmask=None, embed=None, y=P, B=2, T=8, H=64),
     ["x=None", "y=None", "tmask=P", "B=0", "T=0", "H=0", "H=6", "B=1<<31", "B=1<<21, T=1<<20", "x=0x1004", "y=0x1008", "tmask=P, embed=0x1004", "fmask=0x1002", "x=None, H=6", "H=6, x=0x1004"]),
    ("tav_specaug_bwd", dict(dy=P, tmask=None, fmask=None, dx=P, dembed=None, workspace=None, workspace_bytes=0, B=2, T=8, H=64),
     ["dy=None", "dx=None", "dembed=P", "dembed=P, workspace=P", "dembed=P, workspace=P, workspace_bytes=255", "B=0", "H=6", "dy=0x1004", "dx=0x1008",
      "dembed=0x1004, workspace=P, workspace_bytes=256", "dembed=P, workspace=0x1008, workspace_bytes=256", "fmask=0x1002", "dembed=P, workspace=P, dy=0x1004", "dx=None, H=6"]),

    ("tav_video_clip_transform", dict(src=P, dst=P, x=("ClipXform", CLIP)),
     ["src=None", "dst=None", "x=None", "src_dtype=BF16", "src_dtype=I16", "T=0", "H=0", "W=0", "H=%d" % (K["VX_MAX"] + 1), "crop_h=0", "out_h=0", "out_w=%d" % (K["VX_MAX"] + 1), "sT=-1", "sC=-1", "nf=0", "nf=33",
      "frame=(0, 4)", "frame=(-1, 0)", "crop_top=1", "crop_left=1", "crop_w=33", "mid_h=8", "mid_w=8", "mid_h=8, mid_w=%d" % (K["VX_MAX"] + 1), "src_dtype=BF16, T=0", "src=None, src_dtype=BF16"]),
    ("tav_audio_resample", dict(src=P, table=P, first=P, values=P, mask=None, a=("ResampleArgs", RES)),
     ["src=None", "table=None", "first=None", "values=None", "a=None", "src_dtype=BF16", "src_dtype=U8", "C=0", "C=33", "L=0", "L=(1<<40)+1, T_row=1<<40", "sC=-1", "sL=-1", "o=0", "n=0",
      "n=(1<<20)+1", "ntap=0", "width=-1", "n=1<<20, ntap=17, first_max=0, width=8", "first_max=-1", "first_max=1", "T_row=999", "T_row=(1<<40)+1", "o=1000, L=100000",
      "src_dtype=BF16, C=0", "src=None, src_dtype=BF16"]),
]

# Answered by the recorded commit only behind its first launches; now in front of them, with the same code.  Never called on that commit.
HAND = [
    ["tav_weight_norm_fwd", "dtype=FP8", -3], ["tav_weight_norm_fwd", "dtype=7", -3], ["tav_weight_norm_fwd", "w=None, dtype=7", -1], ["tav_weight_norm_fwd", "H=60, dtype=7", -2],
    ["tav_text_embed_fwd", "y_f32=None", -1], ["tav_text_embed_fwd", "W=1028", -2], ["tav_text_embed_fwd", "S=1025, W=1028", -2],
]
# the dtype codes (or source / destination pairs) every entry with a dtype argument accepts; everything else is in the cases above as -3
ACCEPTED_DTYPES = {"floats": [BF16, F32], "tav_cast2d": [[F32, BF16], [BF16, F32], [F32, F32], [BF16, BF16]], "tav_group_pad": [[F32, BF16], [F32, F32], [BF16, BF16]],
                   "tav_video_clip_transform": [U8, F32], "tav_audio_resample": [F32, I16]}


def _lib_module():
    from tav_amd import _lib
    return _lib


def _items_cases(h):
    """tav_ln_param_reduce_multi takes a host array of items."""
    L = _lib_module()

    def call(n=2, null=False, **edit):
        items = (L.LnReduceItem * 65)()
        for it in items:
            it.partials, it.dgamma, it.dbeta, it.nblocks, it.W, it.accumulate = P, P, P, 4, 64, 0
        for k, v in edit.items():
            setattr(items[1], k, v)
        return lambda: h.tav_ln_param_reduce_multi(None if null else items, n, None)
    e = "tav_ln_param_reduce_multi"
    return [(e, "items=None", call(null=True)), (e, "n=0", call(n=0)), (e, "n=65", call(n=65)), (e, "partials=None (1)", call(partials=None)),
            (e, "dgamma=None, dbeta=None (1)", call(dgamma=None, dbeta=None)), (e, "W=0 (1)", call(W=0)), (e, "W=1028 (1)", call(W=1028)), (e, "W=66 (1)", call(W=66)),
            (e, "nblocks=0 (1)", call(nblocks=0)), (e, "nblocks=%d (1)" % (K["LN_MAX_BLOCKS"] + 1), call(nblocks=K["LN_MAX_BLOCKS"] + 1)),
            (e, "partials=None, W=66 (1)", call(partials=None, W=66)), (e, "n=65, partials=None (1)", call(n=65, partials=None))]


def _thunk(h, entry, base, case):
    L = _lib_module()
    edit = eval("dict(%s)" % case, {"P": P, "F32": F32, "BF16": BF16, "FP8": FP8, "U8": U8, "I16": I16})

    def run():
        args = []
        left = dict(edit)
        for name, val in base.items():
            if isinstance(val, tuple):                      # a struct argument
                if name in left:
                    assert left.pop(name) is None
                    args.append(None)
                    continue
                s = getattr(L, val[0])()
                fields = dict(val[1])
                names = {f[0] for f in s._fields_}
                fields.update({k: left.pop(k) for k in list(left) if k in names and k not in base})
                for k, v in fields.items():
                    if isinstance(v, tuple):
                        for i, x in enumerate(v):
                            getattr(s, k)[i] = x
                    else:
                        setattr(s, k, v)
                args.append(C.byref(s))
            else:
                args.append(left.pop(name) if name in left else val)
        assert not left, f"{entry} [{case}]: no such argument {sorted(left)}"
        return getattr(h, entry)(*args, None)
    return run


def invalid_cases(h, hand=False):
    """[(entry point, case, thunk -> rc)]; with `hand` the HAND cases instead."""
    specs = {e: base for e, base, _ in ENTRIES}
    if hand:
        return [(e, c, _thunk(h, e, specs[e], c)) for e, c, _ in HAND]
    out = []
    for entry, base, cases in ENTRIES:
        assert len(set(cases)) == len(cases), entry
        out += [(entry, c, _thunk(h, entry, base, c)) for c in cases]
        if entry == "tav_ln_bwd":
            out += _items_cases(h)
    return out


def invalid_rows(h):
    rows = []
    for entry, name, thunk in invalid_cases(h):
        rc = thunk()
        assert rc in (-1, -2, -3, -4), f"{entry} [{name}] returned {rc}: not an argument fault -- it must not be in this table"
        rows.append([entry, name, rc])
    return rows


def table(h):
    return {"size_queries": query_rows(h), "invalid_arguments": invalid_rows(h), "refused_before_launch_by_hand": HAND, "accepted_dtypes": ACCEPTED_DTYPES}


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True)
    ap.add_argument("--commit", required=True)
    ap.add_argument("--out", default=GOLDEN)
    a = ap.parse_args()
    os.environ["TAV_LIB"] = os.path.abspath(a.lib)
    sys.path.insert(0, os.path.dirname(HERE))
    import tav_amd  # noqa: F401
    from tav_amd import _lib
    doc = {"recorded_from_commit": a.commit, "made_by": "tests/make_entry_plan_golden.py"}
    doc.update(table(_lib.lib()))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(a.out, os.path.getsize(a.out), "bytes;", sum(len(v) for v in doc["size_queries"].values()), "size queries,", len(doc["invalid_arguments"]), "invalid-argument cases")
