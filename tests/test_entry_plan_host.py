"""CPU: the host decisions of the entry points outside gemm.hip (csrc/entry_plan.h) against the table recorded from the parent of the commit
that moved them out of the .hip files (tests/golden/entry_plan_golden.json, made by tests/make_entry_plan_golden.py), twice: through the
built library, and through the header compiled stand-alone under AddressSanitizer + UndefinedBehaviorSanitizer
(tests/host/entry_plan_check.cpp, built and run by tests/host_program.py), which also checks the invariants of every launch geometry and
workspace layout over a sweep that includes the caps."""
import functools
import json
import os
import re

import make_entry_plan_golden as G
from host_program import run_alone_under_sanitizers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Accepted shapes whose narrowing to dim3 / int loses bits (entry_plan_check.cpp prints them as findings; profiles/entry_host_refactor.txt
# says what happens there).  None of them writes out of bounds: a y or z extent past 65535 is refused by the launch, an x extent past 2^31
# needs a tensor of 2^39 elements.  The two that could -- a wrapped tav_gn_workspace_floats / tav_conv0_bwd_partials -- are refused by the
# validators.  A new name here is a new narrowing: look at it before adding it.
KNOWN_NARROWINGS = {
    "one-dimensional element grid", "tav_attn_probs", "tav_attn_probs sizes", "tav_cast_weight R", "tav_conv0_fwd", "tav_embed_add_bwd rows per part",
    "tav_fp8_quantize rows", "tav_gn_gelu B", "tav_gn_gelu T", "tav_mean_pool_fwd B / tav_patchify B / tav_conv0 B", "tav_specaug_fwd",
}


@functools.lru_cache(maxsize=None)
def golden():
    with open(G.GOLDEN) as f:
        doc = json.load(f)
    assert len(doc["recorded_from_commit"]) == 40
    return doc


def test_library_reproduces_the_recorded_decisions():
    """Every size query over its axes, and the code each launching entry point returns for invalid arguments: single faults, pairs that pin
    the precedence, refused dtype codes.  Nothing here launches: only cases recorded as argument faults are called."""
    import tav_amd  # noqa: F401
    from tav_amd import _lib
    h = _lib.lib()
    axes, got = G.query_axes(), G.query_rows(h)
    assert list(got) == list(golden()["size_queries"])
    for name, want in golden()["size_queries"].items():
        assert len(axes[name]) == len(want) == len(got[name])
        for case, a, b in zip(axes[name], got[name], want):
            assert a == b, f"{name}{case}: {a}, recorded {b}"
    launching = {e for e, _, _ in G.ENTRIES} | {"tav_ln_param_reduce_multi"}
    for hand in (False, True):
        rows = golden()["refused_before_launch_by_hand" if hand else "invalid_arguments"]
        recorded = {(e, n): rc for e, n, rc in rows}
        cases = G.invalid_cases(h, hand=hand)
        assert len(recorded) == len(cases) == len(rows)
        for entry, name, thunk in cases:
            want_rc = recorded[(entry, name)]
            assert want_rc in (-1, -2, -3, -4)               # an argument fault, refused before the launch: only then is the call made
            assert thunk() == want_rc, f"{entry} [{name}]"
        assert {e for e, _, _ in cases} <= launching
    assert {e for e, _, _ in G.invalid_cases(h)} == launching
    # every entry point of the library is either a GEMM one (tests/test_gemm_plan_host.py), a query, a collective, or in the table
    others = {"tav_version", "tav_error_string", "tav_gemm_nt", "tav_gemm_nt_schedule", "tav_gemm_tn_splits", "tav_gemm_tn", "tav_gemm_tn_grouped",
              "tav_gemm_tn_grouped_ws_bytes", "tav_gemm_tn_grouped_ws", "tav_colsum", "tav_comm_rccl_version", "tav_comm_unique_id", "tav_comm_init_rank",
              "tav_comm_destroy", "tav_allreduce_bucket"}
    assert launching | set(axes) | others == set(_lib.declared_symbols())


def _recorded_dtypes(entry):
    """The recorded accepted set of an entry as {(code,)} or {(source, destination)}; `floats` for every entry without a list of its own."""
    acc = golden()["accepted_dtypes"]
    return {tuple(c) if isinstance(c, list) else (c,) for c in acc.get(entry, acc["floats"])}


def test_dispatch_lists_accept_what_the_record_says():
    """The dtype cases an enqueue dispatches over (`dtypes<on<...>...>` in the .hip files, `floats` in tavhip_internal.h) against the recorded
    accepted set of its entry point -- the same record the validators are held to in test_header_alone_under_sanitizers: a validator and
    its dispatch cannot drift apart."""
    codes = {"TAV_F32": G.F32, "TAV_BF16": G.BF16, "TAV_FP8": G.FP8, "TAV_U8": G.U8, "TAV_I16": G.I16}
    csrc = os.path.join(ROOT, "multi-modal-emotion_amd", "csrc")

    def cases(text):
        return [tuple(codes[c.strip()] for c in m.split(",")) for m in re.findall(r"on<([^<>]*)>", text)]
    helper = open(os.path.join(csrc, "tavhip_internal.h")).read()
    floats = cases(re.search(r"using floats = dtypes<(.*)>;", helper).group(1))
    assert set(floats) == _recorded_dtypes("floats") and len(floats) == 2
    seen = {}
    for name in sorted(os.listdir(csrc)):
        if not name.endswith(".hip"):
            continue
        src = open(os.path.join(csrc, name)).read()
        for m in re.finditer(r"dtypes<((?:on<[^<>]*>,?\s*)+)>", src):
            entry = re.findall(r'extern "C" int (tav_\w+)\(', src[:m.start()])[-1]
            seen.setdefault(entry, []).append(cases(m.group(1)))
    assert {"tav_cast2d", "tav_group_pad", "tav_video_clip_transform", "tav_audio_resample", "tav_ln_fwd", "tav_ln_bwd"} <= set(seen), sorted(seen)
    for entry, lists in seen.items():
        for lst in lists:
            assert len(set(lst)) == len(lst), entry
            if entry in golden()["accepted_dtypes"]:
                assert set(lst) == _recorded_dtypes(entry), entry
            else:                                            # (x, lp) of tav_ln_fwd, (x, dy) of tav_ln_bwd: every pair of the float codes
                assert set(lst) == {(a, b) for (a,) in _recorded_dtypes("floats") for (b,) in _recorded_dtypes("floats")}, entry


def test_header_alone_under_sanitizers(tmp_path):
    """entry_plan.h built without HIP, with ASan + UBSan, as a program of its own (no sanitizer runtime is loaded into this process), by
    every host compiler of the machine: nothing reported, every invariant holds, its size queries equal the recorded table, and the
    narrowings it finds are the known ones."""
    for cxx, lines in run_alone_under_sanitizers("entry_plan_check.cpp", tmp_path).items():
        got = {ln.split(" :", 1)[0][len("query "):]: [int(v) for v in ln.split(" :", 1)[1].split()] for ln in lines if ln.startswith("query ")}
        assert got == golden()["size_queries"], cxx
        assert {ln[len("finding "):].split(" : ")[0] for ln in lines if ln.startswith("finding ")} == KNOWN_NARROWINGS, cxx
        accepted = [ln[len("accepts "):].split(" :") for ln in lines if ln.startswith("accepts ")]
        assert len(accepted) == 22
        for names, vals in accepted:                        # the validators against the recorded accepted dtype sets
            got = {tuple(int(c) for c in v.split(">")) for v in vals.split()}
            for entry in names.split():
                want = _recorded_dtypes(entry)
                if entry == "tav_ln_bwd":                    # (x, dy): every pair of the float codes
                    want = {(a, b) for (a,) in want for (b,) in want}
                assert got == want, f"{cxx}: {entry} accepts {sorted(got)}, recorded {sorted(want)}"
