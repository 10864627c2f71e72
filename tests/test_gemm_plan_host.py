"""CPU: the host decisions of the GEMM entry points (csrc/gemm_plan.h) against the table recorded from the parent of the commit that moved
them out of gemm.hip (tests/golden/gemm_plan_golden.json, made by tests/make_gemm_plan_golden.py), twice: through the built library, and
through the header compiled stand-alone under AddressSanitizer + UndefinedBehaviorSanitizer (tests/host/gemm_plan_check.cpp, built and
run by tests/host_program.py), which also checks the invariants of every plan and that the list of gemm_nt_kernel instantiations is
exactly what the launch planner can ask for."""
import functools
import itertools
import json

import make_gemm_plan_golden as G
from host_program import run_alone_under_sanitizers


@functools.lru_cache(maxsize=None)
def golden():
    with open(G.GOLDEN) as f:
        doc = json.load(f)
    assert len(doc["recorded_from_commit"]) == 40
    return doc


@functools.lru_cache(maxsize=None)
def golden_schedule():
    return G.unpack(golden()["nt_schedule"])


def test_library_reproduces_the_recorded_decisions():
    """Every row: tav_gemm_nt_schedule over the full cross product, tav_gemm_tn_splits, tav_gemm_tn_grouped_ws_bytes, and the code each launching
    entry point returns for invalid arguments (single faults, and pairs that pin the precedence).  Nothing here launches."""
    import tav_amd  # noqa: F401
    from tav_amd import _lib
    h = _lib.lib()
    want, got = golden_schedule(), G.nt_schedule_rows(h)
    assert len(got) == len(want) == golden()["nt_schedule"]["count"]
    bad = [k for k, (a, b) in enumerate(zip(got, want)) if a != b]
    assert not bad, f"{len(bad)} schedule rows differ; first: {G.nt_case_of_row(bad[0])} -> {got[bad[0]]}, recorded {want[bad[0]]}"
    axes = list(itertools.product(G.TN_N, G.TN_N, G.TN_ROWS, G.TN_NBATCH))
    got = G.tn_splits_rows(h)
    assert len(got) == len(golden()["tn_splits"]) == len(axes)
    for case, a, b in zip(axes, got, golden()["tn_splits"]):
        assert a == b, f"tav_gemm_tn_splits{case}: {a}, recorded {b}"
    axes = list(itertools.product(G.WS_SHAPES, (1, 2, 3, 4), G.WS_ROWS, (G.BF16, G.F32), G.WS_FLAGS, (True, False)))
    got = G.ws_bytes_rows(h)
    assert len(got) == len(golden()["tn_grouped_ws_bytes"]) == len(axes)
    for case, a, b in zip(axes, got, golden()["tn_grouped_ws_bytes"]):
        assert a == b, f"tav_gemm_tn_grouped_ws_bytes{case}: {a}, recorded {b}"
    recorded = {(e, n): rc for e, n, rc in golden()["invalid_arguments"]}
    cases = G.invalid_cases(h)
    assert len(recorded) == len(cases) == len(golden()["invalid_arguments"])
    for entry, name, thunk in cases:
        want_rc = recorded[(entry, name)]
        assert want_rc in (-1, -2, -3, -4)                   # an argument fault, refused before the launch: only then is the call made
        assert thunk() == want_rc, f"{entry} [{name}]"
    assert {e for e, _, _ in cases} == {"tav_gemm_nt", "tav_gemm_tn", "tav_gemm_tn_grouped", "tav_gemm_tn_grouped_ws", "tav_colsum"}


def _expand(rle):
    out = []
    for tok in rle.split():
        n, code = tok.split("*")
        out += [code] * int(n)
    return out


def test_header_alone_under_sanitizers(tmp_path):
    """gemm_plan.h built without HIP, with ASan + UBSan, as a program of its own (no sanitizer runtime is loaded into this process), by
    every host compiler of the machine: nothing reported, its invariants hold, every kernel key is in the list and every list entry is
    reached, and its planner lines equal the recorded table."""
    for cxx, lines in run_alone_under_sanitizers("gemm_plan_check.cpp", tmp_path).items():
        keys = [ln for ln in lines if ln.startswith("nt_keys ")]
        assert len(keys) == 1 and keys[0].endswith("compiled for nothing: none"), keys

        got = [c for ln in lines if ln.startswith("nt_schedule ") for c in _expand(ln.split(" :", 1)[1])]
        want = golden_schedule()
        assert len(got) == len(want)
        bad = [k for k, (a, b) in enumerate(zip(got, want)) if a != b]
        assert not bad, f"{len(bad)} schedule rows differ; first: {G.nt_case_of_row(bad[0])} -> {got[bad[0]]}, recorded {want[bad[0]]}"
        got = [[int(v) for v in ln.split(" : ")[1].split()] for ln in lines if ln.startswith("tn_splits ")]
        assert got == golden()["tn_splits"]
        got = [int(ln.split(" : ")[1]) for ln in lines if ln.startswith("tn_grouped_ws_bytes ")]
        assert got == golden()["tn_grouped_ws_bytes"]
