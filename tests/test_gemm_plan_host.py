"""CPU: the host decisions of the GEMM entry points (csrc/gemm_plan.h) against the table recorded from the parent of the commit that moved
them out of gemm.hip (tests/golden/gemm_plan_golden.json, made by tests/make_gemm_plan_golden.py), twice: through the built library, and
through the header compiled stand-alone under AddressSanitizer + UndefinedBehaviorSanitizer (tests/host/gemm_plan_check.cpp), which also
checks the invariants of every plan and that the list of gemm_nt_kernel instantiations is exactly what the launch planner can ask for."""
import functools
import itertools
import json
import os
import shutil
import subprocess

import pytest

import make_gemm_plan_golden as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def _host_compiler():
    """(compiler, extra flags): the sanitizer runtimes linked statically (clang's default), so that the program starts whatever the
    environment preloads into every process."""
    for cxx, extra in (("/opt/rocm/llvm/bin/clang++", []), ("clang++", []), ("g++", ["-static-libasan", "-static-libubsan"])):
        path = shutil.which(cxx)
        if path:
            return path, extra
    return None, []


def _expand(rle):
    out = []
    for tok in rle.split():
        n, code = tok.split("*")
        out += [code] * int(n)
    return out


def test_header_alone_under_sanitizers(tmp_path):
    """gemm_plan.h built without HIP, with ASan + UBSan, as a program of its own (no sanitizer runtime is loaded into this process): its
    invariants hold, every kernel key is in the list and every list entry is reached, and its planner lines equal the recorded table."""
    cxx, extra = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (g++ or clang++) on this machine")
    exe = tmp_path / "gemm_plan_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *extra,
                    os.path.join(ROOT, "tests", "host", "gemm_plan_check.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    lines = run.stdout.splitlines()
    failed = [ln for ln in lines if ln.startswith("FAILED")]
    assert run.returncode == 0 and not failed, "\n".join(failed[:20]) + "\n" + run.stderr[-4000:]
    assert lines[-1] == "ok: 0 failed checks"
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
