"""Writes tests/golden/ctc_align_golden.npz: what the reference's own get_trellis / backtrack give for ctc_align_ref.CASES.

    python tests/make_ctc_align_golden.py /path/to/reference

The three definitions (Point, get_trellis, backtrack) are cut out of the reference's run_scripts/get_times.py with `ast` when this runs
and executed with torch alone (the file itself imports torchaudio and pandas, which need not be there); none of their text is kept here
or in the record.  Per case the record holds the emission, the tokens, the path the reference returned (token index, frame, probability as
f32), whether it raised 'Failed to align', and -- for the small cases -- its trellis."""
import ast
import os
import sys

import numpy as np
import torch

import ctc_align_ref as R


def reference_functions(root):
    src = open(os.path.join(root, "run_scripts", "get_times.py")).read()
    tree = ast.parse(src)
    keep = [n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in ("Point", "get_trellis", "backtrack")]
    assert [n.name for n in keep] == ["Point", "get_trellis", "backtrack"]
    from dataclasses import dataclass
    ns = {"torch": torch, "dataclass": dataclass}
    exec(compile(ast.Module(body=keep, type_ignores=[]), "get_times.py", "exec"), ns)
    return ns["get_trellis"], ns["backtrack"]


def main(root):
    get_trellis, backtrack = reference_functions(root)
    out, on_path_ties, tied_maxima, failures = {}, 0, 0, 0
    for name, T, N, V, _ in R.CASES:
        em, tokens = R.case_inputs(name)
        emission = torch.from_numpy(em)
        tr = get_trellis(emission, tokens.tolist())
        try:
            path, failed = backtrack(tr, emission, tokens.tolist()), 0
        except ValueError as e:
            assert str(e) == "Failed to align"
            path, failed = [], 1
        out[name + ".emission"], out[name + ".tokens"] = em, tokens
        out[name + ".path_token"] = np.array([p.token_index for p in path], np.int32)
        out[name + ".path_frame"] = np.array([p.time_index for p in path], np.int32)
        out[name + ".path_prob"] = np.array([p.score for p in path], np.float32)
        out[name + ".failed"] = np.array(failed, np.int32)
        if (T + 1) * (N + 1) <= R.TRELLIS_STORED_UP_TO:
            out[name + ".trellis"] = tr.numpy().astype(np.float32)
        n, tied = R.ties(em, tokens)
        on_path_ties, tied_maxima, failures = on_path_ties + n, tied_maxima + tied, failures + failed
        print(f"{name}: T {T} N {N} V {V} points {len(path)} failed {failed} on-path ties {n} tied maxima {tied}")
    assert on_path_ties and tied_maxima and failures, "the record needs a case of each tie kind and a failing one"
    np.savez_compressed(R.GOLDEN, **out)
    print(f"{R.GOLDEN}: {os.path.getsize(R.GOLDEN)} bytes")


if __name__ == "__main__":
    main(sys.argv[1])
