"""Host model of the forced-alignment kernels (csrc/ctc_align.hip): our own numpy restatement of the reference's get_trellis / backtrack
(run_scripts/get_times.py) in f32, the outputs tav_ctc_align defines on top of them, and the fp64 log-softmax with its per-element bound.

f32 add and max are correctly rounded on the host and on the device and the recurrence has one order, so the trellis is compared bit for
bit and every `changed > stayed` decision -- hence the path -- element for element.  tests/golden/ctc_align_golden.npz holds what the
reference's own functions gave for CASES (tests/make_ctc_align_golden.py); test_ctc_align_host.py holds this model to that record.

Bounds (u = 2^-24, the unit roundoff of f32; 1 ulp <= 2 u relative):
  path_prob   the device takes expf of the f32 emission the step took.  HIP's math API documents expf with a maximum error of
              EXPF_ULP = 1 ulp, so |kernel - exp64(e)| <= (EXPF_ULP + 0.5) ulp(exp64(e)): the function's error plus the rounding of the
              exact value that 1 ulp is measured from.
  log-softmax y = (x - m) - log(s), s = sum_i exp(x_i - m).  d_i = x_i - m is one rounding (u |d_i|), expf turns it into a relative
              u |d_i| of the term and adds 2 u EXPF_ULP of its own, every term then passes through at most ceil(V / 64) - 1 + 6 additions
              (a lane's ascending partial, six butterfly steps) of u each; logf (LOGF_ULP = 1 ulp documented) adds 2 u LOGF_ULP |log s| to
              the relative error of s, and the final subtraction rounds once more:
                  |kernel - Y| <= u (|d| + sum_i e_i (|d_i| + 2 EXPF_ULP + ceil(V / 64) + 5) / s + 2 LOGF_ULP |log s| + |Y|) (1 + 2^-7)
              where 2^-7 covers the second-order terms (u times at most 104, the largest |d| that does not underflow), plus V 2^-126:
              a term below the f32 normal range may come out as 0, and s >= 1.
"""
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "ctc_align_golden.npz")
U = 2.0 ** -24
EXPF_ULP = 1.0          # HIP math API, "expf": maximum ulp error 1
LOGF_ULP = 1.0          # HIP math API, "logf": maximum ulp error 1

# (name, T, N, V, kind): kind "ls" = log-softmax of random logits, "int" = small non-positive integers (exact ties on the path and tied
# maxima in the last column).  blank_id = 0 throughout: the reference's backtrack reads column 0 for a step that stayed.
CASES = [("t1n1", 1, 1, 4, "ls"), ("t5n5", 5, 5, 4, "ls"), ("t4n5_fails", 4, 5, 4, "ls"), ("t50n7", 50, 7, 29, "ls"), ("t130n65", 130, 65, 32, "ls"),
         ("t300n129", 300, 129, 32, "ls"), ("t40n9_int", 40, 9, 8, "int"), ("t64n64_int", 64, 64, 5, "int"), ("t200n64_int", 200, 64, 29, "int")]
TRELLIS_STORED_UP_TO = 5000        # (T + 1) (N + 1) elements: the record keeps the reference's trellis for the small cases only


def case_inputs(name):
    """(emission f32 [T, V], tokens int32 [N]) of a recorded case: made here, from the case's own seed."""
    idx, (_, T, N, V, kind) = next((i, c) for i, c in enumerate(CASES) if c[0] == name)
    rng = np.random.default_rng(1000 + idx)
    if kind == "ls":
        x = rng.standard_normal((T, V)) * 2.0
        em = (x - np.log(np.exp(x).sum(1, keepdims=True))).astype(np.float32)
    else:
        em = -rng.integers(0, 4, size=(T, V)).astype(np.float32)
    tokens = rng.integers(1, V, size=N).astype(np.int32)
    return em, tokens


def trellis(em, tokens, blank=0):
    em = np.asarray(em, np.float32)
    tok = np.asarray(tokens, np.int64)
    T, N = em.shape[0], len(tok)
    tr = np.full((T + 1, N + 1), -np.inf, np.float32)
    tr[:, 0] = 0
    for t in range(T):
        tr[t + 1, 1:] = np.maximum(tr[t, 1:] + em[t, blank], tr[t, :-1] + em[t, tok])
    return tr


def backtrack(tr, em, tokens, blank=0):
    """-> ([(token index, frame, changed)] in ascending frame order, t_start, failed)."""
    tok = np.asarray(tokens, np.int64)
    j = tr.shape[1] - 1
    t_start = int(np.argmax(tr[:, j]))
    path = []
    for t in range(t_start, 0, -1):
        stayed = tr[t - 1, j] + em[t - 1, blank]
        changed = tr[t - 1, j - 1] + em[t - 1, tok[j - 1]]
        ch = bool(changed > stayed)
        path.append((j - 1, t - 1, ch))
        if ch:
            j -= 1
            if j == 0:
                return path[::-1], t_start, False
    return [], t_start, True


def ties(em, tokens, blank=0):
    """(exact changed == stayed ties on the path, whether the last column's maximum is reached at more than one t)."""
    tr = trellis(em, tokens, blank)
    path, _, failed = backtrack(tr, em, tokens, blank)
    n = 0
    for j, t, _ in path:
        stayed, changed = tr[t, j + 1] + em[t, blank], tr[t, j] + em[t, tokens[j]]
        n += bool(np.isfinite(stayed) and stayed == changed)
    col = tr[:, -1]
    return n, (not failed) and int((col == col.max()).sum()) > 1


def align(em, tokens, V=None, blank=0, Tmax=None, Nmax=None):
    """What tav_ctc_align writes for one utterance, as a dict: trellis [T + 1, N + 1], path_token [Tmax], column [Tmax] (the emission
    column path_prob is the exp of, -1 off the path), seg [Nmax, 2], span [4]."""
    em = np.asarray(em, np.float32)
    T = em.shape[0]
    V = em.shape[1] if V is None else V
    tokens = np.asarray(tokens, np.int64)
    N = len(tokens)
    Tmax, Nmax = T if Tmax is None else Tmax, N if Nmax is None else Nmax
    tok = np.clip(tokens, 0, V - 1)
    status = 2 if (tok != tokens).any() else 0
    tr = trellis(em[:, :V], tok, blank)
    path, t_start, failed = backtrack(tr, em, tok, blank)
    path_token, column = np.full(Tmax, -1, np.int32), np.full(Tmax, -1, np.int64)
    seg = np.full((Nmax, 2), -1, np.int32)
    for j, t, ch in path:
        path_token[t] = j
        column[t] = tok[j] if ch else blank
        if ch:
            seg[j, 0] = t
        seg[j, 1] = t + 1
    span = np.array([-1, -1, 0, status | 1] if failed else [path[0][1], t_start, len(path), status], np.int32)
    return dict(trellis=tr, path_token=path_token, column=column, seg=seg, span=span, failed=failed)


def prob_bounds(em, column):
    """fp64 exp of the taken emissions and the margin of the documented expf error plus one rounding; 0 off the path (exact)."""
    on = column >= 0
    want = np.zeros(len(column), np.float64)
    want[on] = np.exp(np.asarray(em, np.float64)[np.nonzero(on)[0], column[on]])
    ulp = np.spacing(want.astype(np.float32)).astype(np.float64)
    return want, np.where(on, (EXPF_ULP + 0.5) * ulp, 0.0)


def seg_scores(path_prob, seg):
    """The f64 sum of a token's path_prob in ascending frame order / count, rounded once; 0.0 where seg is -1."""
    out = np.zeros(len(seg), np.float32)
    for j, (s, e) in enumerate(seg):
        if s >= 0:
            acc = 0.0
            for t in range(s, e):
                acc += float(path_prob[t])
            out[j] = np.float32(acc / (e - s))
    return out


def log_softmax_bounds(x):
    """fp64 row log-softmax of f32 logits [R, V] and the per-element bound of the module docstring."""
    x = np.asarray(x, np.float32).astype(np.float64)
    V = x.shape[1]
    m = x.max(1, keepdims=True)
    d = x - m
    e = np.exp(d)
    s = e.sum(1, keepdims=True)
    Y = d - np.log(s)
    per_term = np.where(e > 0, np.abs(d) + 2 * EXPF_ULP + math.ceil(V / 64) + 5, 0.0)          # (a -inf logit contributes an exact 0)
    with np.errstate(invalid="ignore"):
        terms = np.where(e > 0, e * per_term, 0.0).sum(1, keepdims=True)
        bound = U * (np.abs(d) + terms / s + 2 * LOGF_ULP * np.abs(np.log(s)) + np.abs(Y)) * (1 + 2.0 ** -7) + V * 2.0 ** -126
    return Y, bound
