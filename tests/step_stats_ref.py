"""numpy reference of tav_step_stats (include/tavhip.h): the prediction of a logits row is torch.argmax's -- the first index of the maximal
value, a NaN counting as greater than everything -- the confusion matrix is int64 bins over the rows whose target and prediction lie in
[0, C), and the loop accumulator is updated in call order with a double running sum.  Shared by the host and the GPU tests, which also take
their inputs from make_case()."""
import numpy as np

BATCHES = [1, 2, 7, 63, 64, 65, 255, 256, 257, 1000]         # under a wave, a wave, the workgroup size +-1, several passes
CLASSES = [1, 2, 7, 64]


def argmax_rows(logits):
    """int64 [B]: per row the first NaN if there is one, else the first maximum."""
    z = np.asarray(logits, dtype=np.float32)
    out = np.empty(z.shape[0], dtype=np.int64)
    for r, row in enumerate(z):
        nan = np.isnan(row)
        out[r] = int(np.flatnonzero(nan)[0]) if nan.any() else int(np.flatnonzero(row == row.max())[0])
    return out


def new_acc():
    return dict(loss_sum=0.0, steps=0, rows=0, nonfinite=0, bad_rows=0, status=0, first_bad_step=-1)


def step(C, target, logits=None, preds=None, cm=None, loss=None, status=None, acc=None):
    """One call.  cm (int64 [C, C] or None) and acc (new_acc() dict or None) are updated in place."""
    assert (logits is None) != (preds is None)
    target = np.asarray(target, dtype=np.int64)
    pred = argmax_rows(logits) if logits is not None else np.asarray(preds, dtype=np.int64)
    ok = (target >= 0) & (target < C) & (pred >= 0) & (pred < C)
    if cm is not None:
        np.add.at(cm, (target[ok], pred[ok]), 1)
    if acc is not None:
        if loss is not None:
            v = float(np.float32(loss))
            acc["loss_sum"] = acc["loss_sum"] + v              # Python float = IEEE double, one add per call
            acc["nonfinite"] += int(not np.isfinite(v))
        if status is not None and int(status):
            if acc["first_bad_step"] < 0:
                acc["first_bad_step"] = acc["steps"]
            acc["status"] |= int(status)
        acc["steps"] += 1
        acc["rows"] += len(target)
        acc["bad_rows"] += int((~ok).sum())


def special_rows(C):
    """The rows every case carries (float32 [7, C]): all logits equal, the maximum repeated, the maximum in the last column, -inf everywhere,
    a +inf, one NaN, two NaNs (the first NaN must win, also over a +inf before it)."""
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    base = (np.arange(C, dtype=np.float32) % 5) * np.float32(0.25) - np.float32(0.5)
    equal = np.full(C, 0.75, np.float32)
    repeated = base.copy()
    repeated[[C // 3, C - 1]] = 3.0
    last = base.copy()
    last[C - 1] = 9.0
    ninf = np.full(C, -inf, np.float32)
    pinf = base.copy()
    pinf[C // 2] = inf
    one_nan = base.copy()
    one_nan[0] = inf
    one_nan[C - 1] = nan
    two_nan = base.copy()
    two_nan[C // 2] = nan
    two_nan[C - 1] = nan
    return np.stack([equal, repeated, last, ninf, pinf, one_nan, two_nan])


def make_case(B, C, seed=0):
    """-> (logits float32 [B, C], target int64 [B]): random rows on a coarse grid (so that maxima repeat) with special_rows(C) in rows
    0, 9, 18, ... in turn, and targets over [0, C) with -1 in rows 3, 14, 25, ... and C in rows 5, 16, 27, ..."""
    rng = np.random.default_rng(1000 * B + C + seed)
    logits = (rng.integers(-4, 5, size=(B, C)) * 0.5).astype(np.float32)
    sp = special_rows(C)
    for k, r in enumerate(range(0, B, 9)):
        logits[r] = sp[(k + B) % len(sp)]
    target = rng.integers(0, C, size=B).astype(np.int64)
    target[3::11] = -1
    target[5::11] = C
    return logits, target
