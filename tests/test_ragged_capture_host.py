"""CPU: ragged video rows at a bucketed capacity (runtime.set_visual_rows("ragged", bucket=g)) -- the capacity arithmetic, the validation of
the switch, the graph-mode signature against stand-in steppers, the CLI flag and the tav_ragged_lens entry point (argument validation only:
nothing is launched without a GPU)."""
import ctypes as C

import pytest
import torch

import tav_amd  # noqa: F401
from tav_amd import _lib, ops, runtime
from tav_amd.models.tav import collate_batch, resolve_visual_caps
from tav_amd.train_model import graphed as G
from tav_amd.utils.global_functions import arg_parse


@pytest.fixture
def bucket4():
    runtime.set_visual_rows("ragged", bucket=4)
    yield
    runtime.set_visual_rows("equal")


def test_capacity_arithmetic():
    cap = runtime.visual_capacities
    # g = 1: the natural sizes, max(nt) and ntok - min(nt)
    assert cap([3, 5, 4, 1], 32, 1) == (5, 31)
    assert cap([104], 1568, 1) == (104, 1464)
    # counts straddling a bucket edge: 64 stays in its bucket, 65 opens the next one; min 63 / 64 likewise
    assert cap([64, 64], 1568, 64) == (64, 1568 - 64)
    assert cap([64, 65], 1568, 64) == (128, 1568 - 64)
    assert cap([63, 64], 1568, 64) == (64, 1568)
    assert cap([78, 127], 1568, 64) == (128, 1504)              # the reference's range of counts: one bucket
    assert cap([78, 129], 1568, 64) == (192, 1504)
    # the clamp at ntok
    assert cap([30, 31], 32, 8) == (32, 32 - 24)
    assert cap([5, 7], 8, 3) == (8, 8 - 3)
    # min(nt) < g: nothing can be taken off the video encoder's rows
    assert cap([3, 5], 32, 8) == (8, 32)
    assert cap([1, 200], 1568, 64) == (256, 1568)
    # the capacities always hold every row
    for nt, ntok, g in [([3, 5, 4, 1], 32, 4), ([17, 9, 31], 32, 5), ([100, 90, 127, 78], 1568, 64)]:
        ct, ck = cap(nt, ntok, g)
        assert max(nt) <= ct <= ntok and ntok - min(nt) <= ck <= ntok
    for bad in ([0, 3], [3, 33], []):
        with pytest.raises(ValueError):
            cap(bad, 32, 4)
    with pytest.raises(ValueError):
        cap([3, 5], 32, 0)
    with pytest.raises(ValueError):
        cap([32, 32], 32, 4)                                     # nothing left for the video encoder


def test_bucket_validation_and_default_off():
    assert runtime.visual_bucket() == 0
    for bad in (-1, 2.0, "4", True):
        with pytest.raises(ValueError):
            runtime.set_visual_rows("ragged", bucket=bad)
    with pytest.raises(ValueError):
        runtime.set_visual_rows("equal", bucket=4)
    assert runtime.visual_rows() == "equal" and runtime.visual_bucket() == 0          # a refused call changes nothing
    try:
        for off in (None, 0):
            runtime.set_visual_rows("ragged", bucket=off)
            assert runtime.visual_rows() == "ragged" and runtime.visual_bucket() == 0
        runtime.set_visual_rows("ragged", bucket=64)
        assert runtime.visual_bucket() == 64
        runtime.set_visual_rows("ragged")                                             # today's call: today's behaviour
        assert runtime.visual_bucket() == 0
        runtime.set_visual_rows("ragged", bucket=8)
    finally:
        runtime.set_visual_rows("equal")
    assert runtime.visual_bucket() == 0


def test_collate_accepts_the_bucket_and_draws_the_same():
    g = torch.Generator().manual_seed(0)
    items = [([{"input_ids": torch.arange(8), "attention_mask": torch.ones(8)}, torch.randn(400 + 10 * b, generator=g),
               torch.randn(16, 3, 32, 32, generator=g)], b % 7) for b in range(4)]
    torch.manual_seed(1)
    (_, _, v0), _ = collate_batch(items, "train", visual_rows="ragged")
    torch.manual_seed(1)
    (_, _, v1), _ = collate_batch(items, "train", visual_rows="ragged", bucket=8)
    assert torch.equal(v0["attention_mask"], v1["attention_mask"])
    with pytest.raises(ValueError):
        collate_batch(items, "train", visual_rows="equal", bucket=8)
    with pytest.raises(ValueError):
        collate_batch(items, "train", visual_rows="ragged", bucket=-8)


def test_capacities_resolve_from_counts_bucket_or_caller(bucket4):
    m = torch.zeros(2, 32, dtype=torch.bool)
    m[0, :3], m[1, :5] = True, True
    assert resolve_visual_caps(m) == (8, 32)                     # counted from the mask
    assert resolve_visual_caps(m, [6, 7]) == (8, 28)             # counts given: no read
    assert resolve_visual_caps(m, 4) == (4, 28)                  # equal rows take the same path
    assert resolve_visual_caps(m, None, (12, 30)) == (12, 30)    # explicit capacities win
    with pytest.raises(ValueError):
        resolve_visual_caps(m, None, (0, 30))
    with pytest.raises(ValueError):
        resolve_visual_caps(m, None, (12, 33))
    runtime.set_visual_rows("ragged")
    assert resolve_visual_caps(m) is None and resolve_visual_caps(m, [3, 5]) is None


# ---------------------------------------------------------------------------------------------- the signature, against stand-ins
class _Opt:
    generation = 0


class _Crit:
    epoch_switch = 2


class _Stepper:
    reducer = None

    def __init__(self):
        self.opt, self.criterion, self.model, self.pre = _Opt(), _Crit(), None, None


def _batch(counts, ntok=32, given=False):
    B = len(counts)
    vm = torch.zeros(B, ntok, dtype=torch.bool)
    for b, n in enumerate(counts):
        vm[b, torch.randperm(ntok)[:n]] = True
    vis = {"visual_embeds": torch.zeros(B, 16, 3, 32, 32), "attention_mask": vm}
    if given:
        vis["n_visual_true"] = list(counts)
    return ([{"input_ids": torch.zeros(B, 16, dtype=torch.int64), "attention_mask": torch.ones(B, 16)},
             {"audio_features": torch.zeros(B, 800), "attention_mask": torch.ones(B, 800)}, vis], torch.zeros(B))


def test_signature_is_shared_inside_a_bucket(bucket4):
    gs = G.GraphedSteps(_Stepper())
    a = gs.signature(*_batch([5, 7]), 0, False)
    b = gs.signature(*_batch([6, 8]), 0, False)
    c = gs.signature(*_batch([7, 5]), 0, False)
    assert a is not None and a == b == c
    assert a[2] == ("ragged", 8, 28)
    # equal rows inside the bucket: the same signature, hence the same (padded) path
    assert gs.signature(*_batch([6, 6]), 0, False) == a
    # the counts the collate supplied stand for the mask's (no read), and the list does not enter the shapes
    assert gs.signature(*_batch([6, 8], given=True), 0, False) == a
    # another bucket on either side, another loop kind, another epoch branch: other signatures
    assert gs.signature(*_batch([5, 9]), 0, False)[2] == ("ragged", 12, 28)
    assert gs.signature(*_batch([3, 7]), 0, False)[2] == ("ragged", 8, 32)
    assert gs.signature(*_batch([5, 7]), 0, True) != a and gs.signature(*_batch([5, 7]), 1, False) != a
    assert len({gs.signature(*_batch(c), 0, False) for c in ([5, 7], [5, 9], [3, 7])}) == 3


def test_signature_without_a_bucket_is_as_before():
    gs = G.GraphedSteps(_Stepper())
    runtime.set_visual_rows("ragged")
    try:
        assert gs.signature(*_batch([5, 7]), 0, False) is None
        assert gs.signature(*_batch([6, 6]), 0, False)[2] == 6
    finally:
        runtime.set_visual_rows("equal")
    assert gs.signature(*_batch([5, 7]), 0, False) is None
    assert gs.signature(*_batch([6, 6]), 0, False)[2] == 6


def test_graphed_step_replays_ragged_batches_of_one_bucket(monkeypatch, bucket4):
    """Host schedule with stand-ins: first batch of the bucket eager (with the counts the signature used) then captured FROM THE CAPACITIES,
    later batches of the bucket replayed, a batch of another bucket eager when the cache is full."""
    from tav_amd.train_model import tav_train as T
    calls = []

    class Loss:
        def item(self):
            return 1.0

        def backward(self):
            calls.append("backward")

    class Graph:
        loss, logits, label, status = torch.tensor(0.5), torch.zeros(2, 7), torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int32)

        def feed(self, input, label):
            calls.append("feed")

        def replay(self):
            calls.append("replay")

        def release(self):
            pass
    st = _Stepper()
    st.update = lambda clip=True: calls.append("update")
    st.opt.sync_lr = lambda: None
    monkeypatch.setattr(T, "get_statistics", lambda input, label, *a, **k: (calls.append(("eager", k.get("n_visual_true"))), Loss())[1])
    monkeypatch.setattr(G.GraphedSteps, "_capture", lambda self, input, label, epoch, accum, nv: (calls.append(("capture", nv)), Graph())[1])
    gs = G.GraphedSteps(st, max_graphs=1)
    for counts in ([5, 7], [6, 8], [7, 5], [5, 9], [8, 6]):
        gs.step(*_batch(counts), 0, None)
    assert calls == [("eager", [5, 7]), "backward", "update", ("capture", ("ragged", 8, 28)),
                     "feed", "replay", "feed", "replay",
                     ("eager", [5, 9]), "backward", "update",
                     "feed", "replay"]
    assert (gs.eager_steps, gs.captures, gs.replays) == (2, 1, 3)
    Graph.status = torch.ones(1, dtype=torch.int32)                  # the safety net: a status word left by a replay is an error
    with pytest.raises(ValueError, match="capacit"):
        gs.step(*_batch([6, 6]), 0, None)


def test_visual_bucket_flag_parses():
    assert arg_parse("TAV", []).visual_bucket == 0 and arg_parse("TAV", []).visual_rows == "equal"
    a = arg_parse("TAV", ["--visual-rows", "ragged", "--visual-bucket", "64"])
    assert (a.visual_rows, a.visual_bucket) == ("ragged", 64)
    with pytest.raises(SystemExit):
        arg_parse("TAV", ["--visual-bucket", "many"])
    with pytest.raises(ValueError):                                   # what tav_nn.main does with the pair
        runtime.set_visual_rows(arg_parse("TAV", ["--visual-bucket", "64"]).visual_rows, bucket=64)
    assert runtime.visual_bucket() == 0


def test_ragged_lens_symbol_and_argument_validation():
    h = _lib.lib()
    assert hasattr(h, "tav_ragged_lens") and "tav_ragged_lens" in _lib.declared_symbols()
    assert h.tav_version() == _lib.ABI_VERSION == 7
    assert (ops.RAGGED_OVER_TRUE, ops.RAGGED_OVER_KEEP) == (1, 2) and callable(ops.ragged_lens)
    f = h.tav_ragged_lens
    p = [C.c_void_p(4096 * (i + 1)) for i in range(5)]            # never dereferenced: every call below is rejected first
    for i in range(5):
        q = list(p)
        q[i] = None
        assert f(*q, 2, 32, 8, 28, 40, None) == -1
    for B, ntok, ct, ck, base in [(0, 32, 8, 28, 40), (-1, 32, 8, 28, 40), (2, 0, 8, 28, 40), (2, 32, 0, 28, 40), (2, 32, 33, 28, 40),
                                  (2, 32, 8, 0, 40), (2, 32, 8, 33, 40), (2, 32, 8, -3, 40), (2, 32, 8, 28, -1)]:
        assert f(*p, B, ntok, ct, ck, base, None) == -2, (B, ntok, ct, ck, base)
