"""Process-wide execution context: precision policy + weight-operand cache (one per process = one per GPU)."""
from . import engine

_ctx = None


def set_precision(policy="bf16"):
    """'bf16' (bf16 operands / f32 accumulate, the benchmarked mode), 'fp32' (exact-f32 MFMA, parity mode), one of the 'fp8*' names, or an
    engine.Policy built by the caller (e.g. Policy("fp8", fp8_fwd=1): an fp8 policy with its own e4m3 masks)."""
    global _ctx
    _ctx = engine.Ctx(policy)
    return _ctx


def ctx():
    global _ctx
    if _ctx is None:
        _ctx = engine.Ctx("bf16")
    return _ctx


def precision():
    return ctx().pol.name


# ---- visual rows: "equal" (every row of a batch keeps the same number of video tokens; unequal rows raise ValueError) or "ragged"
# (each utterance keeps its own count: the video and fusion stacks run on padded rows with per-row lengths)
_visual_rows = ["equal"]
# ragged rows at a bucketed capacity (opt-in): with a bucket g > 0 the two shapes a ragged batch gives the step -- the video segment of the
# fusion rows and the row length of the video encoder -- are rounded outwards to multiples of g (visual_capacities), so batches whose counts
# fall into the same bucket share their shapes (and a captured graph, train_model/graphed.py); the counts themselves live on the device.
_visual_bucket = [0]


def check_visual_rows(mode, bucket=None):
    """Validate a (mode, bucket) pair -> the bucket as an int (0: off).  Shared by set_visual_rows, the collate functions and the CLI."""
    if mode not in ("equal", "ragged"):
        raise ValueError(f"visual rows must be 'equal' or 'ragged', got {mode!r}")
    if bucket is None:
        bucket = 0
    if isinstance(bucket, bool) or not isinstance(bucket, int) or bucket < 0:
        raise ValueError(f"visual rows: bucket must be a positive int (None or 0: off), got {bucket!r}")
    if bucket and mode != "ragged":
        raise ValueError("visual rows: a bucket only applies to 'ragged' rows")
    return bucket


def set_visual_rows(mode="equal", bucket=None):
    """bucket (ragged only): a positive int rounds the padded sizes to multiples of it; None or 0 = natural sizes (max / min of the batch)."""
    _visual_bucket[0] = check_visual_rows(mode, bucket)
    _visual_rows[0] = mode
    return mode


def visual_rows():
    return _visual_rows[0]


def visual_bucket():
    """The bucket of ragged rows (0: off)."""
    return _visual_bucket[0] if _visual_rows[0] == "ragged" else 0


def visual_capacities(nt, ntok, g):
    """(cap_true, cap_keep) of a batch whose rows keep `nt` True tokens of `ntok`, for bucket g >= 1:
      cap_true = min(ntok, ceil(max(nt) / g) * g)    video segment of the fusion rows (PreFormer)
      cap_keep = ntok - floor(min(nt) / g) * g       row length of the video encoder
    g = 1 gives the natural sizes max(nt) and ntok - min(nt).  Every row needs at least one True token (the device check of
    tav_ragged_lens refuses such a row too) and the video encoder at least one token to keep."""
    nt = [int(c) for c in nt]
    ntok, g = int(ntok), int(g)
    if g < 1:
        raise ValueError(f"visual_capacities: bucket must be >= 1, got {g}")
    if not nt or min(nt) < 1 or max(nt) > ntok:
        raise ValueError(f"visual_capacities: every row must keep between 1 and {ntok} True tokens, got {nt}")
    cap_true = min(ntok, -(-max(nt) // g) * g)
    cap_keep = ntok - (min(nt) // g) * g
    if cap_keep < 1:
        raise ValueError(f"visual_capacities: every row is all True ({ntok} tokens): the video encoder keeps nothing")
    return cap_true, cap_keep


# ---- SpecAugment sampler (PreFormer._mask_hidden_states, train=True only):
#   "torch"      spans drawn with torch ops on the device from torch's generator (the default; also runs on CPU tensors)
#   "device"     spans drawn by tav_specaug_draw from the dropout seed words (dropout_seeds): the k-th training forward of a PreFormer draws the
#                same masks whether it ran eagerly or as a graph replay; applied and differentiated by engine.SpecAugFn
#   "reference"  spans drawn on the host from numpy's global generator by HF _compute_mask_indices, as the reference does; same SpecAugFn.
#                Reads the host, so it cannot be captured into a hipGraph
SPECAUGMENT_MODES = ("torch", "device", "reference")
_specaugment = ["torch"]


def check_specaugment(mode):
    if mode not in SPECAUGMENT_MODES:
        raise ValueError(f"specaugment must be one of {SPECAUGMENT_MODES}, got {mode!r}")
    return mode


def set_specaugment(mode="torch"):
    _specaugment[0] = check_specaugment(mode)
    return mode


def specaugment():
    return _specaugment[0]


# ---- branch streams: text / audio / video encoders run beside the fusion encoder (reference models/tav.py:476-487 are
# four independent sub-graphs that meet only at the concat, :495).  Autograd replays each branch's backward on the stream its
# forward used, so the backward overlaps the same way; under hipGraph capture the fork/join becomes parallel graph branches.
_streams = {}
_inputs_event = [None]
multistream = [True]


def branch_streams(n=3):
    """(audio, video, text) streams.  All at the default priority: a high-priority video stream broke the overlap under graph replay
    (measured: 55 vs 37.7 ms)."""
    import torch
    dev = torch.cuda.current_device()
    if dev not in _streams:
        _streams[dev] = [torch.cuda.Stream(device=dev) for _ in range(n)]
    _register_branches(_streams[dev])
    return _streams[dev]


# ---- capture guard.  Round 3 lost a run to a core dump (`hipStreamEndCapture` inside torch/cuda/graphs.py capture_end, ROCm 7.2): while a
# stream capture is in progress, a dependency edge between a BRANCH stream and any stream other than the capture's ORIGIN -- branch to
# branch, or to a stream the capture never forked -- builds a graph the runtime crashes on when the capture ends.  The legal topology is a
# star: a branch forks from the origin (waits for an event recorded there) and is joined by the origin (origin waits for the branch).
# Every cross-stream dependency of this package goes through stream_wait(); captures go through capture(); while one is active an illegal
# edge raises RuntimeError naming the two streams instead of producing that graph.  Pure host logic (stream identity only): tested on the CPU.
_capture = None          # {"origin": stream, "branches": [streams handed out or forked while the capture is active]}


def _same(a, b):
    return a is b or a == b


def _register_branches(streams):
    if _capture is not None:
        for st in streams:
            if not _same(st, _capture["origin"]) and not any(_same(st, b) for b in _capture["branches"]):
                _capture["branches"].append(st)


def capture_active():
    return _capture is not None


def check_edge(waiter, producer):
    """Raise if `waiter` waiting for `producer` is an edge the capture in progress cannot hold (no-op outside a capture)."""
    if _capture is None or _same(waiter, producer):
        return
    origin, branches = _capture["origin"], _capture["branches"]

    def known(st):
        return _same(st, origin) or any(_same(st, b) for b in branches)
    for st in (waiter, producer):
        if not known(st):
            raise RuntimeError(f"hipGraph capture on {origin}: stream {st} is neither the capture's origin nor one of its registered branches "
                               f"(runtime.branch_streams / fork); a dependency on it ({waiter} waits for {producer}) would crash hipStreamEndCapture")
    if not _same(waiter, origin) and not _same(producer, origin):
        raise RuntimeError(f"hipGraph capture on {origin}: dependency between two branch streams ({waiter} waits for {producer}); under capture every "
                           f"edge must start or end at the origin stream (ROCm 7.2 crashes in hipStreamEndCapture otherwise) -- join through the origin")


def stream_wait(waiter, producer, event=None):
    """`waiter` waits for everything `producer` has been given so far (or for `event`, which was recorded on `producer`).  The one place
    cross-stream dependencies are made, so the capture guard sees them all."""
    check_edge(waiter, producer)
    if event is not None:
        waiter.wait_event(event)
    else:
        waiter.wait_stream(producer)


class capture:
    """`with runtime.capture(graph, stream, **kw):` = torch.cuda.graph(graph, stream=stream, **kw) with the guard above armed: `stream` is the
    origin; streams handed out by branch_streams() inside the block (or passed as `branches=`) are its branches.
    Dropout drawn inside the block reads its seeds from device words that live as long as the graph does (see dropout_seeds): a plain
    graph.replay() repeats the draws that followed the capture, capture.replay() takes fresh ones as eager calls would."""

    def __init__(self, graph, stream, branches=(), **kw):
        import torch
        self._cm = torch.cuda.graph(graph, stream=stream, **kw)
        self.graph = graph
        self._origin, self._branches = stream, list(branches)
        self.seeds = []              # dropout draws the captured work takes, in call order (dropout_seeds)
        self.seed_words = None

    def __enter__(self):
        global _capture
        import torch
        if _capture is not None:
            raise RuntimeError("runtime.capture: a capture is already in progress in this process")
        # allocated BEFORE the capture: a buffer allocated inside it comes from the graph's pool, where memory that earlier nodes of the
        # same graph used is handed out again -- a replay would overwrite the host-written seeds before the dropout kernels read them.
        # A capture that draws nothing (check="val", the optimizer's graphs) hands the buffer on to the next one (__exit__).
        dev = self._origin.device
        words = _spare_words.pop(str(dev), None)
        self.seed_words = words if words is not None else torch.zeros(SEED_WORDS, dtype=torch.int64, device=dev)
        _capture = {"origin": self._origin, "branches": list(self._branches), "seeds": self.seeds, "words": self.seed_words, "used": 0}
        try:
            return self._cm.__enter__()
        except BaseException:
            _capture = None
            raise

    def __exit__(self, *exc):
        global _capture
        import torch
        used = _capture["used"] if _capture is not None else 0
        try:
            return self._cm.__exit__(*exc)
        finally:
            _capture = None
            if used == 0:
                _spare_words[str(self._origin.device)] = self.seed_words
                self.seed_words = None
            elif exc[0] is None:
                # the captured kernels read these words at every replay: they live as long as the graph object, whether or not the caller
                # keeps this capture object, and start out with the seeds of the draws that followed the capture (what a plain
                # graph.replay() then repeats); capture.replay() rewrites them before each replay
                try:
                    self.graph._tav_seed_words = self.seed_words
                except AttributeError:
                    _kept_words.append(self.seed_words)
                with torch.cuda.stream(self._origin):
                    write_seeds(self.seeds, advance=False)

    def advance_seeds(self):
        """Take the dropout draws of one replay: every module that drew under the capture advances its counter as its eager call would
        have, and its device seed words get the seeds of those draws.  Enqueued on the current stream (fill kernels: the value travels
        as a kernel argument, no host staging buffer that a later step could overwrite before the copy ran)."""
        write_seeds(self.seeds, advance=True)

    def replay(self):
        """advance_seeds() + the graph's replay, on the current stream (which must be the stream the graph was captured on)."""
        self.advance_seeds()
        self.graph.replay()


class guard_only:
    """The guard without a hipGraph (CPU tests of the logic; `origin` / branches are any objects with identity)."""

    def __init__(self, origin, branches=()):
        self._origin, self._branches = origin, list(branches)
        self.seeds = []

    def __enter__(self):
        global _capture
        import torch
        _capture = {"origin": self._origin, "branches": list(self._branches), "seeds": self.seeds,
                    "words": torch.empty(SEED_WORDS, dtype=torch.int64), "used": 0}

    def __exit__(self, *exc):
        global _capture
        _capture = None


# ---- dropout seeds.  Every dropout site keeps a per-module call counter k on the host (the heads of TAVForMAE, BertClassifier and the
# text+audio model: `_drop_calls`, one draw per forward; TransformerEncoder: `_calls`, one draw per layer) and draw k uses the seed
# initial_seed + GOLDEN * k.  Eager, the counter advances and the seed goes to the kernel by value.  Under a capture the counter does NOT
# advance (the capture runs nothing); the site draws from device words instead and is recorded on the capture, whose advance_seeds()
# -- called before each replay -- advances the counter and writes the words.  So the k-th forward call of a module gets the same masks
# whether call k ran eagerly or as a replay, in any interleaving of the two.
GOLDEN = 0x9E3779B97F4A7C15
_U64 = 0xFFFFFFFFFFFFFFFF
SEED_WORDS = 256             # device seed words per capture (one per dropout draw the captured work takes)
_spare_words = {}            # device -> a seed-word buffer no graph reads (left by a capture that drew nothing)
_kept_words = []             # seed words of graphs that take no attributes: kept for the life of the process


def dropout_seed(k):
    """Seed of a module's k-th draw (1-based)."""
    import torch
    return (torch.initial_seed() + GOLDEN * k) & _U64


def _as_i64(v):
    return v - (1 << 64) if v >= (1 << 63) else v


def dropout_seeds(owner, attr, n=1, draw=True):
    """Seeds of the next `n` draws of `owner` (counter attribute `attr`).  Outside a capture: advances the counter by n and returns n ints.
    Under a capture: leaves the counter alone, records the site on the capture and returns n one-word int64 device tensors (views of the
    capture's seed words) that ops.dropout_fwd reads when the kernel runs -- or n placeholders when `draw` is False (p = 0: the counter still
    has to advance per replay, as it does per eager call, but no kernel reads a seed)."""
    if _capture is None:
        k0 = getattr(owner, attr)
        setattr(owner, attr, k0 + n)
        return [dropout_seed(k0 + j + 1) for j in range(n)]
    words = None
    if draw:
        used = _capture["used"]
        if used + n > _capture["words"].numel():
            raise RuntimeError(f"runtime.capture: more than {SEED_WORDS} dropout draws in one capture (raise runtime.SEED_WORDS)")
        words = _capture["words"][used:used + n]
        _capture["used"] = used + n
    _capture["seeds"].append((owner, attr, n, words))
    return [words[j:j + 1] for j in range(n)] if draw else [0] * n


def write_seeds(sites, advance=True):
    """Write the seeds of every recorded site's next draws into its words; advance=True also moves the counters past them (a replay takes
    those draws), advance=False only initialises the words (end of a capture)."""
    for owner, attr, n, words in sites:
        k0 = getattr(owner, attr)
        if advance:
            setattr(owner, attr, k0 + n)
        if words is not None:
            for j in range(n):
                words[j:j + 1].fill_(_as_i64(dropout_seed(k0 + j + 1)))


def advance_seeds(sites):
    write_seeds(sites, advance=True)


def share_with(stream, *tensors):
    """Tensors allocated under the caller's stream (e.g. a batch just shipped to the device) that a branch stream will read, also in its
    backward: tell the caching allocator, or the block is handed out again on the caller's stream the moment the last reference dies on
    the HOST -- while the branch's kernels that read it may not have run yet (found as a wrong conv0 weight gradient at full size)."""
    for t in tensors:
        if t is not None and t.is_cuda:
            t.record_stream(stream)


def mark_inputs_ready():
    """Record 'the batch is resident' on the current stream (called at the start of PreFormer.forward): the encoder branches of
    TAVForMAE wait for this event only, not for PreFormer's own kernels."""
    import torch
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream())
    _inputs_event[0] = ev
    return ev


def take_inputs_event():
    ev, _inputs_event[0] = _inputs_event[0], None
    return ev


# ---- backward segments (ddp.GraphedStep): while a recorder is active every encoder stack reports the residual-stream tensor that
# enters chosen layers; the data-parallel step cuts its backward there so that the gradients of the upper layers can travel over xGMI
# while the lower layers are still being differentiated.
_cut_rec = None
CUT_FRACTIONS = (1.0 / 12.0, 1.0 / 3.0, 2.0 / 3.0)      # of a stack's depth: the lowest segment (front-ends, embeddings, first layer) stays light


def begin_cuts(fractions=CUT_FRACTIONS):
    global _cut_rec
    _cut_rec = {"fractions": tuple(fractions), "pts": {}}


def end_cuts():
    """-> {branch: [(x, x_cut) in forward order]}: x belongs to the graph below the cut, x_cut (a detached leaf) starts the graph above."""
    global _cut_rec
    rec, _cut_rec = _cut_rec, None
    return rec["pts"] if rec is not None else {}


def cut_point(branch, i, L, x):
    """Called by an encoder stack before its layer i (of L) with the f32 residual stream entering that layer; returns the tensor the
    stack continues with.  Without a recorder that is x itself.  With one, at the chosen depths, it is a DETACHED leaf: the autograd
    graph is physically cut there (the engine cannot be told to stop at an interior node -- it walks through it whenever a requested
    leaf is also reachable underneath), and ddp.SegmentedBackward chains the pieces by handing x_cut's gradient to x."""
    if _cut_rec is None or i == 0 or not x.requires_grad:
        return x
    marks = sorted({min(L - 1, max(1, int(round(f * L)))) for f in _cut_rec["fractions"]})
    if i not in marks:
        return x
    xc = x.detach().requires_grad_(True)
    _cut_rec["pts"].setdefault(branch, []).append((x, xc))
    return xc


# ---- gradient arena (ddp.GraphedStep): while a data-parallel step is being captured, the weight-gradient kernels of a transformer layer
# write straight into the bucket that will be all-reduced, so that bucket needs no pack copy.  `grad_slots` maps parameter.data_ptr() -> its f32
# view inside the bucket (the backward sees the parameters as unpacked saved tensors: other Python objects, same storage); `layer_groups` collects, during the forward, the parameter tuples whose gradients one grouped launch produces
# (wq, wk, wv share ONE fused [3H, K] output, so their views must be adjacent and in that order).
grad_slots = {}
layer_groups = None


def begin_layer_groups():
    global layer_groups
    layer_groups = []


def end_layer_groups():
    global layer_groups
    g, layer_groups = layer_groups, None
    return g or []


def note_layer_group(wq, wk, wv, bq, bk, bv, wo, bo, w1, b1, w2, b2):
    if layer_groups is not None:
        layer_groups.append((wq, wk, wv, bq, bk, bv, wo, bo, w1, b1, w2, b2))


def fused_slot(params):
    """The arena views of `params` as ONE contiguous tensor [sum of rows, ...] if every one has a slot and they are adjacent in this order."""
    views = [grad_slots.get(p.data_ptr()) if p is not None else None for p in params]
    if any(v is None for v in views):
        return None
    ptr = views[0].data_ptr()
    for v in views:
        if v.data_ptr() != ptr:
            return None
        ptr += v.numel() * 4
    base = views[0]
    rows = sum(v.shape[0] for v in views)
    return base.as_strided((rows,) + tuple(base.shape[1:]), base.stride())
