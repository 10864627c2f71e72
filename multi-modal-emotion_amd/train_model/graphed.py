"""Graph mode of the TAV training loop (`train_tav_network(..., graphs=True)`): each training batch replays a captured step -- forward,
loss, backward, clip_grad_norm_, AdamW, weight re-casts -- instead of launching its ~3000 kernels one by one from Python.  Results equal the
eager loop's bit for bit.

What is captured: tav_train._statistics (PreFormer + TAVForMAE + criterion, Metric=None) on static input buffers, the division by the dialogue
length (grad_accum) as a multiplication by a device scalar, backward and TrainStep.update().  What runs between replays, on the host:
  * the batch is copied into the static buffers; the dialogue-length scale and the learning rate the scheduler set are written to their device
    words (fill kernels: the value is a kernel argument, no host staging buffer can be overwritten before the device read it);
  * the dropout sites advance their call counters and write the seeds of this replay's draws (runtime.capture.replay);
  * the weight-cast cache is told the parameters moved (engine.bump_weight_epoch), so an eager validate() re-casts;
  * metrics and the running loss are taken from the static logits / loss.  With sync="step" (the default) that is a host sync per step,
    the reference's per-batch loss.item() (plus the read of the ragged status word and the metrics' copy of predictions and labels).  With
    sync="log" it is one ordinary ops.step_stats launch after the replay -- not part of the capture -- that adds the loss to the loop's
    device accumulator, ORs in the status word and counts the predictions into the on-device Metrics' matrix: the host reads nothing
    until the loop logs, so it may run ahead of the device by as many replays as the runtime queues.  (A batch whose video mask lives on
    the device and comes without `n_visual_true` still costs _visual_counts one host read, remembered per tensor: hand the counts over
    with the batch.)
A batch whose signature (input shapes and dtypes, video tokens per row, loss branch, loop kind) has not been seen in this epoch runs the
eager step -- the same code as graphs=False -- and is then captured (at most `max_graphs` per epoch; later new signatures stay eager).
Ragged video rows: without a bucket a batch of unequal rows has no signature and stays eager.  With runtime.set_visual_rows("ragged", bucket=g)
the signature carries ("ragged", cap_true, cap_keep) -- runtime.visual_capacities of the batch's counts -- in place of the per-row count:
the captured step is built from the two capacities alone and reads every length from the mask in its static buffer (ops.ragged_lens), so all
batches whose counts fall into the bucket replay one graph.  The host knows the counts before it replays, so a batch that does not fit never
reaches a graph; the status word the step leaves is read together with the loss all the same.
SpecAugment: in "device" mode the PreFormer's draw is a dropout site like the others (its seed word is rewritten before each replay), so the
replayed step masks what the eager step would have; in "reference" mode the masks come from the host, no batch has a signature and every
training step runs eagerly.
Graphs are freed at the end of every epoch and whenever the optimizer's state was reloaded (load_model builds new moment tensors).
"""
import weakref

import numpy as np
import torch

from .. import engine, runtime
from . import tav_train as T


def _recip32(n):
    """1 / n as torch's CUDA division by a Python scalar computes it (float32 reciprocal, then a multiply): the replay multiplies by this,
    which reproduces the eager `loss / accum_iter` and its backward bit for bit."""
    return float(np.float32(1.0) / np.float32(n))


class _Captured:
    """One captured step and its static tensors."""

    def __init__(self, cap, static_in, static_label, scale, loss, logits, label, status=None):
        self.cap, self.static_in, self.static_label, self.scale = cap, static_in, static_label, scale
        self.loss, self.logits, self.label, self.status = loss, logits, label, status

    def feed(self, input, label):
        for d, sd in zip(input, self.static_in):
            if sd is not None:
                for k, t in sd.items():
                    t.copy_(d[k], non_blocking=True)
        self.static_label.copy_(label, non_blocking=True)

    def set_scale(self, v):
        self.scale.fill_(v)

    def replay(self):
        self.cap.replay()

    def release(self):
        self.cap.graph.reset()
        self.cap = self.static_in = self.static_label = self.scale = self.loss = self.logits = self.label = self.status = None


class GraphedSteps:
    """The training step of not_grad_accum / grad_accum for one TrainStep, replayed from hipGraphs where the batch allows it."""

    def __init__(self, stepper, max_graphs=2):
        if stepper.reducer is not None:
            raise ValueError("train_tav_network(graphs=True) does not support data-parallel training yet (TrainStep has a gradient reducer); "
                             "run with graphs=False, or use ddp.GraphedStep")
        if runtime.ctx().pol.fp8:
            raise ValueError(f"train_tav_network(graphs=True) supports the bf16 and fp32 policies, not {runtime.precision()!r}: the fp8 scale "
                             "roll-over runs on the host after every step")
        self.stepper, self.max_graphs = stepper, max_graphs
        self.graphs = {}
        self._generation = stepper.opt.generation
        self.eager_steps = self.captures = self.replays = 0
        self._nv_seen = {}

    # ---- what makes a batch replayable by a graph
    def _visual_counts(self, input):
        """True video tokens of every row, a host list: the counts the collate put next to the mask (`n_visual_true`) when it did, else
        read from the mask.  A mask on the device costs a host read: remembered per tensor object (weak reference) and version, so
        batches cycled on the device are counted once."""
        given = input[2].get("n_visual_true")
        if given is not None:
            return [int(c) for c in (given.tolist() if torch.is_tensor(given) else given)]
        vm = input[2]["attention_mask"]
        hit = self._nv_seen.get(id(vm))
        if hit is not None and hit[0]() is vm and hit[1] == vm._version:
            return hit[2]
        counts = [int(c) for c in vm.sum(1).cpu().tolist()]
        if vm.is_cuda:
            if len(self._nv_seen) >= 64:
                self._nv_seen.clear()
            self._nv_seen[id(vm)] = (weakref.ref(vm), vm._version, counts)
        return counts

    def _n_visual(self, input):
        """Video tokens per row (every row must keep the same number; None if they differ -- the eager step then raises as it always did,
        or, in ragged mode without a bucket, runs the batch at its natural sizes)."""
        c = self._visual_counts(input)
        return c[0] if c and all(v == c[0] for v in c) else None

    def signature(self, input, label, epoch, accum):
        if runtime.specaugment() == "reference":
            return None                          # the masks are drawn on the host (numpy): training batches run the eager step
        if runtime.visual_bucket():
            # ragged rows at a bucketed capacity: the two padded sizes stand for the counts (equal rows included -- one path per bucket)
            nv = ("ragged",) + runtime.visual_capacities(self._visual_counts(input), input[2]["attention_mask"].shape[1], runtime.visual_bucket())
        else:
            nv = self._n_visual(input)
            if nv is None:
                return None
        crit = self.stepper.criterion
        branch = (epoch % crit.epoch_switch == 0) if hasattr(crit, "epoch_switch") else None      # NewCrossEntropyLoss: weighted or not
        shapes = tuple(None if d is None else tuple((k, tuple(v.shape), v.dtype) for k, v in sorted(d.items()) if torch.is_tensor(v)) for d in input)
        return (shapes, (tuple(label.shape), label.dtype), nv, "train", branch, bool(accum), runtime.specaugment())

    # ---- one training step
    def step(self, input, label, epoch, Metric, accum_iter=None, sync=None):
        """-> the batch loss as a float (what the loops add to total_loss_train).  accum_iter: grad_accum's divisor, None in not_grad_accum.
        sync: the loop's tav_train.LogSync -- loss, status word and metrics go to the device accumulator instead, nothing is read and the
        result is None."""
        if self.stepper.opt.generation != self._generation:
            self.invalidate()                    # optimizer state reloaded: captured pointer tables are stale
        sig = self.signature(input, label, epoch, accum_iter is not None)
        g = self.graphs.get(sig) if sig is not None else None
        kw = {} if sync is None else {"sync": sync}
        if g is not None:
            return self._replay(g, input, label, Metric, accum_iter, **kw)
        v = self._eager(input, label, epoch, Metric, accum_iter, **kw)
        if sig is not None and len(self.graphs) < self.max_graphs:
            self.graphs[sig] = self._capture(input, label, epoch, accum_iter is not None, sig[2])
            self.captures += 1
        return v

    def _eager(self, input, label, epoch, Metric, accum_iter, sync=None):
        """Exactly the eager loop's step (tav_train.not_grad_accum / grad_accum without a reducer)."""
        st = self.stepper
        # (at a bucketed capacity the counts signature() already has go along: the step pads as the eager loop does, without a second host read)
        kw = {"n_visual_true": self._visual_counts(input)} if runtime.visual_bucket() else {}
        if sync is not None:
            loss = T.recorded_loss(sync.train, input, label, st.model, st.pre, st.criterion, Metric, check="train", epoch=epoch,
                                   divide_by=accum_iter, **kw)
            loss.backward()
            st.update()
            self.eager_steps += 1
            return None
        loss = T.get_statistics(input, label, st.model, st.pre, st.criterion, Metric, check="train", epoch=epoch, **kw)
        if accum_iter is not None:
            loss = loss / accum_iter
        v = loss.item()
        T.check_visual_rows(st.model)
        loss.backward()
        st.update()
        self.eager_steps += 1
        return v

    def _replay(self, g, input, label, Metric, accum_iter, sync=None):
        g.feed(input, label)
        if accum_iter is not None:
            g.set_scale(_recip32(accum_iter))
        self.stepper.opt.sync_lr()               # the scheduler moved opt.lr after the last step; the replay reads the device copy
        g.replay()                               # (advances the dropout counters and writes this replay's seeds first)
        engine.bump_weight_epoch()               # the replayed AdamW moved the weights behind the cast cache's back
        if sync is not None:
            # an ordinary launch behind the replay, on the same stream: g.loss is the captured step's loss (already times the scale)
            sync.record(sync.train, Metric, g.logits, g.label, g.loss, getattr(g, "status", None))
            self.replays += 1
            return None
        if Metric is not None:
            Metric.update_metrics(torch.argmax(g.logits, dim=1), g.label)
        self.replays += 1
        v = g.loss.item()
        status = getattr(g, "status", None)
        if status is not None and int(status.item()):        # (cannot happen: signature() sized the capacities from this batch's counts)
            raise ValueError(f"replayed ragged step: a row of the batch did not fit the captured capacities (status {int(status.item())})")
        return v

    def _capture(self, input, label, epoch, accum, n_visual_true):
        """Capture the step on the current stream (the one the loop runs on).  Runs right after an eager step of the same signature: the
        optimizer's moments exist, and the capture itself executes nothing -- no dropout draw, no update is consumed.
        n_visual_true: the signature's entry -- the per-row count, or ("ragged", cap_true, cap_keep): then only the two capacities shape the
        captured step, nothing derived from this batch's own counts."""
        st = self.stepper
        dev = torch.device("cuda", torch.cuda.current_device())
        kw = {"n_visual_true": n_visual_true}
        if isinstance(n_visual_true, tuple):
            kw = {"visual_caps": n_visual_true[1:]}
        static_in = [None if d is None else {k: v.to(dev, copy=True) for k, v in d.items() if torch.is_tensor(v)} for d in input]
        static_label = label.to(dev, copy=True)
        scale = torch.ones((), dtype=torch.float32, device=dev) if accum else None
        st.opt.sync_lr()                         # (so that the captured AdamW records no learning-rate upload of its own)
        engine.bump_weight_epoch()               # the operand casts must be part of the captured step
        graph = torch.cuda.CUDAGraph()
        cap = runtime.capture(graph, torch.cuda.current_stream())
        with cap:
            loss, logits, lab = T._statistics(static_in, static_label, st.model, st.pre, st.criterion, None, check="train", epoch=epoch, **kw)
            status = getattr(st.model, "_visual_status", None)
            if scale is not None:
                loss = loss * scale
            loss.backward()
            st.update()
        st.model._visual_status = None           # (the word belongs to the graph; an eager check must not read a capture's placeholder)
        return _Captured(cap, static_in, static_label, scale, loss.detach(), logits.detach(), lab, status)

    def invalidate(self):
        """Free every captured step (end of an epoch, reloaded optimizer state)."""
        if self.graphs:
            if torch.cuda.is_initialized():
                torch.cuda.synchronize()         # (epoch ends and reloads only) the last replays have finished reading their pinned uploads
            for g in self.graphs.values():
                g.release()
            self.graphs.clear()
            self.stepper.opt.captures_released()
        self._generation = self.stepper.opt.generation


def run_graphed(train_epochs, stepper, model, PREFormer, *args, max_graphs=2, sync="step"):
    """train_tav_network's epochs in graph mode: warm-up, captures, replays, eager fallbacks and validate() all run on ONE side stream (autograd
    ties each parameter's gradient accumulation to the stream of its first backward, and a capture cannot use the legacy default stream)."""
    graphs = GraphedSteps(stepper, max_graphs=max_graphs)
    caller = torch.cuda.current_stream()
    work = torch.cuda.Stream()
    work.wait_stream(caller)
    try:
        with torch.cuda.stream(work):
            return train_epochs(stepper, model, PREFormer, *args, graphs=graphs, sync=sync)
    finally:
        graphs.invalidate()
        caller.wait_stream(work)
