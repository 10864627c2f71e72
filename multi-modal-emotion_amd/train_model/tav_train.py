"""Drop-in for the reference's train_model/tav_train.py: same function names and argument order
(get_statistics :15-48, not_grad_accum :52-83, validate :121-130, one_epoch :133-144, train_tav_network :147-164,
evaluate_tav :166-167), running on libtavhip.  Differences, all forced by the MI355X design:
  * no `assert video.shape == (1,16,3,224,224)` (reference :32 pins batch 1);
  * AdamW + clip_grad_norm_ are the fused multi-tensor kernels of optim.py (identical update rule);
  * wandb / checkpoint paths are optional (no network, no cluster paths);
  * with torch.distributed initialised, gradients are averaged over ranks by ddp.BucketedAllReduce overlapped with backward.
"""
import math
import os

import torch

from .. import ddp as tav_ddp
from .. import ops
from ..optim import FusedAdamW, default_param_groups
from ..utils.global_functions import checkpoint_file, load_model, save_model

try:                                    # optional, as in the reference's environment
    import wandb
except Exception:                       # pragma: no cover
    wandb = None

PATIENCE_ITER = 0


class CosineWarmRestarts:
    """torch CosineAnnealingWarmRestarts(T_0=T_max, T_mult=1, eta_min=0).step(epoch_float) for FusedAdamW: one base learning rate per
    parameter group, every group moved by every step() (an optimizer object without param_groups counts as one group, its `lr`)."""

    def __init__(self, optimizer, T_0):
        self.opt, self.T_0 = optimizer, T_0
        self.base_lrs = self._lrs()

    def _lrs(self):
        groups = getattr(self.opt, "param_groups", None)
        return [self.opt.lr] if groups is None else [g["lr"] for g in groups]

    def _set_lrs(self, lrs):
        groups = getattr(self.opt, "param_groups", None)
        if groups is None:
            self.opt.lr = lrs[0]
            return
        if len(lrs) != len(groups):
            raise ValueError(f"scheduler has {len(lrs)} learning rates, the optimizer {len(groups)} parameter groups")
        for g, lr in zip(groups, lrs):
            g["lr"] = lr

    @property
    def base_lr(self):
        return self.base_lrs[0]

    def step(self, epoch):
        t_cur = epoch % self.T_0
        self._t_cur, self._last_epoch = t_cur, epoch
        self._set_lrs([base_lr * (1 + math.cos(math.pi * t_cur / self.T_0)) / 2 for base_lr in self.base_lrs])

    def get_last_lr(self):
        return self._lrs()

    def state_dict(self):
        """Keys of torch.optim.lr_scheduler.CosineAnnealingWarmRestarts.state_dict() that define the schedule."""
        return {"T_0": self.T_0, "T_i": self.T_0, "T_mult": 1, "eta_min": 0, "T_cur": getattr(self, "_t_cur", 0), "base_lrs": list(self.base_lrs),
                "last_epoch": getattr(self, "_last_epoch", 0), "_last_lr": self._lrs()}

    def load_state_dict(self, sd):
        if len(sd["base_lrs"]) != len(self.base_lrs):
            raise ValueError(f"scheduler state has {len(sd['base_lrs'])} base learning rates, the optimizer {len(self.base_lrs)} parameter groups")
        self.T_0, self.base_lrs = sd["T_0"], list(sd["base_lrs"])
        self._t_cur, self._last_epoch = sd.get("T_cur", 0), sd.get("last_epoch", 0)
        if sd.get("_last_lr"):
            self._set_lrs(list(sd["_last_lr"]))


def get_statistics(input, label, model, PREFormer, criterion, Metric, check="train", epoch=None, n_visual_true=None, visual_caps=None):
    return _statistics(input, label, model, PREFormer, criterion, Metric, check, epoch, n_visual_true, visual_caps)[0]


def check_visual_rows(model):
    """After the step's host sync (loss.item()): a ragged batch run at a bucketed capacity reports rows that did not fit (ValueError)."""
    chk = getattr(model, "check_visual_status", None)
    if chk is not None:
        chk()


def _statistics(input, label, model, PREFormer, criterion, Metric, check="train", epoch=None, n_visual_true=None, visual_caps=None):
    """get_statistics -> (batch loss, logits, labels as int64 on the device): the captured step of graphed.py keeps the last two for the metrics.
    n_visual_true defaults to the per-row counts the collate put next to the mask (collate_batch_device(visual_rows="ragged")), if any;
    visual_caps = (cap_true, cap_keep) fixes the padded sizes of a ragged batch (a captured step: nothing is read from the host)."""
    device = "cuda"
    batch_size = len(label)
    text, audio_features, video_embeds = input[0], input[1], input[2]
    text_input_ids, text_attention_mask = text["input_ids"], text["attention_mask"]
    audio_input_ids, audio_attention_mask = audio_features["audio_features"], audio_features["attention_mask"]
    video_input_ids, video_attention_mask = video_embeds["visual_embeds"], video_embeds["attention_mask"]
    if n_visual_true is None and visual_caps is None:
        n_visual_true = video_embeds.get("n_visual_true")
    caps = {} if visual_caps is None else {"visual_caps": visual_caps}
    tav, tav_embed, attention_mask = PREFormer(input_ids=text_input_ids, audio_features=audio_input_ids, video_embeds=video_input_ids,
                                               text_mask=text_attention_mask, audio_mask=audio_attention_mask, visual_mask=video_attention_mask,
                                               device=device, train=True if check == "train" else False, n_visual_true=n_visual_true, **caps)
    output = model(input_ids=text_input_ids.to(device), text_attention_mask=text_attention_mask.to(device), audio_features=audio_input_ids.to(device),
                   video_embeds=video_input_ids.to(device), visual_mask=video_attention_mask.to(device), hidden_states=tav.to(device),
                   pos_embed=tav_embed.to(device), attention_mask=attention_mask.to(device), batch_size=batch_size, check=check,
                   n_visual_true=n_visual_true, **caps)
    label = label.to(device).long()          # (the reference's .type(torch.LongTensor) would bounce through the host)
    if Metric is not None:
        from_logits = getattr(Metric, "update_from_logits", None)
        if from_logits is not None:
            from_logits(output, label)               # (an on-device Metrics takes the argmax inside its counting kernel)
        else:
            Metric.update_metrics(torch.argmax(output, dim=1), label.long())
    batch_loss = None
    if criterion is not None:
        batch_loss = criterion(output, label, epoch=epoch if epoch is not None else 1)
    return batch_loss, output, label


class LogSync:
    """State of the loops' sync="log" mode: nothing is read from the device per step.  After every step one ops.step_stats launch on the
    loop's stream adds the step's loss scalar to a device accumulator (a double: the sum equals the host's `total += loss.item()` bit for
    bit), ORs in the ragged status word, and counts the step's predictions into the on-device Metrics' confusion matrix.  The loops read
    the accumulator where they log: `train` lives for an epoch, `val` for one validate() call."""

    def __init__(self, Metric, device=None):
        if Metric is not None and not getattr(Metric, "on_device", False):
            raise ValueError('sync="log" needs the confusion matrix on the device: build the metrics with Metrics(..., on_device=True) '
                             '(a host-resident Metrics costs a device-to-host copy per step), or pass Metric=None')
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
        self.train, self.val = ops.loop_acc_new(dev), ops.loop_acc_new(dev)

    @staticmethod
    def record(acc, Metric, logits, label, loss, status=None):
        """The per-step launch: logits f32 [B, C] and label int64 [B] on the device, loss a one-element f32 tensor or None."""
        ops.step_stats(logits=logits.detach(), target=label, cm=None if Metric is None else Metric.cm,
                       loss=None if loss is None else loss.detach().reshape(1), status=status, acc=acc)

    @staticmethod
    def read(acc, what):
        """The accumulator as a dict (the one host read of a logging window), after the checks the per-step reads made in "step" mode."""
        r = ops.loop_acc_read(acc)
        if r["status"]:
            from ..models.tav import STATUS_TEXT
            why = "; ".join(text for bit, text in STATUS_TEXT.items() if r["status"] & bit)
            raise ValueError(f"ragged video rows exceed the batch's capacity (status {r['status']}): {why}; first seen at step "
                             f"{r['first_bad_step']} of this {what} window")
        if r["nonfinite"] or r["bad_rows"]:
            print(f"{what}: {r['nonfinite']} of {r['steps']} steps had a non-finite loss, {r['bad_rows']} of {r['rows']} rows a label or "
                  "prediction outside the classes", flush=True)
        return r


def _as_sync(sync, Metric):
    """"step" -> None, "log" -> a new LogSync; a LogSync passes through (the loops hand theirs to validate)."""
    if sync is None or isinstance(sync, LogSync):
        return sync
    if sync not in ("step", "log"):
        raise ValueError(f'sync must be "step" or "log", got {sync!r}')
    return LogSync(Metric) if sync == "log" else None


def recorded_loss(acc, input, label, model, PREFormer, criterion, Metric, check="train", epoch=None, divide_by=None, **kw):
    """get_statistics for sync="log": the forward with its loss (divided by `divide_by`, grad_accum's dialogue length), then the step_stats
    launch in place of loss.item(), check_visual_rows() and the Metric update.  -> the loss tensor (None without a criterion)."""
    loss, logits, lab = _statistics(input, label, model, PREFormer, criterion, None, check, epoch, **kw)
    if loss is not None and divide_by is not None:
        loss = loss / divide_by
    status = getattr(model, "_visual_status", None)
    if status is not None:
        model._visual_status = None              # (consumed, as check_visual_status does)
    LogSync.record(acc, Metric, logits, lab, loss, status)
    return loss


class TrainStep:
    """One optimisation step of reference :56-65: get_statistics -> backward -> (all-reduce) -> clip_grad_norm_ -> AdamW."""

    def __init__(self, model, PREFormer, criterion, lr=1e-6, weight_decay=1e-4, clip=1.0, bucket_mb=48.0, reduce_dtype=None, zero_grad_like_torch_1_10=False,
                 param_groups=None, encoder_lr_scale=1.0, no_decay_norm_bias=False):
        """param_groups: torch's list of dicts for the optimizer (FusedAdamW); None builds optim.default_param_groups(encoder_lr_scale,
        no_decay_norm_bias) -- with their defaults the flat parameter list, one group, as ever."""
        self.model, self.pre, self.criterion, self.clip = model, PREFormer, criterion, clip
        # what `model.zero_grad()` (reference :64-65, :98-99, :104-105) does to .grad: torch 1.10 -- the version the reference pins,
        # requirements.txt:100 -- zero-FILLS; torch >= 2.0 sets None.  Matters only for grad_accum's second step (see there).
        self.zero_to_none = not zero_grad_like_torch_1_10
        if param_groups is None:
            param_groups = default_param_groups(model, PREFormer, lr, weight_decay, encoder_lr_scale, no_decay_norm_bias)
        elif encoder_lr_scale != 1.0 or no_decay_norm_bias:
            raise ValueError("TrainStep: pass either param_groups or encoder_lr_scale / no_decay_norm_bias, not both")
        self.opt = FusedAdamW(param_groups, lr=lr, weight_decay=weight_decay)
        self.params = self.opt.params                # (flat, in group order: the reducer's buckets and the optimizer walk the same list)
        self.reducer = None
        alone_ok = os.environ.get("TAV_DDP_SINGLE_RANK", "0") == "1"         # exercise the RCCL path with one rank (tests)
        if torch.distributed.is_available() and torch.distributed.is_initialized() and (torch.distributed.get_world_size() > 1 or alone_ok):
            self.reducer = tav_ddp.BucketedAllReduce(self.params, bucket_mb=bucket_mb, reduce_dtype=reduce_dtype, single_rank_ok=alone_ok)

    def forward_loss(self, input, label, check="train", epoch=0, n_visual_true=None):
        return get_statistics(input, label, self.model, self.pre, self.criterion, None, check=check, epoch=epoch, n_visual_true=n_visual_true)

    def forward_backward(self, input, label, check="train", epoch=0, n_visual_true=None):
        loss = self.forward_loss(input, label, check, epoch, n_visual_true)
        loss.backward()
        if self.reducer is not None:
            self.reducer.finish()
        return loss

    def update(self, clip=True):
        norm = self.opt.clip_and_step(self.clip if clip else None)
        self.opt.zero_grad(set_to_none=self.zero_to_none)
        return norm

    def __call__(self, input, label, check="train", epoch=0, n_visual_true=None):
        loss = self.forward_backward(input, label, check, epoch, n_visual_true)
        return loss, self.update()


def validate(val_dataloader, model, PREFormer, criterion, Metric, name="val", sync="step"):
    """sync="log": no host read per batch; loss sum, status word and counts are read once, after the last batch."""
    sync = _as_sync(sync, Metric)
    if sync is not None:
        ops.loop_acc_reset(sync.val)
        with torch.no_grad():
            for val_input, val_label in val_dataloader:
                recorded_loss(sync.val, val_input, val_label, model, PREFormer, criterion, Metric, name, epoch=None)
            total = LogSync.read(sync.val, name)["loss_sum"]
            log(Metric, total / len(val_dataloader) if criterion is not None else 0, name)
        return total / len(val_dataloader)
    total = 0.0
    with torch.no_grad():
        for val_input, val_label in val_dataloader:
            loss = get_statistics(val_input, val_label, model, PREFormer, criterion, Metric, name, epoch=None)
            if criterion is not None:
                total += loss.item()
            check_visual_rows(model)
        log(Metric, total / len(val_dataloader) if criterion is not None else 0, name)
    return total / len(val_dataloader)


def _save_if_better(val_loss, prev_val_loss, model, PREFormer, stepper, criterion, scheduler, epoch, batch_idx, path, log_val, patience):
    """reference :72-82 / :108-118: keep the best validation loss, save best.pt on improvement, count patience otherwise."""
    global PATIENCE_ITER
    if val_loss < prev_val_loss:
        PATIENCE_ITER = 0
        print(f"we have seen loss decrease the previous best and we are updating our best loss val to {val_loss}")
        if path is not None:
            save_model(model, PREFormer, stepper.opt, criterion, scheduler, epoch, batch_idx, path, log_val)
        return val_loss, False
    PATIENCE_ITER += 1
    print(f"we have seen loss increase for {PATIENCE_ITER} steps and validation loss is {val_loss}, and previous best validtion loss is {prev_val_loss}")
    return prev_val_loss, PATIENCE_ITER == patience


def not_grad_accum(epoch, train_dataloader, val_dataloader, model, PREFormer, criterion, stepper, scheduler, patience, Metric, prev_val_loss, log_val, path=None,
                   graphs=None, sync=None):
    """reference :52-83: one optimisation step per batch.  graphs: a graphed.GraphedSteps that takes the step instead (replays of a captured one).
    sync: a LogSync -- the loss sum lives in its `train` accumulator and is read where the loop logs, not after every step."""
    iters = len(train_dataloader)
    total_loss_train = 0.0
    if sync is not None:
        ops.loop_acc_reset(sync.train)
    for batch_idx, (train_input, train_label) in enumerate(train_dataloader):
        if sync is not None:
            if graphs is not None:
                graphs.step(train_input, train_label, epoch, Metric, sync=sync)
            else:
                loss = recorded_loss(sync.train, train_input, train_label, model, PREFormer, criterion, Metric, check="train", epoch=epoch)
                loss.backward()
                if stepper.reducer is not None:
                    stepper.reducer.finish()
                stepper.update()
        elif graphs is not None:
            total_loss_train += graphs.step(train_input, train_label, epoch, Metric)
        else:
            loss = get_statistics(train_input, train_label, model, PREFormer, criterion, Metric, check="train", epoch=epoch)
            total_loss_train += loss.item()
            check_visual_rows(model)
            loss.backward()
            if stepper.reducer is not None:
                stepper.reducer.finish()
            stepper.update()
        scheduler.step(epoch + batch_idx / iters)
        if ((batch_idx + 1) % log_val == 0) or (batch_idx + 1 == iters):
            if sync is not None:
                total_loss_train = LogSync.read(sync.train, "train")["loss_sum"]
            log(Metric, total_loss_train / iters, "train")
            val_loss = validate(val_dataloader, model, PREFormer, criterion, Metric, name="val", sync=sync)
            prev_val_loss, stop = _save_if_better(val_loss, prev_val_loss, model, PREFormer, stepper, criterion, scheduler, epoch, batch_idx, path, log_val, patience)
            if stop:
                break
    return prev_val_loss


def grad_accum(epoch, train_dataloader, val_dataloader, model, PREFormer, criterion, stepper, scheduler, patience, Metric, prev_val_loss, log_val, path=None,
               graphs=None, sync=None):
    """reference :87-119, the dialogue-level variant used on epochs with epoch % epoch_switch != 0.  Kept with its quirk: the loss is
    divided by the dialogue length (`dataset.retGradAccum(i)` -> (accum_iter, accum_sum)) but the optimizer still steps -- and the
    gradients are zeroed -- after EVERY batch (:96-100), so the extra, unclipped `optimizer.step()` at a dialogue end (:102-106) runs on zeroed
    gradients.  What that step does depends on the torch version behind `model.zero_grad()`:
      * torch >= 2.0 (`set_to_none=True`): every .grad is None, AdamW skips every parameter -- nothing changes but the scheduler call
        (the default here: `TrainStep(zero_grad_like_torch_1_10=False)`);
      * torch 1.10, the version the reference pins (README_and_Requirements/requirements.txt:100; `set_to_none=False`): the gradients are
        zero TENSORS, so AdamW still runs -- weights decay by (1 - lr * wd), both moments shrink by their betas, the step counter advances and
        the parameters move along the remaining momentum (`TrainStep(zero_grad_like_torch_1_10=True)` /
        `train_tav_network(..., zero_grad_like_torch_1_10=True)`).
    Both readings are tested (tests/test_abi_and_host.py on the call sequence, tests/test_model_gpu.py against torch.optim.AdamW).
    graphs: as in not_grad_accum; the division by the dialogue length is then a device scalar the replay reads.
    sync: as in not_grad_accum; what is accumulated is the loss already divided by the dialogue length."""
    iters = len(train_dataloader)
    total_loss_train = 0.0
    if sync is not None:
        ops.loop_acc_reset(sync.train)
    for batch_idx, (train_input, train_label) in enumerate(train_dataloader):
        accum_iter, accum_sum = train_dataloader.dataset.retGradAccum(i=batch_idx)
        if sync is not None:
            if graphs is not None:
                graphs.step(train_input, train_label, epoch, Metric, accum_iter=accum_iter, sync=sync)
            else:
                loss = recorded_loss(sync.train, train_input, train_label, model, PREFormer, criterion, Metric, check="train", epoch=epoch,
                                     divide_by=accum_iter)
                loss.backward()
                if stepper.reducer is not None:
                    stepper.reducer.finish()
                stepper.update()
        elif graphs is not None:
            total_loss_train += graphs.step(train_input, train_label, epoch, Metric, accum_iter=accum_iter)
        else:
            loss = get_statistics(train_input, train_label, model, PREFormer, criterion, Metric, check="train", epoch=epoch) / accum_iter
            total_loss_train += loss.item()
            check_visual_rows(model)
            loss.backward()
            if stepper.reducer is not None:
                stepper.reducer.finish()
            stepper.update()
        scheduler.step(epoch + batch_idx / iters)
        if ((batch_idx + 1) % accum_sum == 0) or (batch_idx + 1 == iters):
            stepper.update(clip=False)           # reference :103: optimizer.step() without clip_grad_norm_; no-op or a momentum / decay step (docstring)
            scheduler.step(epoch + batch_idx / iters)
        if ((batch_idx + 1) % log_val == 0) or (batch_idx + 1 == iters):
            if sync is not None:
                total_loss_train = LogSync.read(sync.train, "train")["loss_sum"]
            log(Metric, total_loss_train / iters, "train")
            val_loss = validate(val_dataloader, model, PREFormer, criterion, Metric, name="val", sync=sync)
            prev_val_loss, stop = _save_if_better(val_loss, prev_val_loss, model, PREFormer, stepper, criterion, scheduler, epoch, batch_idx, path, log_val, patience)
            if stop:
                break
    return prev_val_loss


def one_epoch(epoch, train_dataloader, val_dataloader, model, PREFormer, criterion, stepper, scheduler, epoch_switch, patience, Metric, prev_val_loss,
              path=None, log_val=2400, graphs=None, sync=None):
    """reference :133-144: alternate the two loops by epoch parity, then reload the best checkpoint of the run (:143).  graphs (graph mode): the
    epoch's captured steps are freed at its end -- the next epoch has the other loop and loss branch, and the reload replaces the optimizer's
    moment tensors that a captured step points at."""
    loop = not_grad_accum if (epoch % epoch_switch == 0 or not hasattr(train_dataloader.dataset, "retGradAccum")) else grad_accum
    kw = {} if sync is None else {"sync": sync}
    if graphs is None:
        prev_val_loss = loop(epoch, train_dataloader, val_dataloader, model, PREFormer, criterion, stepper, scheduler, patience, Metric, prev_val_loss, log_val, path,
                             **kw)
    else:
        prev_val_loss = loop(epoch, train_dataloader, val_dataloader, model, PREFormer, criterion, stepper, scheduler, patience, Metric, prev_val_loss, log_val, path,
                             graphs=graphs, **kw)
        graphs.invalidate()
    if path is not None and os.path.exists(checkpoint_file(path)):
        load_model(model, PREFormer, stepper.opt, criterion, path)
    return prev_val_loss


def train_tav_network(model, PREFormer, train_dataloader, val_dataloader, criterion, learning_rate, epochs, weight_decay, T_max, Metric, patience, clip,
                      epoch_switch, checkpoint=None, path=None, log_val=2400, zero_grad_like_torch_1_10=False, graphs=False, sync="step",
                      encoder_lr_scale=1.0, no_decay_norm_bias=False):
    """reference :147-164.  `path` (None = keep nothing on disk) replaces the cluster path hard-coded at :137; `checkpoint` is a loaded
    best.pt dict whose optimizer / scheduler state resumes the run (:152-155).  graphs=True: every training batch whose shapes match an
    earlier one of the epoch replays a captured step (graphed.py; same results bit for bit); the whole run then executes on one side stream.
    sync="log" (needs Metrics(on_device=True) or Metric=None): the host reads nothing per step -- loss sum, ragged status word and confusion
    matrix stay on the device (LogSync) and are read every log_val batches, at the end of an epoch and at the end of validate(); losses,
    matrices, patience and best.pt decisions are the same numbers at the same places as with "step".
    encoder_lr_scale / no_decay_norm_bias: optim.default_param_groups -- the pretrained encoders train at learning_rate * encoder_lr_scale, biases
    and norm weights without weight decay (up to four parameter groups in one fused update; the defaults keep the single group)."""
    if sync not in ("step", "log"):
        raise ValueError(f'sync must be "step" or "log", got {sync!r}')
    if sync == "log" and Metric is not None and not getattr(Metric, "on_device", False):
        LogSync(Metric)                          # raises: says to pass on_device=True
    stepper = TrainStep(model, PREFormer, criterion, lr=learning_rate, weight_decay=weight_decay, clip=clip, zero_grad_like_torch_1_10=zero_grad_like_torch_1_10,
                        encoder_lr_scale=encoder_lr_scale, no_decay_norm_bias=no_decay_norm_bias)
    if graphs:
        from .graphed import run_graphed
        return run_graphed(_train_epochs, stepper, model, PREFormer, train_dataloader, val_dataloader, criterion, epochs, T_max, Metric, patience,
                           epoch_switch, checkpoint, path, log_val, sync=sync)
    return _train_epochs(stepper, model, PREFormer, train_dataloader, val_dataloader, criterion, epochs, T_max, Metric, patience, epoch_switch, checkpoint,
                         path, log_val, sync=sync)


def _train_epochs(stepper, model, PREFormer, train_dataloader, val_dataloader, criterion, epochs, T_max, Metric, patience, epoch_switch, checkpoint, path,
                  log_val, graphs=None, sync="step"):
    sync = _as_sync(sync, Metric)                # (built here: in graph mode this already runs on the loop's side stream)
    scheduler = CosineWarmRestarts(stepper.opt, T_0=T_max)
    prev_val_loss = 100
    if checkpoint is not None:
        stepper.opt.load_state_dict(checkpoint["optimizer_state_dict"])
        sched = checkpoint.get("scheduler_state_dict", checkpoint.get("scheduler"))      # the reference saves 'scheduler' (:223) and reads 'scheduler_state_dict' (:155)
        if sched is not None:
            scheduler.load_state_dict(sched)
    for epoch_num in range(epochs):
        if wandb is not None and getattr(wandb, "run", None) is not None:
            wandb.log({"epoch": epoch_num, "learning_rate": scheduler.get_last_lr()[0]})
        stepper.opt.zero_grad()
        prev_val_loss = one_epoch(epoch_num, train_dataloader, val_dataloader, model, PREFormer, criterion, stepper, scheduler, epoch_switch, patience,
                                  Metric, prev_val_loss, path, log_val, graphs=graphs, sync=sync)
        if PATIENCE_ITER == patience:
            return model, PREFormer
    return model, PREFormer


def evaluate_tav(model, PREFormer, test_dataloader, Metric, sync="step"):
    validate(test_dataloader, model, PREFormer, None, Metric, name="test", sync=sync)


def log(Metric, loss, check="train"):
    if Metric is None:
        return
    multiAcc, multiF1, multiRec, multiPrec, Acc, F1Macro, F1Weighted, Rec, Prec, cm = Metric.compute_scores(f"{check}")
    d1 = {f"{check}/loss": loss, f"{check}/acc": Acc, f"{check}/precision": Prec, f"{check}/recall": Rec, f"{check}/weighted-f1-score": F1Weighted,
          f"{check}/macro-f1-score": F1Macro}
    print(f"\n in {check} \n loss = {loss:.5f} acc = {Acc:.4f} \n Confusion Matrix = {cm} \n", flush=True)
    if wandb is not None and getattr(wandb, "run", None) is not None:
        wandb.log({**d1, **multiF1, **multiRec, **multiPrec, **multiAcc})
    Metric.reset_metrics()
