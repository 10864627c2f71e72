"""The one training loop behind the ablation baselines: SingleModels/train_model/*_training.py and DoubleModels/train_model/
text_audio_training.py keep the reference's names, bind these functions with their few options and say what they keep of the reference.
A baseline supplies `forward(model, input, check) -> logits` and wraps label_statistics in a get_statistics of the reference's signature.
  * The audio / visual loop (one_epoch, validate, train_classifier, evaluate): forward, zero_grad, backward, an UNCLIPPED FusedAdamW.step();
    the cosine rate moves once per epoch, after the training pass, so an epoch trains with the rate set at the end of the previous one.
  * The text / text+audio loop (ClipStep, clip_step_epochs): forward, backward, clip_and_step(clip), zero_grad; no scheduler, no test pass.
Neither calls .eval(): validation and test run in whatever mode the model is in."""
import math

import torch

from ..optim import FusedAdamW
from ..utils.early_stopping import EarlyStopping


def cosine_annealing_lr(base, epoch, T_max):
    """Learning rate after `epoch` scheduler steps of torch's CosineAnnealingLR(T_max, eta_min=0) from `base` (epoch 0: base itself).  It is
    periodic in 2 T_max: past T_max the rate climbs back."""
    return 0.5 * base * (1.0 + math.cos(math.pi * epoch / T_max))


def forward_on_device(model, input, check):
    return model(input.to(next(model.parameters()).device))


def label_statistics(forward, input, label, model, criterion, Metric, check="train", **loss_kw):
    """One batch: label to the model's device, forward, the loss (None without a criterion), then the batch counted into Metric (if any)."""
    label = label.to(next(model.parameters()).device)
    output = forward(model, input, check)
    batch_loss = criterion(output, label.long(), **loss_kw) if criterion is not None else None
    if Metric is not None:
        Metric.update_metrics(torch.argmax(output.detach(), dim=1), label.long())
    return batch_loss


def summed_statistics(forward, input, label, model, criterion, total_loss, Metric, check="train"):
    """label_statistics with the reference's running sum: -> (batch_loss, total_loss + batch_loss.item())."""
    batch_loss = label_statistics(forward, input, label, model, criterion, Metric, check)
    return batch_loss, total_loss + (batch_loss.item() if batch_loss is not None else 0.0)


def one_epoch(get_statistics, train_dataloader, model, criterion, optimizer, clip, Metric):
    """-> (model, optimizer, last batch loss, loss sum / rows seen).  get_statistics(input, label, model, criterion, total, Metric) ->
    (batch_loss, total + batch_loss.item()).  `clip` is accepted and unused: the reference's update is unclipped."""
    total_loss_train, train_batch_loss, seen = 0.0, None, 0
    for train_input, train_label in train_dataloader:
        train_batch_loss, total_loss_train = get_statistics(train_input, train_label, model, criterion, total_loss_train, Metric)
        optimizer.zero_grad()
        train_batch_loss.backward()
        optimizer.step()
        seen += len(train_label)
    return model, optimizer, train_batch_loss, total_loss_train / max(1, seen)


def validate(get_statistics, val_dataloader, model, criterion, Metric, name="val"):
    """-> (last batch loss, loss sum / rows seen), without gradients.  Rows seen is len(loader.dataset), the reference's denominator, for
    every loader that keeps its last batch and has no sampler, which is every loader the entry points build."""
    total_loss_val, val_batch_loss, seen = 0.0, None, 0
    with torch.no_grad():
        for val_input, val_label in val_dataloader:
            val_batch_loss, total_loss_val = get_statistics(val_input, val_label, model, criterion, total_loss_val, Metric, name)
            seen += len(val_label)
    return val_batch_loss, total_loss_val / max(1, seen)


def train_classifier(get_statistics, model, train_dataloader, val_dataloader, criterion, learning_rate, epochs, weight_decay, T_max, Metric,
                     patience=None, clip=None, log=None, early_stopping=False, full_log=False):
    """-> model.  log: an optional list that receives one dict per epoch (losses, scores, the two confusion matrices).
    early_stopping: with a patience, EarlyStopping on the validation loss restores the best weights and the loop goes on; the log entry says
    `restored`.  full_log: the epoch's rate in the printed line and the log entry, and the last validation batch loss in the log entry."""
    optimizer = FusedAdamW([p for p in model.parameters() if p.requires_grad], lr=learning_rate, weight_decay=weight_decay)
    earlystop = EarlyStopping("", model, patience, model_name=model.__class__.__name__) if early_stopping else None
    for epoch_num in range(epochs):
        optimizer.zero_grad()
        lr = optimizer.lr
        model, optimizer, train_batch_loss, train_loss = one_epoch(get_statistics, train_dataloader, model, criterion, optimizer, clip, Metric)
        *_, acc, f1, _, rec, prec, cm_train = Metric.compute_scores("train")
        print(f"epoch {epoch_num}: {f'lr {lr:.6e} ' if full_log else ''}train loss {train_loss:.4f} batch loss {float(train_batch_loss.detach()):.4f} "
              f"acc {acc:.3f} f1 {f1:.3f}", flush=True)
        Metric.reset_metrics()
        optimizer.lr = cosine_annealing_lr(learning_rate, epoch_num + 1, T_max)
        val_batch_loss, val_loss = validate(get_statistics, val_dataloader, model, criterion, Metric)
        *_, vacc, vf1, _, vrec, vprec, cm_val = Metric.compute_scores("val")
        print(f"epoch {epoch_num}: val loss {val_loss:.4f} acc {vacc:.3f} f1 {vf1:.3f}", flush=True)
        Metric.reset_metrics()
        restored = earlystop is not None and patience is not None and earlystop(model, val_loss)
        if restored:
            model = earlystop.best_state               # restores and keeps looping, as the reference does
        if log is not None:
            log.append({"epoch": epoch_num, "train/batch_loss": float(train_batch_loss.detach()), "train/train_loss": train_loss, "train/acc": acc,
                        "train/f1-score": f1, "train/cm": cm_train, "val/total_loss_val": val_loss, "val/total_acc_val": vacc, "val/f1-score": vf1,
                        "val/cm": cm_val, **({"lr": lr, "val/batch_loss": float(val_batch_loss.detach())} if full_log else {}),
                        **({"restored": restored} if early_stopping else {})})
    return model


def evaluate(get_statistics, model, test_dataloader, Metric, criterion=None):
    """-> the test scores; with a criterion the test loss is printed and returned as well."""
    _, test_loss = validate(get_statistics, test_dataloader, model, criterion, Metric, name="test")
    *_, acc, f1, _, rec, prec, cm = Metric.compute_scores("test")
    if criterion is not None:
        print(f"test: loss {test_loss:.4f}", flush=True)
    print(f"test: acc {acc:.3f} f1 {f1:.3f} recall {rec:.3f} precision {prec:.3f}\nConfusion Matrix = {cm}", flush=True)
    Metric.reset_metrics()
    return {"test/total_acc_test": acc, "test/precision": prec, "test/recall": rec, "test/f1-score": f1, "test/ConfusionMatrix": cm,
            **({"test/total_loss_test": test_loss} if criterion is not None else {})}


class ClipStep:
    """forward + loss + backward + clip_grad_norm_ + AdamW.step + zero_grad.  A subclass sets `statistics`, its module's
    get_statistics(input, label, model, criterion, Metric, check=, epoch=) -> loss."""

    def __init__(self, model, criterion, lr=1e-6, weight_decay=1e-4, clip=1.0):
        self.model, self.criterion, self.clip = model, criterion, clip
        self.opt = FusedAdamW([p for p in model.parameters() if p.requires_grad], lr=lr, weight_decay=weight_decay)

    def __call__(self, input, label, check="train", epoch=0):
        loss = self.statistics(input, label, self.model, self.criterion, None, check=check, epoch=epoch)
        loss.backward()
        norm = self.opt.clip_and_step(self.clip)
        self.opt.zero_grad()
        return loss, norm


def clip_step_epochs(step, Metric, df_train, df_val, epochs, prepare_dataloader, batch_size):
    """The epoch loop of the text and text+audio runModel: a training pass with `step` (a ClipStep) and a no-grad validation pass that
    counts into Metric; the training sum is over len(df_train) batches, the validation mean over the batches seen."""
    for epoch in range(epochs):
        total = 0.0
        for inp, lab in prepare_dataloader(df_train, batch_size, None, None):
            loss, _ = step(inp, lab, check="train", epoch=epoch)
            total += loss.item()
        print(f"epoch {epoch}: train loss {total / max(1, len(df_train)):.4f}", flush=True)
        with torch.no_grad():
            vl = [step.statistics(i, l, step.model, step.criterion, Metric, check="val", epoch=epoch).item() for i, l in prepare_dataloader(df_val, 0, None, None)]
        print(f"epoch {epoch}: val loss {sum(vl) / max(1, len(vl)):.4f}", flush=True)
    return step.model
