"""Drop-in for the reference's SingleModels/train_model/audio_training.py: get_statistics (:10-21), one_epoch (:24-37), validate (:42-48),
train_audio_network (:51-107) and evaluate_audio (:109-120), on this package's fused AdamW.

Kept from the reference:
  * one_epoch clips the gradients of the PREVIOUS step (clip_grad_norm_ runs before zero_grad and backward), so the update it applies is
    never clipped: the step here is FusedAdamW.step(), without a clip, and `clip` is accepted and unused;
  * the learning rate follows CosineAnnealingLR(T_max) with eta_min 0, stepped once per epoch (cosine_annealing_lr is its closed form);
  * neither loop calls .eval(), and the model's dropout follows self.training, so validation and test run with dropout on: two passes
    over the same loader give different losses;
  * early stopping does not stop: when EarlyStopping returns True the best weights are restored and the loop goes on (:103-105).
wandb logging is left out; `log`, an optional list, receives one dict per epoch instead."""
import math

import torch

from ...optim import FusedAdamW
from ...utils.early_stopping import EarlyStopping


def cosine_annealing_lr(base, epoch, T_max):
    """Learning rate after `epoch` scheduler steps of torch's CosineAnnealingLR(T_max, eta_min=0) from `base` (epoch 0: base itself).  It is
    periodic in 2 T_max: past T_max the rate climbs back."""
    return 0.5 * base * (1.0 + math.cos(math.pi * epoch / T_max))


def get_statistics(input, label, model, criterion, total_loss, Metric, check="train"):
    dev = next(model.parameters()).device
    label = label.to(dev)
    output = model(input.to(dev))
    batch_loss = None
    if criterion is not None:
        batch_loss = criterion(output, label.long())
        total_loss += batch_loss.item()
    Metric.update_metrics(torch.argmax(output.detach(), dim=1), label.long())
    return batch_loss, total_loss


def one_epoch(train_dataloader, model, criterion, optimizer, clip, Metric):
    total_loss_train, train_batch_loss = 0.0, None
    for train_input, train_label in train_dataloader:
        train_batch_loss, total_loss_train = get_statistics(train_input, train_label, model, criterion, total_loss_train, Metric)
        optimizer.zero_grad()
        train_batch_loss.backward()
        optimizer.step()                       # unclipped, as the reference's update is (module docstring)
    return model, optimizer, train_batch_loss, total_loss_train / max(1, len(train_dataloader.dataset))


def validate(val_dataloader, model, criterion, Metric, name="val"):
    total_loss_val, val_batch_loss = 0.0, None
    with torch.no_grad():
        for val_input, val_label in val_dataloader:
            val_batch_loss, total_loss_val = get_statistics(val_input, val_label, model, criterion, total_loss_val, Metric, name)
    return val_batch_loss, total_loss_val / max(1, len(val_dataloader.dataset))


def train_audio_network(model, train_dataloader, val_dataloader, criterion, learning_rate, epochs, weight_decay, T_max, Metric, patience=None, clip=None,
                        log=None):
    """-> model.  log: an optional list that receives one dict per epoch (the learning rate the epoch trained with, losses, scores, the two
    confusion matrices and whether the best weights were restored after it)."""
    optimizer = FusedAdamW([p for p in model.parameters() if p.requires_grad], lr=learning_rate, weight_decay=weight_decay)
    earlystop = EarlyStopping("", model, patience, model_name=model.__class__.__name__)
    for epoch_num in range(epochs):
        optimizer.zero_grad()
        lr = optimizer.lr
        model, optimizer, train_batch_loss, train_loss = one_epoch(train_dataloader, model, criterion, optimizer, clip, Metric)
        *_, acc, f1, _, rec, prec, cm_train = Metric.compute_scores("train")
        print(f"epoch {epoch_num}: lr {lr:.6e} train loss {train_loss:.4f} batch loss {float(train_batch_loss.detach()):.4f} acc {acc:.3f} f1 {f1:.3f}",
              flush=True)
        Metric.reset_metrics()
        optimizer.lr = cosine_annealing_lr(learning_rate, epoch_num + 1, T_max)
        val_batch_loss, val_loss = validate(val_dataloader, model, criterion, Metric)
        *_, vacc, vf1, _, vrec, vprec, cm_val = Metric.compute_scores("val")
        print(f"epoch {epoch_num}: val loss {val_loss:.4f} acc {vacc:.3f} f1 {vf1:.3f}", flush=True)
        Metric.reset_metrics()
        restored = False
        if patience is not None:
            if earlystop(model, val_loss):
                model = earlystop.best_state           # restores and keeps looping, as the reference does
                restored = True
        if log is not None:
            log.append({"epoch": epoch_num, "lr": lr, "train/batch_loss": float(train_batch_loss.detach()), "train/train_loss": train_loss,
                        "train/acc": acc, "train/f1-score": f1, "train/cm": cm_train, "val/batch_loss": float(val_batch_loss.detach()),
                        "val/total_loss_val": val_loss, "val/total_acc_val": vacc, "val/f1-score": vf1, "val/cm": cm_val, "restored": restored})
    return model


def evaluate_audio(model, test_dataloader, Metric, criterion=None):
    """The reference passes no criterion and reports scores only; with one, the test loss is printed and returned as well."""
    _, test_loss = validate(test_dataloader, model, criterion, Metric, name="test")
    *_, acc, f1, _, rec, prec, cm = Metric.compute_scores("test")
    if criterion is not None:
        print(f"test: loss {test_loss:.4f}", flush=True)
    print(f"test: acc {acc:.3f} f1 {f1:.3f} recall {rec:.3f} precision {prec:.3f}\nConfusion Matrix = {cm}", flush=True)
    Metric.reset_metrics()
    return {"test/total_acc_test": acc, "test/precision": prec, "test/recall": rec, "test/f1-score": f1, "test/ConfusionMatrix": cm,
            **({"test/total_loss_test": test_loss} if criterion is not None else {})}
