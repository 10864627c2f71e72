"""Drop-in for the reference's SingleModels/train_model/visual_training.py: get_statistics (:9-29), one_epoch (:33-49), validate (:52-64),
visual_train (:70-117) and evaluate_visual (:120-131), on this package's fused AdamW.

The reference's one_epoch clips the gradients of the PREVIOUS step (clip_grad_norm_ runs before zero_grad and backward), so the update it
applies is never clipped.  That is kept: the step here is FusedAdamW.step(), without a clip, and `clip` is accepted and unused.  wandb logging
and the EarlyStopping checkpoint are left out (no files are written); the cosine schedule is the reference's CosineAnnealingLR(T_max)."""
import math

import torch

from ...optim import FusedAdamW


def get_statistics(input, label, model, criterion, total_loss, Metric):
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
    total_loss_train, train_batch_loss, seen = 0.0, None, 0
    for train_input, train_label in train_dataloader:
        train_batch_loss, total_loss_train = get_statistics(train_input, train_label, model, criterion, total_loss_train, Metric)
        optimizer.zero_grad()
        train_batch_loss.backward()
        optimizer.step()                       # unclipped, as the reference's update is (module docstring)
        seen += len(train_label)
    return model, optimizer, train_batch_loss, total_loss_train / max(1, seen)


def validate(val_dataloader, model, criterion, Metric, name="val"):
    total_loss_val, val_batch_loss, seen = 0.0, None, 0
    with torch.no_grad():
        for val_input, val_label in val_dataloader:
            val_batch_loss, total_loss_val = get_statistics(val_input, val_label, model, criterion, total_loss_val, Metric)
            seen += len(val_label)
    return val_batch_loss, total_loss_val / max(1, seen)


def visual_train(model, train_dataloader, val_dataloader, criterion, learning_rate, epochs, weight_decay, T_max, Metric, patience=None, clip=None, log=None):
    """-> model.  log: an optional list that receives one dict per epoch (losses, scores and the two confusion matrices)."""
    optimizer = FusedAdamW([p for p in model.parameters() if p.requires_grad], lr=learning_rate, weight_decay=weight_decay)
    for epoch_num in range(epochs):
        optimizer.zero_grad()
        model, optimizer, train_batch_loss, train_loss = one_epoch(train_dataloader, model, criterion, optimizer, clip, Metric)
        *_, acc, f1, _, rec, prec, cm_train = Metric.compute_scores("train")
        print(f"epoch {epoch_num}: train loss {train_loss:.4f} batch loss {float(train_batch_loss.detach()):.4f} acc {acc:.3f} f1 {f1:.3f}", flush=True)
        Metric.reset_metrics()
        optimizer.lr = 0.5 * learning_rate * (1.0 + math.cos(math.pi * (epoch_num + 1) / T_max))       # CosineAnnealingLR(T_max), eta_min 0
        val_batch_loss, val_loss = validate(val_dataloader, model, criterion, Metric)
        *_, vacc, vf1, _, vrec, vprec, cm_val = Metric.compute_scores("val")
        print(f"epoch {epoch_num}: val loss {val_loss:.4f} acc {vacc:.3f} f1 {vf1:.3f}", flush=True)
        Metric.reset_metrics()
        if log is not None:
            log.append({"epoch": epoch_num, "train/batch_loss": float(train_batch_loss.detach()), "train/train_loss": train_loss, "train/acc": acc, "train/f1-score": f1,
                        "train/cm": cm_train, "val/total_loss_val": val_loss, "val/total_acc_val": vacc, "val/f1-score": vf1, "val/cm": cm_val})
    return model


def evaluate_visual(model, test_dataloader, Metric):
    validate(test_dataloader, model, None, Metric, name="test")
    *_, acc, f1, _, rec, prec, cm = Metric.compute_scores("test")
    print(f"test: acc {acc:.3f} f1 {f1:.3f} recall {rec:.3f} precision {prec:.3f}\nConfusion Matrix = {cm}", flush=True)
    Metric.reset_metrics()
    return {"test/total_acc_test": acc, "test/precision": prec, "test/recall": rec, "test/f1-score": f1, "test/ConfusionMatrix": cm}
