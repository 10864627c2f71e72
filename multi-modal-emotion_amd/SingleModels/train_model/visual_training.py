"""Drop-in for the reference's SingleModels/train_model/visual_training.py: get_statistics (:9-29), one_epoch (:33-49), validate (:52-64),
visual_train (:70-117) and evaluate_visual (:120-131), on this package's fused AdamW.  The loop itself is
train_model/classifier_loop.py, shared with the other baselines; this file binds it.

The reference's one_epoch clips the gradients of the PREVIOUS step (clip_grad_norm_ runs before zero_grad and backward), so the update it
applies is never clipped.  That is kept: the step here is FusedAdamW.step(), without a clip, and `clip` is accepted and unused.  wandb logging
and the EarlyStopping checkpoint are left out (no files are written, `patience` is accepted and unused); the cosine schedule is the
reference's CosineAnnealingLR(T_max)."""
from functools import partial

from ...train_model import classifier_loop as L


get_statistics = partial(L.summed_statistics, L.forward_on_device)     # (input, label, model, criterion, total_loss, Metric, check="train")
one_epoch = partial(L.one_epoch, get_statistics)           # (train_dataloader, model, criterion, optimizer, clip, Metric)
validate = partial(L.validate, get_statistics)             # (val_dataloader, model, criterion, Metric, name="val")


def visual_train(model, train_dataloader, val_dataloader, criterion, learning_rate, epochs, weight_decay, T_max, Metric, patience=None, clip=None, log=None):
    """-> model.  log: an optional list that receives one dict per epoch (losses, scores and the two confusion matrices)."""
    return L.train_classifier(get_statistics, model, train_dataloader, val_dataloader, criterion, learning_rate, epochs, weight_decay, T_max, Metric,
                              patience, clip, log)


def evaluate_visual(model, test_dataloader, Metric):
    return L.evaluate(get_statistics, model, test_dataloader, Metric)
