"""Drop-in for the reference's SingleModels/train_model/audio_training.py: get_statistics (:10-21), one_epoch (:24-37), validate (:42-48),
train_audio_network (:51-107) and evaluate_audio (:109-120), on this package's fused AdamW.  The loop itself is
train_model/classifier_loop.py, shared with the other baselines; this file binds it.

Kept from the reference:
  * one_epoch clips the gradients of the PREVIOUS step (clip_grad_norm_ runs before zero_grad and backward), so the update it applies is
    never clipped: the step here is FusedAdamW.step(), without a clip, and `clip` is accepted and unused;
  * the learning rate follows CosineAnnealingLR(T_max) with eta_min 0, stepped once per epoch (cosine_annealing_lr is its closed form);
  * neither loop calls .eval(), and the model's dropout follows self.training, so validation and test run with dropout on: two passes
    over the same loader give different losses;
  * early stopping does not stop: when EarlyStopping returns True the best weights are restored and the loop goes on (:103-105);
  * epoch losses are sums of batch losses over len(loader.dataset) (:37, :48): the rows the shared passes count, for a loader that keeps
    its last batch and has no sampler.
wandb logging is left out; `log`, an optional list, receives one dict per epoch instead."""
from functools import partial

from ...train_model import classifier_loop as L
from ...train_model.classifier_loop import cosine_annealing_lr  # noqa: F401  (re-exported: callers import the rule from here)


get_statistics = partial(L.summed_statistics, L.forward_on_device)     # (input, label, model, criterion, total_loss, Metric, check="train")
one_epoch = partial(L.one_epoch, get_statistics)           # (train_dataloader, model, criterion, optimizer, clip, Metric)
validate = partial(L.validate, get_statistics)             # (val_dataloader, model, criterion, Metric, name="val")


def train_audio_network(model, train_dataloader, val_dataloader, criterion, learning_rate, epochs, weight_decay, T_max, Metric, patience=None, clip=None,
                        log=None):
    """-> model.  log: an optional list that receives one dict per epoch (the learning rate the epoch trained with, losses, scores, the two
    confusion matrices and whether the best weights were restored after it)."""
    return L.train_classifier(get_statistics, model, train_dataloader, val_dataloader, criterion, learning_rate, epochs, weight_decay, T_max, Metric,
                              patience, clip, log, early_stopping=True, full_log=True)


def evaluate_audio(model, test_dataloader, Metric, criterion=None):
    """The reference passes no criterion and reports scores only; with one, the test loss is printed and returned as well."""
    return L.evaluate(get_statistics, model, test_dataloader, Metric, criterion)
