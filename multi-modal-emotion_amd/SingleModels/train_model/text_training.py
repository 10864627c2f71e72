"""Drop-in for the reference's SingleModels/train_model/text_training.py: `get_statistics` (:14-29) and the per-batch step of
`not_grad_accum` (:31-56: backward, clip_grad_norm_, AdamW step, cosine warm restarts), on the fused clip+AdamW of this package.  The step
and the statistics are train_model/classifier_loop.py's, shared with the other baselines."""
from ...train_model.classifier_loop import ClipStep, label_statistics
from ...utils.global_functions import CrossEntropyLoss  # noqa: F401  (re-exported for callers that build the criterion here)


def _forward(model, input, check):
    dev = next(model.parameters()).device
    mask = input["attention_mask"].to(dev)
    input_id = input["input_ids"].squeeze(1).to(dev)                      # reference :20
    if getattr(model, "LSTM_layers", None) is None:
        return model(input_id, mask, check)
    if model.training != (check == "train"):                              # LSTMClassifier.forward(x): dropout follows model.training
        model.train(check == "train")
    return model(input_id)


def get_statistics(input, label, model, criterion, Metric, check="train", epoch=None):
    return label_statistics(_forward, input, label, model, criterion, Metric, check, epoch=epoch if epoch is not None else 1)


class TextTrainStep(ClipStep):
    """forward + loss + backward + clip_grad_norm_ + AdamW.step for the text-only classifier (reference :36-43)."""
    statistics = staticmethod(get_statistics)
