"""Step of the text+audio dual path: forward + loss + backward + clip_grad_norm_ + AdamW (same shape as
train_model/tav_train.py:56-65 of the reference, which is the loop every *_nn.py entrypoint repeats).  The step and the statistics are
train_model/classifier_loop.py's, shared with the other baselines."""
from ...train_model.classifier_loop import ClipStep, label_statistics


def _forward(model, input, check):
    text, audio = input[0], input[1]
    return model(text["input_ids"], text["attention_mask"], audio["audio_features"], check=check)


def get_statistics(input, label, model, criterion, Metric, check="train", epoch=None):
    return label_statistics(_forward, input, label, model, criterion, Metric, check, epoch=epoch if epoch is not None else 1)


class TextAudioTrainStep(ClipStep):
    statistics = staticmethod(get_statistics)
