"""Drop-in for the reference's SingleModels/audio_nn.py (audio-only entrypoint): same prepare_dataloader / runModel / main shape and CLI
flags; the model is Wav2Vec2ForSpeechClassification (wav2vec2 -> mean over frames -> dropout -> Linear) trained with class-weighted
cross entropy through the library's kernel.

The reference decodes and resamples each file with torchaudio inside collate_batch (models/audio.py:13-38); offline, `--synthetic N` draws
N seeded decoded utterances (mono float PCM at --sampling-rate, of unequal length) and collate_batch_device runs each through the waveform
transform kernel into its row of the zero-padded [B, Tmax] batch.  New flags: --audio-seconds MIN,MAX (synthetic utterance lengths, drawn
per utterance) and --sampling-rate (of the synthetic PCM; anything but 16000 exercises the resampler).  --preset defaults to the audio
block of preset B, the wav2vec2-base the reference loads, whatever the other entrypoints default to."""
import math
from argparse import ArgumentParser

import torch
from torch.utils.data import DataLoader, Dataset

from .. import config as C
from ..utils.entrypoint import common_params, refuse_tav_only, start, synthetic_splits
from ..utils.global_functions import CrossEntropyLoss, Metrics, arg_parse
from .models.audio import Wav2Vec2ForSpeechClassification, collate_batch_device
from .train_model.audio_training import evaluate_audio, train_audio_network

MIN_SAMPLES_16K = 400            # the conv stack's receptive field: a shorter utterance leaves no frame


class SyntheticUtterances(Dataset):
    """n seeded decoded utterances: ({"pcm": f32 [L], "sampling_rate"}, label), L drawn per utterance from `seconds` = (min, max)."""

    def __init__(self, n, seconds, sampling_rate, num_classes, seed):
        self.n, self.seconds, self.sampling_rate, self.num_classes, self.seed = int(n), tuple(seconds), int(sampling_rate), int(num_classes), int(seed)

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        g = torch.Generator().manual_seed(self.seed * 100003 + i)
        lo, hi = self.seconds
        label = int(torch.randint(0, self.num_classes, (1,), generator=g))
        L = max(1, int(round((lo + (hi - lo) * float(torch.rand(1, generator=g))) * self.sampling_rate)))
        t = torch.arange(L, dtype=torch.float32) / self.sampling_rate
        pcm = 0.1 * torch.randn(L, generator=g) + 0.05 * torch.sin(2 * math.pi * (200.0 + 150.0 * label) * t)     # a faint class signal, so that a loss can fall
        return {"pcm": pcm, "sampling_rate": self.sampling_rate}, label


def prepare_dataloader(df, batch_size, label_task=None, pin_memory=False, num_workers=0, shuffle=True):
    return DataLoader(df, batch_size=batch_size, pin_memory=pin_memory, num_workers=num_workers, drop_last=False, shuffle=shuffle,
                      collate_fn=collate_batch_device)


def runModel(rank, df_train, df_val, df_test, param_dict, model_param, wandb=None):
    criterion = CrossEntropyLoss(weight=param_dict["weights"].to(rank))           # reference :66
    Metric = Metrics(num_classes=model_param["output_dim"], id2label=param_dict["id2label"], rank=rank)
    loaders = [prepare_dataloader(d, param_dict["batch_size"], param_dict.get("label_task")) for d in (df_train, df_val, df_test)]
    model = Wav2Vec2ForSpeechClassification(model_param, dropout=model_param.get("dropout", .5), config=model_param.get("config")).to(rank)
    model = train_audio_network(model, loaders[0], loaders[1], criterion, param_dict["lr"], param_dict["epoch"], param_dict["weight_decay"],
                                param_dict["T_max"], Metric, param_dict["patience"], param_dict["clip"], log=param_dict.get("log"))
    evaluate_audio(model, loaders[2], Metric, criterion)
    return model


def parse_args(argv=None):
    """The reference's flags (utils.global_functions.arg_parse) plus --audio-seconds MIN,MAX and --sampling-rate; --preset defaults to B."""
    own = ArgumentParser(add_help=False, allow_abbrev=False)
    own.add_argument("--audio-seconds", dest="audio_seconds", default="1,4", help="MIN,MAX seconds of the synthetic utterances (drawn per utterance)")
    own.add_argument("--sampling-rate", dest="sampling_rate", default=16000, type=int, help="sampling rate of the synthetic PCM (default 16000)")
    own.add_argument("--preset", default=None, help="encoder geometry (default: the audio block of preset B, the reference's wav2vec2-base)")
    mine, rest = own.parse_known_args(argv)
    args = arg_parse("MLP_test_audio", rest)
    try:
        seconds = tuple(float(v) for v in mine.audio_seconds.split(","))
    except ValueError:
        seconds = ()
    if len(seconds) != 2 or not 0 < seconds[0] <= seconds[1]:
        raise SystemExit(f"--audio-seconds takes MIN,MAX with 0 < MIN <= MAX, got {mine.audio_seconds!r}")
    if mine.sampling_rate < 1:
        raise SystemExit(f"--sampling-rate must be positive, got {mine.sampling_rate}")
    if seconds[0] * 16000 < MIN_SAMPLES_16K + 1:
        raise SystemExit(f"--audio-seconds: the shortest utterance must exceed {MIN_SAMPLES_16K} samples at 16 kHz ({MIN_SAMPLES_16K / 16000} s), "
                         f"got {seconds[0]} s")
    args.audio_seconds, args.sampling_rate, args.preset = seconds, mine.sampling_rate, mine.preset
    return args


def main(argv=None):
    args = parse_args(argv)
    refuse_tav_only(args)
    start(args)
    param_dict = common_params(args, model=args.model, T_max=args.T_max, seed=args.seed, label_task=args.label_task)
    model_param = {"input_dim": args.input_dim, "output_dim": args.output_dim, "lstm_layers": args.lstm_layers, "hidden_layers": args.hidden_layers,
                   "dropout": args.dropout, "config": C.preset(args.preset) if args.preset is not None else None}
    mk = lambda n, seed: SyntheticUtterances(n, args.audio_seconds, args.sampling_rate, args.output_dim, seed)          # noqa: E731
    return runModel("cuda", *synthetic_splits(mk, args), param_dict, model_param)


if __name__ == "__main__":
    main()
