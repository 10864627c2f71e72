"""What the main() of every entry point (tav_nn.py, SingleModels/*_nn.py, DoubleModels/text_audio_nn.py) does before it builds a model: seeding and
precision, the common param_dict, the criterion of --loss, the seeded synthetic splits, the refusal of flags only tav_nn implements; and the dataset of collated batches."""
import numpy as np
import torch
from torch.utils.data import Dataset

from .. import config as C
from .. import runtime, synthetic
from .global_functions import CrossEntropyLoss, FBetaLoss, NewCrossEntropyLoss, PrecisionLoss

# flags of utils.global_functions.arg_parse that only tav_nn implements: (attribute, flag, default, what it selects)
TAV_ONLY = (("graph", "--graph", 0, "graph mode"), ("loop_sync", "--loop-sync", "step", "the loop without per-step host reads"),
            ("encoder_lr_scale", "--encoder-lr-scale", 1.0, "the encoders' own learning rate"),
            ("no_decay_norm_bias", "--no-decay-norm-bias", 0, "the no-decay parameter group"), ("visual_rows", "--visual-rows", "equal", "ragged video rows"),
            ("visual_bucket", "--visual-bucket", 0, "the ragged-row bucket"), ("specaugment", "--specaugment", "torch", "the choice of SpecAugment sampler"))


def start(args, preset=False):
    """Seeds numpy and torch with --seed and sets the precision policy; preset=True also makes --preset the default geometry."""
    np.random.seed(args.seed)
    torch.random.manual_seed(args.seed)
    if preset:
        C.set_default_preset(args.preset)
    runtime.set_precision(args.dtype)


def common_params(args, **own):
    """The param_dict keys every entry point shares, then `own`, then the class weights and the label names."""
    id2label = {i: f"class{i}" for i in range(args.output_dim)}
    return {"epoch": args.epoch, "patience": args.patience, "lr": args.learning_rate, "clip": args.clip, "batch_size": args.batch_size,
            "weight_decay": args.weight_decay, **own, "weights": torch.linspace(0.6, 0.95, args.output_dim),     # reference: 1 - class frequency (tav_nn.py:171)
            "label2id": {v: k for k, v in id2label.items()}, "id2label": id2label}


def build_criterion(param_dict, output_dim, device):
    """The training criterion of --loss (reference tav_nn.py:85-98): "CrossEntropy" -> CrossEntropyLoss(), "FBeta" ->
    FBetaLoss(num_classes, beta=--beta), "Precision" -> PrecisionLoss(num_classes), every other name -> NewCrossEntropyLoss on the class
    weights with --epoch_switch."""
    name = param_dict["loss"]
    if name == "CrossEntropy":
        return CrossEntropyLoss()
    if name == "FBeta":
        return FBetaLoss(num_classes=output_dim, beta=param_dict["beta"])
    if name == "Precision":
        return PrecisionLoss(num_classes=output_dim)
    return NewCrossEntropyLoss(class_weights=param_dict["weights"].to(device), epoch_switch=param_dict["epoch_switch"])


def synthetic_splits(mk, args):
    """mk(n, seed) -> dataset.  -> (train, val, test): --synthetic utterances for training, a quarter (at least one batch) for the others."""
    n_eval = max(args.batch_size, args.synthetic // 4)
    return mk(args.synthetic, 1000), mk(n_eval, 2000), mk(n_eval, 3000)


def refuse_tav_only(args, what="this entrypoint"):
    """SystemExit when a flag that only tav_nn implements is away from its default: a baseline must not accept it and do nothing."""
    for attr, flag, default, noun in TAV_ONLY:
        if getattr(args, attr) != default:
            raise SystemExit(f"{flag} {getattr(args, attr)}: {noun} exists for the tri-modal loop only (tav_nn); run {what} with {flag} {default}")


class SyntheticBatches(Dataset):
    """Each item is one already collated batch: synthetic.make_batch(cfg, batch_size, seed=seed + i, **make_batch_kw), n_utterances //
    batch_size of them (at least one)."""

    def __init__(self, cfg, n_utterances, batch_size, seed, **make_batch_kw):
        self.cfg, self.n, self.bs, self.seed, self.kw = cfg, max(1, n_utterances // batch_size), batch_size, seed, make_batch_kw

    def __len__(self):
        return self.n

    def __getitem__(self, i, **kw):
        return synthetic.make_batch(self.cfg, self.bs, seed=self.seed + i, **{**self.kw, **kw})
