"""Drop-in for the reference's SingleModels/visual_nn.py (visual-only entrypoint): same prepare_dataloader / runModel / main shape and CLI
flags; the default model is VisualClassification (Conv3d -> GELU stack, flatten, Linear, Sigmoid) trained with class-weighted cross entropy.
`--model Video` (ResNet50Classification) raises: its torch.hub weights cannot be had offline.

The reference decodes each file with pytorchvideo inside collate_batch (:110-128); offline, `--synthetic N` draws N seeded decoded clips
(uint8 [T, H, W, 3] frames, as synthetic.make_items does for the tri-modal path) and collate_batch_device runs them through the video
transform kernel (ops.video_clip_transform: temporal subsample, /255, normalise, resize) into the [B, 1, 3, T, H, W] batch the model takes.
New flags: --clip-shape T,H,W (default 16,224,224; --clip is already the gradient clip) and --synthetic.  input_dim follows the clips (3)."""
from argparse import ArgumentParser

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset

from .. import ops
from ..models.tav import subsample_indices
from ..utils.entrypoint import common_params, refuse_tav_only, start, synthetic_splits
from ..utils.global_functions import CrossEntropyLoss, Metrics, arg_parse
from .models.visual import ResNet50Classification, VisualClassification, hidden_layer_list
from .train_model.visual_training import evaluate_visual, visual_train


class SyntheticClips(Dataset):
    """n seeded decoded clips: (uint8 [T_raw, H_raw, W_raw, 3] frames, label).  The raw size is a little larger than the model's clip so that
    the transform really subsamples and resizes."""

    def __init__(self, n, clip_shape, num_classes, seed):
        self.n, self.clip_shape, self.num_classes, self.seed = int(n), tuple(clip_shape), int(num_classes), int(seed)

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        g = torch.Generator().manual_seed(self.seed * 100003 + i)
        T, H, W = self.clip_shape
        label = int(torch.randint(0, self.num_classes, (1,), generator=g))
        frames = torch.randint(0, 256, (T + 2, H + H // 8, W + W // 8, 3), generator=g, dtype=torch.uint8)
        frames[:, :, :, label % 3] //= 2                                         # a faint class signal, so that a loss can fall
        return frames, label


def collate_batch_device(batch, clip_shape, device="cuda"):
    """[(frames, label)] -> (f32 [B, 1, 3, T, H, W] on the device, labels float [B]): one transform launch per clip into its slab."""
    T, H, W = clip_shape
    clips = torch.empty(len(batch), T, 3, H, W, dtype=torch.float32, device=device)
    for k, (frames, _) in enumerate(batch):
        src = torch.as_tensor(frames).to(device, non_blocking=True)
        x = ops.clip_xform(src, subsample_indices(src.shape[0], T).tolist(), layout="THWC", out_hw=(H, W))
        ops.video_clip_transform(src, clips[k], x)
    return clips.permute(0, 2, 1, 3, 4).unsqueeze(1), torch.Tensor(np.array([label for _, label in batch]))


def prepare_dataloader(df, batch_size, pin_memory=False, num_workers=0, clip_shape=(16, 224, 224), shuffle=True):
    return DataLoader(df, batch_size=batch_size, pin_memory=pin_memory, num_workers=num_workers, drop_last=False, shuffle=shuffle,
                      collate_fn=lambda batch: collate_batch_device(batch, clip_shape))


def runModel(rank, df_train, df_val, df_test, param_dict, model_param, wandb=None):
    criterion = CrossEntropyLoss(weight=param_dict["weights"].to(rank))           # reference :66
    Metric = Metrics(num_classes=model_param["output_dim"], id2label=param_dict["id2label"], rank=rank)
    shape = tuple(model_param.get("clip_shape", (16, 224, 224)))
    loaders = [prepare_dataloader(d, param_dict["batch_size"], clip_shape=shape) for d in (df_train, df_val, df_test)]
    if param_dict["model"] == "Video":
        model = ResNet50Classification(model_param).to(rank)
    else:
        model = VisualClassification(model_param).to(rank)
    model = visual_train(model, loaders[0], loaders[1], criterion, param_dict["lr"], param_dict["epoch"], param_dict["weight_decay"], param_dict["T_max"],
                         Metric, param_dict["patience"], param_dict["clip"])
    evaluate_visual(model, loaders[2], Metric)
    return model


def parse_args(argv=None):
    """The reference's flags (utils.global_functions.arg_parse) plus --clip-shape T,H,W."""
    own = ArgumentParser(add_help=False, allow_abbrev=False)        # (or "--clip 0.5", the gradient clip, would be read as a prefix of --clip-shape)
    own.add_argument("--clip-shape", dest="clip_shape", default="16,224,224", help="T,H,W of the clips the model takes (default: the reference's 16,224,224)")
    mine, rest = own.parse_known_args(argv)
    args = arg_parse("MLP_test_visual", rest)
    shape = tuple(int(v) for v in mine.clip_shape.split(","))
    if len(shape) != 3 or min(shape) < 1:
        raise SystemExit(f"--clip-shape takes T,H,W, got {mine.clip_shape!r}")
    args.clip_shape = shape
    return args


def main(argv=None):
    args = parse_args(argv)
    refuse_tav_only(args)
    start(args)
    param_dict = common_params(args, model=args.model, T_max=args.T_max, seed=args.seed)
    model_param = {"input_dim": 3, "output_dim": args.output_dim, "lstm_layers": args.lstm_layers,
                   "hidden_layers": hidden_layer_list(args.hidden_layers), "clip_shape": args.clip_shape}
    mk = lambda n, seed: SyntheticClips(n, args.clip_shape, args.output_dim, seed)          # noqa: E731
    return runModel("cuda", *synthetic_splits(mk, args), param_dict, model_param)


if __name__ == "__main__":
    main()
