"""Entrypoint of the text+audio dual path (reference DoubleModels/text_audio_nn.py, which does not run: SURVEY.md §8f row 2).
Same main()/runModel() shape as tav_nn.py; synthetic batches of 10 s audio (160000 samples -> 499 audio frames) and 128 text tokens
(BASELINE.json configs[3])."""
from torch.utils.data import DataLoader

from .. import config as C
from ..train_model.classifier_loop import clip_step_epochs
from ..utils.entrypoint import SyntheticBatches, build_criterion, common_params, refuse_tav_only, start, synthetic_splits
from ..utils.global_functions import Metrics, arg_parse
from .models.text_audio import BertAudioClassifier
from .train_model.text_audio_training import TextAudioTrainStep


class SyntheticTextAudioBatches(SyntheticBatches):
    def __init__(self, cfg, n_utterances, batch_size, seed, s_text=128, t_audio=160000):
        super().__init__(cfg, n_utterances, batch_size, seed, s_text=s_text, t_audio=t_audio, with_video=False)

    def __getitem__(self, i):
        (tx, au, _), lab = super().__getitem__(i)
        return [tx, au], lab


def prepare_dataloader(df, batch_size, label_task, epoch_switch, pin_memory=True, num_workers=0, check="train"):
    return DataLoader(df, batch_size=None, shuffle=False, num_workers=num_workers, pin_memory=pin_memory)


def runModel(accelerator, df_train, df_val, df_test, param_dict, model_param):
    device = accelerator
    criterion = build_criterion(param_dict, model_param["output_dim"], device)
    Metric = Metrics(num_classes=model_param["output_dim"], id2label=param_dict["id2label"], rank=device)
    model = BertAudioClassifier(model_param).to(device)
    step = TextAudioTrainStep(model, criterion, lr=param_dict["lr"], weight_decay=param_dict["weight_decay"], clip=param_dict["clip"])
    return clip_step_epochs(step, Metric, df_train, df_val, param_dict["epoch"], prepare_dataloader, param_dict["batch_size"])


def main(argv=None):
    args = arg_parse("TextAudio", argv)
    refuse_tav_only(args)
    start(args, preset=True)
    cfg = C.default_config()
    param_dict = common_params(args, loss=args.loss, beta=args.beta, epoch_switch=args.epoch_switch)
    model_param = {"output_dim": args.output_dim, "dropout": args.dropout}
    small = cfg["video"]["image"] != 224
    mk = lambda n, seed: SyntheticTextAudioBatches(cfg, n, args.batch_size, seed, s_text=16 if small else 128, t_audio=8000 if small else 160000)   # noqa: E731
    return runModel("cuda", *synthetic_splits(mk, args)[:2], None, param_dict, model_param)


if __name__ == "__main__":
    main()
