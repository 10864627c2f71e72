"""Drop-in for the reference's SingleModels/text_nn.py (text-only entrypoint, BASELINE.json configs[0]): same main() / runModel()
shape and CLI flags; `--model LSTM --lstm_layers L --hidden_layers H` trains the reference's LSTMClassifier baseline (hyper_parameter_config/
lstm.yaml), with `--synthetic` on a seeded random vector table of width H.  The reference tokenises a dataset pickle (text_nn.py:28-57); offline, batches come from synthetic.make_batch
with the contract of its DataLoader: ({"input_ids": int64 [b,1,S], "attention_mask": float [b,S]}, labels)."""
import torch
from torch.utils.data import DataLoader

from .. import config as C
from ..train_model.classifier_loop import clip_step_epochs
from ..utils.entrypoint import SyntheticBatches, build_criterion, common_params, refuse_tav_only, start, synthetic_splits
from ..utils.global_functions import Metrics, arg_parse
from .models.text import BertClassifier, LSTMClassifier
from .train_model.text_training import TextTrainStep


class SyntheticVectors:
    """Stands in for torchtext's GloVe offline: `.vectors` is a seeded normal table [vocab, width] at GloVe's scale (std 0.4)."""

    def __init__(self, vocab, width, seed):
        self.vectors = torch.randn(vocab, width, generator=torch.Generator().manual_seed(seed)) * 0.4


class SyntheticTextBatches(SyntheticBatches):
    def __init__(self, cfg, n_utterances, batch_size, seed, s_text=128):
        super().__init__(cfg, n_utterances, batch_size, seed, s_text=s_text, t_audio=400, n_visual_true=4, text_only=True)

    def __getitem__(self, i):
        (tx, _, _), lab = super().__getitem__(i)
        return {"input_ids": tx["input_ids"].unsqueeze(1), "attention_mask": tx["attention_mask"]}, lab


def prepare_dataloader(df, batch_size, label_task, epoch_switch, pin_memory=True, num_workers=0, check="train"):
    return DataLoader(df, batch_size=None, shuffle=False, num_workers=num_workers, pin_memory=pin_memory)


def runModel(accelerator, df_train, df_val, df_test, param_dict, model_param):
    device = accelerator
    criterion = build_criterion(param_dict, model_param["output_dim"], device)
    Metric = Metrics(num_classes=model_param["output_dim"], id2label=param_dict["id2label"], rank=device)
    if model_param.get("model") == "LSTM":
        model = LSTMClassifier(model_param["glove_vec"], model_param).to(device)
    else:
        model = BertClassifier(model_param).to(device)
    step = TextTrainStep(model, criterion, lr=param_dict["lr"], weight_decay=param_dict["weight_decay"], clip=param_dict["clip"])
    return clip_step_epochs(step, Metric, df_train, df_val, param_dict["epoch"], prepare_dataloader, param_dict["batch_size"])


def main(argv=None):
    args = arg_parse("Text", argv)
    refuse_tav_only(args)
    start(args, preset=True)
    cfg = C.default_config()
    param_dict = common_params(args, loss=args.loss, beta=args.beta, epoch_switch=args.epoch_switch)
    model_param = {"output_dim": args.output_dim, "dropout": args.dropout}
    s_text = 128
    if args.model == "LSTM":
        from .models.text import _first_hidden
        model_param.update(model="LSTM", lstm_layers=args.lstm_layers, hidden_layers=args.hidden_layers,
                           glove_vec=SyntheticVectors(cfg["text"]["vocab"], _first_hidden(args.hidden_layers), args.seed))
        s_text = 70                                                            # the reference pads every utterance to 70 tokens for this model
    mk = lambda n, seed: SyntheticTextBatches(cfg, n, args.batch_size, seed, s_text)   # noqa: E731
    return runModel("cuda", *synthetic_splits(mk, args)[:2], None, param_dict, model_param)


if __name__ == "__main__":
    main()
