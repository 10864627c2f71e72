"""Drop-in for the reference's tav_nn.py (entrypoint of the TAV path): same main() / runModel() / prepare_dataloader()
shape and the same CLI flags (utils/global_functions.arg_parse).  The reference reads a dataset pickle + mp4/wav files and a
wandb sweep config (tav_nn.py:116-188); offline there is neither, so utterances come from synthetic.make_batch with the
contract of collate_batch."""
import torch
from torch.utils.data import DataLoader

from . import config as C
from . import runtime
from .models.tav import PreFormer, TAVForMAE
from .train_model.tav_train import evaluate_tav, train_tav_network
from .utils.entrypoint import SyntheticBatches, build_criterion, common_params, start, synthetic_splits
from .utils.global_functions import Metrics, arg_parse


class SyntheticTAVBatches(SyntheticBatches):
    """Each item is one already-collated batch (the reference's DataLoader yields ([text, audio, visual], labels))."""

    def __init__(self, cfg, n_utterances, batch_size, seed, s_text=70, t_audio=80000):
        super().__init__(cfg, n_utterances, batch_size, seed, s_text=s_text, t_audio=t_audio)

    def __getitem__(self, i):
        nv = 104 if self.cfg["video"]["image"] == 224 else 4
        if runtime.visual_rows() == "ragged":     # unequal rows around the same mean (a seeded spread of +-2 tokens)
            g = torch.Generator().manual_seed(self.seed + i)
            nv = [nv + int(d) for d in torch.randint(-2, 3, (self.bs,), generator=g)]
        return super().__getitem__(i, n_visual_true=nv)


def prepare_dataloader(df, batch_size, label_task, epoch_switch, pin_memory=True, num_workers=0, check="train"):
    """`df` is a SyntheticTAVBatches here (reference: a pandas frame of file paths, tav_nn.py:28-57)."""
    return DataLoader(df, batch_size=None, shuffle=False, num_workers=num_workers, pin_memory=pin_memory)


def runModel(accelerator, df_train, df_val, df_test, param_dict, model_param):
    device = accelerator
    criterion = build_criterion(param_dict, model_param["output_dim"], device)
    sync = param_dict.get("loop_sync", "step")
    Metric = Metrics(num_classes=model_param["output_dim"], id2label=param_dict["id2label"], rank=device, on_device=sync == "log")
    bs, lt, es = param_dict["batch_size"], param_dict["label_task"], param_dict["epoch_switch"]
    dl_train = prepare_dataloader(df_train, bs, lt, es, check="train")
    dl_val = prepare_dataloader(df_val, bs, lt, es, check="val")
    dl_test = prepare_dataloader(df_test, bs, lt, es, check="val")
    model = TAVForMAE(model_param).to(device)
    PREFormer = PreFormer().to(device)
    model, PREFormer = train_tav_network(model, PREFormer, dl_train, dl_val, criterion, param_dict["lr"], param_dict["epoch"], param_dict["weight_decay"],
                                         param_dict["T_max"], Metric, param_dict["patience"], param_dict["clip"], es, None,
                                         graphs=bool(param_dict.get("graph", 0)), sync=sync, encoder_lr_scale=param_dict.get("encoder_lr_scale", 1.0),
                                         no_decay_norm_bias=bool(param_dict.get("no_decay_norm_bias", 0)))
    evaluate_tav(model, PREFormer, dl_test, Metric, sync=sync)
    return model, PREFormer


def main(argv=None):
    args = arg_parse("TAV", argv)
    start(args, preset=True)
    runtime.set_visual_rows(args.visual_rows, bucket=args.visual_bucket)
    runtime.set_specaugment(args.specaugment)
    cfg = C.default_config()
    param_dict = common_params(args, model=args.model, T_max=args.T_max, seed=args.seed, label_task=args.label_task, mask=args.mask, loss=args.loss,
                               beta=args.beta, epoch_switch=args.epoch_switch)
    param_dict.update(graph=args.graph, loop_sync=args.loop_sync, encoder_lr_scale=args.encoder_lr_scale,      # last in the dict printed below
                      no_decay_norm_bias=args.no_decay_norm_bias)
    model_param = {"output_dim": args.output_dim, "dropout": args.dropout, "early_div": args.early_div, "num_layers": args.num_layers,
                   "learn_PosEmbeddings": args.learn_PosEmbeddings}
    small = cfg["video"]["image"] != 224
    mk = lambda n, seed: SyntheticTAVBatches(cfg, n, args.batch_size, seed, s_text=16 if small else 70, t_audio=8000 if small else 80000)   # noqa: E731
    print(f" in main \n param_dict = { {k: v for k, v in param_dict.items() if k != 'weights'} } \n model_param = {model_param} \n synthetic utterances = {args.synthetic}")
    return runModel("cuda", *synthetic_splits(mk, args), param_dict, model_param)


if __name__ == "__main__":
    main()
