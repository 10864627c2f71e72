"""-m gpu: the shared epoch loop (train_model/classifier_loop.py) through its two drop-in names, visual_train and train_audio_network, on
tiny models: each keeps its own log record, counts every row, trains each epoch with the cosine rate set at the end of the previous one
(read from the optimizer at every step), and leaves finite losses."""
import math

import pytest
import torch

import tav_amd  # noqa: F401
from tav_amd import config as C
from tav_amd import runtime
from tav_amd.SingleModels import audio_nn, visual_nn
from tav_amd.SingleModels.models.audio import Wav2Vec2ForSpeechClassification
from tav_amd.SingleModels.models.visual import VisualClassification
from tav_amd.SingleModels.train_model.audio_training import cosine_annealing_lr, train_audio_network
from tav_amd.SingleModels.train_model.visual_training import visual_train
from tav_amd.train_model import classifier_loop
from tav_amd.utils.global_functions import CrossEntropyLoss, Metrics

pytestmark = pytest.mark.gpu
O = 7
COMMON_KEYS = {"epoch", "train/batch_loss", "train/train_loss", "train/acc", "train/f1-score", "train/cm", "val/total_loss_val", "val/total_acc_val",
               "val/f1-score", "val/cm"}


def _visual():
    clip = (6, 12, 20)
    model = VisualClassification({"input_dim": 3, "output_dim": O, "hidden_layers": "16,32", "clip_shape": clip}).cuda()
    train = visual_nn.prepare_dataloader(visual_nn.SyntheticClips(6, clip, O, 1), 3, clip_shape=clip, shuffle=False)
    val = visual_nn.prepare_dataloader(visual_nn.SyntheticClips(3, clip, O, 2), 3, clip_shape=clip, shuffle=False)
    return model, train, val, dict(run=visual_train, base=1e-3, epochs=2, patience=None, n_train=6, n_val=3, keys=COMMON_KEYS)


def _audio():
    model = Wav2Vec2ForSpeechClassification({"output_dim": O}, config=C.preset("B-tiny")).cuda()
    train = audio_nn.prepare_dataloader(audio_nn.SyntheticUtterances(6, (0.1, 0.3), 16000, O, 1), 2, shuffle=False)
    val = audio_nn.prepare_dataloader(audio_nn.SyntheticUtterances(6, (0.1, 0.3), 16000, O, 2), 2, shuffle=False)
    return model, train, val, dict(run=train_audio_network, base=1e-4, epochs=3, patience=1, n_train=6, n_val=6,
                                   keys=COMMON_KEYS | {"lr", "val/batch_loss", "restored"})


@pytest.mark.parametrize("case", [_visual, _audio], ids=["visual", "audio"])
def test_each_drop_in_keeps_its_record_and_the_cosine_rate(gpu, monkeypatch, case):
    stepped = []

    class Spy(classifier_loop.FusedAdamW):
        def step(self):
            stepped.append(self.lr)
            return super().step()

    monkeypatch.setattr(classifier_loop, "FusedAdamW", Spy)
    torch.manual_seed(0)
    runtime.set_precision("bf16")
    model, train, val, k = case()
    T_max, log = 2, []
    k["run"](model, train, val, CrossEntropyLoss(weight=torch.linspace(0.6, 0.95, O)), k["base"], k["epochs"], 1e-4, T_max, Metrics(num_classes=O, rank="cuda"),
             patience=k["patience"], clip=1.0, log=log)
    assert [e["epoch"] for e in log] == list(range(k["epochs"])) and all(set(e) == k["keys"] for e in log), [sorted(e) for e in log]
    assert all(int(e["train/cm"].sum()) == k["n_train"] and int(e["val/cm"].sum()) == k["n_val"] for e in log)
    # every step of epoch e ran with the closed form's rate for e: the rate is moved after the training pass, so it holds from the next epoch on
    per_epoch = len(train)
    want = [cosine_annealing_lr(k["base"], e, T_max) for e in range(k["epochs"])]
    assert len(stepped) == k["epochs"] * per_epoch
    assert all(stepped[e * per_epoch + i] == want[e] for e in range(k["epochs"]) for i in range(per_epoch)), (stepped, want)
    if "lr" in k["keys"]:
        assert [e["lr"] for e in log] == want
    losses = [e[n] for e in log for n in ("train/batch_loss", "train/train_loss", "val/total_loss_val", "val/batch_loss") if n in e]
    print(f"{case.__name__}: rates {want}, losses {losses}")
    assert all(math.isfinite(v) for v in losses), losses
