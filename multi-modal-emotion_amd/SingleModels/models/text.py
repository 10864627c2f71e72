"""Drop-ins for the reference's SingleModels/models/text.py.  `LSTMClassifier` (:9-39): frozen GloVe embedding -> nn.LSTM(hidden, hidden,
num_layers, batch_first=True) -> Linear(hidden, output_dim) -> Dropout(0.5) -> mean over time -> LogSigmoid, on the recurrence kernels of
include/tavhip_rnn.h ("LSTM recurrence").  `BertClassifier` (:41-69): text encoder -> pooler -> dropout (only when
check == "train") -> Linear(768, output_dim), executed by libtavhip (BASELINE.json configs[0]).
The reference builds the encoder with `BertModel.from_pretrained('j-hartmann/emotion-english-distilroberta-base')` (:48), a network
fetch; here the geometry comes from the preset's "text" block (config.py) and weights are loaded by the caller."""
import math

import torch
from torch import nn

from ... import config as C
from ... import engine as E
from ... import ops
from ... import runtime
from ...encoders import TextEncoder


class BertClassifier(nn.Module):
    def __init__(self, args, dropout=0.5, config=None):
        super().__init__()
        cfg = config if config is not None else C.default_config()
        self.cfg = cfg
        self.dropout_p = float(args["dropout"])          # reference :44 (the `dropout` keyword is shadowed there as well)
        self.output_dim = args["output_dim"]
        self.bert = TextEncoder(cfg["text"])
        self.linear = nn.Linear(768, self.output_dim)
        self._drop_calls = 0

    def forward(self, input_id, mask, check):
        dev = self.linear.weight.device
        if dev.type != "cuda":
            raise RuntimeError("BertClassifier runs on libtavhip (GPU) only; there is no CPU fallback")
        _, x = self.bert(input_id.to(dev), mask.to(dev))                                    # :58 (pooled output)
        p = self.dropout_p if check == "train" else 0.0                                      # :61-62
        seed, = runtime.dropout_seeds(self, "_drop_calls", draw=p > 0.0)        # (a device word under a capture)
        return E.HeadFn.apply(x, p, seed, self.linear.weight, self.linear.bias)              # :65


def _first_hidden(v):
    """args['hidden_layers'] as the reference reads it: its first entry, given as an int, a list / tuple, or a string such as "300" or "300,300"."""
    if isinstance(v, str):
        v = [p for p in v.replace(",", " ").split() if p]
    if isinstance(v, (list, tuple)):
        if not v:
            raise ValueError("hidden_layers is empty")
        v = v[0]
    return int(v)


class _LstmWeights(nn.Module):
    """The parameters of nn.LSTM(input, hidden, num_layers) under torch's names and initialisation (U(-1/sqrt(hidden), 1/sqrt(hidden)))."""

    def __init__(self, input_size, hidden_size, num_layers):
        super().__init__()
        self.input_size, self.hidden_size, self.num_layers = input_size, hidden_size, num_layers
        k = 1.0 / math.sqrt(hidden_size)
        for layer in range(num_layers):
            for name, shape in ((f"weight_ih_l{layer}", (4 * hidden_size, input_size if layer == 0 else hidden_size)), (f"weight_hh_l{layer}", (4 * hidden_size, hidden_size)),
                                (f"bias_ih_l{layer}", (4 * hidden_size,)), (f"bias_hh_l{layer}", (4 * hidden_size,))):
                self.register_parameter(name, nn.Parameter(torch.empty(shape).uniform_(-k, k)))

    def layer(self, k):
        return tuple(getattr(self, f"{n}_l{k}") for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))


class LSTMClassifier(nn.Module):
    """glove_vec: any object with a `.vectors` [V, E] tensor (torchtext's GloVe has one).  state_dict keys are torch's own: embedding.weight,
    lstm.weight_ih_l{k} / weight_hh_l{k} / bias_ih_l{k} / bias_hh_l{k}, fc2.weight, fc2.bias -- a checkpoint of the reference loads as it is."""

    def __init__(self, glove_vec, args):
        super().__init__()
        self.output_dim = args["output_dim"]
        self.hidden_dim = _first_hidden(args["hidden_layers"])
        self.LSTM_layers = int(args["lstm_layers"])
        self.dropout_p = 0.5                                                                # reference :20
        vectors = torch.as_tensor(glove_vec.vectors).detach().to(torch.float32)
        if vectors.dim() != 2 or vectors.shape[1] != self.hidden_dim:
            raise ValueError(f"LSTMClassifier: the embedding width {tuple(vectors.shape)[-1]} must equal hidden_dim {self.hidden_dim} "
                             "(nn.LSTM(input_size=hidden_dim, ...) of the reference cannot run otherwise)")
        self.embedding = nn.Embedding.from_pretrained(vectors.clone(), freeze=True)          # reference :22
        self.lstm = _LstmWeights(self.hidden_dim, self.hidden_dim, self.LSTM_layers)
        self.fc2 = nn.Linear(self.hidden_dim, self.output_dim)
        self._drop_calls = 0

    def forward(self, x):
        dev = self.fc2.weight.device
        if dev.type != "cuda":
            raise RuntimeError("LSTMClassifier runs on libtavhip (GPU) only; there is no CPU fallback")
        ectx = runtime.ctx()
        if ectx.pol.fp8:
            raise ValueError(f"LSTMClassifier runs under the bf16 and fp32 policies, not {ectx.pol.name!r}")
        B, T = x.shape
        V, Ew = self.embedding.weight.shape
        Ep = (Ew + 63) // 64 * 64
        table, _ = ectx.cache.padded_f32(self.embedding.weight, V, Ep)
        ids = x.to(dev).t().contiguous().to(torch.int32).view(-1)                            # time-major rows (t, b): the layout of the recurrence
        out = ops.gather_rows(table, ids)                                                  # :31
        for k in range(self.LSTM_layers):                                                    # :32 (no dropout between the layers: torch's default)
            out, _, _ = E.LstmLayerFn.apply(out, *self.lstm.layer(k), None, None, ectx, B, T)
        p = self.dropout_p if self.training else 0.0
        seed, = runtime.dropout_seeds(self, "_drop_calls", draw=p > 0.0)
        return E.LstmTailFn.apply(out, self.fc2.weight, self.fc2.bias, p, seed, ectx, B, T)  # :34-37
