"""Writes tests/golden/audio_classifier_golden.npz: what the Hugging Face module the reference calls gives for the audio-only classifier
on audio_classifier_ref's batch.

    python tests/make_audio_classifier_golden.py [/path/to/reference]

Per preset (A-tiny, B-tiny) a transformers Wav2Vec2Model is built from a LOCAL Wav2Vec2Config (eager attention, .eval(); no checkpoint is
fetched) next to a Linear(hidden, 7) under the reference's attribute names (wav2vec2, dropout, out_proj), filled with the closed-form
weights of tests/closed_form.py (f32 values; no weight blobs are stored), and run as the reference composes it: wav2vec2(input_values)[0],
mean over dim 1, dropout (off under .eval()), out_proj; then cross entropy and backward.  The record holds the logits, the pooled hidden
states, the loss and the global gradient norm.  The modules run in float64 (module.double()): the record pins HF's arithmetic, not one
float32 rounding of it -- in float32 the A-tiny logits of the same modules sit 2e-5 from these (gradient norm 2.5e3, closed-form weights),
B-tiny 3e-7.

With the reference's root given, the body of its Wav2Vec2ForSpeechClassification.forward is cut out of SingleModels/models/audio.py with
`ast` when this runs and executed on the same modules (the file itself imports torchaudio, which need not be there); it must agree bit
for bit with the composition written here, and the record is taken from it.  None of its text is kept here or in the record."""
import ast
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import audio_classifier_ref as R  # noqa: E402
import closed_form as cf  # noqa: E402
from oracle import tav_oracle as O  # noqa: E402
from oracle.validate_vs_reference import bind_reference, hf_audio  # noqa: E402


class RefSpeechClassifier(torch.nn.Module):
    """The reference's module from a local config: same attribute names, so the same state_dict keys."""

    def __init__(self, audio_cfg):
        super().__init__()
        self.output_dim = R.OUTPUT_DIM
        self.wav2vec2 = hf_audio(audio_cfg)
        self.dropout = torch.nn.Dropout(.5)
        self.out_proj = torch.nn.Linear(audio_cfg["hidden"], R.OUTPUT_DIM)
        cf.fill_module_(self)
        self.eval()

    def forward(self, input_values):
        return self.out_proj(self.dropout(torch.mean(self.wav2vec2(input_values)[0], dim=1)))


def reference_forward(root):
    path = os.path.join(root, "SingleModels", "models", "audio.py")
    with open(path) as f:
        tree = ast.parse(f.read(), filename=path)
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Wav2Vec2ForSpeechClassification")
    fwd = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "forward"]
    assert len(fwd) == 1
    ns = {"torch": torch, "nn": torch.nn}
    exec(compile(ast.Module(body=fwd, type_ignores=[]), path, "exec"), ns)
    return {("Wav2Vec2ForSpeechClassification", "forward"): ns["forward"]}


def main(root=None):
    fns = reference_forward(root) if root else None
    wave, labels = R.batch()
    wave = wave.double()
    out = {}
    for name in R.PRESETS:
        cfg = O.preset(name)
        ref = RefSpeechClassifier(cfg["audio"]).double()
        hidden = ref.wav2vec2(wave)[0]
        assert hidden.shape[1] == R.SA
        logits = ref(wave)
        if fns is not None:
            logits_x = bind_reference(ref, "Wav2Vec2ForSpeechClassification", fns).forward(wave)
            assert torch.equal(logits_x, logits), "the composition written here differs from the reference's own forward"
            logits = logits_x
        loss = torch.nn.functional.cross_entropy(logits, labels)
        loss.backward()
        named = dict(ref.named_parameters())
        assert named["wav2vec2.masked_spec_embed"].grad is None
        gn = torch.sqrt(sum((p.grad.double() ** 2).sum() for p in named.values() if p.grad is not None)).item()
        o = R.oracle_run(ref.state_dict(), cfg["audio"], wave, labels)
        errs = dict(logits=((o["logits"] - logits.detach().double()).abs().max() / o["logits"].abs().max()).item(),
                    loss=abs(o["loss"] - loss.item()) / abs(o["loss"]), gradnorm=abs(o["gradnorm"] - gn) / o["gradnorm"])
        print(f"{name}: loss {loss.item():.6f} gradnorm {gn:.4e}; HF vs oracle, both float64: " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items())
              + ("; reference forward body executed, bitwise equal" if fns else ""))
        assert max(errs.values()) < 1e-5
        out[f"{name}_logits"] = logits.detach().numpy()
        out[f"{name}_pooled"] = torch.mean(hidden, dim=1).detach().numpy()
        out[f"{name}_loss"] = np.array([loss.item()])
        out[f"{name}_gradnorm"] = np.array([gn])
    np.savez_compressed(R.GOLDEN, **out)
    print(f"{R.GOLDEN}: {os.path.getsize(R.GOLDEN)} bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
