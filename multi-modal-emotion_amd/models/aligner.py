"""The CTC model the forced alignment runs on (reference run_scripts/get_times.py: torchaudio's WAV2VEC2_ASR_BASE_960H bundle).

wav2vec2-base with a vocabulary head: the audio geometry of preset B (GroupNorm conv stack, post-LN encoder), which encoders.AudioEncoder
already runs on libtavhip, and a Linear(768, vocab) on top.  The state_dict keys are those of HF Wav2Vec2ForCTC (`wav2vec2.*`,
`lm_head.*`), so a converted checkpoint of the model the reference uses loads as it is.  The head is the NT GEMM of the library with the
weight padded to a multiple of four rows (zero rows; tav_ctc_log_softmax leaves the pad columns out)."""
import torch
from torch import nn

from .. import config as cfgmod
from .. import ops, runtime
from ..encoders import AudioEncoder


class CTCAligner(nn.Module):
    def __init__(self, cfg=None, vocab=29):
        super().__init__()
        cfg = cfgmod.preset("B") if cfg is None else cfg
        self.cfg = cfg
        self.vocab = int(vocab)
        self.wav2vec2 = AudioEncoder(cfg["audio"])
        self.lm_head = nn.Linear(cfg["audio"]["hidden"], self.vocab)
        self._head = None                      # (key, padded weight operand, padded bias)

    @property
    def vocab_padded(self):
        return (self.vocab + 3) // 4 * 4

    def _head_operands(self, dtype):
        w, b = self.lm_head.weight, self.lm_head.bias
        key = (w.data_ptr(), w._version, b.data_ptr(), b._version, dtype, w.device)
        if self._head is None or self._head[0] != key:
            Vp, H = self.vocab_padded, w.shape[1]
            wp = torch.zeros(Vp, H, dtype=torch.float32, device=w.device)
            bp = torch.zeros(Vp, dtype=torch.float32, device=w.device)
            wp[:self.vocab].copy_(w.detach())
            bp[:self.vocab].copy_(b.detach())
            self._head = (key, wp if dtype == torch.float32 else ops.cast2d(wp, dtype), bp)
        return self._head[1], self._head[2]

    def logits_padded(self, waveforms):
        """waveforms f32 [B, L] on the device -> logits f32 [B, T', vocab_padded]; columns [vocab, vocab_padded) are the zero rows' 0.0."""
        with torch.no_grad():
            x, x_lp, T = self.wav2vec2(waveforms)
            pol = runtime.ctx().pol
            a = x if pol.f32 else x_lp
            w, b = self._head_operands(pol.lp)
            y = ops.gemm_nt(a, w, bias=b, out_dtype=torch.float32)
        return y.view(waveforms.shape[0], T, self.vocab_padded)

    def forward(self, waveforms):
        """(logits [B, T', vocab], lengths): the call shape of the reference's `emissions, _ = model(waveform)`; lengths is None, as
        torchaudio returns it when no lengths were passed."""
        return self.logits_padded(waveforms)[..., :self.vocab], None

    def emission(self, waveforms, out=None):
        """Log-probabilities f32 [B, T', vocab_padded] with `vocab` valid columns: what ops.ctc_align reads (V = self.vocab)."""
        return ops.ctc_log_softmax(self.logits_padded(waveforms), V=self.vocab, out=out)
