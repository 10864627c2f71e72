"""Drop-in for the reference's SingleModels/models/visual.py::VisualClassification (:176-219), the default model of SingleModels/visual_nn.py:

    Conv3d(input_dim, h0, 3) -> GELU -> [Conv3d(h_i, h_i+1, 3) -> GELU]* -> flatten -> Linear(h_last T' H' W', output_dim) -> Sigmoid

on libtavhip's dense 3-D convolution (include/tavhip_conv.h): the clip is packed once into padded channels-last, every Conv3d + GELU is one
engine.Conv3dGeluFn, and flatten + Linear + Sigmoid is engine.FlatLinearSigmoidFn, which reads out_layer.weight in torch's own [O, C T' H' W']
flatten order.  state_dict keys are torch's: in_layer.*, hidden_layers.{i}.*, out_layer.*.

Deviations from the reference: hidden_layers is an nn.ModuleList (the reference's plain list leaves those layers
unregistered: on the CPU and untrained); out_layer.in_features is computed from args.get("clip_shape", (16, 224, 224)) and equals the
reference's hard-coded 18585600 at the defaults with hidden_layers 32,32; forward takes [B, 1, C, T, H, W] or [B, C, T, H, W] and returns
[B, output_dim] (flattened with .view(-1) only when output_dim == 1: the reference's cross entropy cannot take a flat [B * 7]).
ResNet50Classification needs torch.hub's slow_r50 weights, which cannot be had offline: it raises."""
import torch
from torch import nn

from ... import engine as E
from ... import ops, runtime


def hidden_layer_list(hidden_layers):
    """The reference's hidden_layer_count: "32,32" -> [32, 32]; ints, lists and tuples pass."""
    if isinstance(hidden_layers, str):
        return [int(h) for h in hidden_layers.split(",") if h.strip()]
    if isinstance(hidden_layers, int):
        return [hidden_layers]
    return [int(h) for h in hidden_layers]


class ResNet50Classification(nn.Module):
    def __init__(self, args):
        super().__init__()
        raise RuntimeError("ResNet50Classification (--model Video) loads the pretrained slow_r50 from torch.hub "
                           "('facebookresearch/pytorchvideo'); those hub weights are not available offline and the model is out of scope. "
                           "Run the default VisualClassification instead")


class VisualClassification(nn.Module):
    def __init__(self, args):
        super().__init__()
        self.input_dim = int(args["input_dim"])
        self.output_dim = int(args["output_dim"])
        self.hidden_dim = hidden_layer_list(args["hidden_layers"])
        self.clip_shape = tuple(int(v) for v in args.get("clip_shape", (16, 224, 224)))
        if not self.hidden_dim or len(self.clip_shape) != 3:
            raise ValueError(f"VisualClassification: hidden_layers {args['hidden_layers']!r} and clip_shape {self.clip_shape} must name at least one "
                             "width and (T, H, W)")
        shrink = 2 * len(self.hidden_dim)
        if min(self.clip_shape) <= shrink:
            raise ValueError(f"VisualClassification: {len(self.hidden_dim)} valid 3x3x3 convolutions leave nothing of a {self.clip_shape} clip")
        self.in_layer = nn.Conv3d(self.input_dim, self.hidden_dim[0], kernel_size=3)
        self.hidden_layers = nn.ModuleList(nn.Conv3d(self.hidden_dim[i], self.hidden_dim[i + 1], kernel_size=3) for i in range(len(self.hidden_dim) - 1))
        T, H, W = (s - shrink for s in self.clip_shape)
        self.out_layer = nn.Linear(self.hidden_dim[-1] * T * H * W, self.output_dim)

    def forward(self, x):
        dev = self.out_layer.weight.device
        if dev.type != "cuda":
            raise RuntimeError("VisualClassification runs on libtavhip (GPU) only; there is no CPU fallback")
        ectx = runtime.ctx()
        if ectx.pol.fp8:
            raise ValueError(f"VisualClassification runs under the bf16 and fp32 policies, not {ectx.pol.name!r}")
        if x.dim() == 6:
            x = x.squeeze(1)                                                              # reference :202
        if x.dim() != 5 or tuple(x.shape[1:]) != (self.input_dim,) + self.clip_shape:
            raise ValueError(f"VisualClassification: expected clips [B, {self.input_dim}, {', '.join(map(str, self.clip_shape))}] "
                             f"(or with a singleton second axis), got {tuple(x.shape)}")
        x = x.to(dev, torch.float32).contiguous()
        a = ops.conv3d_pack_input(x, ectx.pol.lp)
        for layer in [self.in_layer, *self.hidden_layers]:                                # :209-215
            a = E.Conv3dGeluFn.apply(a, layer.weight, layer.bias, ectx)
        out = E.FlatLinearSigmoidFn.apply(a, self.out_layer.weight, self.out_layer.bias, self.hidden_dim[-1], ectx)   # :216-218
        return out.view(-1) if self.output_dim == 1 else out
