"""Writes tests/golden/soft_f_loss_golden.npz: what the reference's own soft F1 gives for soft_f_ref.GOLDEN_INPUTS.

    python tests/make_soft_f_golden.py /path/to/reference

The class F1_Loss is cut out of the reference's notebooks/loss.ipynb with `json` and `ast` when this runs and executed with torch alone;
none of its text is kept here or in the record.  Per case the record holds the logits, the targets, and -- with `weights` 1 and with the
vector soft_f_ref.class_weights(C) -- the loss and its autograd gradient as the notebook's f32 arithmetic gives them."""
import ast
import json
import os
import sys

import numpy as np
import torch

import soft_f_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "soft_f_loss_golden.npz")


def reference_class(root):
    nb = json.load(open(os.path.join(root, "notebooks", "loss.ipynb")))
    found = None
    for cell in nb["cells"]:
        if cell["cell_type"] != "code":
            continue
        try:
            tree = ast.parse("".join(cell["source"]))
        except SyntaxError:                                   # (a cell of shell magics)
            continue
        for node in tree.body:
            if isinstance(node, ast.ClassDef) and node.name == "F1_Loss":
                found = node                                  # the last definition is the one the notebook ends with
    assert found is not None
    ns = {"torch": torch, "nn": torch.nn, "F": torch.nn.functional}
    exec(compile(ast.Module(body=[found], type_ignores=[]), "loss.ipynb", "exec"), ns)
    return ns["F1_Loss"]


def main(root):
    F1 = reference_class(root)
    out = {}
    for B, C, scale, seed in R.GOLDEN_INPUTS:
        z, t = R.named_inputs(B, C, scale, seed)
        name = f"B{B}_C{C}_x{scale:g}_s{seed}"
        out[name + ".z"], out[name + ".t"] = z.numpy(), t.numpy()
        for tag, w in (("w1", 1), ("wv", R.class_weights(C))):
            zz = z.clone().requires_grad_(True)
            loss = F1(num_classes=C, weights=w)(zz, t)
            loss.backward()
            out[f"{name}.{tag}.loss"], out[f"{name}.{tag}.grad"] = loss.detach().numpy().astype(np.float32), zz.grad.numpy().astype(np.float32)
            print(f"{name} {tag}: loss {loss.item():.7f}")
    np.savez_compressed(GOLDEN, **out)
    print(f"{GOLDEN}: {os.path.getsize(GOLDEN)} bytes")


if __name__ == "__main__":
    main(sys.argv[1])
