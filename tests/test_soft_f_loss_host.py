"""CPU: the soft F-beta / soft precision loss's host side.

tests/soft_f_ref.py's twin at beta = 1 against what the reference's own soft F1 gave (tests/golden/soft_f_loss_golden.npz, written by
tests/make_soft_f_golden.py); the clamp guard on every named and exact case; csrc/tavhip_loss.h against its private binding table type by
type; every refusal of the validator through the built library; csrc/loss_plan.h alone under ASan + UBSan as a program of its own
(tests/host_program.py); the criteria, the criterion of --loss, and the flags' defaults."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import abi_check
import soft_f_ref as R
import tav_amd  # noqa: F401
from host_program import host_compilers, run_alone_under_sanitizers
from tav_amd import _lib, ops
from tav_amd.utils import global_functions as GF
from tav_amd.utils.entrypoint import build_criterion

ERR_NULL, ERR_SHAPE = -1, -2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi-modal-emotion_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "soft_f_loss_golden.npz")


# ---------------------------------------------------------------------------------------------- the twin against the reference's own function
def _f32_chain_bounds(z, t, w, loss, g_own_other):
    """Bounds on what the notebook's f32 arithmetic (torch, CPU) may differ from float64 by, in the construction of soft_f_ref: roundings
    times u times summed magnitudes.  delta = the roundings on a class sum: 14 + max |z - m| for a probability (soft_f_ref's r + r_se + u
    with expf at 6 u, twice, and the division) and B for the f32 sum over the rows.  P and R are quotients of positive sums, 2 delta + 3
    each; F = 2 P R / (P + R + eps): N_F = 6 delta + 20.  The loss adds the C weighted terms: (N_F + C + 1) u sum_k |w_k| F_k, and u |loss|.
    A coefficient dL/dtp, dL/dfp, dL/dfn is a sum of same-signed products of such quotients with three times the occurrences:
    N_g = 3 N_F; dlogits = p (g - sum_j p_j g_j): (N_g + 2 delta + C + 3) u p (|g| + sum_j p_j |g_j|)."""
    B, Cn = z.shape
    zz = z.double().numpy()
    delta = 14 + float(np.abs(zz - zz.max(1, keepdims=True)).max()) + B
    n_f = 6 * delta + 20
    p = torch.softmax(z.double(), 1)
    F = R.f_score(*R.counts(p, t), 1.0, "FBeta").clamp(R.EPS, 1 - R.EPS)
    loss_b = (n_f + Cn + 1) * R.U * float((w.abs() * F).sum()) + R.U * abs(loss)
    own, other = g_own_other
    oh = (t[:, None] == torch.arange(Cn)[None, :])
    g = torch.where(oh, own[None, :], other[None, :]).abs()
    grad_b = (3 * n_f + 2 * delta + Cn + 3) * R.U * (p * (g + (p * g).sum(1, keepdim=True))).numpy() + R.TINY
    return loss_b, grad_b


def test_twin_at_beta_one_reproduces_the_reference_f1_loss():
    gold = np.load(GOLDEN)
    worst = 0.0
    for B, Cn, scale, seed in R.GOLDEN_INPUTS:
        name = f"B{B}_C{Cn}_x{scale:g}_s{seed}"
        z, t = R.named_inputs(B, Cn, scale, seed)
        assert np.array_equal(gold[name + ".z"], z.numpy()) and np.array_equal(gold[name + ".t"], t.numpy()), name     # the record's inputs are the list's
        for tag, w in (("w1", None), ("wv", R.class_weights(Cn))):
            ref = R.reference(z, t, w, 1.0, "FBeta")
            w64 = torch.ones(Cn, dtype=torch.float64) if w is None else w.double()
            d1, _ = R._class_derivatives(*(torch.from_numpy(s) for s in ref["stats"]), w64, 1.0, "FBeta", R.EPS)
            loss_b, grad_b = _f32_chain_bounds(z, t, w64, ref["loss"][0], (torch.from_numpy(d1[0] - d1[2]), torch.from_numpy(d1[1])))
            rl = R.ratio(gold[f"{name}.{tag}.loss"].reshape(1), ref["loss"], loss_b)
            rg = R.ratio(gold[f"{name}.{tag}.grad"], ref["dlogits"], grad_b)
            print(f"{name} {tag}: loss error / bound {rl:.3f}, gradient {rg:.3f}")
            worst = max(worst, rl, rg)
            assert rl <= 1.0 and rg <= 1.0, (name, tag, rl, rg)
    assert worst > 0.0                                       # f32 against f64: they are not the same numbers


def test_every_named_and_exact_case_passes_the_clamp_guard():
    assert len(R.NAMED) == 864 and len(set(R.NAMED)) == 864
    seen = set()
    for B, Cn, beta, mode, scale, seed in R.NAMED:
        ok, F64, F32, br = R.guard(*R.named_inputs(B, Cn, scale, seed), beta, mode)
        assert ok, (B, Cn, beta, mode, scale, seed, F64.tolist(), F32.tolist())
        seen.update(br.tolist())
    for name, beta, mode in R.EXACT:
        z, t = R.exact_inputs(name)
        ok, F64, F32, br = R.guard(z, t, beta, mode)
        assert ok, (name, beta, mode)
        seen.update(br.tolist())
        if name == "saturated":                              # both sides compute the same float64 numbers: p is 0 or 1 exactly
            assert torch.equal(F64, F32) and br.tolist() == [1, 1, 1, -1]
            g = R.exact_reference(name, beta, mode)["dlogits"]
            assert not g.any()                               # every class is clamped: no gradient at all
        if name == "absent_p0":
            assert br[2] == -1 and F64[2] == 0 and not R.exact_reference(name, beta, mode)["dlogits"][:, 2].any()
    assert seen == {-1, 0, 1}                                # the lists reach both clamp edges and the pass-through


def test_reference_refuses_a_case_that_fails_the_guard():
    """The generator asserts the guard.  One row of two classes with p_0 = 1 - eps puts P_0 = p_0 / (p_0 + eps) on the upper edge; f32 holds
    no number within 1.9e-8 of that p_0, so the two F differ by far more than a sixteenth of the distance to the edge: refused, not measured."""
    z, t = torch.tensor([[0.0, -math.log(1e7 - 1)]]), torch.tensor([0])
    assert not R.guard(z, t, 1.0, "Precision")[0]
    with pytest.raises(AssertionError, match="clamp guard"):
        R.reference(z, t, None, 1.0, "Precision")
    assert R.guard(torch.zeros(1, 2), t, 1.0, "Precision")[0]


def test_twin_gradient_is_the_issue_formula():
    """dz = p (g - sum_j p_j g_j) with g from the stated partial derivatives, against autograd, on a case with every clamp branch."""
    for name, beta, mode in R.EXACT:
        z, t = R.exact_inputs(name)
        _, dl, stats = R.twin(z, t, R.class_weights(z.shape[1]), beta, mode)
        tp, fp, fn = (torch.from_numpy(s) for s in stats)
        eps, b2, w = R.EPS, beta * beta, R.class_weights(z.shape[1]).double()
        dp, dr = tp + fp + eps, tp + fn + eps
        P, Rc = tp / dp, tp / dr
        if mode == "Precision":
            F, dF = P, ((fp + eps) / dp ** 2, -tp / dp ** 2, torch.zeros_like(tp))
        else:
            Q = b2 * P + Rc + eps
            F = (1 + b2) * P * Rc / Q
            fP, fR = (1 + b2) * Rc * (Rc + eps) / Q ** 2, (1 + b2) * P * (b2 * P + eps) / Q ** 2
            dF = (fP * (fp + eps) / dp ** 2 + fR * (fn + eps) / dr ** 2, fP * -tp / dp ** 2, fR * -tp / dr ** 2)
        passes = ((F >= eps) & (F <= 1 - eps)).double()
        a, b, c = (-w * passes * d for d in dF)
        p = torch.softmax(z.double(), 1)
        oh = (t[:, None] == torch.arange(z.shape[1])[None, :])
        g = torch.where(oh, (a - c)[None, :], b[None, :])
        want = p * (g - (p * g).sum(1, keepdim=True))
        assert np.abs(want.numpy() - dl).max() <= 1e-12 * max(1.0, np.abs(dl).max()), (name, beta, mode)


# ---------------------------------------------------------------------------------------------- loss_plan.h alone
def test_loss_plan_header_alone_under_sanitizers(tmp_path):
    for cxx, lines in run_alone_under_sanitizers("loss_plan_check.cpp", tmp_path).items():
        assert any(ln.startswith("accepted ") for ln in lines), cxx


# ---------------------------------------------------------------------------------------------- private header against its binding
def _private_header():
    src = open(os.path.join(CSRC, "tavhip_loss.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_private_loss_binding_matches_its_header_type_by_type(tmp_path):
    (abi,) = _lib.PRIVATE_ABIS
    assert abi.header == "tavhip_loss.h" and abi.sigs is _lib._LOSS_SIGS and abi.version == _lib.LOSS_ABI_VERSION == 1
    assert not os.path.exists(os.path.join(abi_check.INCLUDE, abi.header))               # private for now: not a public header
    structs, protos = abi_check.parse_header_text(_private_header())
    assert set(protos) == set(abi.sigs) == {"tav_loss_version", "tav_soft_f_loss"}
    for name, (res, args) in protos.items():
        cres, cargs = abi.sigs[name]
        assert abi_check._ctypes_class(cres) == res and len(cargs) == len(args), name
        for k, (ct, (kind, struct)) in enumerate(zip(cargs, args)):
            assert abi_check._ctypes_class(ct) == kind, f"{name}: argument {k}"
            assert struct is None or ct._type_ is abi.structs[struct], f"{name}: argument {k}"
    assert set(structs) == set(abi.structs) == {"tav_soft_f_args"}
    fields = structs["tav_soft_f_args"]
    assert [f for f, _ in _lib.SoftFArgs._fields_] == [f[0] for f in fields]
    for (fname, ct), (_, kind, dim) in zip(_lib.SoftFArgs._fields_, fields):
        assert dim == 0 and abi_check._ctypes_class(ct) == kind, fname
    # sizeof / offsetof as a C++ host compiler lays the struct out (the header is read by C++ only until it is promoted)
    cxx = host_compilers()[0][0]
    lines = ['#include <cstdio>', '#include <cstddef>', f'#include "{os.path.join(CSRC, "tavhip_loss.h")}"', 'int main() {',
             '    std::printf("tav_soft_f_args %zu\\n", sizeof(tav_soft_f_args));']
    lines += [f'    std::printf("{f} %zu\\n", offsetof(tav_soft_f_args, {f}));' for f, _, _ in fields]
    lines += ['    std::printf("modes %d %d\\n", TAV_SOFT_F_FBETA, TAV_SOFT_F_PRECISION);', '    return 0;', '}']
    (tmp_path / "layout.cpp").write_text("\n".join(lines) + "\n")
    subprocess.run([cxx, "-std=c++17", str(tmp_path / "layout.cpp"), "-o", str(tmp_path / "layout")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines()
    laid = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in out}
    assert C.sizeof(_lib.SoftFArgs) == laid["tav_soft_f_args"][0]
    for f, _ in _lib.SoftFArgs._fields_:
        assert getattr(_lib.SoftFArgs, f).offset == laid[f][0], f
    assert laid["modes"] == [_lib.SOFT_F_FBETA, _lib.SOFT_F_PRECISION] == [ops.SOFT_F_MODES["FBeta"], ops.SOFT_F_MODES["Precision"]]
    h = _lib.lib()
    assert h.tav_loss_version() == 1 and h.tav_soft_f_loss.argtypes == abi.sigs["tav_soft_f_loss"][1]
    for public in _lib.ABIS:                                  # the private names stay out of the recorded public tables
        assert set(public.sigs).isdisjoint(abi.sigs)
        assert "soft_f" not in abi_check.header_text(public.header, comments=True)


def test_a_library_without_the_loss_entry_points_or_of_another_version_is_refused(monkeypatch):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LOSS_ABI_VERSION", 2)
    with pytest.raises(RuntimeError, match=r"libtavhip loss ABI 1 != binding 2; rebuild"):
        _lib.lib()
    assert _lib._lib is None
    monkeypatch.undo()
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setitem(_lib._LOSS_SIGS, "tav_no_such_loss", (C.c_int, []))
    with pytest.raises(RuntimeError, match=r"tav_no_such_loss.*csrc/tavhip_loss\.h.*; rebuild$"):
        _lib.lib()
    monkeypatch.undo()
    assert _lib.lib().tav_loss_version() == 1


# ---------------------------------------------------------------------------------------------- argument faults, nothing launches
def _args(**kw):
    a = _lib.SoftFArgs()
    for f in ("logits", "target", "loss", "dlogits"):
        setattr(a, f, 4096)                                   # only tested for NULL-ness before a fault is found
    a.B, a.C, a.ld, a.beta, a.eps, a.grad_scale, a.mode = 4, 7, 7, 0.5, 1e-7, 1.0, _lib.SOFT_F_FBETA
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_invalid_arguments_are_refused_before_any_launch():
    h = _lib.lib()
    call = lambda **kw: h.tav_soft_f_loss(C.byref(_args(**kw)), None)          # noqa: E731
    assert h.tav_soft_f_loss(None, None) == ERR_NULL
    assert call(logits=None) == ERR_NULL and call(target=None) == ERR_NULL and call(loss=None, dlogits=None) == ERR_NULL
    assert call(loss=None, dlogits=None, stats=4096) == ERR_NULL
    for kw in (dict(B=0), dict(B=65537), dict(C=0), dict(C=17), dict(ld=6), dict(ld=(1 << 40) + 1), dict(B=-3), dict(C=-1)):
        assert call(**kw) == ERR_SHAPE, kw
    inf, nan = float("inf"), float("nan")
    for v in (0.0, -1.0, inf, -inf, nan):
        assert call(beta=v) == ERR_SHAPE and call(eps=v) == ERR_SHAPE, v
    assert call(eps=0.5) == ERR_SHAPE and call(eps=0.75) == ERR_SHAPE
    assert call(mode=2) == ERR_SHAPE and call(mode=-1) == ERR_SHAPE
    assert call(B=0, logits=None) == ERR_NULL                                   # pointers, then sizes
    assert h.tav_error_string(ERR_SHAPE).decode() == "unsupported shape"


def test_wrapper_refuses_what_the_kernel_cannot_read(monkeypatch):
    z, t = torch.zeros(3, 4), torch.zeros(3, dtype=torch.int64)
    with pytest.raises(ValueError, match="mode"):
        ops.soft_f_loss(z, t, None, 1.0, "Recall")
    with pytest.raises(ValueError, match="f32"):
        ops.soft_f_loss(z.double(), t, None, 1.0, "FBeta")
    with pytest.raises(ValueError, match="f32"):
        ops.soft_f_loss(z.t(), t[:4], None, 1.0, "FBeta")
    with pytest.raises(ValueError, match="targets"):
        ops.soft_f_loss(z, t[:2], None, 1.0, "FBeta")
    with pytest.raises(ValueError, match="weight"):
        ops.soft_f_loss(z, t, torch.ones(3), 1.0, "FBeta")
    with pytest.raises(ValueError, match="stats"):
        ops.soft_f_loss(z, t, None, 1.0, "FBeta", stats=torch.zeros(3, 3))
    # the range check of the targets reads them back, so it runs on request only; it raises before anything is launched
    monkeypatch.setattr(ops, "_DEBUG_CHECKS", True)
    for bad in (-1, 4):
        with pytest.raises(ValueError, match=r"outside \[0, 4\)"):
            ops.soft_f_loss(z, torch.tensor([0, bad, 1]), None, 1.0, "FBeta")


# ---------------------------------------------------------------------------------------------- criteria and flags
def test_criteria_carry_their_arguments_and_refuse_bad_ones():
    f = GF.FBetaLoss(num_classes=7, beta=0.5)
    assert (f.num_classes, f.beta, f.epsilon, f.weights, f.mode) == (7, 0.5, 1e-7, None, "FBeta") and not hasattr(f, "epoch_switch")
    p = GF.PrecisionLoss(num_classes=7)
    assert (p.num_classes, p.epsilon, p.weights, p.mode) == (7, 1e-7, None, "Precision") and not hasattr(p, "epoch_switch")
    assert GF.FBetaLoss(3, weights=[1, 2, 3]).weights.tolist() == [1.0, 2.0, 3.0] and GF.FBetaLoss(3, weights=1).weights.tolist() == [1.0, 1.0, 1.0]
    assert GF.PrecisionLoss(3, weights=torch.tensor([0.5, 1.0, 2.0]), epsilon=1e-6).epsilon == 1e-6
    for beta in (0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="beta"):
            GF.FBetaLoss(7, beta=beta)
    for eps in (0, 0.5, float("nan")):
        with pytest.raises(ValueError, match="epsilon"):
            GF.FBetaLoss(7, epsilon=eps)
    with pytest.raises(ValueError, match="classes"):
        GF.FBetaLoss(17)
    with pytest.raises(ValueError, match="weights"):
        GF.PrecisionLoss(3, weights=[1, 2])
    with pytest.raises(ValueError, match="logits"):
        f(torch.zeros(2, 6), torch.zeros(2, dtype=torch.int64))
    import inspect
    assert list(inspect.signature(GF.FBetaLoss.forward).parameters) == ["self", "logits", "target", "epoch"]
    assert list(inspect.signature(GF.FBetaLoss.__init__).parameters) == ["self", "num_classes", "beta", "weights", "epsilon"]
    assert list(inspect.signature(GF.PrecisionLoss.__init__).parameters) == ["self", "num_classes", "weights", "epsilon"]


def test_criterion_of_the_loss_flag():
    pd = {"weights": torch.linspace(0.6, 0.95, 7), "epoch_switch": 3, "beta": 0.5}
    c = build_criterion({**pd, "loss": "FBeta"}, 7, "cpu")
    assert type(c) is GF.FBetaLoss and (c.num_classes, c.beta) == (7, 0.5)
    assert build_criterion({**pd, "loss": "FBeta", "beta": 2}, 5, "cpu").beta == 2.0
    c = build_criterion({**pd, "loss": "Precision"}, 7, "cpu")
    assert type(c) is GF.PrecisionLoss and c.num_classes == 7
    c = build_criterion({**pd, "loss": "CrossEntropy"}, 7, "cpu")
    assert type(c) is GF.CrossEntropyLoss and c.weight is None
    for name in ("NewCrossEntropy", "SomethingElse", "fbeta"):
        c = build_criterion({**pd, "loss": name}, 7, "cpu")
        assert type(c) is GF.NewCrossEntropyLoss and c.epoch_switch == 3 and torch.equal(c.class_weights, pd["weights"]), name
    for beta in (0, -0.5):
        with pytest.raises(ValueError, match="beta"):
            build_criterion({**pd, "loss": "FBeta", "beta": beta}, 7, "cpu")
    # the three entry points that read --loss build their criterion there
    import tav_amd.DoubleModels.text_audio_nn as ta
    import tav_amd.SingleModels.text_nn as tx
    import tav_amd.tav_nn as tav
    for mod in (tav, tx, ta):
        assert mod.build_criterion is build_criterion
        src = open(mod.__file__).read()
        assert "build_criterion(param_dict" in src and "NewCrossEntropyLoss(" not in src


def test_arg_parse_defaults_are_unchanged():
    a = GF.arg_parse("TAV", [])
    assert (a.loss, a.beta, a.epoch_switch, a.output_dim) == ("NewCrossEntropy", 1, 2, 7)
    a = GF.arg_parse("TAV", ["--loss", "FBeta", "--beta", "0.5"])
    assert (a.loss, a.beta) == ("FBeta", 0.5)
    assert GF.arg_parse("TAV", ["-ls", "Precision", "-beta", "2"]).beta == 2.0
