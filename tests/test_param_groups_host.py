"""Parameter groups of the fused AdamW, host side (no GPU): the C ABI's argument validation, FusedAdamW's constructor and attributes, the
checkpoint format against torch.optim.AdamW with the same groups, CosineWarmRestarts against torch's scheduler over three groups,
optim.default_param_groups on stand-in modules, the two CLI flags, and the data-parallel paths that refuse more than one group."""
import ctypes as C
import types

import pytest
import torch

import tav_amd  # noqa: F401
from tav_amd import _lib, ddp
from tav_amd.optim import FusedAdamW, ShardedAdamW, default_param_groups
from tav_amd.train_model.tav_train import CosineWarmRestarts
from tav_amd.utils.global_functions import arg_parse

TAV_ERR_NULL, TAV_ERR_SHAPE = -1, -2


def _params(*shapes, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in shapes]


# ---------------------------------------------------------------------------------------------- C ABI
def test_grouped_adamw_validates_its_arguments_without_a_gpu():
    """Every refusal returns before anything is launched: the pointers below are host words that no kernel may ever see."""
    h = _lib.lib()
    assert h.tav_version() == 7 and _lib.ABI_VERSION == 7
    assert h.tav_optim_max_groups() == 64
    word = (C.c_int64 * 4)()
    a = C.addressof(word)

    def call(ngroups=3, group_of=a, hyper=a, ntensors=1, nchunks=1, params=a, step=a):
        return h.tav_adamw_chunked_groups(params, a, a, a, a, a, ntensors, nchunks, None, group_of, hyper, ngroups, 0.9, 0.999, 1e-8, step, a, None)
    assert call(ngroups=0) == TAV_ERR_SHAPE
    assert call(ngroups=-1) == TAV_ERR_SHAPE
    assert call(ngroups=h.tav_optim_max_groups() + 1) == TAV_ERR_SHAPE
    assert call(group_of=None) == TAV_ERR_NULL
    assert call(hyper=None) == TAV_ERR_NULL
    assert call(params=None) == TAV_ERR_NULL and call(step=None) == TAV_ERR_NULL
    # ntensors / nchunks <= 0 as the sibling call treats them
    sibling = lambda nt, nc: h.tav_adamw_chunked(a, a, a, a, a, a, nt, nc, None, a, 0.9, 0.999, 1e-8, 0.0, a, a, None)      # noqa: E731
    for nt, nc in ((0, 1), (1, 0), (-3, 1)):
        assert call(ntensors=nt, nchunks=nc) == sibling(nt, nc) == TAV_ERR_SHAPE
    assert all(v == 0 for v in word)


# ---------------------------------------------------------------------------------------------- constructor and attributes
def test_flat_list_is_one_group_and_lr_is_group_zero():
    ps = _params((4, 3), (5,))
    frozen = torch.nn.Parameter(torch.zeros(2), requires_grad=False)
    opt = FusedAdamW(ps + [frozen], lr=3e-4, weight_decay=0.05)
    assert len(opt.param_groups) == 1 and opt.lr == 3e-4 and opt.weight_decay == 0.05
    assert [id(p) for p in opt.params] == [id(p) for p in ps]
    g = opt.param_groups[0]
    assert {"lr", "weight_decay", "betas", "eps", "params"} <= set(g) and g["params"] is not None and len(g["params"]) == 2
    opt.lr = 1e-5                                   # the attribute IS group 0
    opt.weight_decay = 0.0
    assert g["lr"] == 1e-5 and g["weight_decay"] == 0.0
    g["lr"] = 7e-6                                  # and the other way round (a scheduler writes the dict)
    assert opt.lr == 7e-6
    assert FusedAdamW(iter(ps)).lr == 1e-6          # any iterable, the constructor's default


def test_dict_list_builds_groups_in_order():
    ps = _params((4, 3), (5,), (2, 2), (7,))
    opt = FusedAdamW([{"params": [ps[2], ps[0]], "lr": 0.1}, {"params": [ps[3]], "weight_decay": 0.0}, {"params": [ps[1]], "lr": 0.5, "weight_decay": 0.25}],
                     lr=1e-3, weight_decay=1e-2)
    assert [(g["lr"], g["weight_decay"]) for g in opt.param_groups] == [(0.1, 1e-2), (1e-3, 0.0), (0.5, 0.25)]       # missing keys: the defaults
    assert [id(p) for p in opt.params] == [id(ps[i]) for i in (2, 0, 3, 1)]                                          # flat, in group order
    assert all(g["betas"] == (0.9, 0.999) and g["eps"] == 1e-8 for g in opt.param_groups)
    assert opt.lr == 0.1 and opt.weight_decay == 1e-2                                                                # reading: group 0
    with pytest.raises(AttributeError, match="param_groups"):
        opt.lr = 1.0
    with pytest.raises(AttributeError, match="param_groups"):
        opt.weight_decay = 1.0
    assert opt.param_groups[0]["lr"] == 0.1


def test_constructor_refusals():
    ps = _params((3,), (3,), (3,))
    with pytest.raises(ValueError, match="more than one parameter group"):
        FusedAdamW([{"params": [ps[0], ps[1]]}, {"params": [ps[1], ps[2]]}])
    with pytest.raises(ValueError, match="ONE step counter"):
        FusedAdamW([{"params": [ps[0]]}, {"params": [ps[1]], "betas": (0.8, 0.999)}])
    with pytest.raises(ValueError, match="ONE bias"):
        FusedAdamW([{"params": [ps[0]]}, {"params": [ps[1]], "eps": 1e-6}])
    FusedAdamW([{"params": [ps[0]]}, {"params": [ps[1]], "betas": (0.9, 0.999), "eps": 1e-8}])        # the optimizer's own values: fine
    many = _params(*[(1,)] * 65)
    FusedAdamW([{"params": [p]} for p in many[:64]])
    with pytest.raises(ValueError, match="65 parameter groups"):
        FusedAdamW([{"params": [p]} for p in many])


# ---------------------------------------------------------------------------------------------- checkpoint format
_SHAPES = [(4, 3), (5,), (2, 2), (7,), (3, 1, 2)]
_SPLIT = [(0, 2), (2, 3), (3, 5)]
_HYPER = [(1e-3, 1e-2), (5e-4, 0.0), (2e-3, 0.3)]


def _dicts(ps, hyper=_HYPER):
    return [{"params": ps[a:b], "lr": lr, "weight_decay": wd} for (a, b), (lr, wd) in zip(_SPLIT, hyper)]


def _torch_after_two_steps():
    ps = _params(*_SHAPES, seed=1)
    ref = torch.optim.AdamW(_dicts(ps))
    g = torch.Generator().manual_seed(2)
    for _ in range(2):
        for p in ps:
            p.grad = torch.randn(p.shape, generator=g)
        ref.step()
    return ps, ref


def test_state_dict_has_torchs_layout_with_groups():
    ps, ref = _torch_after_two_steps()
    sd = ref.state_dict()
    opt = FusedAdamW(_dicts(ps, [(9.0, 9.0)] * 3), lr=5.0, weight_decay=0.5)
    opt.load_state_dict(sd)                                                     # a torch.optim.AdamW state with three groups loads
    assert [(g["lr"], g["weight_decay"]) for g in opt.param_groups] == _HYPER   # every group's pair is adopted
    assert opt._loaded_step == 2 and opt.step_count == 2
    for i, p in enumerate(ps):                                                  # the moments belong to the right parameters
        assert torch.equal(opt.state[p][0], sd["state"][i]["exp_avg"]) and torch.equal(opt.state[p][1], sd["state"][i]["exp_avg_sq"])
    out = opt.state_dict()
    assert set(out) == set(sd) and set(out["state"]) == set(sd["state"]) == set(range(5))
    assert [g["params"] for g in out["param_groups"]] == [g["params"] for g in sd["param_groups"]] == [[0, 1], [2], [3, 4]]
    for mine, theirs in zip(out["param_groups"], sd["param_groups"]):
        assert set(mine) <= set(theirs) and all(mine[k] == theirs[k] for k in mine)
    for i in range(5):
        assert set(out["state"][i]) == set(sd["state"][i]) and float(out["state"][i]["step"]) == 2.0
    fresh = torch.optim.AdamW(_dicts(ps, [(1.0, 1.0)] * 3))
    fresh.load_state_dict(out)                                                  # and back into torch
    assert [(g["lr"], g["weight_decay"]) for g in fresh.param_groups] == _HYPER and float(fresh.state[ps[4]]["step"]) == 2.0


def test_state_dict_indices_follow_group_order_before_any_step():
    ps = _params(*_SHAPES)
    mine, theirs = FusedAdamW(_dicts(ps)).state_dict(), torch.optim.AdamW(_dicts(ps)).state_dict()
    assert set(mine) == set(theirs) and mine["state"] == theirs["state"] == {}
    assert [g["params"] for g in mine["param_groups"]] == [g["params"] for g in theirs["param_groups"]]
    assert [(g["lr"], g["weight_decay"], g["betas"], g["eps"]) for g in mine["param_groups"]] == \
           [(g["lr"], g["weight_decay"], g["betas"], g["eps"]) for g in theirs["param_groups"]]


def test_load_state_dict_refuses_other_group_sizes_and_bumps_generation():
    ps, ref = _torch_after_two_steps()
    sd = ref.state_dict()
    other = FusedAdamW([{"params": ps[:1]}, {"params": ps[1:3]}, {"params": ps[3:]}])            # same five parameters, groups of 1 / 2 / 2
    with pytest.raises(ValueError, match="parameter groups"):
        other.load_state_dict(sd)
    with pytest.raises(ValueError):
        FusedAdamW(ps).load_state_dict(sd)                                                        # one group of five
    opt = FusedAdamW(_dicts(ps))
    gen = opt.generation
    opt.load_state_dict(sd)
    assert opt.generation == gen + 1


def test_single_group_state_in_the_layout_before_groups_still_loads():
    ps = _params((4, 3), (5,))
    old = {"state": {i: {"step": torch.tensor(3.0), "exp_avg": torch.full_like(p, 0.5), "exp_avg_sq": torch.full_like(p, 0.25)} for i, p in enumerate(ps)},
           "param_groups": [{"lr": 2e-5, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 1e-4, "amsgrad": False, "maximize": False, "foreach": None,
                             "capturable": False, "differentiable": False, "fused": None, "params": [0, 1]}]}
    opt = FusedAdamW(ps, lr=1.0, weight_decay=1.0)
    opt.load_state_dict(old)
    assert opt.lr == 2e-5 and opt.weight_decay == 1e-4 and opt.step_count == 3 and torch.equal(opt.state[ps[1]][1], torch.full((5,), 0.25))
    out = opt.state_dict()
    assert list(out["param_groups"][0]) == list(old["param_groups"][0]) and out["param_groups"][0] == old["param_groups"][0]


# ---------------------------------------------------------------------------------------------- scheduler
def test_cosine_warm_restarts_moves_every_group_like_torch():
    ps = _params(*_SHAPES)
    ref_opt = torch.optim.AdamW(_dicts(ps))
    opt = FusedAdamW(_dicts(ps))
    ref = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(ref_opt, T_0=2)
    mine = CosineWarmRestarts(opt, T_0=2)
    assert mine.base_lrs == ref.base_lrs == [h[0] for h in _HYPER]
    iters, seen = 4, []
    for epoch in range(3):                                                      # twelve steps, restarts at 2.0 (and 0.0)
        for i in range(iters):
            ref.step(epoch + i / iters)
            mine.step(epoch + i / iters)
            assert mine.get_last_lr() == ref.get_last_lr() == [g["lr"] for g in opt.param_groups]      # the same floats, not close ones
            seen.append(tuple(mine.get_last_lr()))
    assert len(set(seen)) == 8 and seen[8] == seen[0] and len(seen[0]) == 3
    sd, rsd = mine.state_dict(), ref.state_dict()
    for k in ("T_0", "T_i", "T_mult", "eta_min", "T_cur", "base_lrs", "_last_lr"):
        assert sd[k] == rsd[k], k
    assert len(sd["base_lrs"]) == len(sd["_last_lr"]) == 3
    opt2 = FusedAdamW(_dicts(ps, [(1.0, 0.0)] * 3))
    again = CosineWarmRestarts(opt2, T_0=9)
    again.load_state_dict(sd)                                                   # round trip: the schedule and the rates it had set
    assert again.T_0 == 2 and again.base_lrs == mine.base_lrs and again.get_last_lr() == mine.get_last_lr()
    again.step(3.0)
    mine.step(3.0)
    assert again.get_last_lr() == mine.get_last_lr()
    from_torch = CosineWarmRestarts(FusedAdamW(_dicts(ps, [(1.0, 0.0)] * 3)), T_0=9)
    from_torch.load_state_dict(rsd)                                             # torch's own scheduler state resumes here
    assert from_torch.get_last_lr() == ref.get_last_lr()
    with pytest.raises(ValueError):
        CosineWarmRestarts(FusedAdamW(ps), T_0=2).load_state_dict(sd)           # three rates into one group


# ---------------------------------------------------------------------------------------------- default_param_groups
class _Stack(torch.nn.Module):
    def __init__(self, width):
        super().__init__()
        self.dense = torch.nn.Linear(width, width)
        self.norm = torch.nn.LayerNorm(width)


class _Net(torch.nn.Module):
    """Stand-in with the attribute names of TAVForMAE / PreFormer (the real modules are far larger than this test needs)."""

    def __init__(self, with_head):
        super().__init__()
        self.bert, self.wav2vec2, self.videomae = _Stack(4), _Stack(3), _Stack(2)
        self.encoder = _Stack(5)
        self.masked_spec_embed = torch.nn.Parameter(torch.zeros(3))
        if with_head:
            self.linear = torch.nn.Linear(5, 7)


def test_default_param_groups():
    model, pre = _Net(True), _Net(False)
    model.bert.dense.weight.requires_grad_(False)                               # a frozen pretrained matrix
    pre.encoder.norm.bias.requires_grad_(False)                                 # and a frozen new vector
    flat = default_param_groups(model, pre, 1e-4, 1e-2)
    want = [p for p in model.parameters() if p.requires_grad] + [p for p in pre.parameters() if p.requires_grad]
    assert isinstance(flat, list) and all(torch.is_tensor(p) for p in flat) and [id(p) for p in flat] == [id(p) for p in want]

    groups = default_param_groups(model, pre, 1e-4, 1e-2, encoder_lr_scale=0.1, no_decay_norm_bias=True)
    assert [(g["lr"], g["weight_decay"]) for g in groups] == [(1e-4, 1e-2), (1e-4, 0.0), (1e-4 * 0.1, 1e-2), (1e-4 * 0.1, 0.0)]
    ids = [id(p) for g in groups for p in g["params"]]
    assert len(ids) == len(set(ids)) and set(ids) == {id(p) for p in want}      # disjoint, every trainable parameter once
    frozen = {id(model.bert.dense.weight), id(pre.encoder.norm.bias)}
    assert not frozen & set(ids)
    pretrained = {id(p) for m in (model, pre) for s in (m.bert, m.wav2vec2, m.videomae) for p in s.parameters()}
    for gi, g in enumerate(groups):
        assert g["params"]
        for p in g["params"]:
            assert (id(p) in pretrained) == (gi >= 2) and (p.ndim <= 1) == (gi % 2 == 1)
    assert id(model.linear.weight) in {id(p) for p in groups[0]["params"]} and id(model.masked_spec_embed) in {id(p) for p in groups[1]["params"]}
    opt = FusedAdamW(groups, lr=1e-4, weight_decay=1e-2)                       # what TrainStep does with them
    assert len(opt.param_groups) == 4 and len(opt.params) == len(want)

    two = default_param_groups(model, pre, 1e-4, 1e-2, encoder_lr_scale=0.5)    # one axis in use: two groups, new before pretrained
    assert [(g["lr"], g["weight_decay"]) for g in two] == [(1e-4, 1e-2), (5e-5, 1e-2)]
    assert all((id(p) in pretrained) == (gi == 1) for gi, g in enumerate(two) for p in g["params"])
    nod = default_param_groups(model, pre, 1e-4, 1e-2, no_decay_norm_bias=True)
    assert [(g["lr"], g["weight_decay"]) for g in nod] == [(1e-4, 1e-2), (1e-4, 0.0)]
    for m in (model, pre):                                                      # nothing new left to train: the empty groups are dropped
        for name, p in m.named_parameters():
            if not name.startswith(("bert.", "wav2vec2.", "videomae.")):
                p.requires_grad_(False)
    only = default_param_groups(model, pre, 1e-4, 1e-2, encoder_lr_scale=0.1, no_decay_norm_bias=True)
    assert [(g["lr"], g["weight_decay"]) for g in only] == [(1e-4 * 0.1, 1e-2), (1e-4 * 0.1, 0.0)]
    with pytest.raises(ValueError):
        default_param_groups(model, pre, 1e-4, 1e-2, encoder_lr_scale=0.0)


# ---------------------------------------------------------------------------------------------- CLI
def test_cli_flags():
    args = arg_parse("x", [])
    assert args.encoder_lr_scale == 1.0 and args.no_decay_norm_bias == 0
    args = arg_parse("x", ["--encoder-lr-scale", "0.1", "--no-decay-norm-bias", "1"])
    assert args.encoder_lr_scale == 0.1 and args.no_decay_norm_bias == 1
    for bad in (["--encoder-lr-scale", "0"], ["--encoder-lr-scale", "-0.5"], ["--no-decay-norm-bias", "2"]):
        with pytest.raises(SystemExit):
            arg_parse("x", bad)


# ---------------------------------------------------------------------------------------------- data-parallel paths with one group only
def test_sharded_and_graphed_data_parallel_refuse_groups():
    ps = _params((4, 3), (5,))
    two = FusedAdamW([{"params": ps[:1], "lr": 0.1}, {"params": ps[1:]}])
    with pytest.raises(ValueError, match="parameter groups"):
        ShardedAdamW.from_replicated(two, 2, 0)
    with pytest.raises(ValueError, match="one parameter group"):
        ShardedAdamW([{"params": ps[:1]}, {"params": ps[1:]}], 2, 0)
    with pytest.raises(ValueError, match="one parameter group"):
        ddp.GraphedStep(types.SimpleNamespace(opt=two, reducer=None), lambda: None)
    one = ShardedAdamW.from_replicated(FusedAdamW(ps, lr=0.25, weight_decay=0.5), 2, 1)             # one group: as before
    assert one.lr == 0.25 and one.weight_decay == 0.5 and len(one.param_groups) == 1
