"""-m gpu: parameter groups of the fused AdamW.  tav_adamw_chunked_groups against the fp64 step of tests/step_end_ref.py (per element, its
bounds), against tav_adamw_chunked bit for bit, at the edges of the group table; FusedAdamW with groups against torch.optim.AdamW, eager and
replayed from a hipGraph; train_tav_network with the default groups, graphs against eager and across a best.pt."""
import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

import guarded
import step_end_ref as SR
import tav_amd  # noqa: F401
from tav_amd import config as C
from tav_amd import runtime, synthetic
from tav_amd._lib import check, lib, ptr, stream
from tav_amd.models.tav import PreFormer, TAVForMAE
from tav_amd.optim import FusedAdamW
from tav_amd.train_model import graphed as G
from tav_amd.train_model import tav_train as T
from tav_amd.utils import global_functions as GF

pytestmark = pytest.mark.gpu
DEV = "cuda"
GAP = 36                                         # floats of 0xFF between two slices (a multiple of 4: alignment is decided by `mis` alone)
HYPER3 = [(0.1, 1e-2), (0.025, 0.0), (0.0, 0.3)]


def _i32bits(t):
    return t.contiguous().view(torch.int32)


class _Arena:
    """The tensors of one role as slices of ONE buffer under guard (tests/guarded.py: 0xFF all around, 1 MiB either side), 0xFF gaps between
    the slices; mis = True starts every slice 4 bytes past a 16-byte boundary.  role "in": an operand (verify() wants it bit-identical);
    "out": the kernel writes the slices (verify() checks the bands, gaps() the space between the slices)."""

    def __init__(self, guard, sizes, mis, role, flat):
        self.starts, c = [], GAP
        for n in sizes:
            self.starts.append(c + (1 if mis else 0))
            c = (self.starts[-1] + n + 3) // 4 * 4 + GAP
        idx = torch.cat([torch.arange(s, s + n) for s, n in zip(self.starts, sizes)])
        host = torch.full((c,), -1, dtype=torch.int32).view(torch.float32).clone()           # 0xFF everywhere
        host[idx] = torch.as_tensor(np.asarray(flat), dtype=torch.float32)
        if role == "in":
            self.buf = guard.input(host.to(DEV))
        else:
            self.buf = guard.empty(c, dtype=torch.float32, device=DEV)
            _i32bits(self.buf).copy_(_i32bits(host).to(DEV))
        assert self.buf.data_ptr() % 16 == 0
        self.idx = idx.to(DEV)
        gap = torch.ones(c, dtype=torch.bool)
        gap[idx] = False
        self.gap_idx = gap.nonzero().flatten().to(DEV)
        self.ptrs = [self.buf.data_ptr() + 4 * s for s in self.starts]
        assert all(p_ % 16 == (4 if mis else 0) for p_ in self.ptrs)
        self.table = guard.input(torch.tensor(self.ptrs, dtype=torch.int64).to(DEV))

    def get(self):
        return self.buf[self.idx].cpu().numpy()

    def gaps_untouched(self):
        return bool((_i32bits(self.buf[self.gap_idx]) == -1).all())


class _Case:
    """One optimizer state for the raw C calls: parameters, gradients and both moments in guarded arenas, the tables the calls take, `hyper` and
    `group_of` under guard as well."""

    def __init__(self, sizes, group_of, hyper, mis=False, seed=0):
        self.g = guarded.Guard()
        self.sizes, self.group_of, self.nt = list(sizes), list(group_of), len(sizes)
        n_all = sum(sizes)
        self.p0, self.g0 = SR.make_inputs(n_all, seed=seed)
        self.cuts = np.cumsum([0] + self.sizes)
        self.G = _Arena(self.g, sizes, mis, "in", self.g0)
        self.A = {k: _Arena(self.g, sizes, mis, "out", self.p0 if k == "p" else np.zeros(n_all)) for k in "pmv"}
        self.t_s = self.g.input(torch.tensor(self.sizes, dtype=torch.int64).to(DEV))
        pre, self.nchunks = SR.chunk_prefix(self.sizes, int(lib().tav_optim_chunk_elems()))
        self.t_c = self.g.input(torch.tensor(pre, dtype=torch.int32).to(DEV))
        self.t_go = self.g.input(torch.tensor(self.group_of, dtype=torch.int32).to(DEV))
        self.ngroups = len(hyper)
        self.hyper = self.g.empty((self.ngroups, 2), dtype=torch.float32, device=DEV)
        self.hyper.copy_(torch.tensor(hyper, dtype=torch.float32))
        self.scal = self.g.empty(8, dtype=torch.float32, device=DEV)          # [1] clip coefficient, [4] lr of the single-group call, [5:7] bias_corr
        self.step = self.g.zeros(1, dtype=torch.int32, device=DEV)

    def state(self):
        return {k: self.A[k].get() for k in "pmv"}

    def _coef(self, cc, with_ptr):
        self.scal[1] = cc
        return ptr(self.scal[1:2]) if with_ptr else None

    def launch_groups(self, cc=1.0, with_ptr=False):
        b1, b2 = SR.BETAS
        check(lib().tav_adamw_chunked_groups(ptr(self.A["p"].table), ptr(self.G.table), ptr(self.A["m"].table), ptr(self.A["v"].table), ptr(self.t_s),
                                             ptr(self.t_c), self.nt, self.nchunks, self._coef(cc, with_ptr), ptr(self.t_go), ptr(self.hyper), self.ngroups,
                                             b1, b2, SR.EPS, ptr(self.step), ptr(self.scal[5:7]), stream()), "adamw_chunked_groups")

    def launch_single(self, lr, wd, cc=1.0, with_ptr=False):
        b1, b2 = SR.BETAS
        self.scal[4] = lr
        check(lib().tav_adamw_chunked(ptr(self.A["p"].table), ptr(self.G.table), ptr(self.A["m"].table), ptr(self.A["v"].table), ptr(self.t_s),
                                      ptr(self.t_c), self.nt, self.nchunks, self._coef(cc, with_ptr), ptr(self.scal[4:5]), b1, b2, SR.EPS, wd,
                                      ptr(self.step), ptr(self.scal[5:7]), stream()), "adamw_chunked")

    def effective_group(self, t):
        return min(max(self.group_of[t], 0), self.ngroups - 1)

    def worst_ratios(self, before, after, s, cc):
        """Worst |got - fp64| / bound over the elements of every tensor, the reference taken tensor by tensor with the {lr, wd} words of that
        tensor's group as the device table holds them."""
        hyper = self.hyper.cpu().numpy().astype(np.float64)
        worst = dict(p=0.0, m=0.0, v=0.0)
        for t in range(self.nt):
            a, b = self.cuts[t], self.cuts[t + 1]
            lr, wd = hyper[self.effective_group(t)]
            ref = SR.ref_step(before["p"][a:b], self.g0[a:b], before["m"][a:b], before["v"][a:b], s, lr, wd, cc)
            for k, r in SR.ratios(ref, after["p"][a:b], after["m"][a:b], after["v"][a:b]).items():
                worst[k] = max(worst[k], r)
        return worst

    def verify(self):
        """Guard bands and operands (gradients, every table, group_of) untouched, the gaps between the slices still 0xFF."""
        self.g.verify()
        assert all(self.A[k].gaps_untouched() for k in "pmv"), "a store between two tensors"


def _three_steps_against_fp64(case, halve_group, tag):
    """SR.step_plan's clip sequence (no pointer / CLIP_STEP2 / coefficient 1.0), every step from the kernel's own f32 state; before step 3 a
    fill halves the learning rate of `halve_group` in the device table and touches nothing else."""
    hyper0 = case.hyper.cpu().clone()
    for (s, _, cc, with_ptr) in SR.step_plan():
        if s == 3:
            case.hyper[halve_group, 0].fill_(float(hyper0[halve_group, 0]) * 0.5)
            hyper0[halve_group, 0] *= 0.5
        before = case.state()
        case.launch_groups(cc, with_ptr)
        after = case.state()
        worst = case.worst_ratios(before, after, s, cc)
        print(f"{tag} step {s}: worst ratio to bound p {worst['p']:.3f} m {worst['m']:.3f} v {worst['v']:.3f}")
        assert worst["p"] <= 1.0 and worst["m"] <= 1.0 and worst["v"] <= 1.0, (tag, s, worst)
        assert int(case.step.item()) == s
        assert torch.equal(_i32bits(case.hyper.cpu()), _i32bits(hyper0)), "the kernel wrote into the hyper table"
        for t in range(case.nt):
            a, b = case.cuts[t], case.cuts[t + 1]
            lr = float(hyper0[case.effective_group(t), 0])
            if lr == 0.0:            # a group at lr = 0: weights bit-identical (also under weight decay: the decay is 1 - lr * wd), moments move
                assert np.array_equal(before["p"][a:b].view(np.int32), after["p"][a:b].view(np.int32)), (tag, s, t)
                if np.any(case.g0[a:b] != 0):
                    assert not np.array_equal(before["m"][a:b], after["m"][a:b]) and not np.array_equal(before["v"][a:b], after["v"][a:b])
        case.verify()                # (gradients, tables and group_of bit-identical; nothing written outside the tensors)


# ---------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("list_name", ["many", "edges"])
def test_grouped_adamw_against_fp64(gpu, list_name):
    sizes = SR.SIZE_LISTS[list_name]
    case = _Case(sizes, [t % 3 for t in range(len(sizes))], HYPER3, seed=len(sizes))
    _three_steps_against_fp64(case, halve_group=0, tag=f"groups[{list_name}]")
    assert abs(float(case.hyper[0, 0].item()) - SR.f32(0.1) * 0.5) == 0.0 and float(case.hyper[1, 0].item()) == SR.f32(0.025)


@pytest.mark.parametrize("mis", [False, True])
@pytest.mark.parametrize("list_name", ["many", "edges"])
def test_grouped_adamw_equals_the_single_group_kernel_bit_for_bit(gpu, list_name, mis):
    """All three groups at one {lr, wd}: two steps (no clip pointer, then CLIP_STEP2) give the bits of tav_adamw_chunked on copies, with every
    tensor on a 16-byte boundary (the 16-byte loops) and 4 bytes past one (the scalar loop)."""
    sizes = SR.SIZE_LISTS[list_name]
    a = _Case(sizes, [t % 3 for t in range(len(sizes))], [(SR.LR, SR.WD)] * 3, mis=mis, seed=7)
    b = _Case(sizes, [0] * len(sizes), [(9.0, 9.0)], mis=mis, seed=7)
    for cc, with_ptr in ((1.0, False), (SR.CLIP_STEP2, True)):
        a.launch_groups(cc, with_ptr)
        b.launch_single(SR.LR, SR.WD, cc, with_ptr)
        sa, sb = a.state(), b.state()
        for k in "pmv":
            assert np.isfinite(sa[k]).all() and np.array_equal(sa[k].view(np.int32), sb[k].view(np.int32)), (list_name, mis, k)
        assert not np.array_equal(sa["p"], a.p0)
    assert int(a.step.item()) == int(b.step.item()) == 2
    a.verify()
    b.verify()


_EDGE_CASES = {
    # name: (sizes, group_of, hyper, the group whose lr is halved before step 3)
    "one multi-chunk tensor in group 2 of 3": ([2 * 16384 + 7], [2], [(0.5, 0.5), (0.25, 0.1), (0.1, 1e-2)], 2),
    "every tensor in group 0": (SR.SIZE_LISTS["nt3"], [0, 0, 0], [(0.1, 1e-2), (0.5, 0.5), (0.25, 0.25)], 0),
    "groups descending": (SR.SIZE_LISTS["nt3"], [2, 1, 0], HYPER3, 1),
    "64 groups, one tiny tensor each": ([1 + (3 * i) % 7 for i in range(64)], list(range(64)),
                                        [(0.1 / (1 + i % 5), 0.0 if i % 4 == 0 else 1e-2 * (1 + i % 3)) for i in range(64)], 63),
    "indices outside the table are clamped into it": (SR.SIZE_LISTS["nt3"], [-7, 1, 1000], HYPER3, 0),
}


@pytest.mark.parametrize("name", list(_EDGE_CASES))
def test_group_lookup_at_the_tables_edges(gpu, name):
    sizes, group_of, hyper, halve = _EDGE_CASES[name]
    if len(hyper) == 64:
        assert len(hyper) == lib().tav_optim_max_groups()
    _three_steps_against_fp64(_Case(sizes, group_of, hyper, seed=len(sizes) + 11), halve, name)


# ---------------------------------------------------------------------------------------------- FusedAdamW
def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


_SHAPES = [(300, 70), (3072,), (7, 3072), (5,), (50, 3, 10), (1,), (129, 127), (64,), (33000,), (3, 3), (768,), (16384,)]
_GROUP_OF_SHAPE = [0, 1, 0, 1, 2, 2, 0, 1, 2, 0, 1, 2]
_GROUP_HYPER = [(1e-3, 1e-2), (5e-4, 0.0), (2e-3, 0.1)]


def _grouped(ps):
    return [{"params": [p for p, g in zip(ps, _GROUP_OF_SHAPE) if g == gi], "lr": lr, "weight_decay": wd} for gi, (lr, wd) in enumerate(_GROUP_HYPER)]


def test_fused_adamw_with_groups_matches_torch(gpu):
    """Three groups, five clipped steps, both cosine schedulers moving every group's rate after each step, one parameter without a gradient on
    step 3 (the active set and its group_of table change).  Tolerances of test_model_gpu.test_fused_adamw_matches_torch: 1e-5.  FusedAdamW keeps
    ONE step counter (optim.py), torch one per parameter that a skipped step does not advance: the skipped parameter's counter is advanced by
    hand so that both sides correct its later steps for the same bias."""
    torch.manual_seed(0)
    ps = [torch.nn.Parameter(torch.randn(s, device="cuda")) for s in _SHAPES]
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    ref, opt = torch.optim.AdamW(_grouped(qs)), FusedAdamW(_grouped(ps))
    s_ref, s_opt = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(ref, T_0=2), T.CosineWarmRestarts(opt, T_0=2)
    order = {id(p): i for i, p in enumerate(ps)}
    skipped = 4                                   # (50, 3, 10), group 2
    for step in range(5):
        for i, (p, q) in enumerate(zip(ps, qs)):
            g = torch.randn_like(p) * (3.0 if step == 1 else 0.1)
            p.grad, q.grad = (None, None) if (step == 2 and i == skipped) else (g.clone(), g.clone())
        n_ref = torch.nn.utils.clip_grad_norm_(qs, 1.0)
        ref.step()
        if step == 2:
            ref.state[qs[skipped]]["step"] += 1
        n = opt.clip_and_step(1.0)
        assert abs(n.item() - n_ref.item()) / n_ref.item() < 1e-5
        for p in opt.params:
            assert rel(p, qs[order[id(p)]]) < 1e-5, (step, order[id(p)])
        s_ref.step((step + 1) / 4)
        s_opt.step((step + 1) / 4)
        assert s_opt.get_last_lr() == s_ref.get_last_lr()
    assert opt.step_count == 5
    table = opt._hyper.cpu()                      # the device table follows the scheduler at the next step (or sync_lr)
    opt.sync_lr()
    assert [float(v) for v in opt._hyper[:, 0].cpu()] == [SR.f32(lr) for lr in s_opt.get_last_lr()] and not torch.equal(table, opt._hyper.cpu())
    assert [float(v) for v in opt._hyper[:, 1].cpu()] == [SR.f32(wd) for _, wd in _GROUP_HYPER]


def _capture_run(captured):
    """Seven clipped steps of a two-group optimizer on fixed gradients, every group's rate moved by the scheduler between them.  captured:
    step 1 eager, steps 2-5 four replays of one hipGraph, step 6 one replay of a second hipGraph, then both graphs are destroyed, their
    upload slots released and step 7 runs eagerly."""
    torch.manual_seed(3)
    shapes = [(300, 70), (5,), (33000,), (7, 33), (1,), (2 * 16384,)]
    ps = [torch.nn.Parameter(torch.randn(s, device="cuda")) for s in shapes]
    for p in ps:
        p.grad = torch.randn_like(p) * 0.3
    opt = FusedAdamW([{"params": ps[:3], "lr": 1e-2, "weight_decay": 1e-2}, {"params": ps[3:], "lr": 3e-3, "weight_decay": 0.0}])
    sch = T.CosineWarmRestarts(opt, T_0=2)
    lrs, slots, caps = [], [], []
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        opt.clip_and_step(1.0)
        for k in range(1, 7):
            sch.step(0.3 * k)
            lrs.append(tuple(sch.get_last_lr()))
            if not captured:
                opt.clip_and_step(1.0)
                continue
            if k in (1, 5):                       # captures: the table is brought up to date first, the capture records no fill
                opt.sync_lr()
                torch.cuda.synchronize()
                cap = runtime.capture(torch.cuda.CUDAGraph(), s)
                with cap:
                    opt.clip_and_step(1.0)
                slots.append((opt._group_table.cap_used, [t.cap_used for t in opt._tables]))
                caps.append(cap)
            if k < 6:
                opt.sync_lr()
                cap.replay()
            else:
                torch.cuda.synchronize()
                for c in caps:
                    c.graph.reset()
                opt.captures_released()
                slots.append((opt._group_table.cap_used, [t.cap_used for t in opt._tables]))
                opt.clip_and_step(1.0)
        torch.cuda.synchronize()
    return dict(p=[p.detach().clone() for p in ps], m=[opt.state[p][0].clone() for p in ps], v=[opt.state[p][1].clone() for p in ps],
                step=opt.step_count, lrs=lrs, slots=slots, hyper=opt._hyper.cpu())


def test_captured_grouped_step_replays_with_the_schedulers_rates(gpu):
    a, b = _capture_run(False), _capture_run(True)
    assert a["step"] == b["step"] == 7 and a["lrs"] == b["lrs"] and len(set(a["lrs"])) == 6 and all(x[0] != x[1] for x in a["lrs"])
    for k in "pmv":
        for x, y in zip(a[k], b[k]):
            assert torch.isfinite(x).all() and torch.equal(x, y), k
    assert torch.equal(a["hyper"], b["hyper"])
    # every capture took one pinned upload slot of each table, group_of's like the pointer tables'; released together
    assert b["slots"] == [(1, [1] * 5), (2, [2] * 5), (0, [0] * 5)]


# ---------------------------------------------------------------------------------------------- the loop
ARGS = dict(output_dim=7, dropout=0.5, learn_PosEmbeddings=True, num_layers=12)
_LOG = T.log


def _models(cfg, dropout=0.5):
    torch.manual_seed(0)
    pre, model = PreFormer(cfg), TAVForMAE(dict(ARGS, dropout=dropout), cfg)
    synthetic.seeded_init_(pre, 1)
    synthetic.seeded_init_(model, 2)
    return pre.cuda(), model.cuda()


def _tiny_cfg():
    runtime.set_precision("bf16")
    cfg = C.preset("B-tiny")
    cfg["audio"]["mask_time_prob"] = 0.0           # SpecAugment off: torch's Philox stream differs between eager calls and replays
    return cfg


def _train(monkeypatch, graphs, path):
    """The geometry and the data of tests/test_graphed_loop_gpu.py (two epochs: not_grad_accum, then grad_accum with its unclipped dialogue-end
    steps on zero-filled gradients), with the pretrained encoders at a tenth of the rate and no decay on vectors: four groups."""
    from test_graphed_loop_gpu import _Dialogues
    cfg = _tiny_cfg()
    pre, model = _models(cfg)
    train = DataLoader(_Dialogues(cfg, [2, 2, 2, 2, 2, 1], [2, 4], 100), batch_size=None)
    val = DataLoader(_Dialogues(cfg, [2, 2], [2], 200), batch_size=None)
    crit = GF.NewCrossEntropyLoss(class_weights=torch.linspace(0.6, 0.95, 7).cuda(), epoch_switch=2)
    made, logged, replays = [], [], []

    class Rec(T.TrainStep):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)
    replay = G.GraphedSteps._replay
    monkeypatch.setattr(T, "TrainStep", Rec)
    monkeypatch.setattr(G.GraphedSteps, "_replay", lambda self, *a, **k: (replays.append(1), replay(self, *a, **k))[1])
    monkeypatch.setattr(T, "log", lambda M, loss, check="train": (logged.append((check, loss)), _LOG(M, loss, check)))
    T.PATIENCE_ITER = 0
    T.train_tav_network(model, pre, train, val, crit, 1e-4, 2, 1e-2, 2, GF.Metrics(7), 10, 1.0, 2, path=str(path), log_val=3,
                        zero_grad_like_torch_1_10=True, graphs=graphs, encoder_lr_scale=0.1, no_decay_norm_bias=True)
    torch.cuda.synchronize()
    opt = made[-1].opt
    out = dict(params=[p.detach().clone() for p in opt.params], moments=[tuple(t.clone() for t in opt.state[p]) if p in opt.state else None for p in opt.params],
               step=opt.step_count, groups=[(g["lr"], g["weight_decay"], len(g["params"])) for g in opt.param_groups], logged=logged, replays=len(replays),
               saved=torch.load(GF.checkpoint_file(str(path)), weights_only=False)["optimizer_state_dict"]["param_groups"])
    monkeypatch.undo()
    return out


def test_graphed_loop_with_groups_equals_eager(gpu, monkeypatch, tmp_path):
    a, b = _train(monkeypatch, False, tmp_path / "eager"), _train(monkeypatch, True, tmp_path / "graph")
    assert a["replays"] == 0 and b["replays"] == 8
    assert len(a["groups"]) == 4 and a["groups"] == b["groups"]                 # per-group lr (as the scheduler left it), wd, sizes
    assert [g[1] for g in a["groups"]] == [1e-2, 0.0, 1e-2, 0.0]
    assert a["groups"][0][0] == a["groups"][1][0] > 0 and a["groups"][2][0] == a["groups"][3][0] > 0
    assert abs(a["groups"][2][0] / a["groups"][0][0] - 0.1) < 1e-9
    assert a["step"] == b["step"] > 0
    assert len(a["logged"]) == 8 and a["logged"] == b["logged"]
    assert all(torch.equal(x, y) for x, y in zip(a["params"], b["params"]))
    for ma, mb in zip(a["moments"], b["moments"]):
        assert (ma is None) == (mb is None) and (ma is None or (torch.equal(ma[0], mb[0]) and torch.equal(ma[1], mb[1])))
    assert any(m is not None for m in a["moments"])
    assert len(a["saved"]) == 4 and [len(g["params"]) for g in a["saved"]] == [g[2] for g in a["groups"]]        # best.pt holds the four groups


def _steps(stepper, sched, batches, first):
    for k, (inp, lab) in enumerate(batches):
        stepper(inp, lab, epoch=0)
        sched.step((first + k + 1) / 8)


def test_best_pt_with_groups_resumes_to_the_same_bits(gpu, tmp_path):
    """Two steps, best.pt, two more steps -- against a fresh model and a fresh four-group optimizer that load that best.pt and take the same two
    steps.  (Dropout 0: a fresh module's dropout counters restart, its masks would differ.)"""
    cfg = _tiny_cfg()
    batches = [synthetic.make_batch(cfg, 2, seed=300 + i, s_text=16, t_audio=8000, n_visual_true=4) for i in range(4)]
    crit = GF.CrossEntropyLoss()
    kw = dict(lr=1e-3, weight_decay=1e-2, clip=1.0, encoder_lr_scale=0.1, no_decay_norm_bias=True)
    pre, model = _models(cfg, dropout=0.0)
    st = T.TrainStep(model, pre, crit, **kw)
    sched = T.CosineWarmRestarts(st.opt, T_0=2)
    _steps(st, sched, batches[:2], 0)
    GF.save_model(model, pre, st.opt, crit, sched, 0, 1, str(tmp_path), 2400)
    _steps(st, sched, batches[2:], 2)
    torch.cuda.synchronize()

    pre2, model2 = _models(cfg, dropout=0.0)
    st2 = T.TrainStep(model2, pre2, crit, **kw)
    assert len(st2.opt.param_groups) == 4
    GF.load_model(model2, pre2, st2.opt, crit, str(tmp_path))
    sched2 = T.CosineWarmRestarts(st2.opt, T_0=2)
    sched2.load_state_dict(torch.load(GF.checkpoint_file(str(tmp_path)), weights_only=False)["scheduler"])
    assert st2.opt.step_count == 2 and len(sched2.base_lrs) == 4
    _steps(st2, sched2, batches[2:], 2)
    torch.cuda.synchronize()
    assert st.opt.step_count == st2.opt.step_count == 4
    assert [(g["lr"], g["weight_decay"]) for g in st.opt.param_groups] == [(g["lr"], g["weight_decay"]) for g in st2.opt.param_groups]
    for p, q in zip(st.opt.params, st2.opt.params):
        assert p.shape == q.shape and torch.equal(p, q)
        assert (p in st.opt.state) == (q in st2.opt.state)
        if p in st.opt.state:
            assert torch.equal(st.opt.state[p][0], st2.opt.state[q][0]) and torch.equal(st.opt.state[p][1], st2.opt.state[q][1])


def test_default_groups_are_real_in_the_first_step(gpu):
    """One step of TrainStep(encoder_lr_scale=0.1, no_decay_norm_bias=True) at lr 1e-2, wd 0.1: a pretrained matrix moves as the fp64 step at
    lr / 10 says, element by element within step_end_ref's bounds (and not as the step at the full rate says); a vector outside the encoders
    takes the fp64 step with wd = 0 (and not the decayed one).  The clip coefficient is the word the step itself computed."""
    cfg = _tiny_cfg()
    pre, model = _models(cfg, dropout=0.0)
    lr, wd = 1e-2, 0.1
    st = T.TrainStep(model, pre, GF.CrossEntropyLoss(), lr=lr, weight_decay=wd, clip=1.0, encoder_lr_scale=0.1, no_decay_norm_bias=True)
    groups = st.opt.param_groups
    assert [(g["lr"], g["weight_decay"]) for g in groups] == [(lr, wd), (lr, 0.0), (lr * 0.1, wd), (lr * 0.1, 0.0)]
    inp, lab = synthetic.make_batch(cfg, 2, seed=300, s_text=16, t_audio=8000, n_visual_true=4)
    st.forward_backward(inp, lab, epoch=0)
    bert = {id(p) for p in model.bert.parameters()}
    picks = {"pretrained matrix": next(p for p in groups[2]["params"] if id(p) in bert and p.ndim == 2 and p.grad is not None),
             "pretrained vector": next(p for p in groups[3]["params"] if p.grad is not None and float(p.detach().abs().max()) > 0.5),
             "new matrix": next(p for p in groups[0]["params"] if p.ndim == 2 and p.grad is not None),
             "new vector": next(p for p in groups[1]["params"] if p.grad is not None and float(p.detach().abs().max()) > 0.5)}     # (norm weights)
    before = {k: (p.detach().cpu().numpy().ravel().copy(), p.grad.detach().cpu().numpy().ravel().copy()) for k, p in picks.items()}
    st.update()
    torch.cuda.synchronize()
    cc = float(st.opt._scal[1].item())
    assert 0.0 < cc <= 1.0 and st.opt.step_count == 1
    right = {"pretrained matrix": (lr * 0.1, wd), "pretrained vector": (lr * 0.1, 0.0), "new matrix": (lr, wd), "new vector": (lr, 0.0)}
    wrong = {"pretrained matrix": (lr, wd), "pretrained vector": (lr * 0.1, wd), "new matrix": (lr * 0.1, wd), "new vector": (lr, wd)}
    for k, p in picks.items():
        p0, g0 = before[k]
        z = np.zeros_like(p0)
        got = (p.detach().cpu().numpy().ravel(), st.opt.state[p][0].cpu().numpy().ravel(), st.opt.state[p][1].cpu().numpy().ravel())
        r = SR.ratios(SR.ref_step(p0, g0, z, z, 1, SR.f32(right[k][0]), right[k][1], cc), *got)
        w = SR.ratios(SR.ref_step(p0, g0, z, z, 1, SR.f32(wrong[k][0]), wrong[k][1], cc), *got)
        print(f"{k}: ratio to bound p {r['p']:.3f} m {r['m']:.3f} v {r['v']:.3f}; with the other group's values p {w['p']:.3g}")
        assert r["p"] <= 1.0 and r["m"] <= 1.0 and r["v"] <= 1.0, (k, r)
        assert w["p"] > 1.0, (k, w)
        assert np.any(g0 != 0) and not np.array_equal(got[0], p0)
