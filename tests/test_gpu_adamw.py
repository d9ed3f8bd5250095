"""hvk_adamw_step (DDP mean + clip + AdamW + EMA in one fused pass) on the GPU: against the
foreach path of the same optimizer, its edge cases and argument checks, and wired into the
Trainer, eagerly and as a captured HIP graph."""
import copy
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

LR, WD = 1e-2, 0.05
SHAPES = [(288, 96), (96,), (3, 1, 1), (70001,)]  # several 16384-element chunks, a ragged scalar tail
N_TINY = 66  # 5 + 66 tensors: the list crosses the 64-tensor kernel-argument batch


def _tensor_list():
    """The test's parameters on the GPU: SHAPES, a misaligned view (pointer 4 B past a 16-B
    boundary: the scalar path at n % 4 == 0) and N_TINY 5-element tensors."""
    ps = [torch.nn.Parameter(torch.randn(s, device="cuda")) for s in SHAPES]
    ps.append(torch.nn.Parameter(torch.randn(4097, device="cuda")[1:]))
    assert ps[-1].data_ptr() % 16 == 4 and ps[-1].is_contiguous()
    ps += [torch.nn.Parameter(torch.randn(5, device="cuda")) for _ in range(N_TINY)]
    return ps


def _groups(ps):
    decay = [ps[0], ps[2], ps[4]] + ps[5::2]
    ids = set(map(id, decay))
    return [{"params": decay}, {"params": [p for p in ps if id(p) not in ids], "weight_decay": 0.0}]


def _rel(a, b):
    return ((a - b).norm() / a.norm().clamp_min(1e-12)).item()


@pytest.mark.parametrize("decoupled", [False, True])
@pytest.mark.parametrize("gscale,ema", [(1.0, False), (0.5, True)])
def test_fused_adamw_step_matches_foreach_path(gscale, ema, decoupled):
    """The fused step against the foreach path of the same optimizer on CPU copies: three steps
    (first-step state init, then the moment updates; the lr changed before the third), decay and
    no-decay groups, clipping active, float4 and scalar paths, two kernel-argument batches; with
    gscale the gradients are rank sums whose 1/world mean is folded in, with ema the EMA rides on
    the same pass.  rtol 1e-5 / atol 1e-6 on p, exp_avg, exp_avg_sq and the EMA."""
    from hvamd.optim import AdamW
    torch.manual_seed(0)
    ps_gpu = _tensor_list()
    ps_cpu = [torch.nn.Parameter(p.detach().cpu().clone()) for p in ps_gpu]
    em_gpu = [p.detach().clone() + 0.1 for p in ps_gpu]
    em_cpu = [e.cpu().clone() for e in em_gpu]
    og = AdamW(_groups(ps_gpu), lr=LR, weight_decay=WD, decoupled=decoupled)
    oc = AdamW(_groups(ps_cpu), lr=LR, weight_decay=WD, decoupled=decoupled)
    for step in range(3):
        if step == 2:
            for o in (og, oc):
                for g in o.param_groups:
                    g["lr"] = 0.3 * LR
        for pg, pc in zip(ps_gpu, ps_cpu):
            g = torch.randn(pg.shape) * 3
            pg.grad, pc.grad = g.cuda(), g.clone()
        for o, ps, es in ((og, ps_gpu, em_gpu), (oc, ps_cpu, em_cpu)):
            o.pending_clip = 2.0
            o.pending_grad_scale = gscale
            if ema:
                o.pending_ema = ([(id(p), e) for p, e in zip(ps, es)], 0.8)
        assert og._fused_eligible()
        og.step()
        oc.step()
        for i, (pg, pc) in enumerate(zip(ps_gpu, ps_cpu)):
            assert float(og.state[pg]["step"]) == step + 1
            assert torch.allclose(pg.detach().cpu(), pc.detach(), rtol=1e-5, atol=1e-6), ("p", i, step)
            for key in ("exp_avg", "exp_avg_sq"):
                assert torch.allclose(og.state[pg][key].cpu(), oc.state[pc][key], rtol=1e-5,
                                      atol=1e-6), (key, i, step)
        for i, (eg, ec) in enumerate(zip(em_gpu, em_cpu)):
            assert torch.allclose(eg.cpu(), ec, rtol=1e-5, atol=1e-6), ("ema", i, step)
    assert og.pending_grad_scale == 1.0 and og.pending_ema is None and og.pending_clip is None


def test_first_step_zero_gradient_only_decays():
    """A first-step all-zero gradient: 0 / (0 + eps) = 0, so p moves by the decay factor alone
    and both moments are exactly 0 (no NaN), next to a tensor with an ordinary gradient."""
    from hvamd.optim import AdamW
    torch.manual_seed(1)
    a = torch.nn.Parameter(torch.randn(1000, device="cuda"))
    b = torch.nn.Parameter(torch.randn(37, 9, device="cuda"))
    a0 = a.detach().clone()
    opt = AdamW([a, b], lr=LR, weight_decay=WD)
    a.grad, b.grad = torch.zeros_like(a), torch.randn_like(b)
    opt.pending_clip = 2.0
    opt.step()
    torch.cuda.synchronize()
    assert torch.equal(a.detach(), a0 * (1 - LR * WD))
    assert not opt.state[a]["exp_avg"].any() and not opt.state[a]["exp_avg_sq"].any()
    assert torch.isfinite(b.detach()).all() and opt.state[b]["exp_avg_sq"].gt(0).any()


def _run(ps0, grads, steps, gscale=1.0, clip=None):
    from hvamd.optim import AdamW
    ps = [torch.nn.Parameter(p.clone()) for p in ps0]
    opt = AdamW(_groups(ps), lr=LR, weight_decay=WD)
    for s in range(steps):
        for p, g in zip(ps, grads[s]):
            p.grad = g.clone()
        opt.pending_grad_scale, opt.pending_clip = gscale, clip
        opt.step()
    torch.cuda.synchronize()
    return ([p.detach() for p in ps], [opt.state[p]["exp_avg"] for p in ps],
            [opt.state[p]["exp_avg_sq"] for p in ps])


def _inputs(seed, steps):
    torch.manual_seed(seed)
    ps0 = [p.detach() for p in _tensor_list()]
    return ps0, [[3 * torch.randn_like(p) for p in ps0] for _ in range(steps)]


def test_clip_disabled_is_the_gradient_scale_alone():
    """Without a clip (max_norm <= 0) coef = grad_scale: the same as gradients pre-scaled on the
    host (0.25: the product is exact, so the results are bit-identical)."""
    ps0, grads = _inputs(2, 2)
    a = _run(ps0, grads, 2, gscale=0.25)
    b = _run(ps0, [[0.25 * g for g in gs] for gs in grads], 2)
    for ta, tb in zip(a, b):
        for x, y in zip(ta, tb):
            assert torch.equal(x, y)


def test_two_runs_are_bit_identical():
    """No atomics, a fixed summation order in the norm: p, exp_avg and exp_avg_sq of two runs from
    the same inputs (clip active, two steps) are bit-identical."""
    ps0, grads = _inputs(3, 2)
    a = _run(ps0, grads, 2, clip=2.0)
    b = _run(ps0, grads, 2, clip=2.0)
    for ta, tb in zip(a, b):
        for x, y in zip(ta, tb):
            assert torch.equal(x, y)


def test_bad_arguments_return_a_status_and_launch_nothing():
    from hvamd import _lib
    lib = _lib.load()
    torch.manual_seed(4)
    n = 3
    p, g, m, v = ([torch.rand(100 + i, device="cuda") for i in range(n)] for _ in range(4))
    before = [t.clone() for t in p + m + v]
    P = ctypes.c_void_p * n
    tab = {k: P(*[t.data_ptr() for t in ts]) for k, ts in (("p", p), ("g", g), ("m", m), ("v", v))}
    numel = (ctypes.c_longlong * n)(*[t.numel() for t in p])
    group = (ctypes.c_int * n)(0, 0, 0)
    step_size, decay = (ctypes.c_float * 4)(LR, 0, 0, 0), (ctypes.c_float * 4)(1, 1, 1, 1)
    nb = lib.hvk_adamw_workspace_bytes(n, ctypes.cast(numel, ctypes.c_void_p))
    ws = torch.empty(nb // 4, device="cuda")
    cast = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731

    def call(p_tab=tab["p"], ngroups=1, ws_bytes=nb, beta1=0.9):
        return lib.hvk_adamw_step(n, cast(p_tab) if p_tab is not None else None, cast(tab["g"]),
                                  cast(tab["m"]), cast(tab["v"]), None, cast(numel), cast(group),
                                  cast(step_size), cast(decay), ngroups, None, 1.0, 2.0, beta1, 0.999, 1e-8,
                                  0.03, 0, 0.0, _lib.ptr(ws), ws_bytes, _lib.stream())

    for kwargs, word in (({"p_tab": None}, b"null"), ({"ngroups": 5}, b"groups"),
                         ({"ws_bytes": nb - 4}, b"workspace"), ({"beta1": 1.0}, b"betas")):
        rc = call(**kwargs)
        assert rc != 0 and word in lib.hvk_last_error_string(), (kwargs, lib.hvk_last_error_string())
    torch.cuda.synchronize()
    for t, b in zip(p + m + v, before):
        assert torch.equal(t, b)
    assert call() == 0  # the same call with valid arguments runs
    torch.cuda.synchronize()
    assert not torch.equal(p[0], before[0])


# ---------------------------------------------------------------- Trainer wiring
def _setup(seed=0):
    """The mini SwinV2 + HXE of tests/test_gpu_graph.py."""
    from hvamd import hierarchy, models, swinv2
    torch.manual_seed(seed)
    dev = torch.device("cuda:0")
    tax = hierarchy.Taxonomy.synthetic((2, 3, 4, 5, 6, 7, 12))
    net = swinv2.SwinTransformerV2(img_size=56, embed_dim=32, depths=[2, 2], num_heads=[1, 2],
                                   window_size=7, num_classes=tax.num_leaves,
                                   drop_path_rate=0.0).to(dev)
    loss_fn = hierarchy.HierarchicalCrossEntropy(tax, tree_weights="exponential").to(dev)
    model = models.Model(net, None, None, loss_fn)
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(4, 3, 56, 56, device=dev, generator=g)
    y = torch.tensor(tax.leaf_paths[[1, 5, 9, 11]], device=dev)
    return model, (x, y)


def _trainer(model, decoupled=False):
    from hvamd import optim
    from hvamd.algorithmic import EMA, GradientClipping
    from hvamd.trainer import Trainer
    opt = optim.AdamW(optim.set_weight_decay(model), lr=1e-3, weight_decay=WD, decoupled=decoupled)
    return Trainer(model, opt, [GradientClipping("norm", 2.0), EMA("4ba", "2ba")])


def _ema(trainer):
    return trainer.algorithms[1].ema_params


def twin_errors(model_a, model_b, init, ema_a=None, ema_b=None):
    """{tensor class: (worst error, name)} of two trainers' parameters and EMA copies:
    |a - b| / |a| for the weights of >= 2 dimensions and the 1-D tensors that do not start at
    zero; |a - b| / |a - init| for the zero-initialised 1-D tensors, whose whole value is Adam's
    normalised update (it amplifies gradient rounding noise, and |a| would hide nothing)."""
    worst = {}
    names = [n for n, _ in model_a.named_parameters()]

    def note(prefix, name, a, b):
        p0 = init[name]
        if a.dim() == 1 and not p0.any():
            cls, err = "zero_init_1d", ((a - b).norm() / (a - p0).norm().clamp_min(1e-12)).item()
        else:
            cls, err = ("weights" if a.dim() >= 2 else "other_1d"), _rel(a, b)
        if err > worst.get(prefix + cls, (-1.0, ""))[0]:
            worst[prefix + cls] = (err, name)
    for name, pa, pb in zip(names, model_a.parameters(), model_b.parameters()):
        note("", name, pa.detach(), pb.detach())
    if ema_a is not None:
        for name, ea, eb in zip(names, ema_a, ema_b):
            note("ema_", name, ea, eb)
    return worst


# The project's bound for twin trainers (tests/test_gpu_graph.py) is 1e-2.  The zero-initialised
# 1-D tensors do not hold it even between two runs of the SAME foreach path: the backward's f32
# atomics sum in a run-dependent order and Adam's normalised update turns that rounding noise into
# whole steps of the entries whose gradient is noise (worst everywhere: the 512 entries of
# layers.0.blocks.0.attn.cpb_mlp.0.bias).  Measured on an MI355X (tools/adamw_twin_spread.py,
# profiles/adamw/twin_spread.txt): foreach against foreach, 5 runs = 10 pairs per step sequence
# of this file, worst pair 2.117e-2 (4 steps), 2.528e-2 (5), 5.503e-2 (6), 1.103e-2 (lr schedule)
# for the parameters and 1.813e-2, 1.819e-2, 4.224e-2, 8.323e-3 for their EMA copies.  The figure
# is itself that noisy, so the class takes the largest; its bound is 4 x that spread:
# 4 x 5.503e-2 = 0.2201 and 4 x 4.224e-2 = 0.1690.  No reading of the fused path enters it (for
# information, fused against foreach in the same run: 3.3e-2, 3.4e-2, 5.6e-2, 3.2e-2).
SPREAD = {"zero_init_1d": 5.503e-2, "ema_zero_init_1d": 4.224e-2}
BOUNDS = {"weights": 1e-2, "other_1d": 1e-2, "ema_weights": 1e-2, "ema_other_1d": 1e-2,
          "zero_init_1d": 4 * SPREAD["zero_init_1d"], "ema_zero_init_1d": 4 * SPREAD["ema_zero_init_1d"]}


def _assert_twins(worst):
    print("twin errors:", {k: (f"{e:.3e}", n) for k, (e, n) in worst.items()})
    for cls, (err, name) in worst.items():
        assert err < BOUNDS[cls], (cls, name, err)


def test_trainer_runs_the_fused_step_and_matches_the_foreach_twin(monkeypatch):
    """Trainer + GradientClipping + EMA on AdamW: four steps with the clip and the EMA handed to
    the fused step against a twin on the foreach path (options.fused_optim off); the fused entry
    point is what the first trainer ran, and never the twin.  1e-2 on every tensor class but the
    zero-initialised 1-D tensors, whose bound is 4 x the foreach path's own run-to-run spread
    (BOUNDS: 5.503e-2 -> 0.2201, EMA copies 4.224e-2 -> 0.1690)."""
    from hvamd import _lib, options
    model, batch = _setup()
    model_b = copy.deepcopy(model)
    init = {n: p.detach().clone() for n, p in model.named_parameters()}
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    ta, tb = _trainer(model), _trainer(model_b)
    for _ in range(4):
        ta.train_step(batch)
    assert calls.count("hvk_adamw_step") == 4
    with options.override(fused_optim=False):
        for _ in range(4):
            tb.train_step(batch)
    assert calls.count("hvk_adamw_step") == 4
    torch.cuda.synchronize()
    assert float(ta.optimizer.state[next(model.parameters())]["step"]) == 4
    _assert_twins(twin_errors(model, model_b, init, _ema(ta), _ema(tb)))


def test_graph_replay_matches_eager_adamw():
    """capture(warmup=3) + 3 replays == 6 eager steps: every replay runs with its own step's
    bias corrections, read from the device array."""
    model, batch = _setup()
    model_b = copy.deepcopy(model)
    init = {n: p.detach().clone() for n, p in model.named_parameters()}
    ta, tb = _trainer(model), _trainer(model_b)
    for _ in range(6):
        ta.train_step(batch)
    tb.capture(batch, warmup=3)
    assert tb._live_hyper
    for _ in range(3):
        tb.replay()
    torch.cuda.synchronize()
    assert float(tb.optimizer.state[next(model_b.parameters())]["step"]) == 6
    _assert_twins(twin_errors(model, model_b, init, _ema(ta), _ema(tb)))


def test_graph_replay_follows_lr_schedule_adamw():
    """An lr change between replays reaches the captured update; at lr 0 (decoupled: decay 1) a
    replay leaves the weights bit-unchanged."""
    model, batch = _setup()
    model_b = copy.deepcopy(model)
    init = {n: p.detach().clone() for n, p in model.named_parameters()}
    ta, tb = _trainer(model, decoupled=True), _trainer(model_b, decoupled=True)
    for _ in range(4):
        ta.train_step(batch)
    tb.capture(batch, warmup=3)
    tb.replay()
    for lr in (3e-3, 0.0):
        for t in (ta, tb):
            for grp in t.optimizer.param_groups:
                grp["lr"] = lr
        ta.train_step(batch)
        tb.replay()
        if lr == 0.0:
            before = [p.detach().clone() for p in model_b.parameters()]
            tb.replay()
            torch.cuda.synchronize()
            for b, p in zip(before, model_b.parameters()):
                assert torch.equal(b, p.detach())
    torch.cuda.synchronize()
    _assert_twins(twin_errors(model, model_b, init))


def test_eager_step_after_replay_continues_the_step_count():
    """capture(warmup=3) + replay + one eager step == 5 eager steps: the eager step runs as step
    5 (exp_avg_sq and the weights of a trainer that only ever stepped eagerly; 5e-2 on the state,
    the project's bound for optimizer state of twin trainers, tests/test_gpu_graph.py)."""
    model, batch = _setup()
    model_b = copy.deepcopy(model)
    init = {n: p.detach().clone() for n, p in model.named_parameters()}
    ta, tb = _trainer(model), _trainer(model_b)
    for _ in range(5):
        ta.train_step(batch)
    tb.capture(batch, warmup=3)
    tb.replay()
    tb.train_step(batch)
    torch.cuda.synchronize()
    for (name, pa), (_, pb) in zip(model.named_parameters(), model_b.named_parameters()):
        sa, sb = ta.optimizer.state[pa], tb.optimizer.state[pb]
        assert float(sa["step"]) == float(sb["step"]) == 5, name
        if pa.dim() >= 2:
            assert _rel(sa["exp_avg_sq"], sb["exp_avg_sq"]) < 5e-2, name
    _assert_twins(twin_errors(model, model_b, init))


def test_capture_refuses_the_foreach_path():
    """With the fused step off, capture() raises instead of baking bias corrections into a graph."""
    from hvamd import options
    model, batch = _setup()
    t = _trainer(model)
    with options.override(fused_optim=False):
        with pytest.raises(RuntimeError, match="bias corrections"):
            t.capture(batch, warmup=1)
    torch.cuda.synchronize()
