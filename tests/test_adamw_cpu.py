"""hvamd.optim.AdamW without a GPU: the foreach path against a float64 restatement of AdamW and
against torch.optim.AdamW, the hand-over surface, the state dict, build_optimizer and the C ABI
entries of the fused step."""
import copy
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR0, WD, BETAS, EPS = 1e-2, 0.05, (0.9, 0.999), 1e-8
SHAPES = [(7, 5), (5,), (3, 1, 1), (11,)]


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in SHAPES]


def _groups(ps, wd0=None):
    """decay group (the >= 2-D tensors) and no-decay group"""
    first = {"params": [ps[0], ps[2]]}
    if wd0 is not None:
        first["weight_decay"] = wd0
    return [first, {"params": [ps[1], ps[3]], "weight_decay": 0.0}]


def _grads(step):
    g = torch.Generator().manual_seed(100 + step)
    return [3 * torch.randn(s, generator=g) for s in SHAPES]


def _adamw64(p, g, m, v, t, lr, decay):
    """One AdamW step in float64, written out: returns (p, m, v)."""
    b1, b2 = BETAS
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    p = p * decay
    p = p - (lr / (1 - b1 ** t)) * m / (v.sqrt() / (1 - b2 ** t) ** 0.5 + EPS)
    return p, m, v


@pytest.mark.parametrize("decoupled", [False, True])
def test_foreach_path_matches_float64_adamw_and_torch(decoupled):
    """3 steps, decay and no-decay groups, the lr changed before step 3, fresh gradients each
    step: p, exp_avg and exp_avg_sq against the float64 restatement and against torch.optim.AdamW
    (weight_decay / lr0 for the decoupled form) at rtol 1e-5, atol 1e-6 -- f32 rounding over
    three steps of sums without cancellation is a few 2^-24 relative, the lerp's cancellation a
    few ulp of max(|m|, |g|) ~ 1e-6 at |g| <= 10."""
    from hvamd.optim import AdamW
    ps, pt = _params(), _params()
    opt = AdamW(_groups(ps), lr=LR0, betas=BETAS, eps=EPS, weight_decay=WD, decoupled=decoupled)
    twin = torch.optim.AdamW(_groups(pt), lr=LR0, betas=BETAS, eps=EPS,
                             weight_decay=WD / LR0 if decoupled else WD, foreach=True)
    is_decay = [True, False, True, False]
    p64 = [p.detach().double() for p in ps]
    m64 = [torch.zeros_like(p) for p in p64]
    v64 = [torch.zeros_like(p) for p in p64]
    lr = LR0
    for step in range(1, 4):
        if step == 3:
            lr = 0.3 * LR0
            for o in (opt, twin):
                for g in o.param_groups:
                    g["lr"] = lr
        gs = _grads(step)
        for p, q, g in zip(ps, pt, gs):
            p.grad, q.grad = g.clone(), g.clone()
        opt.step()
        twin.step()
        for i, g in enumerate(gs):
            if not is_decay[i]:
                decay = 1.0
            elif decoupled:
                decay = 1 - WD * lr / LR0
            else:
                decay = 1 - lr * WD
            p64[i], m64[i], v64[i] = _adamw64(p64[i], g.double(), m64[i], v64[i], step, lr, decay)
        for i, (p, q) in enumerate(zip(ps, pt)):
            st, tw = opt.state[p], twin.state[q]
            assert float(st["step"]) == step
            for name, got, want, other in (("p", p.detach(), p64[i], q.detach()),
                                           ("exp_avg", st["exp_avg"], m64[i], tw["exp_avg"]),
                                           ("exp_avg_sq", st["exp_avg_sq"], v64[i], tw["exp_avg_sq"])):
                assert torch.allclose(got.double(), want, rtol=1e-5, atol=1e-6), (name, i, step)
                assert torch.allclose(got, other, rtol=1e-5, atol=1e-6), ("torch", name, i, step)


def test_parameter_without_gradient_keeps_its_step():
    from hvamd.optim import AdamW
    ps = _params()
    opt = AdamW(_groups(ps), lr=LR0)
    for step in (1, 2):
        for i, (p, g) in enumerate(zip(ps, _grads(step))):
            p.grad = None if (i == 1 and step == 2) else g
        opt.step()
    assert [float(opt.state[p]["step"]) for p in ps] == [2.0, 1.0, 2.0, 2.0]


def test_handovers_act_on_the_foreach_path_and_are_reset():
    """pending_grad_scale, pending_clip and pending_ema on the CPU path equal scaling and
    clipping the gradients by hand before a plain step and averaging after it; all three are
    reset by step(), also when it raises."""
    from hvamd.optim import AdamW
    ps, pr = _params(), _params()
    opt = AdamW(_groups(ps), lr=LR0, weight_decay=WD)
    ref = AdamW(_groups(pr), lr=LR0, weight_decay=WD)
    emas = [p.detach().clone() + 0.1 for p in ps]
    ema_ref = [e.clone() for e in emas]
    assert opt.supports_fused_clip() and opt.supports_grad_scale()
    for p, q, g in zip(ps, pr, _grads(1)):
        p.grad, q.grad = g.clone(), 0.5 * g
    opt.pending_grad_scale, opt.pending_clip = 0.5, 2.0
    opt.pending_ema = ([(id(p), e) for p, e in zip(ps, emas)], 0.8)
    norm = torch.nn.utils.clip_grad_norm_(pr, 2.0)
    assert norm > 2.0  # the clip is active
    opt.step()
    ref.step()
    for p, q, e, er in zip(ps, pr, emas, ema_ref):
        assert torch.allclose(p.detach(), q.detach(), rtol=1e-6, atol=1e-7)
        assert torch.allclose(e, 0.8 * er + 0.2 * q.detach(), rtol=1e-6, atol=1e-7)
    assert opt.pending_clip is None and opt.pending_grad_scale == 1.0 and opt.pending_ema is None

    opt.pending_grad_scale, opt.pending_clip = 0.5, 2.0
    opt.pending_ema = ([(id(ps[0]), torch.zeros(2))], 0.8)  # wrong shape: the step raises
    for p, g in zip(ps, _grads(2)):
        p.grad = g
    with pytest.raises(RuntimeError):
        opt.step()
    assert opt.pending_clip is None and opt.pending_grad_scale == 1.0 and opt.pending_ema is None


def test_state_dict_round_trips_into_a_fresh_instance_and_into_torch():
    from hvamd.optim import AdamW
    ps = _params()
    opt = AdamW(_groups(ps), lr=LR0, betas=BETAS, eps=EPS, weight_decay=WD)
    for step in (1, 2):
        for p, g in zip(ps, _grads(step)):
            p.grad = g
        opt.step()
    sd = opt.state_dict()
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    pa = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    pb = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    fresh = AdamW(_groups(pa), lr=1.0, weight_decay=0.5)  # overwritten by the loaded groups
    fresh.load_state_dict(copy.deepcopy(sd))
    twin = torch.optim.AdamW(_groups(pb, wd0=WD), lr=LR0, betas=BETAS, eps=EPS, weight_decay=WD,
                             foreach=True)
    twin.load_state_dict(copy.deepcopy(sd))
    for p, a, b, g in zip(ps, pa, pb, _grads(3)):
        p.grad, a.grad, b.grad = g.clone(), g.clone(), g.clone()
    opt.step()
    fresh.step()
    twin.step()
    for p, a, b in zip(ps, pa, pb):
        assert torch.equal(p.detach(), a.detach())
        assert torch.equal(opt.state[p]["exp_avg_sq"], fresh.state[a]["exp_avg_sq"])
        assert float(fresh.state[a]["step"]) == 3 and float(twin.state[b]["step"]) == 3
        assert torch.allclose(p.detach(), b.detach(), rtol=1e-6, atol=1e-7)
        assert torch.allclose(opt.state[p]["exp_avg"], twin.state[b]["exp_avg"], rtol=1e-6, atol=1e-7)
    # and torch's state loads here
    back = AdamW(_groups(_params()), lr=LR0)
    back.load_state_dict(twin.state_dict())
    assert back.state[back.param_groups[0]["params"][0]]["step"] == 3.0  # torch's tensor -> host number


def test_unsupported_forms_raise():
    from hvamd.optim import AdamW
    with pytest.raises(ValueError):
        AdamW(_params(), amsgrad=True)
    with pytest.raises(ValueError):
        AdamW(_params(), maximize=True)
    with pytest.raises(ValueError):
        AdamW(_params(), betas=(1.0, 0.999))


@pytest.mark.parametrize("name,decoupled", [("AdamW", False), ("DecoupledAdamW", True)])
def test_build_optimizer_returns_the_native_adamw(name, decoupled):
    from hvamd.optim import AdamW, DecoupledSGDW, build_optimizer
    model = torch.nn.Sequential(torch.nn.Linear(4, 3), torch.nn.LayerNorm(3))
    cfg = types.SimpleNamespace(optim=types.SimpleNamespace(name=name, lr=0.02, momentum=0.9,
                                                            weight_decay=0.05))
    opt = build_optimizer(cfg, model)
    assert type(opt) is AdamW
    decay_g, plain_g = opt.param_groups
    assert decay_g["decoupled"] is decoupled and tuple(decay_g["betas"]) == (0.9, 0.999)
    assert [tuple(p.shape) for p in decay_g["params"]] == [(3, 4)] and plain_g["weight_decay"] == 0.0
    for g in opt.param_groups:
        g["lr"] = 0.01
    want = 1 - 0.05 * 0.01 / 0.02 if decoupled else 1 - 0.01 * 0.05
    assert opt._decay(decay_g) == pytest.approx(want, rel=1e-12) and opt._decay(plain_g) == 1.0
    cfg.optim.name = "DecoupledSGDW"
    assert type(build_optimizer(cfg, model)) is DecoupledSGDW


def test_abi_declares_the_adamw_entries():
    from hvamd import _lib
    hdr = open(os.path.join(ROOT, "include", "hvk.h")).read()
    for name in ("hvk_adamw_workspace_bytes", "hvk_adamw_step"):
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    assert len(_lib.SIGNATURES["hvk_adamw_step"][1]) == 23
    lib = _lib.load()
    numel = (torch.tensor([1, 16384, 16385, 70001]).numpy().astype("int64"))
    nb = lib.hvk_adamw_workspace_bytes(4, numel.ctypes.data)
    assert nb == (1 + 1 + 2 + 5 + 1) * 4  # one f32 slot per 16384-element chunk + the coefficient
