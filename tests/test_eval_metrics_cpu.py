"""CPU-only checks of the evaluation pass: hvk_eval_metrics' export and argument validation
(which runs before any HIP call), EvalMetrics' state / compute / cross-rank sum, and Trainer.eval
with the EVAL_* events and EMA's in-place weight exchange on a plain-torch model."""
import ctypes
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HVK_OK, HVK_EINVAL = 0, 1


# --------------------------------------------------------------------------- C ABI
def _args(**over):
    """A valid hvk_eval_metrics argument list (addresses never dereferenced before a launch)."""
    p = ctypes.c_void_p
    a = dict(logits=p(0x1000), dtype=0, B=4, L=10, ld=10, targets=p(0x2000), t_stride=1, t_off=0,
             tree_dists=None, dist_dtype=0, leaf_paths=None, target_paths=None, topk=5, pred=p(0x3000),
             rank=p(0x3000), nll=p(0x4000), dist=p(0x3000), tier_hit=None, state=p(0x6000), stream=None)
    assert set(over) <= set(a)
    a.update(over)
    return list(a.values())


def test_symbol_exported_and_bound():
    from hvamd import _lib
    assert "hvk_eval_metrics" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["hvk_eval_metrics"][1]) == 20
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "hvk_eval_metrics")
    assert _lib.ABI_VERSION >= 17 and _lib.load().hvk_abi_version() == _lib.ABI_VERSION


P = ctypes.c_void_p(0x7000)
BAD = [("B<0", dict(B=-1), b"shape"), ("L<1", dict(L=0), b"shape"), ("ld<L", dict(ld=9), b"shape"),
       ("topk<1", dict(topk=0), b"topk"),
       ("logits", dict(logits=None), b"null"), ("targets", dict(targets=None), b"null"),
       ("pred", dict(pred=None), b"null"), ("rank", dict(rank=None), b"null"), ("nll", dict(nll=None), b"null"),
       ("dist", dict(dist=None), b"null"), ("state", dict(state=None), b"null"),
       ("paths-without-targets", dict(leaf_paths=P), b"target_paths"),
       ("both-sources", dict(tree_dists=P, leaf_paths=P, target_paths=P), b"both"),
       ("logits-dtype", dict(dtype=2), b"dtype"), ("dist-dtype", dict(tree_dists=P, dist_dtype=2), b"dtype"),
       ("t_off", dict(t_stride=7, t_off=7), b"stride"), ("tier_hit", dict(tier_hit=P), b"tier_hit")]


@pytest.mark.parametrize("name,over,word", BAD, ids=[b[0] for b in BAD])
def test_invalid_arguments_refused_before_any_launch(name, over, word):
    from hvamd import _lib
    lib = _lib.load()
    assert lib.hvk_eval_metrics(*_args(**over)) == HVK_EINVAL
    msg = lib.hvk_last_error_string()
    assert b"hvk_eval_metrics" in msg and word in msg, msg


def test_empty_batch_is_ok_without_a_launch():
    from hvamd import _lib
    lib = _lib.load()
    assert lib.hvk_eval_metrics(*_args(B=0)) == HVK_OK
    assert lib.hvk_eval_metrics(*_args(B=0, dtype=1, leaf_paths=P, target_paths=P, tier_hit=P, t_stride=7,
                                       t_off=6)) == HVK_OK
    assert lib.hvk_eval_metrics(*_args(B=0, topk=0)) == HVK_EINVAL  # still validated


def test_ops_wrapper_refuses_cpu_tensors():
    import hvamd.ops as ops
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.eval_metrics(torch.zeros(2, 5), torch.zeros(2, dtype=torch.int64),
                         torch.zeros(16, dtype=torch.float64))


# --------------------------------------------------------------------------- EvalMetrics state
def _state(valid=8, top1=2, topk=6, nll=12.0, dist=20, invalid=0, tiers=(8, 7, 6, 5, 4, 3, 2)):
    return torch.tensor([valid, top1, topk, nll, dist, invalid, *tiers, 0, 0, 0], dtype=torch.float64)


def test_compute_from_hand_set_state_and_state_dict_round_trip():
    from hvamd.hierarchy import EvalMetrics, Taxonomy
    m = EvalMetrics()
    assert list(m.state_dict()) == ["state"] and m.state.dtype == torch.float64 and m.state.shape == (16,)
    m.load_state_dict({"state": _state()})
    assert m.compute() == {"acc@1": 0.25, "acc@5": 0.75, "cross-entropy": 1.5}
    m3 = EvalMetrics(tree_dists=torch.zeros(4, 4, dtype=torch.uint8), topk=3)
    m3.load_state_dict(m.state_dict())
    assert torch.equal(m3.state, _state())
    assert m3.compute() == {"acc@1": 0.25, "acc@3": 0.75, "cross-entropy": 1.5, "tree-dist": 2.5}
    tax = Taxonomy.synthetic((2, 3, 4, 5, 6, 7, 12))
    mt = EvalMetrics(taxonomy=tax)
    assert mt.leaf_paths.dtype == torch.int32 and mt.leaf_paths.shape == (12, 7)
    mt.load_state_dict({"state": _state()})
    out = mt.compute()
    assert out["tree-dist"] == 2.5
    assert [out[f"acc@1/tier{t}"] for t in range(7)] == [1.0, 0.875, 0.75, 0.625, 0.5, 0.375, 0.25]
    assert set(out) == {"acc@1", "acc@5", "cross-entropy", "tree-dist"} | {f"acc@1/tier{t}" for t in range(7)}
    mt.reset()
    assert torch.equal(mt.state, torch.zeros(16, dtype=torch.float64))
    with pytest.raises(ValueError):
        EvalMetrics(topk=0)


def test_compute_raises_on_invalid_rows():
    from hvamd.hierarchy import EvalMetrics
    m = EvalMetrics()
    m.load_state_dict({"state": _state(invalid=3)})
    with pytest.raises(ValueError, match="3 target"):
        m.compute()


def test_update_refuses_float_targets_and_cpu_logits():
    from hvamd.hierarchy import EvalMetrics
    m = EvalMetrics()
    with pytest.raises(ValueError):
        m.update(torch.zeros(2, 5), torch.zeros(2, 5))
    with pytest.raises(RuntimeError, match="GPU only"):
        m.update([torch.zeros(2, 3), torch.zeros(2, 5)], torch.zeros(2, 7, dtype=torch.int64))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from hvamd.hierarchy import EvalMetrics
    m = EvalMetrics(tree_dists=torch.zeros(4, 4, dtype=torch.uint8))
    mine = _state() if rank == 0 else _state(valid=24, top1=6, topk=10, nll=4.0, dist=12)
    m.load_state_dict({"state": mine})
    res = m.compute()
    res["state_untouched"] = bool(torch.equal(m.state, mine))  # the sum is not written back
    out[rank] = res
    dist.destroy_process_group()


def test_two_gloo_ranks_both_get_the_summed_result():
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_rank_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    want = {"acc@1": 8 / 32, "acc@5": 16 / 32, "cross-entropy": 16.0 / 32, "tree-dist": 1.0,
            "state_untouched": True}
    assert out[0] == want and out[1] == want


# --------------------------------------------------------------------------- Trainer.eval on CPU
class _Recorder:
    """An algorithm that records every event it is offered and what the forward would see."""

    def __init__(self):
        self.events = []

    def match(self, event, state):
        self.events.append(event)
        return False


class _Net(torch.nn.Module):
    def __init__(self, fail_at=None):
        super().__init__()
        torch.manual_seed(0)
        self.fc1 = torch.nn.Linear(6, 16)
        self.drop = torch.nn.Dropout(0.5)  # eval() must switch it off
        self.fc2 = torch.nn.Linear(16, 9)
        self.calls, self.fail_at, self.seen = 0, fail_at, []

    def forward(self, x):
        self.calls += 1
        self.seen.append((self.training, torch.is_grad_enabled(), self.fc2.bias.detach().clone()))
        if self.fail_at is not None and self.calls == self.fail_at:
            raise RuntimeError("bad batch")
        return self.fc2(self.drop(torch.relu(self.fc1(x))))


def _cpu_trainer(algorithms=(), fail_at=None):
    from hvamd.models import Model
    from hvamd.trainer import Trainer
    net = _Net(fail_at)
    model = Model(net, train_metrics={}, val_metrics={}, loss_fn=torch.nn.functional.cross_entropy)
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    return Trainer(model, opt, algorithms=algorithms), net


def _batches(sizes=(4, 4, 3)):
    g = torch.Generator().manual_seed(5)
    return [(torch.randn(b, 6, generator=g), torch.randint(0, 9, (b,), generator=g)) for b in sizes]


def _class_metrics():
    from hvamd import hierarchy
    # cross-entropy is scored by the HIP loss kernel in this package: on the CPU, a torch one
    class CE(hierarchy._SumMetric):
        def update(self, preds, targets):
            self.num += torch.nn.functional.cross_entropy(preds, targets, reduction="sum").double()
            self.den += preds.shape[0]
    g = torch.Generator().manual_seed(9)
    td = torch.randint(0, 8, (9, 9), generator=g, dtype=torch.uint8)
    return {"acc@1": hierarchy.Accuracy(9), "acc@5": hierarchy.Accuracy(9, top_k=5),
            "tree-dist": hierarchy.TreeDistance(td), "cross-entropy": CE()}


def test_trainer_eval_cpu_events_results_and_untouched_training_state():
    from hvamd.algorithmic import Event
    rec = _Recorder()
    tr, net = _cpu_trainer([rec])
    batches = _batches()
    tr.train_step(batches[0])  # leaves a timestamp and training mode behind
    for p in tr.model.parameters():  # and gradients that an evaluation must not touch
        p.grad = torch.full_like(p, 0.25)
    grads = [p.grad.clone() for p in tr.model.parameters()]
    before = [p.detach().clone() for p in tr.model.parameters()]
    stamp = tr.state.timestamp_batch
    rec.events.clear()
    net.seen.clear()
    for was_training in (True, False):
        tr.model.train(was_training)
        rec.events.clear()
        got = tr.eval(batches, _class_metrics())
        assert rec.events == [Event.EVAL_START] + [Event.EVAL_BATCH_END] * 3 + [Event.EVAL_END]
        assert tr.model.training is was_training and net.drop.training is was_training
    assert all(s[0] is False and s[1] is False for s in net.seen)  # eval mode, no grad, every batch
    # a hand loop over the same batches, ragged last one included
    net.eval()
    want = _class_metrics()
    with torch.no_grad():
        for x, y in batches:
            for m in want.values():
                m.update(net(x), y)
    assert set(got) == set(want)
    for k in want:
        assert torch.equal(got[k], want[k].compute()), k
    assert tr.state.timestamp_batch == stamp
    for p, g, b in zip(tr.model.parameters(), grads, before):
        assert torch.equal(p.grad, g) and torch.equal(p.detach(), b)


def test_trainer_eval_without_metrics_needs_a_fused_metrics_model():
    from hvamd.trainer import Trainer
    net = torch.nn.Linear(3, 2)
    tr = Trainer(net, torch.optim.SGD(net.parameters(), lr=0.1))
    with pytest.raises(ValueError, match="fused_metrics"):
        tr.eval([])


@pytest.mark.parametrize("fail_at", [None, 2])
def test_ema_weights_are_exchanged_in_place_and_back(fail_at):
    """With an EMA holding known averages the forward sees the averages; afterwards parameters
    and averages are bit-equal to before at unchanged addresses, also when a batch raises."""
    from hvamd.algorithmic import EMA
    ema = EMA(half_life="100ba", update_interval="1ba")
    tr, net = _cpu_trainer([ema], fail_at=fail_at)
    params = list(tr.model.parameters())
    g = torch.Generator().manual_seed(3)
    ema.ema_params = [torch.randn(p.shape, generator=g) for p in params]
    avg = [e.clone() for e in ema.ema_params]
    before = [p.detach().clone() for p in params]
    ptrs = [p.data_ptr() for p in params] + [e.data_ptr() for e in ema.ema_params]
    idx = [i for i, p in enumerate(params) if p is net.fc2.bias][0]
    if fail_at is None:
        tr.eval(_batches(), _class_metrics())
    else:
        with pytest.raises(RuntimeError, match="bad batch"):
            tr.eval(_batches(), _class_metrics())
    assert len(net.seen) == (3 if fail_at is None else 2)
    assert all(torch.equal(s[2], avg[idx]) for s in net.seen)
    assert not torch.equal(avg[idx], before[idx])
    for p, b, e, a in zip(params, before, ema.ema_params, avg):
        assert torch.equal(p.detach(), b) and torch.equal(e, a)
    assert [p.data_ptr() for p in params] + [e.data_ptr() for e in ema.ema_params] == ptrs
    assert tr.model.training


def test_ema_eval_with_ema_false_scores_the_training_weights():
    from hvamd.algorithmic import EMA
    ema = EMA(update_interval="1ba", eval_with_ema=False)
    tr, net = _cpu_trainer([ema])
    ema.ema_params = [torch.zeros_like(p) for p in tr.model.parameters()]
    bias = net.fc2.bias.detach().clone()
    tr.eval(_batches((2,)), _class_metrics())
    assert torch.equal(net.seen[0][2], bias) and all(not e.any() for e in ema.ema_params)


def test_fused_metrics_report_what_the_metric_dicts_report():
    """Model.fused_metrics(is_train) carries tree-dist where models.py:61-101 adds it, and the
    taxonomy (path distance, per-tier accuracies) for the "hxe" variant."""
    from hvamd import configs, hierarchy, models
    mini = dict(img_size=56, embed_dim=32, depths=[2, 2], num_heads=[1, 2], window_size=7)
    tax = hierarchy.Taxonomy.synthetic((2, 3, 4, 5, 6, 7, 12))
    dists = torch.zeros(12, 12, dtype=torch.uint8)
    for variant in ("", "hxe", "multitask"):
        for cfg_train in (True, False):
            cfg = configs.Config()
            cfg.model.name = "swinv2_tiny_window7_224"
            cfg.hierarchy.variant = variant
            cfg.is_train = cfg_train
            nc = tuple(tax.num_classes) if variant == "multitask" else 12
            m = models.build_composer_model(cfg, models.DatasetInfo(num_classes=nc, tree_dists=dists,
                                                                    taxonomy=tax), **mini)
            for is_train in (True, False):
                f = m.fused_metrics(is_train=is_train)
                assert isinstance(f, hierarchy.EvalMetrics) and f.topk == 5
                assert f is not m.fused_metrics(is_train=is_train)
                keys = set(m.get_metrics(is_train=is_train))
                f.load_state_dict({"state": _state()})
                extra = {f"acc@1/tier{t}" for t in range(7)} | {"tree-dist"} if variant == "hxe" else set()
                assert set(f.compute()) == keys | extra, (variant, cfg_train, is_train)
                assert (f.leaf_paths is not None) == (variant == "hxe")
                assert (f.tree_dists is not None) == ("tree-dist" in keys)
    bare = models.Model(torch.nn.Linear(2, 2), {}, {}, None).fused_metrics()
    assert set(bare.compute()) == {"acc@1", "acc@5", "cross-entropy"}


def test_train_metrics_default_off():
    tr, _ = _cpu_trainer()
    assert tr.train_metrics is None
