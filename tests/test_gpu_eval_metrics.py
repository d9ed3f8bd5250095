"""hvk_eval_metrics / hierarchy.EvalMetrics / Trainer.eval on the GPU against the numpy float64
restatement of tests/eval_metrics_ref.py (run on the logits as the kernel sees them: bf16 cases
round first)."""
import functools

import numpy as np
import pytest
import torch

import eval_metrics_ref as ref
from oracle import hierarchy_ref

pytestmark = pytest.mark.gpu

EXACT_STATE = [0, 1, 2, 4, 5, 6, 7, 8, 9, 10, 11, 12]
KINDS = ("randn", "quant", "const", "zeros", "ninf")


@functools.lru_cache(maxsize=None)
def _taxonomy(L):
    from hvamd.hierarchy import Taxonomy
    return Taxonomy.synthetic(tuple(min(s, L) for s in (3, 13, 51, 273, 1103, 4884, L)))


def _logits(kind, B, L, gen):
    """f32 CPU logits; every kind but "randn" is tie-heavy in f32 already."""
    z = torch.randn(B, L, generator=gen)
    if kind == "quant":
        z = (z * 2).round() / 2
    elif kind == "const":  # one constant per row, -inf and both zeros among them
        c = torch.tensor([0.0, -0.0, 1.5, float("-inf"), -3.0])[torch.arange(B) % 5]
        z = c[:, None].expand(B, L).clone()
    elif kind == "zeros":  # -0.0 and +0.0 mixed, a few entries below and (every other row) above
        sign = torch.randint(0, 2, (B, L), generator=gen).bool()
        zero = torch.where(sign, torch.tensor(-0.0), torch.tensor(0.0))
        z = torch.where(z < -1.0, torch.tensor(-1.0), zero)
        z[1::2] = torch.where(torch.randn(B, L, generator=gen)[1::2] > 1.8, torch.tensor(2.0), z[1::2])
    elif kind == "ninf":
        z = (z * 2).round() / 2
        z[torch.rand(B, L, generator=gen) < 0.3] = float("-inf")
    return z


def _targets(z, topk, gen):
    """Classes that sit at the top-k boundary of the stable order (rows 0, 1 of every 4), at the
    top (row 2), anywhere (row 3)."""
    B, L = z.shape
    zn = z.float().numpy().astype(np.float64)
    t = torch.randint(0, L, (B,), generator=gen)
    for b in range(B):
        order = np.argsort(-zn[b], kind="stable")
        if b % 4 == 0:
            t[b] = int(order[min(topk - 1, L - 1)])
        elif b % 4 == 1:
            t[b] = int(order[min(topk, L - 1)])
        elif b % 4 == 2:
            t[b] = int(order[0])
    return t


def _boundary_ties(zn, t, k):
    """Rows whose target is inside a run of equal values that straddles rank k."""
    n = 0
    for b in range(len(t)):
        g = int((zn[b] > zn[b, t[b]]).sum())
        e = int((zn[b] == zn[b, t[b]]).sum())
        n += e >= 2 and g < k < g + e
    return n


def _place(z, layout):
    """The logits on the GPU in one of three memory layouts; returns the [B, L] view."""
    B, L = z.shape
    if layout == "dense":
        return z.cuda()
    if layout == "padded":  # ld > L, every row on a 16-B boundary: vector loads plus a scalar tail
        buf = torch.full((B, (L + 7) // 8 * 8 + 8), 7e4, dtype=z.dtype, device="cuda")
        v = buf[:, :L]
    else:  # "shifted": no row on a 16-B boundary: the element-wise path
        buf = torch.full((B, (L + 1 + 7) // 8 * 8), 7e4, dtype=z.dtype, device="cuda")
        v = buf[:, 1:L + 1]
        assert v.data_ptr() % 16 != 0
    v.copy_(z)
    return v


def _run(zv, t, topk, **kw):
    import hvamd.ops as ops
    state = torch.zeros(16, dtype=torch.float64, device="cuda")
    out = ops.eval_metrics(zv, t, state, topk=topk, **kw)
    return [None if o is None else o.cpu().numpy() for o in out], state.cpu().numpy()


def _check_exact(got, state, r, want_state, what):
    pred, rank, nll, dist, hit = got
    assert np.array_equal(pred, r["pred"]), what
    assert np.array_equal(rank, r["rank"]), what
    assert np.array_equal(dist, r["dist"]), what
    if hit is not None:
        assert np.array_equal(hit, r["tier_hit"]), what
    assert np.array_equal(state[EXACT_STATE], want_state[EXACT_STATE]), (what, state, want_state)
    assert not state[13:].any()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("L", [1, 4, 5, 6, 255, 256, 257, 2049, 10000])
def test_rows_and_counts_equal_the_reference_exactly(L, dtype):
    """pred, rank, dist, tier_hit and every count of the state, in path mode, over tie-heavy
    rows, three memory layouts, [B] and strided [B, 7] targets, topk 1 and 5 (>= L included)."""
    tax = _taxonomy(L)
    paths = torch.from_numpy(tax.leaf_paths.astype(np.int32)).cuda()
    gen = torch.Generator().manual_seed(1000 + L)
    ties = 0
    for B in ((8,) if L == 10000 else (1, 3, 64)):
        for ki, kind in enumerate(KINDS):
            z = _logits(kind, B, L, gen).to(dtype)
            zn = z.float().numpy()  # what the kernel sees
            t = _targets(z, 5, gen)
            tp = torch.from_numpy(tax.leaf_paths[t.numpy()])  # int64 [B, 7], column 6 = leaf id
            assert torch.equal(tp[:, -1], t)
            r = ref.rows(zn, t.numpy(), leaf_paths=tax.leaf_paths, target_paths=tp.numpy())
            if L > 5:
                ties += _boundary_ties(zn.astype(np.float64), t.numpy(), 5)
            for li, layout in enumerate(("dense", "padded", "shifted")):
                zv = _place(z, layout)
                for topk in (1, 5):
                    # [B, 7] labels read through stride 7 / offset 6, or [B] classes
                    tg = tp.cuda() if (ki + li + topk) % 2 else t.cuda()
                    got, state = _run(zv, tg, topk, leaf_paths=paths, target_paths=tp.cuda(), tier_hit=True)
                    _check_exact(got, state, r, ref.state(r, topk, L), (kind, B, layout, topk))
    if L > 5:
        assert ties >= (3 if L == 10000 else 10), ties


def test_bf16_randn_has_targets_tied_at_the_topk_boundary():
    """bf16 randn at L = 10 000 (the shape of real logits): equal values are common, and rows whose
    target is tied across rank 5 must be ranked by index like the stable sort."""
    L, B = 10000, 8
    gen = torch.Generator().manual_seed(17)  # a draw with three such rows among its eight
    z = torch.randn(B, L, generator=gen).bfloat16()
    zn = z.float().numpy().astype(np.float64)
    t = torch.zeros(B, dtype=torch.int64)
    for b in range(B):  # the 5th or 6th entry of the stable order
        t[b] = int(np.argsort(-zn[b], kind="stable")[4 + b % 2])
    assert _boundary_ties(zn, t.numpy(), 5) >= 3
    r = ref.rows(zn, t.numpy())
    got, state = _run(z.cuda(), t.cuda(), 5)
    _check_exact(got, state, r, ref.state(r, 5, L), "bf16 randn")
    assert (got[3] == -1).all() and got[4] is None


def test_out_of_range_targets_are_counted_invalid_and_contribute_nothing():
    gen = torch.Generator().manual_seed(3)
    L = 37
    z = torch.randn(6, L, generator=gen)
    t = torch.tensor([-1, 4, L, 0, L - 1, 2 ** 40])
    td = torch.randint(0, 8, (L, L), generator=gen, dtype=torch.uint8)
    r = ref.rows(z.numpy(), t.numpy(), tree_dists=td.numpy())
    assert list(r["valid"]) == [False, True, False, True, True, False]
    got, state = _run(z.cuda(), t.cuda(), 5, tree_dists=td.cuda())
    _check_exact(got, state, r, ref.state(r, 5, L), "invalid")
    assert state[0] == 3 and state[5] == 3
    assert np.isnan(got[2][[0, 2, 5]]).all() and np.isfinite(got[2][[1, 3, 4]]).all()
    assert abs(state[3] - r["nll"][r["valid"]].sum()) < 1e-4
    from hvamd.hierarchy import EvalMetrics
    m = EvalMetrics().cuda()
    m.update(z.cuda(), t.cuda())
    with pytest.raises(ValueError, match="3 target"):
        m.compute()


def test_nan_logits_do_not_fault_and_indices_stay_in_range():
    L = 300
    z = torch.randn(4, L, generator=torch.Generator().manual_seed(4))
    z[0, :] = float("nan")
    z[1, 5] = float("nan")
    z[2, ::2] = float("nan")
    t = torch.tensor([0, 5, 1, 7])
    got, state = _run(z.cuda(), t.cuda(), 5)
    pred, rank, nll = got[0], got[1], got[2]
    assert ((pred >= 0) & (pred < L)).all() and ((rank >= 0) & (rank < L)).all()
    want = torch.nn.functional.cross_entropy(z.cuda(), t.cuda(), reduction="none").cpu().numpy()
    assert np.array_equal(np.isnan(nll), np.isnan(want)) and np.isnan(nll[:3]).all()
    assert pred[3] == int(z[3].argmax()) and state[0] == 4


def test_path_distance_equals_the_oracle_and_the_matrix_modes():
    """The restatement's path distance is the oracle's tree_dist on synthetic_inat_names; the
    kernel's matrix mode (uint8, f32) and path mode give the same dist."""
    from hvamd.hierarchy import HierarchicalLabel, Taxonomy, build_tree_dist_matrix
    names = hierarchy_ref.synthetic_inat_names((2, 3, 4, 5, 6, 7, 30))
    tax = Taxonomy(names)
    L = tax.num_leaves
    srt = sorted(names)
    oracle = np.array([[hierarchy_ref.tree_dist(a, b) for b in srt] for a in srt])
    mine = np.array([[ref.path_dist(tax.leaf_paths[a], tax.leaf_paths[b]) for b in range(L)] for a in range(L)])
    assert np.array_equal(mine, oracle)
    mat = build_tree_dist_matrix([HierarchicalLabel.parse(n) for n in names])
    assert np.array_equal(mat.numpy(), oracle)
    gen = torch.Generator().manual_seed(5)
    z = torch.randn(64, L, generator=gen)
    t = torch.randint(0, L, (64,), generator=gen)
    tp = torch.from_numpy(tax.leaf_paths[t.numpy()])
    r = ref.rows(z.numpy(), t.numpy(), leaf_paths=tax.leaf_paths, target_paths=tp.numpy())
    assert np.array_equal(r["dist"], oracle[r["pred"], t.numpy()]) and len(set(r["dist"])) > 3
    paths = torch.from_numpy(tax.leaf_paths.astype(np.int32)).cuda()
    by_path, sp = _run(z.cuda(), t.cuda(), 5, leaf_paths=paths, target_paths=tp.cuda(), tier_hit=True)
    by_u8, s8 = _run(z.cuda(), t.cuda(), 5, tree_dists=mat.cuda())
    by_f32, sf = _run(z.cuda(), t.cuda(), 5, tree_dists=mat.float().cuda())
    for got in (by_path, by_u8, by_f32):
        assert np.array_equal(got[3], r["dist"])
    assert sp[4] == s8[4] == sf[4] == r["dist"].sum()
    _check_exact(by_path, sp, r, ref.state(r, 5, L), "path")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_nll_within_four_times_torch_f32_error(dtype):
    """nll against the float64 restatement.  The bound is 4 x the worst row of torch's own f32
    F.cross_entropy(reduction="none") on the same rows (the reduction order differs, nothing
    else).  Measured on MI355X (worst |error| over the 392 rows, kernel / torch): f32 logits
    1.58e-06 / 1.58e-06, bf16 logits 8.2e-07 / 8.2e-07 (profiles/eval_metrics/nll_spread.txt)."""
    gen = torch.Generator().manual_seed(77)
    mine, theirs, lines = [], [], []
    for L in (1, 4, 5, 6, 255, 256, 257, 2049, 10000):
        B = 8 if L == 10000 else 48
        z = (3 * torch.randn(B, L, generator=gen)).to(dtype)
        t = torch.randint(0, L, (B,), generator=gen)
        want = ref.rows(z.float().numpy(), t.numpy())["nll"]
        for layout in ("dense", "shifted"):
            got, _ = _run(_place(z, layout), t.cuda(), 5)
            e = np.abs(got[2].astype(np.float64) - want)
            mine.append(e)
        tt = torch.nn.functional.cross_entropy(z.float().cuda(), t.cuda(), reduction="none").cpu().numpy()
        theirs.append(np.abs(tt.astype(np.float64) - want))
        lines.append(f"L {L:5d} B {B:2d}: kernel max |err| {max(mine[-1].max(), mine[-2].max()):.3e}  "
                     f"torch f32 max |err| {theirs[-1].max():.3e}  max nll {want.max():.3f}")
    worst_mine, worst_torch = np.concatenate(mine).max(), np.concatenate(theirs).max()
    print(f"\nnll spread, {str(dtype).split('.')[-1]} logits, |f32 result - float64 reference|:")
    print("\n".join(lines))
    print(f"worst row: kernel {worst_mine:.3e}, torch {worst_torch:.3e}, bound 4 x torch = {4 * worst_torch:.3e}")
    assert worst_torch > 0
    assert worst_mine <= 4 * worst_torch, (worst_mine, worst_torch)


def _batches3(L, tax, gen, B=(64, 64, 17)):
    out = []
    for b in B:
        z = torch.randn(b, L, generator=gen)
        t = torch.randint(0, L, (b,), generator=gen)
        t[::3] = z[::3].argmax(1)
        out.append((z, t))
    return out


def test_three_updates_accumulate_and_two_runs_are_bit_identical():
    from hvamd.hierarchy import EvalMetrics
    L = 2049
    tax = _taxonomy(L)
    data = _batches3(L, tax, torch.Generator().manual_seed(6))
    want = np.zeros(16)
    for z, t in data:
        tp = tax.leaf_paths[t.numpy()]
        want += ref.state(ref.rows(z.numpy(), t.numpy(), leaf_paths=tax.leaf_paths, target_paths=tp), 5, L)
    states = []
    for _ in range(2):
        m = EvalMetrics(taxonomy=tax).cuda()
        for z, t in data:
            m.update(z.cuda(), t.cuda())
        states.append(m.state.cpu())
        assert m.pred.shape == m.rank.shape == m.nll.shape == m.dist.shape == (17,)  # the last batch's rows
    assert torch.equal(states[0], states[1])
    s = states[0].numpy()
    assert np.array_equal(s[EXACT_STATE], want[EXACT_STATE])
    assert abs(s[3] - want[3]) <= 1e-6 * want[3]
    out = m.compute()
    n = want[0]
    assert out["acc@1"] == want[1] / n and out["acc@5"] == want[2] / n and out["tree-dist"] == want[4] / n
    assert [out[f"acc@1/tier{q}"] for q in range(7)] == [want[6 + q] / n for q in range(7)]
    assert out["acc@1/tier6"] == out["acc@1"] and 0.3 < out["acc@1"] < 0.5
    m.reset()
    assert not m.state.any()


def test_matches_the_metric_classes_on_tie_free_inputs():
    """The returned dict against Accuracy / CrossEntropyMetric / TreeDistance (CE tolerance from
    test_gpu_metrics.py: 1e-5 relative)."""
    from hvamd import hierarchy
    L = 500
    gen = torch.Generator().manual_seed(8)
    td = torch.randint(0, 8, (L, L), generator=gen, dtype=torch.uint8).cuda()
    fused = hierarchy.EvalMetrics(tree_dists=td).cuda()
    classes = {"acc@1": hierarchy.Accuracy(L), "acc@5": hierarchy.Accuracy(L, top_k=5),
               "cross-entropy": hierarchy.CrossEntropyMetric(), "tree-dist": hierarchy.TreeDistance(td)}
    for b in (32, 32, 9):
        z = torch.randn(b, L, generator=gen)
        assert all(len(np.unique(row)) == L for row in z.numpy())  # tie-free
        t = torch.randint(0, L, (b,), generator=gen)
        t[::2] = z[::2].topk(5, dim=1)[1][:, 3]
        t[::4] = z[::4].argmax(1)
        fused.update(z.cuda(), t.cuda())
        for m in classes.values():
            m.cuda().update(z.cuda(), t.cuda())
    out = fused.compute()
    assert set(out) == set(classes)
    for k in ("acc@1", "acc@5", "tree-dist"):
        assert abs(out[k] - classes[k].compute().item()) < 1e-6, k
    ce = classes["cross-entropy"].compute().item()
    assert abs(out["cross-entropy"] - ce) < 1e-5 * abs(ce)
    assert 0.2 < out["acc@1"] < out["acc@5"] < 0.8


def test_update_is_capturable_and_replays_accumulate():
    from hvamd.hierarchy import EvalMetrics
    L, B = 257, 24
    tax = _taxonomy(L)
    gen = torch.Generator().manual_seed(9)
    z = torch.randn(B, L, generator=gen)
    t = torch.randint(0, L, (B,), generator=gen)
    tp = tax.leaf_paths[t.numpy()]
    one = ref.state(ref.rows(z.numpy(), t.numpy(), leaf_paths=tax.leaf_paths, target_paths=tp), 5, L)
    m = EvalMetrics(taxonomy=tax).cuda()
    zc, tc = z.cuda(), t.cuda()
    m.update(zc, tc)  # warm-up outside the capture
    torch.cuda.synchronize()
    m.reset()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        m.update(zc, tc)
    torch.cuda.synchronize()
    assert not m.state.any()  # capturing runs nothing
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    s = m.state.cpu().numpy()
    assert np.array_equal(s[EXACT_STATE], 3 * one[EXACT_STATE])
    assert abs(s[3] - 3 * one[3]) <= 1e-6 * 3 * one[3]


# --------------------------------------------------------------------------- Trainer.eval
MINI = dict(img_size=56, embed_dim=32, depths=[2, 2], num_heads=[1, 2], window_size=7, drop_path_rate=0.0)
MEAN = [0.463 * 255, 0.480 * 255, 0.376 * 255]
STD = [0.209 * 255, 0.200 * 255, 0.231 * 255]
SIZES = (2, 3, 4, 5, 6, 7, 12)


def _composer_model(variant, seed=0, is_train=True):
    from hvamd import configs, hierarchy, models
    torch.manual_seed(seed)
    tax = hierarchy.Taxonomy.synthetic(SIZES)
    names = [hierarchy.HierarchicalLabel.parse(c) for c in tax.classes]
    cfg = configs.Config()
    cfg.model.name = "swinv2_tiny_window7_224"
    cfg.hierarchy.variant = variant
    cfg.is_train = is_train
    nc = tuple(tax.num_classes) if variant == "multitask" else tax.num_leaves
    info = models.DatasetInfo(num_classes=nc, tree_dists=hierarchy.build_tree_dist_matrix(names), taxonomy=tax)
    return models.build_composer_model(cfg, info, **MINI).cuda(), tax, info


def _trainer(model, algorithms=(), lr=0.05, **kw):
    from hvamd import optim
    from hvamd.trainer import Trainer
    opt = optim.DecoupledSGDW(optim.set_weight_decay(model), lr=lr, momentum=0.9, weight_decay=5e-4)
    return Trainer(model, opt, list(algorithms), **kw)


def _u8_batches(tax, sizes, seed):
    gen = torch.Generator().manual_seed(seed)
    out = []
    for b in sizes:
        x = torch.randint(0, 256, (b, 3, 56, 56), generator=gen, dtype=torch.uint8)
        leaf = torch.randint(0, tax.num_leaves, (b,), generator=gen)
        out.append((x.cuda(), torch.from_numpy(tax.leaf_paths[leaf.numpy()]).cuda()))
    return out


def _f32_batch(b):
    return (b[0].float() / 255 - 0.5, b[1])


def _leaf_logits(outputs):
    return (outputs[-1] if isinstance(outputs, list) else outputs).detach()


def _want(logit_batches, target_batches, tax, tree_dists=None, paths=True):
    s = np.zeros(16)
    for z, y in zip(logit_batches, target_batches):
        y = y.cpu().numpy()
        r = ref.rows(z.float().cpu().numpy(), y[:, -1], tree_dists=tree_dists,
                     leaf_paths=tax.leaf_paths if paths else None, target_paths=y)
        s += ref.state(r, 5, z.shape[1])
    return s


@pytest.mark.parametrize("variant", ["hxe", "multitask"])
def test_trainer_eval_mini_swinv2_equals_hand_loop(variant):
    """Trainer.eval at batch 8 (ragged last batch) with NormalizationFn device transforms --
    folded into the model for "hxe", applied per batch for "multitask" -- against a hand-written
    no-grad loop scored by the restatement."""
    from hvamd.algorithmic import Event
    from hvamd.data import NormalizationFn
    model, tax, info = _composer_model(variant)
    norm = NormalizationFn(MEAN, STD)
    events = []

    class Rec:
        def match(self, event, state):
            events.append(event)
            return False

    tr = _trainer(model, [Rec()], device_transforms=norm if variant == "hxe" else (lambda b: norm(b)))
    assert (tr.device_transforms is None) == (variant == "hxe")
    batches = _u8_batches(tax, (8, 8, 5), 21)
    model.train()
    events.clear()
    out = tr.eval(batches)
    assert events == [Event.EVAL_START] + [Event.EVAL_BATCH_END] * 3 + [Event.EVAL_END]
    assert model.training and tr.state.timestamp_batch == 0
    assert all(p.grad is None for p in model.parameters())
    model.eval()
    logits = []
    with torch.no_grad():
        for b in batches:
            b = tr.device_transforms(b) if tr.device_transforms is not None else b
            with torch.autocast("cuda", dtype=torch.bfloat16):
                logits.append(_leaf_logits(model(b)))
    mt = variant == "multitask"
    want = _want(logits, [b[1] for b in batches], tax, tree_dists=info.tree_dists.numpy() if mt else None,
                 paths=not mt)
    n = want[0]
    assert n == 21
    keys = {"acc@1", "acc@5", "cross-entropy", "tree-dist"}
    assert set(out) == (keys if mt else keys | {f"acc@1/tier{q}" for q in range(7)})
    assert out["acc@1"] == want[1] / n and out["acc@5"] == want[2] / n and out["tree-dist"] == want[4] / n
    assert abs(out["cross-entropy"] - want[3] / n) <= 1e-5 * want[3] / n
    if not mt:
        assert [out[f"acc@1/tier{q}"] for q in range(7)] == [want[6 + q] / n for q in range(7)]


def test_trainer_eval_with_ema_leaves_training_untouched():
    """EMA present: the evaluation scores the averages; afterwards the weights, the averages and
    their addresses are as before, and the next train_step's loss equals that of a twin with the
    same weights that never evaluated."""
    from hvamd.algorithmic import EMA
    model, tax, _ = _composer_model("hxe")
    ema = EMA(half_life="2ba", update_interval="1ba")
    tr = _trainer(model, [ema])
    batches = _u8_batches(tax, (8, 8), 22)
    x8 = _f32_batch(batches[0])
    for _ in range(3):
        tr.train_step(x8)
    torch.cuda.synchronize()
    params = list(model.parameters())
    before = [p.detach().clone() for p in params]
    avg = [e.clone() for e in ema.ema_params]
    ptrs = [t.data_ptr() for t in params + ema.ema_params]
    assert any(not torch.equal(b, a) for b, a in zip(before, avg))
    twin, _, _ = _composer_model("hxe")
    twin.load_state_dict(model.state_dict())
    fbatches = [_f32_batch(b) for b in batches]
    out = tr.eval(fbatches)
    # the same evaluation by hand on a model holding the averages
    scored, _, _ = _composer_model("hxe")
    scored.load_state_dict(model.state_dict())
    with torch.no_grad():
        for p, a in zip(scored.parameters(), avg):
            p.copy_(a)
        scored.eval()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            logits = [_leaf_logits(scored(b)) for b in fbatches]
    want = _want(logits, [b[1] for b in fbatches], tax)
    assert out["acc@1"] == want[1] / 16 and out["acc@5"] == want[2] / 16 and out["tree-dist"] == want[4] / 16
    assert abs(out["cross-entropy"] - want[3] / 16) <= 1e-5 * want[3] / 16
    for p, b, e, a in zip(params, before, ema.ema_params, avg):
        assert torch.equal(p.detach(), b) and torch.equal(e, a)
    assert [t.data_ptr() for t in params + ema.ema_params] == ptrs
    la = tr.train_step(x8)
    lb = _trainer(twin).train_step(x8)
    assert torch.equal(la, lb), (la.item(), lb.item())


@pytest.mark.parametrize("captured", [False, True], ids=["eager", "captured"])
def test_train_metrics_count_every_step_and_leave_the_loss_alone(captured):
    """Trainer.train_metrics set, at batch 8 under LabelSmoothing (the metrics must see the
    ORIGINAL targets): the counts equal the per-step restatement and every loss is bit-equal to a
    twin run without train metrics (lr 0: the weights, hence the forward, stay comparable)."""
    from hvamd.algorithmic import LabelSmoothing
    from hvamd.hierarchy import EvalMetrics
    model, tax, _ = _composer_model("hxe")
    twin, _, _ = _composer_model("hxe")
    twin.load_state_dict(model.state_dict())
    ta, tb = _trainer(model, [LabelSmoothing(0.1)]), _trainer(twin, [LabelSmoothing(0.1)])
    for tr in (ta, tb):
        for grp in tr.optimizer.param_groups:
            grp["lr"] = 0.0
    assert tb.train_metrics is None
    ta.train_metrics = EvalMetrics(taxonomy=tax).cuda()
    data = [_f32_batch(b) for b in _u8_batches(tax, (8, 8, 8), 23)]
    logits, la, lb = [], [], []
    if captured:
        x, y = data[0][0].clone(), data[0][1].clone()
        xb, yb = x.clone(), y.clone()
        ta.capture((x, y), warmup=3)
        tb.capture((xb, yb), warmup=3)
        torch.cuda.synchronize()
        assert not ta.train_metrics.state.any()  # the warm-up steps are not counted
        for xi, yi in data:
            x.copy_(xi), y.copy_(yi), xb.copy_(xi), yb.copy_(yi)
            la.append(ta.replay().clone())
            logits.append(_leaf_logits(ta.state.outputs).clone())
            lb.append(tb.replay().clone())
    else:
        for b in data:
            la.append(ta.train_step(b).clone())
            logits.append(_leaf_logits(ta.state.outputs).clone())
            lb.append(tb.train_step(b).clone())
    torch.cuda.synchronize()
    for a, b in zip(la, lb):
        assert torch.equal(a, b), (a.item(), b.item())
    want = _want(logits, [b[1] for b in data], tax)
    s = ta.train_metrics.state.cpu().numpy()
    assert want[0] == 24 and np.array_equal(s[EXACT_STATE], want[EXACT_STATE])
    assert abs(s[3] - want[3]) <= 1e-5 * want[3]
