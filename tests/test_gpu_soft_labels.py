"""Soft-labels loss kernels (hvk_soft_labels_* / _dense_*) against the float64 restatement
(tests/soft_labels_ref.py) and closed forms; the loss through the Trainer, eager and captured.
Tolerances are the HXE kernels' (test_gpu_hxe_soft.py): loss 1e-4 max(1, |ref|), gradient 1e-4
relative L2."""
import copy

import numpy as np
import pytest
import torch

import soft_labels_ref as S
import test_gpu_hxe_soft as X
from hxe_soft_ref import shuffled_tree

pytestmark = pytest.mark.gpu


def _run(tax, z, targets, scale=1.0, **kw):
    """(loss, dlogits) of the product loss for numpy logits and int or dense targets."""
    from hvamd.hierarchy import SoftLabelsCrossEntropy
    fn = SoftLabelsCrossEntropy(tax, **kw).cuda()
    zt = torch.from_numpy(np.asarray(z, np.float32)).cuda().requires_grad_(True)
    targets = np.asarray(targets)
    loss = fn(zt, torch.from_numpy(targets.astype(np.float32) if targets.dtype.kind == "f" else targets).cuda())
    (loss * scale).backward()
    return loss.item(), zt.grad.cpu().numpy()


def _tree(name):
    from hvamd.hierarchy import Taxonomy
    return shuffled_tree(40) if name == "shuffled40" else Taxonomy.synthetic(name)


def _logits(tax, B, seed):
    rng = np.random.default_rng(seed)
    return rng, (3 * rng.standard_normal((B, tax.num_leaves))).astype(np.float32)


@pytest.fixture(scope="module")
def big():
    """The 10 000-leaf tree at B = 2: LabelSmoothing(0.08)'s dense targets and their reference."""
    from hvamd.algorithmic import Event, LabelSmoothing, State
    tax = _tree((3, 13, 51, 273, 1103, 4884, 10000))
    _, z = _logits(tax, 2, 11)
    leaves = np.array([123, 9876])
    state = State(model=None)
    state.batch, state.outputs = (None, torch.from_numpy(tax.leaf_paths[leaves])), torch.from_numpy(z)
    LabelSmoothing(0.08).apply(Event.BEFORE_LOSS, state)
    q = state.batch[1].numpy()
    return tax, z, q, leaves, S.restatement(z, tax, q, S.level_weights64(15.0))


@pytest.mark.parametrize("beta", [4.0, 15.0])
@pytest.mark.parametrize("tree", [(2, 3, 4, 5, 6, 7, 12), "shuffled40"])
def test_hard_and_dense_vs_restatement(tree, beta):
    tax, w = _tree(tree), S.level_weights64(beta)
    rng, z = _logits(tax, 3, 7)
    leaves = rng.integers(tax.num_leaves, size=3)
    ref = S.restatement(z, tax, S.one_hot(leaves, tax.num_leaves), w)
    X._check(_run(tax, z, leaves, beta=beta), ref)
    X._check(_run(tax, z, tax.leaf_paths[leaves], beta=beta), ref)
    assert X.rel(_run(tax, z, leaves, beta=beta, scale=3.0)[1], 3 * ref[1]) < 1e-4  # grad_out reaches the kernel
    q = X._mixed_targets(rng, tax.num_leaves)  # smoothed, two-hot 0.7 / 0.3, all-zero
    ref = S.restatement(z, tax, q, w)
    loss, grad = _run(tax, z, q, beta=beta)
    X._check((loss, grad), ref)
    assert not grad[2].any()
    assert X.rel(_run(tax, z, q, beta=beta, scale=3.0)[1], 3 * ref[1]) < 1e-4


@pytest.mark.parametrize("sizes", [(1, 1, 1, 1, 1, 1, 600), (1, 1, 1, 1, 1, 2, 33),
                                   (1, 1, 1, 1, 2, 40, 80)])
def test_wide_rows_and_coinciding_ranges(sizes):
    """A row wider than the workgroup whose ranges coincide (d must be the FIRST containing
    level); genera either side of the lane / wave threshold; the wave path over child nodes."""
    tax, w = _tree(sizes), S.level_weights64(15.0)
    rng, z = _logits(tax, 2, 8)
    q = rng.random((2, tax.num_leaves))
    q /= q.sum(axis=1, keepdims=True)
    X._check(_run(tax, z, q), S.restatement(z, tax, q, w))
    leaves = np.array([0, tax.num_leaves - 1])
    X._check(_run(tax, z, leaves), S.restatement(z, tax, S.one_hot(leaves, tax.num_leaves), w))


def test_closed_form_anchors_and_max_subtraction():
    from hvamd.hierarchy import soft_cross_entropy
    tax = _tree("shuffled40")
    rng, z = _logits(tax, 3, 9)
    z *= 100.0 / z.max(axis=1, keepdims=True)  # row max 100: exp overflows without the max
    z64, leaves = z.astype(np.float64), np.array([3, 17, 39])
    lse = 100.0 + np.log(np.exp(z64 - 100.0).sum(1))
    uniform, ce = (lse - z64.mean(1)).mean(), (lse - z64[np.arange(3), leaves]).mean()
    flat = soft_cross_entropy(torch.from_numpy(z).cuda(), torch.from_numpy(leaves).cuda()).item()
    for targets in (leaves, S.one_hot(leaves, 40)):
        loss, grad = _run(tax, z, targets, beta=0.0)  # uniform target: LSE(z) - mean(z)
        assert np.isfinite(grad).all() and abs(loss - uniform) < 1e-4 * max(1.0, abs(uniform))
        loss, _ = _run(tax, z, targets, level_weights=[1.0] + [0.0] * 7)  # one-hot target: flat CE
        assert abs(loss - ce) < 1e-4 * max(1.0, abs(ce)) and abs(loss - flat) < 1e-4 * max(1.0, abs(ce))
        X._check(_run(tax, z, targets), S.restatement(z, tax, S.one_hot(leaves, 40), S.level_weights64(15.0)))


def test_big_tree_label_smoothing_and_one_hot(big):
    tax, z, q, leaves, ref = big
    X._check(_run(tax, z, q), ref)
    X._check(_run(tax, z, S.one_hot(leaves, tax.num_leaves)), _run(tax, z, leaves))


def test_deterministic_and_root_sum(big):
    import hvamd.ops as ops
    from hvamd.hierarchy import soft_label_level_weights
    tax, z, q, leaves, _ = big
    dev = torch.device("cuda:0")
    w = soft_label_level_weights(15.0).to(dev)
    inv, qt = tax.soft_label_norms(w.tolist(), dev), torch.from_numpy(q).to(dev)
    runs = []
    for _ in range(2):
        zt = torch.from_numpy(z).to(dev).requires_grad_(True)
        loss, nodes = ops.soft_labels_cross_entropy_dense(zt, qt, inv, *tax.device_soft_tables(dev), w,
                                                          return_nodes=True)
        hard = ops.soft_labels_cross_entropy(zt, torch.from_numpy(tax.leaf_paths[leaves]).to(dev),
                                             *tax.device_tables(dev)[:4], w)
        (loss + hard).backward()
        runs.append((loss.detach(), hard.detach(), nodes, zt.grad))
    assert torch.allclose(runs[0][2][:, -1], (qt * inv).sum(1), rtol=1e-5)  # the root: sum_c q_c / Z_c
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_out_of_range_hard_target_gives_nan():
    tax = _tree((2, 3, 4, 5, 6, 7, 12))
    paths = tax.leaf_paths[[1, 5]].copy()
    paths[1, 6], paths[0, 2] = tax.num_leaves, -1  # only the kernel's guard is exercised: nothing is read
    assert np.isnan(_run(tax, _logits(tax, 2, 10)[1], paths)[0])


def _setup():
    from hvamd.hierarchy import SoftLabelsCrossEntropy
    model, batch = X._setup()
    model.loss_fn = SoftLabelsCrossEntropy(model.loss_fn.taxonomy, beta=15.0).cuda()
    return model, batch


def test_trainer_label_smoothing_step_and_labels():
    from hvamd.algorithmic import smooth_labels
    model, (x, y) = _setup()
    ref_model = copy.deepcopy(model).train()
    with torch.no_grad():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = ref_model((x, y))
        ref = ref_model.loss(out, (x, smooth_labels(out, y[:, -1], 0.08))).item()
    tr = X._trainer(model, 0.08)
    loss = tr.train_step((x, y)).item()
    assert abs(loss - ref) < 1e-4 * abs(ref), (loss, ref)
    assert torch.equal(tr.state.batch[1], y)


def test_trainer_graph_replay_tracks_eager():
    model, batch = _setup()
    ta, tb = X._trainer(model, 0.08), X._trainer(copy.deepcopy(model), 0.08)
    la = [ta.train_step(batch) for _ in range(6)]
    tb.capture(batch, warmup=3)  # 3 eager steps inside, then capture
    lb = [tb.replay().clone() for _ in range(3)]
    torch.cuda.synchronize()
    for a, b in zip(la[3:], lb):
        assert abs(a.item() - b.item()) < 1e-3 * max(1.0, abs(a.item())), (a.item(), b.item())
