"""HXE with soft targets (hvk_hxe_soft_fwd / bwd) against the oracle expectation
sum_c t_c hxe_loss(.., [c]) and, on the big tree, its float64 restatement
(tests/hxe_soft_ref.py, tied to the oracle by tests/test_hxe_soft_cpu.py); LabelSmoothing on
the HXE variant through the Trainer, eager and captured.  Tolerances are the hard kernel's
(test_gpu_model.py::test_hxe_vs_oracle): loss 1e-4 max(1, |ref|), gradient 1e-4 relative."""
import copy

import numpy as np
import pytest
import torch

import hxe_soft_ref as R

pytestmark = pytest.mark.gpu


def rel(a, b):
    a = torch.as_tensor(np.asarray(a, dtype=np.float64))
    b = torch.as_tensor(np.asarray(b, dtype=np.float64))
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _run(tax, z, t, weights, scale=1.0):
    """(loss, dlogits) of the product loss on the GPU for numpy logits / soft targets."""
    from hvamd.hierarchy import HierarchicalCrossEntropy
    fn = HierarchicalCrossEntropy(tax, tree_weights=weights).cuda()
    zt = torch.from_numpy(np.asarray(z, np.float32)).cuda().requires_grad_(True)
    loss = fn(zt, torch.from_numpy(np.asarray(t, np.float32)).cuda())
    (loss * scale).backward()
    return loss.item(), zt.grad.cpu().numpy()


def _check(got, ref):
    (loss, grad), (rloss, rgrad) = got, ref
    print(f"loss {loss:.7f} ref {rloss:.7f} grad rel {rel(grad, rgrad):.2e}")
    assert np.isfinite(loss) and np.isfinite(grad).all()
    assert abs(loss - rloss) < 1e-4 * max(1.0, abs(rloss)), (loss, rloss)
    assert rel(grad, rgrad) < 1e-4


def _mixed_targets(rng, L):
    """B = 3: a dense smoothed row, a two-hot 0.7 / 0.3 row and an all-zero row."""
    t = np.zeros((3, L), np.float32)
    t[0] = 0.1 / L
    t[0, rng.integers(L)] += 0.9
    i, j = rng.choice(L, 2, replace=False)
    t[1, i], t[1, j] = 0.7, 0.3
    return t


@pytest.fixture(scope="module")
def big():
    """The 10 000-leaf tree, logits at B = 2 and LabelSmoothing(0.08)'s dense targets."""
    from hvamd.algorithmic import Event, LabelSmoothing, State
    from hvamd.hierarchy import Taxonomy
    tax = Taxonomy.synthetic()
    rng = np.random.default_rng(11)
    z = (3 * rng.standard_normal((2, tax.num_leaves))).astype(np.float32)
    leaves = np.array([123, 9876])
    state = State(model=None)
    state.batch = (None, torch.from_numpy(tax.leaf_paths[leaves]))
    state.outputs = torch.from_numpy(z)
    LabelSmoothing(0.08).apply(Event.BEFORE_LOSS, state)
    t = state.batch[1].numpy()
    assert t.shape == z.shape and (t > 0).all()
    return tax, z, t, leaves


@pytest.mark.parametrize("weights", ["uniform", "exponential"])
@pytest.mark.parametrize("tree", ["small", "shuffled40"])
def test_soft_hxe_vs_oracle_expectation(tree, weights):
    from hvamd.hierarchy import Taxonomy
    tax = Taxonomy.synthetic((2, 3, 4, 5, 6, 7, 12)) if tree == "small" else R.shuffled_tree(40)
    rng = np.random.default_rng(7)
    z = (3 * rng.standard_normal((3, tax.num_leaves))).astype(np.float32)
    t = _mixed_targets(rng, tax.num_leaves)
    ref = R.expectation(z, tax, t, weights), R.expectation_grad(z, tax, t, weights)
    loss, grad = _run(tax, z, t, weights)
    _check((loss, grad), ref)
    assert not grad[2].any()  # the all-zero row: zero gradient
    _, grad3 = _run(tax, z, t, weights, scale=3.0)  # grad_out reaches the kernel
    assert rel(grad3, 3 * ref[1]) < 1e-4


@pytest.mark.parametrize("sizes", [(1, 1, 1, 1, 1, 1, 600), (1, 1, 1, 1, 1, 2, 300),
                                   (1, 1, 1, 1, 1, 2, 33), (1, 1, 1, 1, 2, 40, 80)])
def test_soft_hxe_wide_and_chain_nodes(sizes):
    """One genus wider than a workgroup under single-child chains: the wave-per-node path, its
    loop over the range, and parents with one child.  (.., 2, 33): genera of 17 and 16 leaves,
    either side of the lane-per-node / wave-per-node threshold; (.., 2, 40, 80): families of 20
    genera, the wave-per-node path over child nodes instead of leaves."""
    from hvamd.hierarchy import Taxonomy
    tax = Taxonomy.synthetic(sizes)
    rng = np.random.default_rng(8)
    z = (3 * rng.standard_normal((2, tax.num_leaves))).astype(np.float32)
    t = rng.random((2, tax.num_leaves)).astype(np.float32)
    t /= t.sum(axis=1, keepdims=True)
    ref = R.expectation(z, tax, t, "exponential"), R.expectation_grad(z, tax, t, "exponential")
    _check(_run(tax, z, t, "exponential"), ref)


def test_soft_hxe_node_far_below_the_row_max():
    """A tier-3 node whose logits all sit 200 below the rest: exp(z - rowmax) is 0 in f32, so
    the node must keep its own max for a finite LSE."""
    tax = R.shuffled_tree(40)
    rng = np.random.default_rng(9)
    z = rng.standard_normal((3, tax.num_leaves)).astype(np.float32)
    node = tax.leaf_paths[17, 3]
    members = tax.leaf_paths[:, 3] == node
    assert 0 < members.sum() < tax.num_leaves
    z[:, members] -= 200.0
    t = np.full((3, tax.num_leaves), 0.1 / tax.num_leaves, np.float32)
    t[0, 17] += 0.9                                   # the target inside the low node
    t[1, np.flatnonzero(~members)[0]] += 0.9          # ... and outside it
    t[2, np.flatnonzero(members)[-1]] += 0.9
    for weights in ("uniform", "exponential"):
        _check(_run(tax, z, t, weights), R.restatement(z, tax, t, weights))


def test_soft_hxe_big_tree_label_smoothing_targets(big):
    tax, z, t, _ = big
    _check(_run(tax, z, t, "exponential"), R.restatement(z, tax, t, "exponential"))


def test_soft_hxe_one_hot_equals_hard_kernel(big):
    from hvamd.hierarchy import HierarchicalCrossEntropy
    tax, z, _, leaves = big
    t = np.zeros_like(z)
    t[np.arange(2), leaves] = 1.0
    fn = HierarchicalCrossEntropy(tax, tree_weights="exponential").cuda()
    zh = torch.from_numpy(z).cuda().requires_grad_(True)
    hard = fn(zh, torch.from_numpy(leaves).cuda())
    hard.backward()
    _check(_run(tax, z, t, "exponential"), (hard.item(), zh.grad.cpu().numpy()))


def test_soft_hxe_is_deterministic(big):
    import hvamd.ops as ops
    from hvamd.hierarchy import hxe_level_coeffs
    tax, z, t, _ = big
    dev = torch.device("cuda:0")
    tables = tax.device_soft_tables(dev)
    coeff = hxe_level_coeffs("exponential").to(dev)
    tt = torch.from_numpy(t).to(dev)
    runs = []
    for _ in range(2):
        zt = torch.from_numpy(z).to(dev).requires_grad_(True)
        loss, node_lse, node_t = ops.hierarchical_cross_entropy_soft(zt, tt, *tables, coeff,
                                                                     return_nodes=True)
        loss.backward()
        runs.append((loss.detach(), node_lse, node_t, zt.grad))
    n_nodes = sum(tax.num_classes[:6])
    assert runs[0][1].shape == runs[0][2].shape == (2, n_nodes + 1)
    assert torch.isfinite(runs[0][1]).all()
    # the root's T is the row sum of the targets, every tier's T adds up to it
    assert torch.allclose(runs[0][2][:, -1].cpu(), torch.from_numpy(t).sum(1), rtol=1e-5)
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ------------------------------------------------------------------ wiring
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


def _trainer(model, smoothing):
    from hvamd import optim
    from hvamd.algorithmic import GradientClipping, LabelSmoothing
    from hvamd.trainer import Trainer
    opt = optim.DecoupledSGDW(optim.set_weight_decay(model), lr=0.05, momentum=0.9,
                              weight_decay=5e-4)
    algs = [GradientClipping("norm", 2.0)]
    if smoothing is not None:
        algs.insert(0, LabelSmoothing(smoothing))
    return Trainer(model, opt, algs)


def test_trainer_label_smoothing_on_hxe_loss_and_labels():
    from hvamd.algorithmic import smooth_labels
    model, (x, y) = _setup()
    ref_model = copy.deepcopy(model).train()
    with torch.no_grad():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = ref_model((x, y))
        soft = smooth_labels(out, y[:, -1], 0.08)
        assert soft.shape == out.shape
        ref = ref_model.loss(out, (x, soft)).item()
        hard = ref_model.loss(out, (x, y)).item()
    tr = _trainer(model, 0.08)
    loss = tr.train_step((x, y)).item()
    print(f"smoothed step loss {loss:.6f} ref {ref:.6f} (hard {hard:.6f})")
    assert abs(loss - ref) < 1e-4 * abs(ref), (loss, ref)
    assert abs(hard - ref) > 1e-3 * abs(ref)  # the smoothing is in the loss
    labels = tr.state.batch[1]
    assert not labels.dtype.is_floating_point and torch.equal(labels, y)


def test_trainer_zero_smoothing_matches_plain_trainer():
    model, batch = _setup()
    model_b = copy.deepcopy(model)
    la = _trainer(model, 0.0).train_step(batch)
    lb = _trainer(model_b, None).train_step(batch)
    torch.cuda.synchronize()
    assert abs(la.item() - lb.item()) < 1e-4 * abs(lb.item())
    for (na, pa), (_, pb) in zip(model.named_parameters(), model_b.named_parameters()):
        r = ((pa - pb).norm() / pb.norm().clamp_min(1e-12)).item()
        assert r < 1e-2, (na, r)


def test_trainer_label_smoothing_graph_replay_tracks_eager():
    model, batch = _setup()
    model_b = copy.deepcopy(model)
    ta, tb = _trainer(model, 0.08), _trainer(model_b, 0.08)
    la = [ta.train_step(batch) for _ in range(6)]
    tb.capture(batch, warmup=3)  # 3 eager steps inside, then capture
    lb = [tb.replay().clone() for _ in range(3)]
    torch.cuda.synchronize()
    for a, b in zip(la[3:], lb):
        assert abs(a.item() - b.item()) < 1e-3 * max(1.0, abs(a.item())), (a.item(), b.item())
