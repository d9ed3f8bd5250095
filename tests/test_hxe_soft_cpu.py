"""Soft-target HXE, host side: the float64 restatement the GPU tests use against the oracle
expectation, the rank-ordered Taxonomy tables of the kernels, LabelSmoothing on [B, 7] labels,
and the new entry points' argument checks."""
import ctypes

import numpy as np
import pytest
import torch

import hxe_soft_ref as R


def _trees():
    from hvamd.hierarchy import Taxonomy
    return {"small": Taxonomy.synthetic((2, 3, 4, 5, 6, 7, 12)), "shuffled40": R.shuffled_tree(40)}


def _targets(rng, L, B=3):
    """dense smoothed, two-hot 0.7 / 0.3 and all-zero rows (cycled)."""
    t = np.zeros((B, L), np.float32)
    for b in range(B):
        if b % 3 == 0:
            t[b] = 0.1 / L
            t[b, rng.integers(L)] += 0.9
        elif b % 3 == 1:
            i, j = rng.choice(L, 2, replace=False)
            t[b, i], t[b, j] = 0.7, 0.3
    return t


@pytest.mark.parametrize("weights", ["uniform", "exponential"])
@pytest.mark.parametrize("tree", ["small", "shuffled40"])
def test_restatement_equals_oracle_expectation(tree, weights):
    tax = _trees()[tree]
    rng = np.random.default_rng(3)
    z = (3 * rng.standard_normal((3, tax.num_leaves))).astype(np.float32)
    t = _targets(rng, tax.num_leaves)
    loss, grad = R.restatement(z, tax, t, weights)
    ref = R.expectation(z, tax, t, weights)
    assert abs(loss - ref) < 1e-10 * max(1.0, abs(ref)), (loss, ref)
    gref = R.expectation_grad(z, tax, t, weights)
    assert np.linalg.norm(grad - gref) < 1e-10 * np.linalg.norm(gref)
    assert not grad[2].any()  # the all-zero row


@pytest.mark.parametrize("tree", ["small", "shuffled40", "inat"])
def test_soft_tables_partition_and_ancestors(tree):
    from hvamd.hierarchy import Taxonomy
    tax = Taxonomy.synthetic() if tree == "inat" else _trees()[tree]
    rank_off, lo, hi, anc, slot_node = tax.soft_tables()
    assert tax.soft_tables()[0] is rank_off  # built once
    L, n_nodes = tax.num_leaves, sum(tax.num_classes[:6])
    assert rank_off.tolist() == [0, *np.cumsum(tax.num_classes[:6]), n_nodes + 1]
    assert lo.shape == hi.shape == (n_nodes + 1,) and anc.shape == (L, 6)
    assert all(a.dtype == np.int32 for a in (rank_off, lo, hi, anc, slot_node))
    ordered = tax.leaf_paths[tax.perm]
    for t in range(6):
        s0, s1 = rank_off[t], rank_off[t + 1]
        # every node of the tier holds exactly one slot
        assert sorted(slot_node[s0:s1]) == list(range(tax.num_classes[t]))
        # the child ranges are non-empty and partition the finer tier (the leaves for tier 5)
        first, last = (0, L) if t == 5 else (rank_off[t + 1], rank_off[t + 2])
        assert (lo[s0:s1] < hi[s0:s1]).all()
        assert lo[s0] == first and hi[s1 - 1] == last
        assert np.array_equal(hi[s0:s1 - 1], lo[s0 + 1:s1])
        # ... and each child is a child: its parent in leaf_paths is the slot's node
        parent_slot = np.repeat(np.arange(s0, s1), hi[s0:s1] - lo[s0:s1])
        if t == 5:
            child_parent = ordered[:, 5]
        else:
            par = np.zeros(tax.num_classes[t + 1], np.int64)
            par[tax.leaf_paths[:, t + 1]] = tax.leaf_paths[:, t]
            child_parent = par[slot_node[first:last]]
        assert np.array_equal(slot_node[parent_slot], child_parent)
        # ancestor slots agree with leaf_paths[perm]
        assert (anc[:, t] >= s0).all() and (anc[:, t] < s1).all()
        assert np.array_equal(slot_node[anc[:, t]], ordered[:, t])
    assert (lo[n_nodes], hi[n_nodes]) == (rank_off[0], rank_off[1])  # the root's children: tier 0
    assert len(tax.device_tables("cpu")) == 5  # the hard path's tables keep their form


@pytest.mark.parametrize("tree", ["shuffled40", "chain"])
def test_bottom_up_pass_over_the_tables_equals_restatement(tree):
    """The kernels' algorithm in float64 numpy, driven only by soft_tables(): tier 5 reduces its
    leaf range, each coarser slot merges its children's (LSE, T), the backward gathers through
    anc -- the loss and gradient of the restatement."""
    from hvamd.hierarchy import Taxonomy
    tax = Taxonomy.synthetic((1, 1, 1, 1, 1, 2, 30)) if tree == "chain" else _trees()[tree]
    rank_off, lo, hi, anc, _ = tax.soft_tables()
    n_nodes, L = rank_off[6], tax.num_leaves
    rng = np.random.default_rng(5)
    z = 3 * rng.standard_normal(L)
    t = rng.random(L)
    c = R.level_coeffs64("exponential")
    zp, tp = z[tax.perm], t[tax.perm]
    lse, T = np.zeros(n_nodes + 1), np.zeros(n_nodes + 1)
    loss = c[0] * (t @ z)
    for q in (5, 4, 3, 2, 1, 0, 6):
        for i in range(rank_off[q], rank_off[q + 1]):
            vals, w = (zp, tp) if q == 5 else (lse, T)
            lse[i] = np.logaddexp.reduce(vals[lo[i]:hi[i]])
            T[i] = w[lo[i]:hi[i]].sum()
            loss += c[6 - q if q < 6 else 7] * T[i] * lse[i]
    grad = c[0] * tp
    for q in range(7):
        i = anc[:, q] if q < 6 else np.full(L, n_nodes)
        grad = grad + c[6 - q if q < 6 else 7] * T[i] * np.exp(zp - lse[i])
    ref, gref = R.restatement(z[None], tax, t[None], "exponential")
    assert abs(loss - ref) < 1e-10 * max(1.0, abs(ref))
    assert np.allclose(grad, gref[0][tax.perm], rtol=1e-10, atol=1e-13)


def test_label_smoothing_on_taxonomy_labels_with_tensor_outputs():
    """One [B, L] logit tensor with [B, 7] tier-id labels (the HXE variant): the leaf column is
    smoothed into a [B, L] probability target; AFTER_LOSS restores the labels."""
    from hvamd.algorithmic import Event, LabelSmoothing, State
    from hvamd.hierarchy import Taxonomy
    tax = Taxonomy.synthetic((2, 3, 4, 5, 6, 7, 12))
    L, s = tax.num_leaves, 0.08
    leaves = [3, 7, 11, 0]
    labels = torch.tensor(tax.leaf_paths[leaves])
    state = State(model=None)
    state.batch = (torch.zeros(4, 3), labels)
    state.outputs = torch.randn(4, L)
    alg = LabelSmoothing(s)
    alg.apply(Event.BEFORE_LOSS, state)
    soft = state.batch[1]
    assert soft.shape == (4, L) and soft.dtype == torch.float32
    want = torch.full((4, L), s / L)
    want[torch.arange(4), torch.tensor(leaves)] = 1 - s + s / L
    assert torch.allclose(soft, want, rtol=1e-6, atol=0)
    alg.apply(Event.AFTER_LOSS, state)
    assert state.batch[1].dtype == torch.int64 and torch.equal(state.batch[1], labels)
    # [B] labels keep today's behaviour
    state.batch = (torch.zeros(4, 3), labels[:, -1].clone())
    alg.apply(Event.BEFORE_LOSS, state)
    assert torch.allclose(state.batch[1], want, rtol=1e-6, atol=0)


def test_hxe_still_refuses_list_targets():
    from hvamd.hierarchy import HierarchicalCrossEntropy, Taxonomy
    tax = Taxonomy.synthetic((2, 3, 4, 5, 6, 7, 12))
    fn = HierarchicalCrossEntropy(tax)
    with pytest.raises(NotImplementedError):
        fn(torch.zeros(2, 12), [torch.zeros(2, 12)])
    with pytest.raises(ValueError):
        fn(torch.zeros(2, 12), torch.zeros(2, 7))  # a float target must cover the leaves


def test_soft_entry_points_validate_arguments_without_gpu():
    from hvamd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(16)
    assert lib.hvk_hxe_soft_fwd(None, p, 2, 12, None, 27, p, p, p, p, p, p, p, None) == 1
    assert b"null" in lib.hvk_last_error_string()
    assert lib.hvk_hxe_soft_fwd(p, p, 0, 12, None, 27, p, p, p, p, p, p, p, None) == 1
    assert lib.hvk_hxe_soft_fwd(p, p, 2, 0, None, 27, p, p, p, p, p, p, p, None) == 1
    assert lib.hvk_hxe_soft_bwd(p, p, 2, 12, None, 27, None, p, p, p, p, p, None) == 1
    assert lib.hvk_hxe_soft_bwd(p, p, 2, -1, None, 27, p, p, p, p, p, p, None) == 1
    assert lib.hvk_hxe_soft_bwd(p, p, 0, 12, None, 27, p, p, p, p, p, p, None) == 1
