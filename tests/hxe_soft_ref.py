"""References for the soft-target HXE tests (test infrastructure only).

The soft loss is the expectation of the hard one, L_b = sum_c t_c L(c).  `expectation` /
`expectation_torch` state exactly that through the oracle (oracle/hierarchy_ref.py);
`restatement` is the collapsed per-node form in float64 numpy, affordable on the 10 000-leaf
tree, which a CPU test ties to the expectation."""
import numpy as np
import torch

from oracle import hierarchy_ref

N_TIERS = 7


def shuffled_tree(n_leaves=40, seed=1):
    """The (2,3,4,5,6,7,n) synthetic tree with class numbers NOT in taxonomic order
    (perm != identity), as tests/test_gpu_model.py builds it."""
    from hvamd.hierarchy import Taxonomy
    names = hierarchy_ref.synthetic_inat_names((2, 3, 4, 5, 6, 7, n_leaves))
    ids = np.random.default_rng(seed).permutation(len(names))
    tax = Taxonomy([f"{ids[i]:05d}" + n[5:] for i, n in enumerate(names)])
    assert not tax.identity_perm
    return tax


def level_coeffs64(weights, alpha=0.1):
    """hxe_level_coeffs in float64: c_0 .. c_7 of L = sum_l c_l LSE_l."""
    lam = hierarchy_ref.hxe_level_weights(weights, alpha)
    return np.array([-lam[0]] + [lam[l - 1] - lam[l] for l in range(1, N_TIERS)] + [lam[-1]])


def expectation(z, tax, t, weights):
    """mean_b sum_c t[b, c] * oracle hxe_loss(z[b], target leaf c)."""
    lam = hierarchy_ref.hxe_level_weights(weights, 0.1)
    total = 0.0
    for b in range(z.shape[0]):
        for c in np.flatnonzero(t[b]):
            total += float(t[b, c]) * hierarchy_ref.hxe_loss(z[b:b + 1], tax.leaf_paths, np.array([c]), lam)
    return total / z.shape[0]


def expectation_grad(z, tax, t, weights):
    """d/dz of the same weighted sum of hxe_loss_torch, by float64 autograd."""
    lam = hierarchy_ref.hxe_level_weights(weights, 0.1)
    zc = torch.from_numpy(np.asarray(z)).double().requires_grad_(True)
    total = zc.new_zeros(())
    for b in range(z.shape[0]):
        for c in np.flatnonzero(t[b]):
            total = total + float(t[b, c]) * hierarchy_ref.hxe_loss_torch(
                zc[b:b + 1], tax.leaf_paths[[c]], tax.perm, tax.node_start, tax.node_end,
                tax.tier_base, lam)
    if total.requires_grad:
        (total / z.shape[0]).backward()
    return zc.grad.numpy() if zc.grad is not None else np.zeros(z.shape)


def restatement(z, tax, t, weights):
    """(loss, dloss/dz) of the collapsed form in float64:
    L_b = c_0 sum_k t_k z_k + sum_{tiers} c_l sum_n T(n) LSE(n) + c_7 (sum_k t_k) LSE_all,
    every node with its own max (straight from leaf_paths, no product table involved)."""
    z = np.asarray(z, np.float64)
    t = np.asarray(t, np.float64)
    c = level_coeffs64(weights)
    B, L = z.shape
    loss = 0.0
    grad = np.zeros_like(z)
    for b in range(B):
        loss += c[0] * float(t[b] @ z[b])
        grad[b] += c[0] * t[b]
        for l in range(1, N_TIERS + 1):
            ids = tax.leaf_paths[:, N_TIERS - 1 - l] if l < N_TIERS else np.zeros(L, np.int64)
            n = int(ids.max()) + 1
            m = np.full(n, -np.inf)
            np.maximum.at(m, ids, z[b])
            s = np.zeros(n)
            np.add.at(s, ids, np.exp(z[b] - m[ids]))
            lse = m + np.log(s)
            T = np.bincount(ids, weights=t[b], minlength=n)
            loss += c[l] * float(np.sum(np.where(T != 0, T * lse, 0.0)))
            grad[b] += c[l] * T[ids] * np.exp(z[b] - lse[ids])
    return loss / B, grad / B
