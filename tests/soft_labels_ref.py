"""float64 restatement of the soft-labels loss (test infrastructure only), the long way round:
tree distances D[c, k] from leaf_paths by tier comparison, T = w[D] / rowsum, t = q @ T, then
the cross-entropy against t.  It shares nothing with the kernels' nested-range form."""
import numpy as np

N_TIERS = 7


def level_weights64(beta):
    return np.exp(-beta * np.arange(N_TIERS + 1) / N_TIERS)


def one_hot(leaves, n_leaves):
    q = np.zeros((len(leaves), n_leaves))
    q[np.arange(len(leaves)), leaves] = 1.0
    return q


def effective_targets(tax, q, w, chunk=1000):
    """(t = q @ T [B, L], Z [L]) with T[c, k] = w[D[c, k]] / Z[c], Z[c] = sum_k w[D[c, k]]; the
    rows of D in chunks, so the 10 000-leaf tree stays affordable."""
    paths, w, q = tax.leaf_paths, np.asarray(w, np.float64), np.asarray(q, np.float64)
    n = len(paths)
    t, Z = np.zeros((q.shape[0], n)), np.zeros(n)
    for c0 in range(0, n, chunk):
        rows = paths[c0:c0 + chunk]
        D = np.full((len(rows), n), N_TIERS)
        for lvl, tier in enumerate(range(N_TIERS - 1, -1, -1)):
            same = rows[:, None, tier] == paths[None, :, tier]
            D = np.where(same & (D == N_TIERS), lvl, D)
        W = w[D]
        Z[c0:c0 + chunk] = W.sum(1)
        t += q[:, c0:c0 + chunk] @ (W / W.sum(1, keepdims=True))
    return t, Z


def restatement(z, tax, q, w):
    """(loss, dloss/dz): loss = mean_b [LSE(z) sum_k t_k - sum_k t_k z_k]."""
    z = np.asarray(z, np.float64)
    t, _ = effective_targets(tax, q, w)
    m = z.max(1, keepdims=True)
    lse = m + np.log(np.exp(z - m).sum(1, keepdims=True))
    ts = t.sum(1, keepdims=True)
    loss = float(np.mean(lse * ts - (t * z).sum(1, keepdims=True)))
    return loss, (np.exp(z - lse) * ts - t) / z.shape[0]
