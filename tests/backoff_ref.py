"""Back-off decoding restated in float64 numpy straight from `leaf_paths` (no slot tables): node
masses by one boolean mask per node, the greedy path by argmax under the tie rule (the lowest
node_start, i.e. the lowest permuted position below the node, among equal masses)."""
import numpy as np


def softmax(z):  # rows of float64 logits; NaN counts as -inf
    z = np.where(np.isnan(z), -np.inf, z)
    e = np.exp(z - z.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def node_masses(p, leaf_paths):  # [7] arrays [B, n_t]: the mass of every node of tier t
    return [np.stack([p[:, leaf_paths[:, t] == n].sum(1) for n in range(leaf_paths[:, t].max() + 1)], 1)
            for t in range(7)]


def children(leaf_paths, perm, d, parent):  # tier-d ids below tier-(d - 1) node `parent` (d = 0: the root), in tie order
    pos = np.empty(len(perm), np.int64)
    pos[perm] = np.arange(len(perm))
    below = np.ones(len(perm), bool) if d == 0 else leaf_paths[:, d - 1] == parent
    ids = np.unique(leaf_paths[below, d])
    return ids[np.argsort([pos[below & (leaf_paths[:, d] == n)].min() for n in ids], kind="stable")]


def greedy(masses, leaf_paths, perm):  # (path int [B, 7], q float64 [B, 7]) of the greedy walk
    path, q = np.zeros((len(masses[0]), 7), np.int64), np.zeros((len(masses[0]), 7))
    for b in range(len(path)):
        for d in range(7):
            kids = children(leaf_paths, perm, d, path[b, d - 1] if d else None)
            path[b, d] = kids[np.argmax(masses[d][b, kids])]  # the first among equals
            q[b, d] = masses[d][b, path[b, d]]
    return path, q


def depth(q, tau):  # D(tau) = max{d : q_d >= tau} per row (q_0 = 1 always stands)
    return (q >= tau).sum(1)


def agreement(path, target_paths):  # m: the leading depths on which the two paths agree
    return np.cumprod(path == target_paths, 1).sum(1)


def fold(path, prob, match, thresholds):  # the state added: [valid, invalid, 5 sums per threshold]
    ok = match >= 0
    s = [ok.sum(), (~ok).sum()]
    for tau in thresholds:
        D, m = depth(prob[ok], np.float32(tau)), match[ok]
        s += [D.sum(), (D <= m).sum(), np.minimum(D, m).sum(), (D == 7).sum(), ((D == 7) & (m == 7)).sum()]
    return np.asarray(s, np.float64)
