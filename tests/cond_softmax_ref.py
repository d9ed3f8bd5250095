"""The conditional softmax restated in float64 torch on the CPU, for the tests of
hvk_cond_softmax_*: sibling groups by brute force from leaf_paths, the gradient by autograd."""
import numpy as np
import torch


def parent_ids(paths):
    """Per tier, the parent (a tier t - 1 id; 0 = the root for tier 0) of every node, from the
    leaves below it."""
    out = [np.zeros(paths[:, 0].max() + 1, np.int64)]
    for t in range(1, 7):
        p = np.full(paths[:, t].max() + 1, -1, np.int64)
        p[paths[:, t]] = paths[:, t - 1]
        out.append(p)
    return out


def group_lse(z, par):
    """z [B, n] float64, par [n]: (LSE over every node's siblings [B, n], |group| per node [n])."""
    par = torch.as_tensor(par)
    ng = int(par.max()) + 1
    m = z.detach().max(1, keepdim=True).values
    s = torch.zeros(z.shape[0], ng, dtype=z.dtype).index_add(1, par, torch.exp(z - m))
    return (torch.log(s) + m)[:, par], torch.bincount(par, minlength=ng)[par]


def log_cond(zs, paths):
    """log p(n | parent) per tier, [B, n_t] each."""
    return [z - group_lse(z, par)[0] for z, par in zip(zs, parent_ids(paths))]


def leaf_logp(zs, paths):
    """log p(leaf k) [B, L]: the conditionals summed along every leaf's path."""
    return sum(lc[:, paths[:, t]] for t, lc in enumerate(log_cond(zs, paths)))


def loss(zs, paths, targets, coeffs, eps):
    """(mean loss, group LSEs [B, 7], per-tier terms [B, 7]) for tier-id targets [B, 7]."""
    rows = torch.arange(zs[0].shape[0])
    lses, terms = [], []
    for t, (z, par) in enumerate(zip(zs, parent_ids(paths))):
        y = torch.as_tensor(targets[:, t])
        lse, size = group_lse(z, par)
        par = torch.as_tensor(par)
        lc = z - lse
        mean = torch.zeros(z.shape[0], int(par.max()) + 1, dtype=z.dtype).index_add(1, par, lc)[:, par] / size
        lses.append(lse[rows, y])
        terms.append(-(1 - eps) * lc[rows, y] - eps * mean[rows, y])
    terms = torch.stack(terms, 1)
    return (terms * torch.tensor(coeffs, dtype=terms.dtype)).sum(1).mean(), torch.stack(lses, 1), terms


def loss_and_grad(zs, paths, targets, coeffs, eps):
    """As loss(), with d loss / d z_t per tier (float64 autograd)."""
    zs = [z.clone().requires_grad_() for z in zs]
    total, lses, terms = loss(zs, paths, targets, coeffs, eps)
    total.backward()
    return total.detach(), lses.detach(), terms.detach(), [z.grad for z in zs]
