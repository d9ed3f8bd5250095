"""numpy float64 restatement of hvk_eval_metrics (include/hvk.h), the reference of
tests/test_gpu_eval_metrics.py.  It runs on the logits as the kernel sees them: a bf16 case
rounds to bf16 first and passes those values in."""
import numpy as np

N_TIERS = 7


def path_dist(pred_path, target_path):
    """Smallest lvl in 0..6 with equal tier ids at tier 6 - lvl, else 7 (HierarchicalLabel.dist
    on tier ids)."""
    for lvl, t in enumerate(range(N_TIERS - 1, -1, -1)):
        if pred_path[t] == target_path[t]:
            return lvl
    return N_TIERS


def rows(z, t, tree_dists=None, leaf_paths=None, target_paths=None):
    """Per-row results for logits z [B, L] (any float dtype, taken to float64) and classes t [B]:
    dict of pred, rank, nll (float64; NaN where the target is out of range), dist, tier_hit,
    valid."""
    z = np.asarray(z, np.float64)
    t = np.asarray(t, np.int64)
    B, L = z.shape
    pred = np.zeros(B, np.int64)
    rank = np.full(B, -1, np.int64)
    nll = np.full(B, np.nan)
    dist = np.full(B, -1, np.int64)
    hit = np.zeros(B, np.int64)
    valid = (t >= 0) & (t < L)
    for b in range(B):
        # first index of the maximum; float compares, so -0.0 and +0.0 tie (np.argmax does that)
        pred[b] = int(np.argmax(z[b]))
        if not valid[b]:
            continue
        order = np.argsort(-z[b], kind="stable")  # -(-0.0) = 0.0 == -(0.0): ties keep index order
        rank[b] = int(np.flatnonzero(order == t[b])[0])
        m = z[b].max()
        with np.errstate(divide="ignore", invalid="ignore"):
            nll[b] = m + np.log(np.exp(z[b] - m).sum()) - z[b, t[b]]
        if tree_dists is not None:
            dist[b] = int(tree_dists[pred[b], t[b]])
        elif leaf_paths is not None:
            dist[b] = path_dist(leaf_paths[pred[b]], target_paths[b])
            hit[b] = sum(1 << q for q in range(N_TIERS) if leaf_paths[pred[b], q] == target_paths[b, q])
    return dict(pred=pred, rank=rank, nll=nll, dist=dist, tier_hit=hit, valid=valid)


def state(r, topk, L):
    """The 16 sums hvk_eval_metrics adds for a batch with per-row results r (float64)."""
    s = np.zeros(16)
    v = r["valid"]
    s[0] = v.sum()
    s[1] = (r["rank"][v] < 1).sum()
    s[2] = (r["rank"][v] < min(topk, L)).sum()
    s[3] = r["nll"][v].sum()
    s[4] = np.maximum(r["dist"][v], 0).sum()
    s[5] = (~v).sum()
    for q in range(N_TIERS):
        s[6 + q] = ((r["tier_hit"][v] >> q) & 1).sum()
    return s
