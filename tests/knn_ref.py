"""numpy float64 restatement of the weighted k-NN evaluation (hvamd.knn, include/hvk.h), written from
the description; its inputs are the bf16-rounded features the kernels read, so its dot products are exact."""
import numpy as np


def bf16_round(x):
    """float32 values rounded to the nearest bfloat16 (ties to even), as float32."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32)


def unit_rows_bf16(x):
    """Rows of x L2-normalised in float64, then rounded to bf16 (returned as float32)."""
    x = np.asarray(x, np.float64)
    return bf16_round((x / np.sqrt((x * x).sum(1, keepdims=True))).astype(np.float32))


def topk(S, k):
    """(sims, idx) [B, k] of the scores S [B, N] by (score descending, index ascending); (-inf, -1) past N."""
    B, N = S.shape
    sims, idx = np.full((B, k), -np.inf), np.full((B, k), -1, np.int64)
    for r in range(B):
        order = np.lexsort((np.arange(N), -S[r]))[:k]
        sims[r, :len(order)], idx[r, :len(order)] = S[r, order], order
    return sims, idx


def weights(sims, idx, temperature):
    """exp((s_i - s_0) / temperature) of one row; 0 for pads."""
    with np.errstate(invalid="ignore"):
        w = np.exp((np.asarray(sims, np.float64) - float(sims[0])) / temperature)
    return np.where(np.asarray(idx) >= 0, w, 0.0)


def votes(w, ids, mask=None):
    """{id: summed weight} over the neighbours (inside `mask`) that carry a non-negative id."""
    mask = (ids >= 0) if mask is None else (mask & (ids >= 0))
    return {int(c): float(w[mask & (ids == c)].sum()) for c in np.unique(ids[mask])}


def _argmax(v):
    return min(v, key=lambda c: (-v[c], c)) if v else 0  # the lower id among equal votes


def predict(sims, idx, labels, kj, temperature):
    """(leaf, path [T]) of one row from its sorted neighbours: the leaf of largest vote among the
    first kj, and the top-down walk (tier t + 1 among the neighbours whose tier-t id was chosen)."""
    labels = np.asarray(labels).reshape(len(labels), -1)
    w = weights(sims, idx, temperature)[:kj]
    valid = np.asarray(idx[:kj]) >= 0
    lab = np.where(valid[:, None], labels[np.where(valid, idx[:kj], 0)], -1)
    path, mask = [], np.ones(kj, bool)
    for t in range(lab.shape[1]):
        path.append(_argmax(votes(w, lab[:, t], mask)))
        mask = lab[:, t] == path[-1]
    return _argmax(votes(w, lab[:, -1])), np.array(path, np.int64)
