"""Weighted k-nearest-neighbour evaluation (Wu et al., CVPR 2018) of a frozen backbone, the third
protocol beside hvamd.simpleshot (nearest centroid) and hvamd.linear_probe: the bank is the
training set's L2-normalised features, a query is classified by the votes of its k most similar
bank rows, each weighted exp((s - s_best) / temperature).  It fits nothing and averages no class
down to one point.

Everything after the backbone runs in libhvk on the device (ops.knn_topk, ops.knn_vote,
include/hvk.h): the bank is kept in bf16, a bf16-MFMA sweep keeps a running top-k per query row
-- no [B, N] score matrix exists -- and a vote kernel walks the taxonomy.  With [N, 7] tier ids it
answers per tier: the top-down path takes at every tier the node of largest vote among the
neighbours inside the node chosen above it.  Single process; no feature cache.
"""
import torch

from . import ops
from .simpleshot import N_TIERS, _features


class KNeighbors:
    """The bank and its labels on the device.  `k` neighbours (an int, or several: the largest is
    searched, predictions are given for each), `temperature` of the vote weights, `capacity` bank
    rows allocated at once (None: grown by doubling), `centered` as ops.ss_prepare."""

    def __init__(self, k=20, temperature=0.07, capacity=None, centered=False):
        self.ks = sorted({int(v) for v in ([k] if isinstance(k, int) else k)})
        if not self.ks or self.ks[0] < 1 or len(self.ks) > 8:
            raise ValueError(f"k must be 1 to 8 positive values, got {k}")
        self.temperature, self.capacity, self.centered = float(temperature), capacity, bool(centered)
        self.reset()

    def reset(self):
        """Forget every row fitted so far."""
        self._bank = self._labels = None
        self.n_ = 0
        return self

    def _prepare(self, X):
        return ops.ss_prepare(X, centered=self.centered, l2_normalized=True).to(torch.bfloat16)

    def _grow(self, rows, D, y):
        cap = 0 if self._bank is None else self._bank.shape[0]
        if self.n_ + rows <= cap:
            return
        new = max(self.n_ + rows, int(self.capacity or 0), 2 * cap)
        bank = torch.empty(new, D, dtype=torch.bfloat16, device=y.device)
        labels = torch.empty((new,) + tuple(y.shape[1:]), dtype=torch.int32, device=y.device)
        if self.n_:
            bank[:self.n_] = self._bank[:self.n_]
            labels[:self.n_] = self._labels[:self.n_]
        self._bank, self._labels = bank, labels

    @torch.no_grad()
    def partial_fit(self, X, y):
        """Add the features X [B, D] with labels y ([B] classes or [B, 7] tier ids) to the bank."""
        if X.ndim != 2 or y.ndim not in (1, 2) or y.shape[0] != X.shape[0] or (y.ndim == 2 and y.shape[1] != N_TIERS):
            raise ValueError(f"X must be [B, D] and y [B] or [B, {N_TIERS}], got {tuple(X.shape)} and {tuple(y.shape)}")
        if y.dtype.is_floating_point or y.dtype == torch.bool:
            raise ValueError("KNeighbors takes integer labels")
        if self._bank is not None and (X.shape[1] != self._bank.shape[1] or y.ndim != self._labels.ndim):
            raise ValueError(f"X {tuple(X.shape)} / y {tuple(y.shape)} do not fit the bank {tuple(self._bank.shape)}")
        x = self._prepare(X)
        B = x.shape[0]
        self._grow(B, x.shape[1], y)
        self._bank[self.n_:self.n_ + B] = x
        self._labels[self.n_:self.n_ + B] = y.to(torch.int32)
        self.n_ += B
        return self

    def fit(self, X, y):
        return self.reset().partial_fit(X, y)

    def _fitted(self):
        if not self.n_:
            raise RuntimeError("not fitted: the bank is empty (partial_fit first)")

    @torch.no_grad()
    def kneighbors(self, X, k=None):
        """(sims f32 [N, k], idx int32 [N, k]) of the largest configured k (or `k`), ordered by
        (similarity descending, bank row ascending); (-inf, -1) past the bank's rows."""
        self._fitted()
        return ops.knn_topk(self._prepare(X), self._bank, int(k or self.ks[-1]), n=self.n_)

    @torch.no_grad()
    def predict_all(self, X):
        """(leaf int64 [n_k, N], path int64 [n_k, N, T]) for every configured k, ascending."""
        sims, idx = self.kneighbors(X)
        leaf, path = ops.knn_vote(sims, idx, self._labels[:self.n_], self.ks, self.temperature)
        return leaf.long(), path.long()

    def predict(self, X, k=None):
        """int64 [N] classes (labels [B]) or the top-down path [N, 7] (labels [B, 7]) at `k`
        (default: the smallest configured)."""
        k = self.ks[0] if k is None else int(k)
        if k not in self.ks:
            raise ValueError(f"k {k} is not one of the configured {self.ks}")
        leaf, path = self.predict_all(X)
        j = self.ks.index(k)
        return leaf[j] if self._labels.ndim == 1 else path[j]


@torch.no_grad()
def evaluate(config, model, train_batches, eval_batches, *, tree_dists=None, device_transforms=None,
             dtype=torch.bfloat16):
    """Weighted k-NN accuracy of a frozen `model` (a models.FeatureOnlyModel, config.model.variant
    "knn"): the features of `train_batches` form the bank, `eval_batches` are scored (iterables of
    (inputs, targets) batches on the device; targets [B] classes or [B, 7] tier ids).
    `config.knn` gives `k` (a list), `temperature` and `centered`.  `device_transforms`, the
    model's train / eval flags and its input normalisation are handled as simpleshot.evaluate does.
    Sums are float64 on the device and read once at the end.

    Returns, per configured K: "acc@1/k{K}" (the flat vote), "tree-dist/k{K}" with `tree_dists`
    ([L, L]), "acc@1/k{K}/tier0" .. "tier6" (the top-down path) with [B, 7] targets; the smallest
    K also fills "acc@1", "tree-dist" and "acc@1/tier0" .. "tier6".  NaN without eval batches."""
    from .models import FeatureOnlyModel
    if not isinstance(model, FeatureOnlyModel):
        raise ValueError(f"knn.evaluate needs a models.FeatureOnlyModel (config.model.variant 'knn'), got "
                         f"{type(model).__name__}")
    kc = config.knn
    clf = KNeighbors(k=list(kc.k), temperature=kc.temperature, centered=kc.centered)
    n_k = len(clf.ks)
    modes = [m.training for m in model.modules()]
    pe = getattr(model.backbone, "patch_embed", None)
    saved_norm = getattr(pe, "input_norm", None)
    if device_transforms is not None and getattr(device_transforms, "fuse_into", None):
        if device_transforms.fuse_into(model.backbone):
            device_transforms = None
    sums = hier = None
    try:
        model.eval()
        for batch in train_batches:
            clf.partial_fit(*_features(model, batch, device_transforms, dtype))
        if not clf.n_:
            raise ValueError("knn.evaluate got no train batches")
        if clf.ks[-1] > 256:
            raise ValueError(f"config.knn.k {clf.ks}: at most 256 neighbours")
        for batch in eval_batches:
            x, y = _features(model, batch, device_transforms, dtype)
            if sums is None:
                hier = y.ndim == 2
                sums = torch.zeros(1 + n_k * (2 + N_TIERS), dtype=torch.float64, device=x.device)
                if tree_dists is not None:
                    tree_dists = tree_dists.to(x.device)
            leaf, path = clf.predict_all(x)
            want = (y if y.ndim == 1 else y[:, -1]).long()
            per_k = sums[1:].view(n_k, 2 + N_TIERS)
            sums[0] += want.shape[0]
            per_k[:, 0] += (leaf == want).sum(1)
            if tree_dists is not None:
                per_k[:, 1] += tree_dists[leaf, want.expand_as(leaf)].sum(1, dtype=torch.float64)
            if hier and path.shape[2] == N_TIERS:
                per_k[:, 2:] += (path == y).sum(1)
    finally:
        if pe is not None and hasattr(pe, "input_norm"):
            pe.input_norm = saved_norm
        for m, t in zip(model.modules(), modes):
            m.training = t
    if sums is None:
        s = [float("nan")] * (1 + n_k * (2 + N_TIERS))
        hier = clf._labels.ndim == 2
    else:
        s = sums.tolist()  # the one host read
    n = s[0]
    div = (lambda v: v / n) if n == n and n else (lambda v: float("nan"))
    out = {}
    for j, K in enumerate(clf.ks):
        row = s[1 + j * (2 + N_TIERS):1 + (j + 1) * (2 + N_TIERS)]
        for suffix in ([f"/k{K}", ""] if j == 0 else [f"/k{K}"]):
            out["acc@1" + suffix] = div(row[0])
            if tree_dists is not None:
                out["tree-dist" + suffix] = div(row[1])
            if hier:
                for t in range(N_TIERS):
                    out[f"acc@1{suffix}/tier{t}"] = div(row[2 + t])
    return out
