"""SimpleShot evaluation -- drop-in for simpleshot.py and hierarchy.HierarchicalNearestCentroid
(hierarchy.py:488-597): pooled features of a frozen backbone, optionally "centered" and
L2-normalised, classified by the nearest class centroid, flat or top-down through the taxonomy.

Everything after the backbone runs in libhvk on the device (ops.ss_*, include/hvk.h): the fit
keeps float64 sums per class that batches are added to as they are produced (no feature ever
goes to the host), the flat prediction is one f32-MFMA GEMM with a running row argmin, the
hierarchical one walks each sample down the tree and compares it with the children of the node
it is in -- about 40 centroids on iNat21 -- where the reference sorts six full distance matrices.

`center` keeps the reference's arithmetic, a division of each row by its own mean
(simpleshot.py:148-154); the SimpleShot paper subtracts the training set's mean vector instead
(Open).  Single process; feature caching, sharded extraction and W&B logging are not
provided.
"""
import numpy as np
import torch

from . import ops

N_TIERS = 7


def l2_normalize(features):
    """features / ||features||_2 per row (simpleshot.py:139-145) as f32 on the device; any
    feature width (SwinV2-T pools 768, which the reference's assert refuses)."""
    return ops.ss_prepare(features, l2_normalized=True)


def center(features):
    """features / mean(features) per row (simpleshot.py:148-154) as f32 on the device."""
    return ops.ss_prepare(features, centered=True)


def children_csr(lookup_vecs):
    """The tree of child -> parent vectors (hierarchy.build_parent_label_lookup) as the CSR
    children lists of include/hvk.h: (tier_sizes, tier_base [T + 1], child_ptr [internal + 1],
    child_idx [nodes below tier 0]) as Python ints / numpy int32.  Node i of tier t owns
    child_idx[child_ptr[tier_base[t] + i] : child_ptr[tier_base[t] + i + 1]], the ids of its
    tier-(t + 1) children in ascending order (they need not be contiguous)."""
    vecs = [np.asarray(v).astype(np.int64).reshape(-1) for v in lookup_vecs]
    if not vecs:
        raise ValueError("children_csr needs at least one child -> parent vector")
    sizes = [int(vecs[0].max()) + 1 if vecs[0].size else 0] + [int(v.size) for v in vecs]
    if min(sizes) < 1:
        raise ValueError(f"every tier needs a node, got sizes {sizes}")
    ptr, idx = [np.zeros(1, np.int64)], []
    for t, v in enumerate(vecs):
        if v.min() < 0 or v.max() >= sizes[t]:
            raise ValueError(f"lookup vector {t} names a parent outside [0, {sizes[t]})")
        idx.append(np.argsort(v, kind="stable"))  # children grouped by parent, ascending id inside
        ptr.append(ptr[-1][-1] + np.cumsum(np.bincount(v, minlength=sizes[t])))
    # positions in child_idx are global; the ids stored are tier-local
    tier_base = np.r_[0, np.cumsum(sizes)].astype(np.int32)
    return (tuple(sizes), tier_base, np.concatenate(ptr).astype(np.int32),
            np.concatenate(idx).astype(np.int32))


class _Centroids:
    """Running float64 class sums on the device and what finalize() makes of them."""

    def __init__(self):
        self.tier_sizes = None  # set by the subclass (flat: on the first fit)
        self._reset()

    def _reset(self):
        self._sums = self._counts = self._state = None
        self._cent = self._cnorm = None
        self._csr_dev = None

    # the tree as the kernels take it
    def _tree(self):
        raise NotImplementedError

    def _alloc(self, D, device):
        n_nodes = int(self._tree()[0][-1])
        self._sums = torch.zeros(n_nodes, D, dtype=torch.float64, device=device)
        self._counts = torch.zeros(n_nodes, dtype=torch.int64, device=device)
        self._state = torch.zeros(4, dtype=torch.float64, device=device)

    def _device_csr(self, device):
        tier_base, child_ptr, child_idx = self._tree()
        if self._csr_dev is None or self._csr_dev[0] != device:
            mk = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
            self._csr_dev = (device, mk(child_ptr), mk(child_idx))
        return tier_base, self._csr_dev[1], self._csr_dev[2]

    def reset(self):
        """Forget every row fitted so far."""
        self._reset()
        return self

    @torch.no_grad()
    def partial_fit(self, X, y):
        """Add a batch of (prepared) features X [B, D] with labels y; finalize() before predict.
        Any split of the training rows into consecutive batches gives bit-identical centroids."""
        self._check_labels(X, y)
        if not X.is_cuda:
            raise RuntimeError("libhvk ops run on the GPU only; got a CPU tensor (X)")
        if self._sums is None:
            self._alloc(X.shape[1], X.device)
        elif X.shape[1] != self._sums.shape[1]:
            raise ValueError(f"X has {X.shape[1]} features, the fitted rows {self._sums.shape[1]}")
        lo = int(self._tree()[0][-2])
        ops.ss_accumulate(X, y, self._sums[lo:], self._counts[lo:], self._state)
        self._cent = self._cnorm = None
        return self

    def finalize(self):
        """Centroids of every class seen (of every node of every tier) from the running sums."""
        if self._sums is None:
            raise RuntimeError("finalize() before any partial_fit()")
        tier_base, cptr, cidx = self._device_csr(self._sums.device)
        self._cent, self._cnorm = ops.ss_finalize(self._sums, self._counts, tier_base, cptr, cidx)
        return self

    def fit(self, X, y):
        """reset() + partial_fit(X, y) + finalize()."""
        self.reset()
        return self.partial_fit(X, y).finalize()

    def _fitted(self):
        if self._cent is None:
            raise RuntimeError("not fitted: call fit(), or finalize() after the last partial_fit()")

    def _tier(self, a, t):
        tier_base = self._tree()[0]
        return a[int(tier_base[t]):int(tier_base[t + 1])]

    @property
    def invalid_(self):
        """Training rows skipped because their label was outside [0, n_classes) (a host read)."""
        return 0 if self._state is None else int(self._state[1].item())


class NearestCentroid(_Centroids):
    """sklearn.neighbors.NearestCentroid (euclidean) as simpleshot.py:180 uses it, on the device.

    Classes are indexed by label: class c's centroid is row c of `centroids_`, a class with no
    training row has no centroid (`counts_[c] == 0`) and is never predicted, and predict returns
    labels.  sklearn indexes by LabelEncoder position and returns `classes_[position]`, which is
    the same thing exactly when every class occurs in the training set.  `n_classes` fixes the
    label range [0, n_classes) (labels outside it are skipped and counted in `invalid_`); when it
    is None, fit() takes max(y) + 1 and partial_fit() needs it given."""

    def __init__(self, n_classes=None):
        super().__init__()
        self.n_classes = n_classes

    def _tree(self):
        return np.array([0, self.tier_sizes[0]], np.int32), None, None

    def _check_labels(self, X, y):
        if X.ndim != 2 or y.ndim != 1 or y.shape[0] != X.shape[0]:
            raise ValueError(f"X must be [N, D] and y [N], got {tuple(X.shape)} and {tuple(y.shape)}")
        if self.tier_sizes is None:
            if self.n_classes is None:
                raise ValueError("partial_fit() needs NearestCentroid(n_classes=...)")
            self.tier_sizes = (int(self.n_classes),)

    def fit(self, X, y):
        if self.n_classes is None:
            if y.numel() == 0:
                raise ValueError("fit() on no rows")
            self.tier_sizes = (max(int(y.max().item()), 0) + 1,)
        return super().fit(X, y)

    @property
    def centroids_(self):
        self._fitted()
        return self._cent

    @property
    def counts_(self):
        self._fitted()
        return self._counts

    @torch.no_grad()
    def predict(self, X):
        """Nearest centroid of every row of X [N, D]: int64 [N] on the device."""
        self._fitted()
        return ops.ss_predict_flat(X, self._cent, self._cnorm).long()


class HierarchicalNearestCentroid(_Centroids):
    """hierarchy.HierarchicalNearestCentroid (hierarchy.py:488-597) on the device: `lookup_vecs`
    are the six child -> parent vectors of build_parent_label_lookup, `y` is [N, 7] tier ids, and
    predict walks top-down, choosing at every tier the nearest centroid among the children of the
    node chosen above it; it returns the whole path, int64 [N, 7].

    Only the leaf column of `y` is read: the centroid of an internal node is the mean of the rows
    under it, which the tree gives (the reference averages by each tier's own label column, the
    same rows when `y` holds paths of this tree).  Classes are indexed by tier id; a class with no
    training row has no centroid and is never predicted.  The reference indexes by LabelEncoder
    position, which is the same thing exactly when every class occurs in the training set."""

    def __init__(self, lookup_vecs):
        super().__init__()
        self.lookup_vecs = lookup_vecs
        self.tier_sizes, self._tier_base, self._child_ptr, self._child_idx = children_csr(lookup_vecs)

    def _tree(self):
        return self._tier_base, self._child_ptr, self._child_idx

    def _check_labels(self, X, y):
        n = len(self.tier_sizes)
        if X.ndim != 2 or y.ndim != 2 or y.shape != (X.shape[0], n):
            raise ValueError(f"X must be [N, D] and y [N, {n}] tier ids, got {tuple(X.shape)} and "
                             f"{tuple(y.shape)}")

    @property
    def centroids_(self):
        """Per tier, f32 [n_classes of the tier, D]."""
        self._fitted()
        return [self._tier(self._cent, t) for t in range(len(self.tier_sizes))]

    @property
    def counts_(self):
        self._fitted()
        return [self._tier(self._counts, t) for t in range(len(self.tier_sizes))]

    @torch.no_grad()
    def predict(self, X):
        """The top-down path of every row of X [N, D]: int64 [N, 7] tier ids on the device."""
        self._fitted()
        tier_base, cptr, cidx = self._device_csr(self._cent.device)
        return ops.ss_predict_tree(X, self._cent, self._counts, tier_base, cptr, cidx).long()


def _features(model, batch, device_transforms, dtype):
    if device_transforms is not None:
        batch = device_transforms(batch)
    x, y = batch
    with torch.autocast(device_type=x.device.type, dtype=dtype, enabled=x.device.type == "cuda"):
        return model(x), y


@torch.no_grad()
def evaluate(config, model, train_batches, eval_batches, *, lookup_vecs=None, tree_dists=None,
             device_transforms=None, dtype=torch.bfloat16):
    """simpleshot.main (simpleshot.py:157-207) without its IO: fit the nearest-centroid classifier
    on the features of `train_batches`, score `eval_batches` (iterables of (inputs, targets)
    batches on the device, the last of which may be smaller).

    `model` must be a models.FeatureOnlyModel; `config.simpleshot` gives `centered`,
    `l2_normalized` and `hierarchical` (targets are then [B, 7] tier ids and `lookup_vecs` is
    needed; otherwise [B] classes, or [B, 7] whose leaf column counts).  `device_transforms` are
    applied to every batch; a NormalizationFn the backbone can absorb is folded into its patch
    embedding for the duration, as Trainer does.  Per batch: a no-grad forward under autocast,
    ops.ss_prepare, then partial_fit or predict; the hits, per-tier hits (hierarchical) and
    `tree_dists[pred, label]` (uint8 or float [L, L]) are summed in float64 on the device and
    read once at the end.

    Returns {"acc@1"[, "tree-dist"][, "acc@1/tier0" .. "tier6"]} as Python floats, NaN without
    eval batches.  The model's parameters, its train / eval flag and its input normalisation are
    left as found."""
    from .models import FeatureOnlyModel
    if not isinstance(model, FeatureOnlyModel):
        raise ValueError(f"simpleshot.evaluate needs a models.FeatureOnlyModel (config.model.variant "
                         f"'simpleshot'), got {type(model).__name__}")
    ss = config.simpleshot
    hier = bool(ss.hierarchical)
    if hier:
        if lookup_vecs is None:
            raise ValueError("config.simpleshot.hierarchical needs lookup_vecs "
                             "(hierarchy.build_parent_label_lookup)")
        clf = HierarchicalNearestCentroid(lookup_vecs)
    else:
        n = None
        if tree_dists is not None:
            n = int(tree_dists.shape[0])
        elif lookup_vecs is not None:
            n = len(lookup_vecs[-1])
        clf = NearestCentroid(n_classes=n)

    def prepared(batch):
        f, y = _features(model, batch, device_transforms, dtype)
        return ops.ss_prepare(f, centered=ss.centered, l2_normalized=ss.l2_normalized), y

    modes = [m.training for m in model.modules()]
    pe = getattr(model.backbone, "patch_embed", None)
    saved_norm = getattr(pe, "input_norm", None)
    if device_transforms is not None and getattr(device_transforms, "fuse_into", None):
        if device_transforms.fuse_into(model.backbone):
            device_transforms = None
    try:
        model.eval()
        if hier or clf.n_classes is not None:
            for batch in train_batches:
                x, y = prepared(batch)
                clf.partial_fit(x, y if hier or y.ndim == 1 else y[:, -1])
            if clf._sums is None:
                raise ValueError("simpleshot.evaluate got no train batches")
            clf.finalize()
        else:
            # the class count is not known in advance: the labels decide it, which takes the
            # prepared features of the whole training set at once (pass tree_dists or lookup_vecs)
            pairs = [prepared(b) for b in train_batches]
            if not pairs:
                raise ValueError("simpleshot.evaluate got no train batches")
            xs, ys = zip(*pairs)
            clf.fit(torch.cat(xs), torch.cat([y if y.ndim == 1 else y[:, -1] for y in ys]))
        sums = None
        for batch in eval_batches:
            x, y = prepared(batch)
            if sums is None:
                sums = torch.zeros(3 + N_TIERS, dtype=torch.float64, device=x.device)
                if tree_dists is not None:
                    tree_dists = tree_dists.to(x.device)
            pred = clf.predict(x)
            leaf = y if y.ndim == 1 else y[:, -1]
            pleaf = pred[:, -1] if hier else pred
            sums[0] += leaf.shape[0]
            sums[1] += (pleaf == leaf).sum()
            if tree_dists is not None:
                sums[2] += tree_dists[pleaf, leaf.long()].sum(dtype=torch.float64)
            if hier:
                sums[3:] += (pred == y).sum(0)
    finally:
        if pe is not None and hasattr(pe, "input_norm"):
            pe.input_norm = saved_norm
        for m, t in zip(model.modules(), modes):
            m.training = t
    if sums is None:
        sums = torch.full((3 + N_TIERS,), float("nan"), dtype=torch.float64, device=clf._state.device)
    *s, _, invalid = torch.cat([sums, clf._state[:2]]).tolist()  # the one host read
    if invalid:
        raise ValueError(f"{int(invalid)} training label(s) outside [0, num_classes) were passed to the fit")
    n = s[0]
    div = (lambda v: v / n) if n == n and n else (lambda v: float("nan"))
    out = {"acc@1": div(s[1])}
    if tree_dists is not None:
        out["tree-dist"] = div(s[2])
    if hier:
        for t in range(N_TIERS):
            out[f"acc@1/tier{t}"] = div(s[3 + t])
    return out
