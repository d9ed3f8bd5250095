"""Linear-probe evaluation -- drop-in for what linear_probe.py does after its features
(linear_probe.py:189-234): StandardScaler, a one-vs-rest logistic classifier, a 5-fold grid search
over its L2 penalty, and acc@1 / tree-dist of the refit model.

Everything after the backbone runs in libhvk on the device (ops.lp_*, include/hvk.h); no feature
goes to the host (the labels do, once, for the fold assignment).

The classifier is the MINIMISER of sklearn's objective, not a replay of its SGD.
SGDClassifier(loss="log_loss") is unseeded, sample-sequential and stops on a noisy criterion: a
stochastic approximation nobody can reproduce.  What it approximates is exact: for every class c,
with y_ic = +1 where label_i == c and -1 elsewhere and x~ the standardised features,

    F_c(w, b) = (1/N) sum_i log(1 + exp(-y_ic (w . x~_i + b))) + (alpha / 2) ||w||^2

(b unpenalised).  LogisticOvR minimises all of them in lock-step by full-batch accelerated gradient
(FISTA momentum with the gradient restart of O'Donoghue & Candes) to max |grad F_c| <= tol.
A class without a positive row has no minimiser (b -> -inf): it is not fitted and never predicted,
as hvamd.simpleshot skips empty classes.  Single process; the reference's .npy feature cache, W&B
logging and loaders are not provided.
"""
import warnings

import numpy as np
import torch
import torch.nn.functional as F

from . import ops

ALPHAS = (1e-4, 1e-2, 1.0)  # linear_probe.py:195


def _f32(X):
    X = X.detach()
    return X if X.dtype == torch.float32 else X.float()


class StandardScaler:
    """sklearn.preprocessing.StandardScaler on the device: float64 column sums that batches are
    added to (any split of the rows into consecutive batches leaves the same bits), population
    variance, and scale 1 for a column whose variance is exactly 0."""

    def __init__(self):
        self.reset()

    def reset(self):
        self._sum = self._sumsq = None
        self.n_samples_seen_ = 0
        self.mean_ = self.var_ = self.scale_ = None
        return self

    @classmethod
    def from_sums(cls, sum_, sumsq, n):
        """The scaler of `n` rows whose float64 column sums are given."""
        s = cls()
        s._sum, s._sumsq, s.n_samples_seen_ = sum_, sumsq, int(n)
        return s.finalize()

    @torch.no_grad()
    def partial_fit(self, X):
        """Add a batch X [B, D]; finalize() before transform."""
        X = _f32(X)
        if X.ndim != 2:
            raise ValueError(f"X must be [B, D], got {tuple(X.shape)}")
        if self._sum is None:
            self._sum = torch.zeros(X.shape[1], dtype=torch.float64, device=X.device)
            self._sumsq = torch.zeros_like(self._sum)
        elif X.shape[1] != self._sum.shape[0]:
            raise ValueError(f"X has {X.shape[1]} features, the fitted rows {self._sum.shape[0]}")
        ops.lp_moments(X, self._sum, self._sumsq)
        self.n_samples_seen_ += int(X.shape[0])
        self.mean_ = None
        return self

    def finalize(self):
        """mean_, var_ and scale_ (float64 [D] on the device) from the running sums."""
        if self._sum is None or self.n_samples_seen_ < 1:
            raise RuntimeError("finalize() before any row was fitted")
        n = float(self.n_samples_seen_)
        self.mean_ = self._sum / n
        self.var_ = (self._sumsq / n - self.mean_ * self.mean_).clamp_min_(0.0)
        self.scale_ = torch.where(self.var_ > 0, self.var_.sqrt(), torch.ones_like(self.var_))
        return self

    def fit(self, X):
        """reset() + partial_fit(X) + finalize()."""
        return self.reset().partial_fit(X).finalize()

    @torch.no_grad()
    def transform(self, X):
        """(X - mean_) / scale_ as dense f32 on the device."""
        if self.mean_ is None:
            raise RuntimeError("not fitted: call fit(), or finalize() after the last partial_fit()")
        return ops.lp_standardize(_f32(X), self._sum, self._sumsq, self.n_samples_seen_)[0]


def _lipschitz_lambda(xs, mask, n_eff, iters=64):
    """An estimate of lambda_max(Xa^T Xa / N) for Xa = [xs, 1] over the rows in `mask`:
    min(D + 1, 1.1 x the Rayleigh quotient after `iters` power iterations from the constant
    vector).  D + 1 is the trace when the rows were standardised on themselves."""
    D = xs.shape[1]
    v = torch.full((D + 1,), (D + 1) ** -0.5, dtype=torch.float32, device=xs.device)
    q = None
    for it in range(iters + 1):
        u = torch.mv(xs, v[:D]) + v[D]
        if mask is not None:
            u = u * mask
        q = (u.double() ** 2).sum() / n_eff  # v^T M v with ||v|| = 1
        if it == iters:
            break
        w = torch.cat([torch.mv(xs.t(), u), u.sum().reshape(1)]) / n_eff
        v = w / w.norm().clamp_min(1e-30)
    return min(float(D + 1), 1.1 * float(q.item()))


class LogisticOvR:
    """One-vs-rest logistic regression with an L2 penalty `alpha` on the weights, the minimiser
    of SGDClassifier(loss="log_loss", alpha=alpha)'s objective (module docstring).

    `alpha` may be a sequence: the estimator then holds one model per value, all solved together,
    and coef_ / intercept_ / decision_function / predict gain a leading axis of that length.
    Classes are indexed by label in [0, n_classes) (max(y) + 1 when None); labels outside raise.
    After fit: coef_ f32 [L, D], intercept_ f32 [L] (-inf for a class without a row), n_iter_,
    converged_ (bool [L]: max |gradient| <= tol was reached; unfitted classes count as converged)
    and fitted_ (bool [L]: the class had a row)."""

    def __init__(self, alpha=1e-4, tol=1e-4, max_iter=5000, n_classes=None):
        self.alpha, self.tol, self.max_iter, self.n_classes = alpha, float(tol), int(max_iter), n_classes
        self._W = None

    def _alphas(self):
        many = isinstance(self.alpha, (tuple, list, np.ndarray))
        a = [float(v) for v in (self.alpha if many else [self.alpha])]
        if not a or min(a) < 0:
            raise ValueError(f"alpha must be >= 0, got {self.alpha}")
        return many, a

    @torch.no_grad()
    def fit(self, X, y, fold=None, skip_fold=None):
        """X f32 [N, D] (standardised, dense), y int64 [N]; rows with fold[i] == skip_fold (`fold`
        uint8 [N]) are held out without a copy of X."""
        many, alphas = self._alphas()
        if X.ndim != 2 or y.ndim != 1 or y.shape[0] != X.shape[0] or X.shape[0] < 1:
            raise ValueError(f"X must be [N >= 1, D] and y [N], got {tuple(X.shape)} and {tuple(y.shape)}")
        if y.dtype.is_floating_point or y.dtype == torch.bool:
            raise ValueError("fit takes integer class labels")
        if (fold is None) != (skip_fold is None):
            raise ValueError("fold and skip_fold go together")
        y = y.to(torch.int64).contiguous()
        lo, hi = int(y.min().item()), int(y.max().item())
        L = int(self.n_classes) if self.n_classes is not None else max(hi, 0) + 1
        if lo < 0 or hi >= L:
            raise ValueError(f"labels outside [0, {L}): min {lo}, max {hi}")
        X = _f32(X).contiguous()
        dev, (N, D), A = X.device, X.shape, len(alphas)
        R = A * L
        mask = None
        if fold is not None:
            if fold.dtype != torch.uint8 or fold.shape != (N,):
                raise ValueError(f"fold must be uint8 [{N}]")
            fold = fold.contiguous()
            mask = (fold != int(skip_fold)).float()
        counts = torch.bincount(y if mask is None else y[mask.bool()], minlength=L)
        n_eff = int(counts.sum().item())
        if n_eff < 1:
            raise ValueError("no row left to fit on")
        fitted = counts > 0
        frozen = (~fitted).to(torch.uint8).repeat(A)
        target = torch.arange(L, dtype=torch.int32, device=dev).repeat(A)
        alpha_r = torch.tensor(alphas, dtype=torch.float32, device=dev).repeat_interleave(L)
        lip = 0.25 * _lipschitz_lambda(X, mask, n_eff) + max(alphas)
        step = 1.0 / lip

        W, Yw = torch.zeros(R, D, device=dev), torch.zeros(R, D, device=dev)
        b, Yb, t = torch.zeros(R, device=dev), torch.zeros(R, device=dev), torch.ones(R, device=dev)
        gmax = torch.full((R,), float("inf"), device=dev)
        conv = frozen.clone()  # unfitted problems have nothing to converge to
        grads = (torch.empty(R, D, device=dev), torch.empty(R, device=dev),
                 torch.empty(R, dtype=torch.float64, device=dev))
        n_iter = 0
        for it in range(self.max_iter):
            ops.lp_loss_grad(X, y, Yw, Yb, target, alpha_r, fold=fold,
                             skip_fold=-1 if skip_fold is None else int(skip_fold), out=grads, check_labels=False)
            ops.lp_step(W, b, Yw, Yb, grads[0], grads[1], t, step, self.tol, gmax, conv, frozen=frozen)
            n_iter = it + 1
            # the one host read of the loop, every 32nd iteration
            if n_iter % 32 == 0 and bool(conv.all().item()):
                break
        b = torch.where(frozen.bool(), torch.full_like(b, float("-inf")), b)
        self._W, self._b, self._A, self._L, self._many = W, b, A, L, many
        self._Wp = None
        self.n_iter_ = n_iter
        self.step_ = step
        self.loss_ = grads[2].view(A, L) if many else grads[2]
        self.gmax_ = gmax.view(A, L) if many else gmax
        self.converged_ = conv.bool().view(A, L) if many else conv.bool()
        self.fitted_ = fitted
        return self

    def _check(self):
        if self._W is None:
            raise RuntimeError("not fitted: call fit()")

    @property
    def coef_(self):
        self._check()
        return self._W.view(self._A, self._L, -1) if self._many else self._W

    @property
    def intercept_(self):
        self._check()
        return self._b.view(self._A, self._L) if self._many else self._b

    @torch.no_grad()
    def decision_function(self, X):
        """x . w_c + b_c of every row and class: f32 [N, L] ([A, N, L] with a sequence of alphas);
        -inf for a class that was not fitted."""
        self._check()
        s = ops.lp_decision(_f32(X).contiguous(), self._W, self._b)
        return s.view(-1, self._A, self._L).permute(1, 0, 2) if self._many else s

    @torch.no_grad()
    def predict(self, X):
        """argmax_c (x . w_c + b_c), the lowest class among equals: int64 [N] ([A, N]).  It is
        argmin_c (cnorm_c - 2 x . c_c) with c = w and cnorm = -2 b, which hvk_ss_predict_flat
        computes; cnorm = +inf keeps an unfitted class from being chosen."""
        self._check()
        X = _f32(X).contiguous()
        D = X.shape[1]
        pad = -D % 4  # that kernel takes D % 4 == 0: zero columns change no product
        if self._Wp is None:
            self._Wp = (F.pad(self._W, (0, pad)) if pad else self._W, -2.0 * self._b)
        Wp, cn = self._Wp
        if pad:
            X = F.pad(X, (0, pad))
        L = self._L
        preds = [ops.ss_predict_flat(X, Wp[a * L:(a + 1) * L], cn[a * L:(a + 1) * L]).long() for a in range(self._A)]
        return torch.stack(preds) if self._many else preds[0]


def stratified_folds(y, n_splits=5):
    """The test fold of every sample under sklearn's StratifiedKFold(n_splits) without shuffling,
    restated in numpy: uint8 [N].  Classes are taken in order of first appearance; the sorted
    labels are dealt round-robin to the folds, which fixes how many samples of each class a fold
    holds, and every class hands its samples, in order, to the folds in ascending fold index.
    Raises sklearn's ValueError when n_splits exceeds the size of every class and gives its
    warning when it exceeds only the smallest."""
    y = np.asarray(y).reshape(-1)
    n_splits = int(n_splits)
    if not 2 <= n_splits <= 255:
        raise ValueError(f"n_splits must be in [2, 255], got {n_splits}")
    if n_splits > len(y):
        raise ValueError(f"Cannot have number of splits n_splits={n_splits} greater than the number of "
                         f"samples: n_samples={len(y)}.")
    _, first, inv = np.unique(y, return_index=True, return_inverse=True)
    enc = np.argsort(np.argsort(first))[inv.reshape(-1)]  # class ids by first appearance
    n_classes = len(first)
    counts = np.bincount(enc, minlength=n_classes)
    if np.all(n_splits > counts):
        raise ValueError(f"n_splits={n_splits} cannot be greater than the number of members in each class.")
    if n_splits > counts.min():
        warnings.warn(f"The least populated class in y has only {counts.min()} members, which is less than "
                      f"n_splits={n_splits}.", UserWarning)
    order = np.sort(enc)
    alloc = np.stack([np.bincount(order[i::n_splits], minlength=n_classes) for i in range(n_splits)])
    folds = np.empty(len(y), np.uint8)
    for k in range(n_classes):
        folds[enc == k] = np.repeat(np.arange(n_splits, dtype=np.uint8), alloc[:, k])
    return folds


class LinearProbe:
    """The refit pipeline grid_search returns: StandardScaler, then LogisticOvR."""

    def __init__(self, scaler, clf):
        self.scaler, self.clf = scaler, clf

    def decision_function(self, X):
        return self.clf.decision_function(self.scaler.transform(X))

    def predict(self, X):
        return self.clf.predict(self.scaler.transform(X))


@torch.no_grad()
def grid_search(X, y, alphas=ALPHAS, n_splits=5, tol=1e-4, max_iter=5000, n_classes=None):
    """GridSearchCV(make_pipeline(StandardScaler(), SGDClassifier(loss="log_loss")),
    {"sgdclassifier__alpha": alphas}) of linear_probe.py:189-198 with the exact minimiser in the
    classifier's place: per fold of the unshuffled StratifiedKFold, scaler and classifier are
    fitted on the other folds (all alphas at once) and scored by accuracy on the held-out one; the
    best mean score wins, the first alpha among equals, and is refit on every row.

    X [N, D] features and y [N] labels on the device.  Returns (LinearProbe, best_alpha,
    cv_scores float64 numpy [n_alphas, n_splits]); the pipeline also carries cv_n_iter_."""
    alphas = [float(a) for a in alphas]
    X = _f32(X).contiguous()
    y = y.to(torch.int64).contiguous()
    if n_classes is None:
        n_classes = int(y.max().item()) + 1
    fold = torch.from_numpy(stratified_folds(y.cpu().numpy(), n_splits)).to(X.device)
    held = [(fold == f).nonzero().squeeze(1) for f in range(n_splits)]
    # the moments of every fold on its own; a training part is the sum of the others
    parts = [StandardScaler().partial_fit(X[idx]) for idx in held]
    scores = torch.zeros(len(alphas), n_splits, dtype=torch.float64, device=X.device)
    n_iters = []
    for f in range(n_splits):
        others = [p for g, p in enumerate(parts) if g != f]
        scaler = StandardScaler.from_sums(sum(p._sum for p in others), sum(p._sumsq for p in others),
                                          sum(p.n_samples_seen_ for p in others))
        xs = scaler.transform(X)
        clf = LogisticOvR(alphas, tol, max_iter, n_classes).fit(xs, y, fold=fold, skip_fold=f)
        n_iters.append(clf.n_iter_)
        if held[f].numel():
            scores[:, f] = (clf.predict(xs[held[f]]) == y[held[f]]).double().mean(1)
        del xs
    cv = scores.cpu().numpy()
    best = int(np.argmax(cv.mean(1)))  # the first of equal means, as GridSearchCV's rank 1
    scaler = StandardScaler().fit(X)
    clf = LogisticOvR(alphas[best], tol, max_iter, n_classes).fit(scaler.transform(X), y)
    pipe = LinearProbe(scaler, clf)
    pipe.cv_n_iter_ = n_iters
    return pipe, alphas[best], cv


def _features(model, batch, device_transforms, dtype):
    if device_transforms is not None:
        batch = device_transforms(batch)
    x, y = batch
    with torch.autocast(device_type=x.device.type, dtype=dtype, enabled=x.device.type == "cuda"):
        return model(x).float(), (y if y.ndim == 1 else y[:, -1])


@torch.no_grad()
def evaluate(config, model, train_batches, eval_batches, *, tree_dists=None, taxonomy=None, alphas=ALPHAS,
             n_splits=5, device_transforms=None, dtype=torch.bfloat16, tol=1e-4, max_iter=5000):
    """linear_probe.main (linear_probe.py:201-238) without its IO: features of `train_batches`
    through the frozen `model` (a models.FeatureOnlyModel, config.model.variant "linear-probe"),
    grid_search on them, then the refit pipeline on `eval_batches` (iterables of (inputs, targets)
    batches on the device; targets [B] classes or [B, 7] tier ids whose leaf column counts).

    `device_transforms` are applied to every batch; a NormalizationFn the backbone can absorb is
    folded into its patch embedding for the duration, as Trainer does.  The features stay on the
    device; hits and `tree_dists[pred, label]` (uint8 or float [L, L], or built from `taxonomy`, a
    hierarchy.Taxonomy) are summed in float64 there and read once.

    Returns {"acc@1"[, "tree-dist"], "best-alpha", "cv-scores"}; the model's parameters, its
    train / eval flag and its input normalisation are left as found."""
    from .models import FeatureOnlyModel
    assert config.model.variant == "linear-probe", config.model.variant  # linear_probe.py:215
    if not isinstance(model, FeatureOnlyModel):
        raise ValueError(f"linear_probe.evaluate needs a models.FeatureOnlyModel, got {type(model).__name__}")
    if tree_dists is None and taxonomy is not None:
        from . import hierarchy
        tree_dists = hierarchy.build_tree_dist_matrix([hierarchy.HierarchicalLabel.parse(n)
                                                       for n in taxonomy.classes])
    n_classes = int(tree_dists.shape[0]) if tree_dists is not None else None

    modes = [m.training for m in model.modules()]
    pe = getattr(model.backbone, "patch_embed", None)
    saved_norm = getattr(pe, "input_norm", None)
    if device_transforms is not None and getattr(device_transforms, "fuse_into", None):
        if device_transforms.fuse_into(model.backbone):
            device_transforms = None
    try:
        model.eval()
        pairs = [_features(model, b, device_transforms, dtype) for b in train_batches]
        if not pairs:
            raise ValueError("linear_probe.evaluate got no train batches")
        xs, ys = zip(*pairs)
        # the reference shuffles the training rows here (linear_probe.py:209-213), which matters to
        # its sample-sequential SGD only: a full-batch minimiser sums over the rows in any order
        pipe, best_alpha, cv = grid_search(torch.cat(xs), torch.cat(ys), alphas=alphas, n_splits=n_splits, tol=tol,
                                           max_iter=max_iter, n_classes=n_classes)
        del pairs, xs
        sums = None
        for batch in eval_batches:
            f, y = _features(model, batch, device_transforms, dtype)
            if sums is None:
                sums = torch.zeros(3, dtype=torch.float64, device=f.device)
                if tree_dists is not None:
                    tree_dists = tree_dists.to(f.device)
            pred = pipe.predict(f)
            sums[0] += y.shape[0]
            sums[1] += (pred == y).sum()
            if tree_dists is not None:
                sums[2] += tree_dists[pred, y.long()].sum(dtype=torch.float64)
    finally:
        if pe is not None and hasattr(pe, "input_norm"):
            pe.input_norm = saved_norm
        for m, t in zip(model.modules(), modes):
            m.training = t
    n, hits, dist = sums.tolist() if sums is not None else (0.0, 0.0, 0.0)  # the one host read
    div = (lambda v: v / n) if n else (lambda v: float("nan"))
    out = {"acc@1": div(hits)}
    if tree_dists is not None:
        out["tree-dist"] = div(dist)
    out["best-alpha"] = best_alpha
    out["cv-scores"] = cv
    return out
