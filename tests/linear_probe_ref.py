"""numpy float64 restatement of the linear probe (hvamd.linear_probe, include/hvk.h hvk_lp_*), the
reference of tests/test_linear_probe_cpu.py and tests/test_gpu_linear_probe.py: the scaler, the
loss and gradient of the one-vs-rest logistic objective, the exact recurrence of the solver, the
fold assignment, the grid search and the prediction margin."""
import numpy as np

ALPHAS = (1e-4, 1e-2, 1.0)


# --------------------------------------------------------------------------- scaler
def scaler(X):
    """(mean, scale): population standard deviation, 1 where the variance is exactly 0."""
    X = np.asarray(X, np.float64)
    mean = X.mean(0)
    var = ((X - mean) ** 2).mean(0)
    return mean, np.where(var > 0, np.sqrt(var), 1.0)


def standardize(X, mean, scale):
    return (np.asarray(X, np.float64) - mean) / scale


# --------------------------------------------------------------------------- objective
def scores(X, W, b):
    return np.asarray(X, np.float64) @ np.asarray(W, np.float64).T + np.asarray(b, np.float64)


def loss_grad(X, y, W, b, target, alpha, mask=None):
    """(dW [R, D], db [R], loss [R], z [N, R]) of the R binary problems "y == target[r]" with
    penalty alpha[r] over the rows where `mask` (bool [N]) is set."""
    X = np.asarray(X, np.float64)
    W = np.asarray(W, np.float64)
    alpha = np.asarray(alpha, np.float64)
    keep = np.ones(len(X), bool) if mask is None else np.asarray(mask, bool)
    z = scores(X, W, b)
    pos = np.asarray(y)[:, None] == np.asarray(target)[None, :]
    n = max(int(keep.sum()), 1)
    with np.errstate(over="ignore"):
        sig = np.where(z >= 0, 1.0 / (1.0 + np.exp(-np.abs(z))), np.exp(-np.abs(z)) / (1.0 + np.exp(-np.abs(z))))
    r = (sig - pos) * keep[:, None]
    term = (np.maximum(np.where(pos, -z, z), 0.0) + np.log1p(np.exp(-np.abs(z)))) * keep[:, None]
    dW = r.T @ X / n + alpha[:, None] * W
    db = r.sum(0) / n
    loss = term.sum(0) / n + 0.5 * alpha * (W * W).sum(1)
    return dW, db, loss, z


def lipschitz_lambda(X, mask=None, iters=64):
    """min(D + 1, 1.1 x Rayleigh quotient of [X, 1]^T [X, 1] / N after `iters` power iterations
    from the constant vector)."""
    X = np.asarray(X, np.float64)
    if mask is not None:
        X = X[np.asarray(mask, bool)]
    n, D = X.shape
    Xa = np.concatenate([X, np.ones((n, 1))], 1)
    v = np.full(D + 1, (D + 1) ** -0.5)
    for _ in range(iters):
        w = Xa.T @ (Xa @ v) / n
        v = w / max(np.linalg.norm(w), 1e-30)
    u = Xa @ v
    return min(float(D + 1), 1.1 * float(u @ u) / n)


def solve(X, y, target, alpha, step, n_iter, tol=0.0, mask=None, frozen=None):
    """The solver's recurrence for `n_iter` iterations from zero.  Returns a dict with the iterate
    (W, b), the extrapolated point (Yw, Yb), t, gmax, converged, and per iteration the restart dot
    products `dots` [n_iter, R] with their absolute-value sums `dots_abs` (sum |g| |x+ - x|)."""
    R, D = len(target), np.asarray(X).shape[1]
    W, Yw = np.zeros((R, D)), np.zeros((R, D))
    b, Yb, t = np.zeros(R), np.zeros(R), np.ones(R)
    gmax, conv = np.full(R, np.inf), np.zeros(R, bool)
    live = np.ones(R, bool) if frozen is None else ~np.asarray(frozen, bool)
    dots, dots_abs = [], []
    for _ in range(n_iter):
        gW, gb, _, _ = loss_grad(X, y, Yw, Yb, target, alpha, mask)
        xw, xb = Yw - step * gW, Yb - step * gb
        dot = (gW * (xw - W)).sum(1) + gb * (xb - b)
        dots.append(dot)
        dots_abs.append((np.abs(gW) * np.abs(xw - W)).sum(1) + np.abs(gb) * np.abs(xb - b))
        gm = np.maximum(np.abs(gW).max(1), np.abs(gb))
        done = live & (gm <= tol)
        move = live & ~done
        restart = dot > 0
        t1 = np.where(restart, 1.0, 0.5 * (1.0 + np.sqrt(1.0 + 4.0 * t * t)))
        beta = np.where(restart, 0.0, (t - 1.0) / t1)
        nYw, nYb = xw + beta[:, None] * (xw - W), xb + beta * (xb - b)
        W = np.where(done[:, None], Yw, np.where(move[:, None], xw, W))
        b = np.where(done, Yb, np.where(move, xb, b))
        Yw = np.where(move[:, None], nYw, Yw)
        Yb = np.where(move, nYb, Yb)
        t = np.where(move, t1, t)
        gmax = np.where(live, gm, gmax)
        conv = np.where(live, done, conv)
    return dict(W=W, b=b, Yw=Yw, Yb=Yb, t=t, gmax=gmax, converged=conv, dots=np.array(dots),
                dots_abs=np.array(dots_abs))


def fit(X, y, alphas, n_classes, tol=1e-4, max_iter=5000, mask=None):
    """All alphas at once on standardised X: (W [A, L, D], b [A, L] with -inf for classes without a
    row in the mask, n_iter), stopping as the device does (a look every 32 iterations)."""
    alphas = [float(a) for a in alphas]
    A, L = len(alphas), int(n_classes)
    yk = np.asarray(y) if mask is None else np.asarray(y)[np.asarray(mask, bool)]
    frozen = np.tile(np.bincount(yk, minlength=L) == 0, A)
    target = np.tile(np.arange(L), A)
    alpha = np.repeat(alphas, L)
    step = 1.0 / (0.25 * lipschitz_lambda(X, mask) + max(alphas))
    R, D = A * L, np.asarray(X).shape[1]
    W, Yw = np.zeros((R, D)), np.zeros((R, D))
    b, Yb, t = np.zeros(R), np.zeros(R), np.ones(R)
    conv = frozen.copy()
    n_iter = 0
    for it in range(max_iter):
        gW, gb, _, _ = loss_grad(X, y, Yw, Yb, target, alpha, mask)
        xw, xb = Yw - step * gW, Yb - step * gb
        dot = (gW * (xw - W)).sum(1) + gb * (xb - b)
        gm = np.maximum(np.abs(gW).max(1), np.abs(gb))
        done = ~frozen & (gm <= tol)
        move = ~frozen & ~done
        restart = dot > 0
        t1 = np.where(restart, 1.0, 0.5 * (1.0 + np.sqrt(1.0 + 4.0 * t * t)))
        beta = np.where(restart, 0.0, (t - 1.0) / t1)
        nYw, nYb = xw + beta[:, None] * (xw - W), xb + beta * (xb - b)
        W = np.where(done[:, None], Yw, np.where(move[:, None], xw, W))
        b = np.where(done, Yb, np.where(move, xb, b))
        Yw = np.where(move[:, None], nYw, Yw)
        Yb = np.where(move, nYb, Yb)
        t = np.where(move, t1, t)
        conv = frozen | done
        n_iter = it + 1
        if n_iter % 32 == 0 and conv.all():
            break
    b = np.where(frozen, -np.inf, b)
    return W.reshape(A, L, D), b.reshape(A, L), n_iter


# --------------------------------------------------------------------------- prediction
def predict(X, W, b):
    """(pred [N], best, second): argmax of x . w + b, the lowest class among equals; second is
    -inf with a single finite class."""
    z = scores(X, W, b)
    arg = z.argmax(1)
    rows = np.arange(len(z))
    best = z[rows, arg]
    rest = z.copy()
    rest[rows, arg] = -np.inf
    return arg, best, rest.max(1)


def margin_band(X, W, b, best, second, rel=1e-5):
    """Rows a float32 kernel is not asked to agree on: best and second-best score differ by <=
    rel (max_c sum_k |x_k w_ck| + max |b|), the f32-MFMA bound of simpleshot_ref.margin_band
    (1e-5 sum |a b| per dot product covers two compared scores 30 times over)."""
    X = np.abs(np.asarray(X, np.float64))
    W = np.abs(np.asarray(W, np.float64))
    fin = np.isfinite(np.asarray(b, np.float64))
    bmax = float(np.abs(np.asarray(b)[fin]).max()) if fin.any() else 0.0
    tol = rel * ((X @ W.T).max(1) + bmax)
    return (np.asarray(best) - np.asarray(second)) <= tol


# --------------------------------------------------------------------------- folds and grid search
def stratified_folds(y, n_splits=5):
    """Test-fold ids of the unshuffled stratified k-fold, written sample by sample: classes in
    order of first appearance; fold i's share of class k is what dealing the sorted labels
    round-robin gives it; the samples of a class go to the folds in ascending fold order."""
    y = list(np.asarray(y).reshape(-1))
    seen = []
    for v in y:
        if v not in seen:
            seen.append(v)
    enc = [seen.index(v) for v in y]
    order = sorted(enc)
    share = [[0] * len(seen) for _ in range(n_splits)]
    for pos, k in enumerate(order):
        share[pos % n_splits][k] += 1
    out = np.zeros(len(y), np.uint8)
    for k in range(len(seen)):
        seq = [f for f in range(n_splits) for _ in range(share[f][k])]
        for j, i in enumerate(i for i, e in enumerate(enc) if e == k):
            out[i] = seq[j]
    return out


def grid_search(X, y, alphas=ALPHAS, n_splits=5, n_classes=None, tol=1e-4, max_iter=5000):
    """Returns dict(best, best_alpha, cv [A, n_splits], mean, std (mean, scale), W, b of the refit,
    and per fold the held-out rows' predictions / best / second per alpha with that fold's
    standardised rows and weights, for the near-tie band)."""
    X = np.asarray(X, np.float64)
    y = np.asarray(y)
    L = int(n_classes) if n_classes is not None else int(y.max()) + 1
    folds = stratified_folds(y, n_splits)
    cv = np.zeros((len(alphas), n_splits))
    per_fold = []
    for f in range(n_splits):
        tr = folds != f
        mean, scale = scaler(X[tr])
        xs = standardize(X, mean, scale)
        W, b, n_iter = fit(xs, y, alphas, L, tol, max_iter, mask=tr)
        held = np.flatnonzero(~tr)
        rec = []
        for a in range(len(alphas)):
            pred, best, second = predict(xs[held], W[a], b[a])
            cv[a, f] = np.mean(pred == y[held]) if len(held) else 0.0
            rec.append(dict(pred=pred, band=margin_band(xs[held], W[a], b[a], best, second)))
        per_fold.append(dict(held=held, n_iter=n_iter, alphas=rec))
    best = int(np.argmax(cv.mean(1)))
    mean, scale = scaler(X)
    W, b, n_iter = fit(standardize(X, mean, scale), y, [alphas[best]], L, tol, max_iter)
    return dict(best=best, best_alpha=float(alphas[best]), cv=cv, folds=folds, per_fold=per_fold, mean=mean,
                scale=scale, W=W[0], b=b[0], n_iter=n_iter)


def blobs(n_classes, D, per_class, sep, seed, n_eval):
    """Gaussian blobs with well-separated class means: (Xtrain f32, ytrain, Xeval f32, yeval),
    `per_class` training rows per class (a sequence gives unequal sizes) in shuffled order."""
    rng = np.random.default_rng(seed)
    means = sep * rng.standard_normal((n_classes, D))
    per = np.broadcast_to(np.asarray(per_class), (n_classes,))
    ytr = rng.permutation(np.repeat(np.arange(n_classes), per))
    Xtr = (means[ytr] + rng.standard_normal((len(ytr), D)) + 3.0).astype(np.float32)
    yev = rng.integers(0, n_classes, n_eval)
    Xev = (means[yev] + rng.standard_normal((n_eval, D)) + 3.0).astype(np.float32)
    return Xtr, ytr, Xev, yev
