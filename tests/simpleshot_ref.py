"""numpy float64 restatement of SimpleShot (simpleshot.py:139-203) and of the top-down
nearest-centroid classifier (hierarchy.py:488-597), the reference of tests/test_simpleshot_cpu.py
and tests/test_gpu_simpleshot.py, written from the behaviour: conditioning of the features, class
means, the flat and the hierarchical prediction, and the near-tie band inside which an f32 kernel
is not asked to reproduce a float64 argmin."""
import numpy as np

N_TIERS = 7


def prepare(x, centered=False, l2_normalized=False):
    """x / mean(x) per row, then x / ||x||, in float64 (inf / NaN where numpy gives them)."""
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        if centered:
            x = x / x.mean(axis=1, keepdims=True)
        if l2_normalized:
            x = x / np.sqrt((x * x).sum(axis=1, keepdims=True))
    return x


def class_means(X, y, n_classes):
    """(means float64 [n_classes, D], counts [n_classes]); labels outside [0, n_classes) are
    skipped; a class without rows has a zero row and count 0."""
    X = np.asarray(X, np.float64)
    y = np.asarray(y).astype(np.int64)
    ok = (y >= 0) & (y < n_classes)
    X, y = X[ok], y[ok]
    order = np.argsort(y, kind="stable")  # a class's rows in their original order
    counts = np.bincount(y, minlength=n_classes)
    sums = np.zeros((n_classes, X.shape[1]))
    if len(y):
        present = np.flatnonzero(counts)
        starts = np.r_[0, np.cumsum(counts[present])[:-1]]
        sums[present] = np.add.reduceat(X[order], starts, axis=0)
    return sums / np.maximum(counts, 1)[:, None], counts


def fit_tiers(X, y):
    """Per-tier (means, counts) from [N, T] tier ids, each tier averaged by its own label column
    as the reference does; tier sizes are max id + 1 unless given by `fit_tiers_sized`."""
    y = np.asarray(y)
    return [class_means(X, y[:, t], int(y[:, t].max()) + 1) for t in range(y.shape[1])]


def fit_tiers_sized(X, y, sizes):
    y = np.asarray(y)
    return [class_means(X, y[:, t], sizes[t]) for t in range(y.shape[1])]


def sq_dists(X, C, expanded=None):
    """Squared euclidean distances [N, n] in float64: by differences, or (`expanded`; by default
    where the differences would take more than 2^25 elements) by ||x||^2 - 2 x.c + ||c||^2, one
    GEMM, whose cancellation in float64 is some 1e-13 of ||x||^2: nothing against the band."""
    X = np.asarray(X, np.float64)
    C = np.asarray(C, np.float64)
    if expanded is None:
        expanded = X.shape[0] * C.shape[0] * X.shape[1] > 1 << 25
    if expanded:
        return (X * X).sum(1)[:, None] - 2.0 * (X @ C.T) + (C * C).sum(1)[None, :]
    d = X[:, None, :] - C[None, :, :]
    return np.einsum("ncd,ncd->nc", d, d)


def _best_two(d, allowed):
    """(argmin, best, second best) of every row over the allowed columns ([N, n] bool or [n]);
    the lowest index wins ties; second is +inf with a single candidate."""
    d = np.where(allowed, d, np.inf)
    arg = d.argmin(axis=1)
    rows = np.arange(d.shape[0])
    best = d[rows, arg]
    rest = d.copy()
    rest[rows, arg] = np.inf
    return arg, best, rest.min(axis=1)


def predict_flat(X, means, counts, expanded=None):
    """(pred [N], best, second): nearest mean among the classes with rows."""
    d = sq_dists(X, means, expanded)
    return _best_two(d, (np.asarray(counts) > 0)[None, :])


def predict_tree(X, tiers, lookup_vecs):
    """Top-down: tier 0 among all nodes, tier t + 1 among the children (lookup_vecs[t][child] ==
    parent) of the node chosen at tier t; children without rows are skipped.  `tiers` is the list
    of (means, counts).  Returns (pred [N, T], best [N, T], second [N, T])."""
    N = len(X)
    T = len(tiers)
    pred = np.zeros((N, T), np.int64)
    best = np.zeros((N, T))
    second = np.zeros((N, T))
    for t, (means, counts) in enumerate(tiers):
        allowed = np.broadcast_to((np.asarray(counts) > 0)[None, :], (N, len(counts)))
        if t > 0:
            parent = np.asarray(lookup_vecs[t - 1]).astype(np.int64)
            allowed = allowed & (parent[None, :] == pred[:, t - 1][:, None])
        pred[:, t], best[:, t], second[:, t] = _best_two(sq_dists(X, means), allowed)
    return pred, best, second


def margin_band(X, best, second, max_cnorm, rel=1e-5):
    """Rows a float32 kernel is not asked to agree on: best and second-best squared distance
    differ by <= rel * (||x||^2 + max ||c||^2), at any tier when best / second are [N, T].
    rel = 1e-5 is 30 times the f32 MFMA's error bound of about 1.5e-7 sum |a b| per dot product,
    applied twice (two scores are compared)."""
    X = np.asarray(X, np.float64)
    tol = rel * ((X * X).sum(1) + max_cnorm)
    gap = np.asarray(second) - np.asarray(best)
    if gap.ndim == 2:
        return (gap <= tol[:, None]).any(axis=1)
    return gap <= tol


# --------------------------------------------------------------------------- test data
def tree_sizes_lookup(sizes):
    """Child -> parent vectors of the synthetic tree hvamd.hierarchy.Taxonomy.synthetic builds:
    the parent of node i of tier t + 1 is floor(i * n_t / n_{t+1})."""
    return [(np.arange(sizes[t + 1]) * sizes[t] // sizes[t + 1]).astype(np.uint16)
            for t in range(len(sizes) - 1)]


def leaf_paths(sizes):
    """[n_leaves, T] tier ids of every leaf of that tree."""
    vecs = tree_sizes_lookup(sizes)
    p = np.zeros((sizes[-1], len(sizes)), np.int64)
    p[:, -1] = np.arange(sizes[-1])
    for t in range(len(sizes) - 2, -1, -1):
        p[:, t] = vecs[t][p[:, t + 1]]
    return p


def hierarchical_data(sizes, D, seed, per_leaf=3, n_eval=None, noise=0.6):
    """Class means that follow the tree -- every tier-t node adds a normal offset of scale 0.5^t
    to its parent's -- and samples with normal noise: (Xtrain f32, ytrain [N, T], Xeval f32,
    yeval [M, T]), `per_leaf` training rows per leaf in shuffled order."""
    rng = np.random.default_rng(seed)
    paths = leaf_paths(sizes)
    mean = np.zeros((sizes[-1], D))
    for t, n in enumerate(sizes):
        mean += (0.5 ** t) * rng.standard_normal((n, D))[paths[:, t]]
    leaf = rng.permutation(np.repeat(np.arange(sizes[-1]), per_leaf))
    Xtr = (mean[leaf] + noise * rng.standard_normal((len(leaf), D))).astype(np.float32)
    n_eval = n_eval or sizes[-1]
    el = rng.integers(0, sizes[-1], n_eval)
    Xev = (mean[el] + noise * rng.standard_normal((n_eval, D))).astype(np.float32)
    return Xtr, paths[leaf], Xev, paths[el]
