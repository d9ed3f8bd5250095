"""GPU checks of the linear probe (csrc/linear_probe.hip, hvamd.linear_probe) against the float64
restatement tests/linear_probe_ref.py.

The f32 bound used throughout is the project's f32-MFMA figure, 1e-5 sum |a b| per dot product
(simpleshot_ref.margin_band's derivation: 30 x the 1.5e-7 sum |a b| of an f32 accumulation, applied
twice).  Propagated through the loss and gradient (`grad_bound`):

    |dz_ir|  <= 1e-5 (sum_k |x_ik w_rk| + |b_r|)                       the forward product
    |dr_ir|  <= |dz_ir| / 4 + 1e-6                                     |sigma'| <= 1/4; f32 sigma, |r| <= 1
    |ddW_rk| <= (1/N) sum_i (|dr_ir| |x_ik| + 1e-5 |r_ir x_ik|) + 1e-5 alpha_r |w_rk|
    |ddb_r|  <= (1/N) sum_i (|dr_ir| + 1e-5 |r_ir|)

Tile sizes of the kernels: 64 rows x 64 classes x 32 columns forward, 64 classes x 64 columns x 32
rows backward, row chunks of at most 8192 rows; the shapes below sit on both sides of each."""
import warnings

import numpy as np
import pytest
import torch

import linear_probe_ref as ref

pytestmark = pytest.mark.gpu

SHAPES = [(1, 4, 2), (67, 5, 3), (67, 100, 37), (300, 768, 130), (8193, 8, 577)]


def _problem(N, D, R, seed=0, w_scale=1.0, per_row_alpha=False):
    rng = np.random.default_rng(seed + 7 * N + D)
    L = R // 3 if per_row_alpha else R
    X = rng.standard_normal((N, D)).astype(np.float32)
    y = rng.integers(0, L, N)
    W = (w_scale * rng.standard_normal((R, D)) / np.sqrt(D)).astype(np.float32)
    b = (w_scale * rng.standard_normal(R)).astype(np.float32)
    if per_row_alpha:
        target = np.tile(np.arange(L), 3).astype(np.int32)
        alpha = np.repeat(np.float32([1e-4, 1e-2, 1.0]), L)
    else:
        target = np.arange(R, dtype=np.int32)
        alpha = np.full(R, 1e-2, np.float32)
    return X, y, W, b, target, alpha


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def grad_bound(X, y, W, b, target, alpha, mask=None):
    """(bound dW, bound db) of the module docstring, at float64."""
    X64, W64 = np.abs(np.asarray(X, np.float64)), np.abs(np.asarray(W, np.float64))
    keep = np.ones(len(X), bool) if mask is None else np.asarray(mask, bool)
    n = max(int(keep.sum()), 1)
    dz = 1e-5 * (X64 @ W64.T + np.abs(np.asarray(b, np.float64)))
    dr = (dz / 4 + 1e-6) * keep[:, None]
    z = ref.scores(X, W, b)
    r = np.abs(1 / (1 + np.exp(-z)) - (np.asarray(y)[:, None] == np.asarray(target)[None, :])) * keep[:, None]
    bw = (dr.T @ X64 + 1e-5 * (r.T @ X64)) / n + 1e-5 * np.asarray(alpha, np.float64)[:, None] * W64
    return bw, (dr.sum(0) + 1e-5 * r.sum(0)) / n


def _check_loss_grad(X, y, W, b, target, alpha, fold=None, skip=None):
    import hvamd.ops as ops
    mask = None if fold is None else fold != skip
    dX, dy, dW_, db_, dt, da = _dev(X, y.astype(np.int64), W, b, target, alpha)
    dfold = None if fold is None else torch.from_numpy(fold).cuda()
    got = ops.lp_loss_grad(dX, dy, dW_, db_, dt, da, fold=dfold, skip_fold=-1 if skip is None else skip)
    again = ops.lp_loss_grad(dX, dy, dW_, db_, dt, da, fold=dfold, skip_fold=-1 if skip is None else skip)
    assert all(torch.equal(a, c) for a, c in zip(got, again))  # determinism: the same bits
    gW, gb, loss, _ = ref.loss_grad(X, y, W, b, target, alpha, mask)
    bw, bb = grad_bound(X, y, W, b, target, alpha, mask)
    eW = np.abs(got[0].cpu().numpy().astype(np.float64) - gW)
    eb = np.abs(got[1].cpu().numpy().astype(np.float64) - gb)
    el = np.abs(got[2].cpu().numpy() - loss) / np.abs(loss)
    print(f"loss_grad N {X.shape[0]} D {X.shape[1]} R {len(b)}: dW err/bound {np.max(eW / bw):.3g}, "
          f"db err/bound {np.max(eb / bb):.3g}, loss rel {el.max():.3g}")
    assert np.isfinite(got[0].cpu().numpy()).all() and np.isfinite(got[2].cpu().numpy()).all()
    assert (eW <= bw).all() and (eb <= bb).all()
    assert el.max() <= 1e-6


# --------------------------------------------------------------------------- scaler
@pytest.mark.parametrize("B,D", [(1, 4), (67, 5), (67, 100), (300, 768)])
def test_moments_and_standardize_match_float64(B, D):
    """Against float64, rtol 1e-5 (test_prepare_matches_float64's figure, 12 x an f32 row
    operation's rounding) on mean, scale and on the output relative to its operands' size
    (|x| + |mean|) / scale: x - mean cancels, so the result itself is no scale.  Dense and strided
    inputs and any batch split give the same bits; a constant column gets scale 1."""
    from hvamd import linear_probe
    g = torch.Generator().manual_seed(B * 1000 + D)
    x = 2.0 + 0.5 * torch.randn(B, D, generator=g)
    x[:, D - 1] = 0.25  # zero variance
    buf = torch.full((B, D + 12), 7e4, device="cuda")
    view = buf[:, :D]
    view.copy_(x)
    sc = linear_probe.StandardScaler().fit(view)
    dense = linear_probe.StandardScaler().fit(x.cuda())
    assert torch.equal(sc._sum, dense._sum) and torch.equal(sc._sumsq, dense._sumsq)
    split = linear_probe.StandardScaler()
    for lo, hi in ((0, B // 3), (B // 3, B // 3), (B // 3, B)):
        split.partial_fit(x[lo:hi].cuda())
    split.finalize()
    assert torch.equal(sc._sum, split._sum) and torch.equal(sc._sumsq, split._sumsq)
    assert sc.n_samples_seen_ == split.n_samples_seen_ == B
    mean, scale = ref.scaler(x.numpy())
    if B == 1:
        assert (scale == 1).all()
    assert scale[D - 1] == 1.0 and float(sc.scale_[D - 1]) == 1.0 and float(sc.var_[D - 1]) == 0.0
    assert np.abs(sc.mean_.cpu().numpy() - mean).max() <= 1e-5 * np.abs(mean).max()
    assert (np.abs(sc.scale_.cpu().numpy() - scale) <= 1e-5 * scale).all()
    out = sc.transform(view)
    assert out.dtype == torch.float32 and out.shape == (B, D) and out.is_contiguous()
    assert torch.equal(out, sc.transform(x.cuda()))
    want = ref.standardize(x.numpy(), mean, scale)
    size = (np.abs(x.numpy().astype(np.float64)) + np.abs(mean)) / scale
    assert (np.abs(out.cpu().numpy() - want) <= 1e-5 * size).all()


# --------------------------------------------------------------------------- loss and gradient
@pytest.mark.parametrize("N,D,R", SHAPES)
@pytest.mark.parametrize("at", ["random", "zero"])
def test_loss_grad_matches_float64(N, D, R, at):
    """dW and db within `grad_bound` (module docstring) elementwise, loss rtol 1e-6 (float64 sums
    of f32 terms), at W of scale 1 and at W = 0; two calls give the same bits."""
    X, y, W, b, target, alpha = _problem(N, D, R, w_scale=1.0 if at == "random" else 0.0)
    _check_loss_grad(X, y, W, b, target, alpha)


@pytest.mark.parametrize("N,D,R", [(67, 100, 37), (300, 768, 130), (8193, 8, 577)])
def test_loss_grad_with_a_fold_mask(N, D, R):
    """Rows of the held-out fold contribute nothing and are not counted; rows 64 .. 191 (two whole
    row tiles, where there are that many) are masked entirely."""
    X, y, W, b, target, alpha = _problem(N, D, R, seed=1)
    fold = (np.arange(N) % 5).astype(np.uint8)
    fold[64:192] = 3
    _check_loss_grad(X, y, W, b, target, alpha, fold, 3)


def test_loss_grad_three_alphas_per_class():
    """R = 3 L with a penalty per row: the three grid values of a fold in one call."""
    X, y, W, b, target, alpha = _problem(131, 20, 3 * 23, seed=2, per_row_alpha=True)
    _check_loss_grad(X, y, W, b, target, alpha)


def test_loss_grad_saturated_scores_stay_finite():
    """|z| about 80: sigma and softplus go through exp(-|z|), so loss and gradient are finite and
    within the same bounds."""
    X, y, W, b, target, alpha = _problem(67, 8, 5, seed=3)
    X[:, 0] = np.where(np.arange(67) % 2 == 0, 10.0, -10.0)
    W[:, 0] = 8.0
    z = ref.scores(X, W, b)
    assert np.abs(z).max() > 80 and np.abs(z).min() > 60
    _check_loss_grad(X, y, W, b, target, alpha)


def test_workspace_does_not_grow_with_rows():
    from hvamd import _lib
    lib = _lib.load()
    assert lib.hvk_lp_loss_grad_workspace(8192, 768, 130) == lib.hvk_lp_loss_grad_workspace(10 ** 6, 768, 130) > 0
    assert lib.hvk_lp_loss_grad_workspace(64, 768, 130) < lib.hvk_lp_loss_grad_workspace(8192, 768, 130)


# --------------------------------------------------------------------------- solver
def _run_steps(X, y, target, alpha, step, n_iter, tol=0.0, frozen=None):
    import hvamd.ops as ops
    R, D = len(target), X.shape[1]
    dX, dy, dt, da = _dev(X, y.astype(np.int64), target, alpha)
    W, Yw = torch.zeros(R, D, device="cuda"), torch.zeros(R, D, device="cuda")
    b, Yb, t = torch.zeros(R, device="cuda"), torch.zeros(R, device="cuda"), torch.ones(R, device="cuda")
    gmax = torch.zeros(R, device="cuda")
    conv = torch.zeros(R, dtype=torch.uint8, device="cuda")
    fz = None if frozen is None else torch.from_numpy(frozen.astype(np.uint8)).cuda()
    for _ in range(n_iter):
        g = ops.lp_loss_grad(dX, dy, Yw, Yb, dt, da, check_labels=False)
        ops.lp_step(W, b, Yw, Yb, g[0], g[1], t, step, tol, gmax, conv, frozen=fz)
    return W.cpu().numpy(), b.cpu().numpy(), t.cpu().numpy(), conv.cpu().numpy()


@pytest.mark.parametrize("N,D,R,per_row", [(300, 64, 130, False), (131, 20, 111, True)])
def test_step_follows_the_float64_recurrence(N, D, R, per_row):
    """50 iterations from zero against the float64 recurrence: |W - W64| <= 1e-3 max |W64_r| per
    row.  Growth: one iteration perturbs the iterate by step x the gradient bound, e, about 1e-7 of
    the row's scale; a gradient step of length 1 / Lip does not expand differences and the
    extrapolation multiplies them by at most 1 + 2 beta < 3, so differences add up no faster than
    k (k + 1) / 2 e = 1.3e-4 at k = 50.  A restart decision may differ only where the float64
    restart dot product is within (k + 1) 1e-5 sum |g| |x+ - x| of 0 at some iteration k (the
    dot-product bound on the accumulated difference); such rows, at most 2 %, are excluded."""
    X, y, _, _, target, alpha = _problem(N, D, R, seed=4, per_row_alpha=per_row)
    step = 1.0 / (0.25 * ref.lipschitz_lambda(X) + float(alpha.max()))
    frozen = np.zeros(R, bool)
    frozen[5] = True  # left untouched
    want = ref.solve(X, y, target, alpha, step, 50, frozen=frozen)
    W, b, t, conv = _run_steps(X, y, target, alpha, step, 50, frozen=frozen)
    k = np.arange(1, 51)[:, None]
    near = (np.abs(want["dots"]) <= k * 1e-5 * want["dots_abs"]).any(0) & ~frozen
    print(f"step R {R}: rows near a restart tie {int(near.sum())}")
    assert near.sum() <= 0.02 * R
    ok = ~near
    scale = np.abs(want["W"]).max(1, keepdims=True)
    err = np.abs(W - want["W"]) / np.maximum(scale, 1e-30)
    print(f"step R {R}: max row-relative error {err[ok & ~frozen].max():.3g}")
    assert (err[ok & ~frozen] <= 1e-3).all()
    assert (np.abs(b - want["b"])[ok] <= 1e-3 * np.maximum(np.abs(want["b"][ok]), scale[ok, 0])).all()
    assert np.allclose(t[ok], want["t"][ok], rtol=1e-5)
    assert (W[5] == 0).all() and b[5] == 0 and t[5] == 1 and conv[5] == 0


@pytest.fixture(scope="module")
def fitted(golden):
    """The fixture's "wide" case fitted once on the device with all three alphas."""
    from hvamd import linear_probe
    g = golden("linear_probe_golden")
    case = "wide"
    L, D = int(g[f"{case}.n_classes"]), int(g[f"{case}.D"])
    Xtr, ytr, Xev, yev = ref.blobs(L, D, g[f"{case}.per_class"], float(g[f"{case}.sep"]), int(g[f"{case}.seed"]),
                                   int(g[f"{case}.n_eval"]))
    assert np.array_equal(ytr, g[f"{case}.ytrain"])
    sc = linear_probe.StandardScaler().fit(torch.from_numpy(Xtr).cuda())
    xs = sc.transform(torch.from_numpy(Xtr).cuda())
    clf = linear_probe.LogisticOvR(ref.ALPHAS, tol=1e-4, n_classes=L).fit(xs, torch.from_numpy(ytr).cuda())
    return dict(clf=clf, xs=xs.cpu().numpy(), y=ytr, L=L, sc=sc, Xev=Xev, yev=yev)


def test_fit_converges_to_a_small_float64_gradient(fitted):
    """The float64 gradient at the returned (coef_, intercept_) is <= tol + `grad_bound`, every
    problem converged, before max_iter."""
    clf, xs, y, L = fitted["clf"], fitted["xs"], fitted["y"], fitted["L"]
    print("fit iterations (3 alphas in lock-step):", clf.n_iter_)
    assert bool(clf.converged_.all()) and clf.n_iter_ < clf.max_iter and bool(clf.fitted_.all())
    W = clf.coef_.cpu().numpy().reshape(3 * L, -1)
    b = clf.intercept_.cpu().numpy().reshape(-1)
    target, alpha = np.tile(np.arange(L), 3), np.repeat(np.float32(ref.ALPHAS), L)
    gW, gb, _, _ = ref.loss_grad(xs, y, W, b, target, alpha)
    bw, bb = grad_bound(xs, y, W, b, target, alpha)
    print(f"float64 gradient at the solution: max |dW| {np.abs(gW).max():.3g}, max |db| {np.abs(gb).max():.3g}")
    assert (np.abs(gW) <= 1e-4 + bw).all() and (np.abs(gb) <= 1e-4 + bb).all()


def test_decision_function_and_predict_match_float64(fitted):
    """For the device's own W: scores within 1e-5 (sum |x w| + |b|); predictions equal outside
    the near-tie band, which holds at most 2 % of the rows."""
    clf, sc = fitted["clf"], fitted["sc"]
    xe = sc.transform(torch.from_numpy(fitted["Xev"]).cuda())
    z = clf.decision_function(xe).cpu().numpy()
    pred = clf.predict(xe).cpu().numpy()
    xe = xe.cpu().numpy()
    for a in range(3):
        W, b = clf.coef_[a].cpu().numpy(), clf.intercept_[a].cpu().numpy()
        want = ref.scores(xe, W, b)
        assert (np.abs(z[a] - want) <= 1e-5 * (np.abs(xe).astype(np.float64) @ np.abs(W).T + np.abs(b))).all()
        p, best, second = ref.predict(xe, W, b)
        band = ref.margin_band(xe, W, b, best, second)
        assert band.mean() <= 0.02
        assert np.array_equal(pred[a][~band], p[~band])


def test_classes_without_rows_are_not_fitted():
    """A class with no row: coef_ 0, intercept_ -inf, never predicted; a class absent from one
    training fold does not stall grid_search."""
    from hvamd import linear_probe
    Xtr, ytr, Xev, _ = ref.blobs(5, 7, 12, 1.5, 11, 40)
    ytr = np.where(ytr == 2, 4, ytr)  # class 2 is empty, n_classes stays 6
    xs = linear_probe.StandardScaler().fit(torch.from_numpy(Xtr).cuda()).transform(torch.from_numpy(Xtr).cuda())
    clf = linear_probe.LogisticOvR(1e-2, n_classes=6).fit(xs, torch.from_numpy(ytr).cuda())
    assert clf.fitted_.tolist() == [True, True, False, True, True, False]
    for c in (2, 5):
        assert float(clf.intercept_[c]) == float("-inf") and not bool(clf.coef_[c].any())
    assert bool(clf.converged_.all()) and clf.n_iter_ < clf.max_iter
    pred = clf.predict(torch.from_numpy(Xev).cuda())
    assert not bool(((pred == 2) | (pred == 5)).any())
    assert bool((clf.decision_function(xs)[:, 2] == float("-inf")).all())
    # one row of class 5: in four of the five folds' training parts, absent from the fifth
    Xtr[0] += 4.0
    ytr[0] = 5
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        pipe, best, cv = linear_probe.grid_search(torch.from_numpy(Xtr).cuda(), torch.from_numpy(ytr).cuda(),
                                                  n_classes=6)
    assert cv.shape == (3, 5) and np.isfinite(cv).all() and max(pipe.cv_n_iter_) < 5000
    assert bool(pipe.clf.fitted_[5]) and not bool(pipe.clf.fitted_[2])


@pytest.mark.parametrize("case", ["small", "wide"])
def test_grid_search_on_the_fixture(golden, case):
    """cv_scores against the float64 restatement within the near-tie band per held-out row;
    best_alpha equal unless two mean scores differ by less than one held-out row; test accuracy >=
    the lowest recorded accuracy of the reference's pipeline."""
    from hvamd import linear_probe
    g = golden("linear_probe_golden")
    L, D = int(g[f"{case}.n_classes"]), int(g[f"{case}.D"])
    Xtr, ytr, Xev, yev = ref.blobs(L, D, g[f"{case}.per_class"], float(g[f"{case}.sep"]), int(g[f"{case}.seed"]),
                                   int(g[f"{case}.n_eval"]))
    want = ref.grid_search(Xtr, ytr, n_classes=L)
    assert np.array_equal(want["cv"], g[f"{case}.restatement_cv"])
    pipe, best_alpha, cv = linear_probe.grid_search(torch.from_numpy(Xtr).cuda(), torch.from_numpy(ytr).cuda(),
                                                    n_classes=L)
    print(case, "iterations per fold", pipe.cv_n_iter_, "refit", pipe.clf.n_iter_, "restatement",
          [f["n_iter"] for f in want["per_fold"]], want["n_iter"])
    print(case, "cv (device)", cv.mean(1), "cv (float64)", want["cv"].mean(1))
    n_min = min(len(f["held"]) for f in want["per_fold"])
    for f, rec in enumerate(want["per_fold"]):
        n = len(rec["held"])
        for a in range(3):
            assert abs(cv[a, f] - want["cv"][a, f]) * n <= rec["alphas"][a]["band"].sum() + 1e-9, (a, f)
    means = np.sort(want["cv"].mean(1))[::-1]
    if means[0] - means[1] >= 1.0 / (5 * n_min):
        assert best_alpha == want["best_alpha"]
    acc = float((pipe.predict(torch.from_numpy(Xev).cuda()).cpu().numpy() == yev).mean())
    print(case, "test accuracy", acc, "reference", g[f"{case}.ref_acc"], "restatement", float(g[f"{case}.restatement_acc"]))
    assert acc >= g[f"{case}.ref_acc"].min()


# --------------------------------------------------------------------------- end to end
MINI = dict(img_size=32, embed_dim=32, depths=[2, 2], num_heads=[1, 2], window_size=4, drop_path_rate=0.0)
MEAN = [0.463 * 255, 0.480 * 255, 0.376 * 255]
STD = [0.209 * 255, 0.200 * 255, 0.231 * 255]
N_LEAVES = 6


def _u8_batches(sizes, seed):
    gen = torch.Generator().manual_seed(seed)
    pattern = torch.randint(0, 256, (N_LEAVES, 3, 32, 32), generator=torch.Generator().manual_seed(99)).float()
    out = []
    for n in sizes:
        leaf = torch.randint(0, N_LEAVES, (n,), generator=gen)
        noise = torch.randint(0, 256, (n, 3, 32, 32), generator=gen).float()
        out.append(((0.7 * pattern[leaf] + 0.3 * noise).round().clamp(0, 255).to(torch.uint8).cuda(), leaf.cuda()))
    return out


def test_evaluate_mini_swinv2_equals_the_slow_way():
    """linear_probe.evaluate on the mini SwinV2 of the SimpleShot test (32 x 32 uint8 batches, the
    NormalizationFn folded into the patch gather) gives the metrics of features extracted batch by
    batch with the normalisation applied per batch and fed to grid_search directly."""
    from hvamd import configs, linear_probe, models
    from hvamd.data import NormalizationFn
    torch.manual_seed(0)
    cfg = configs.Config()
    cfg.model.name = "swinv2_tiny_window7_224"
    cfg.model.variant = "linear-probe"
    model = models.build_model(cfg, 2, **MINI).cuda()
    norm = NormalizationFn(MEAN, STD)
    train, evalb = _u8_batches((32, 32, 16), 41), _u8_batches((16, 7), 42)
    tree_dists = (torch.arange(N_LEAVES)[:, None] - torch.arange(N_LEAVES)[None, :]).abs().to(torch.uint8)
    flags = [m.training for m in model.modules()]
    out = linear_probe.evaluate(cfg, model, train, evalb, tree_dists=tree_dists, n_splits=3, device_transforms=norm)
    assert set(out) == {"acc@1", "tree-dist", "best-alpha", "cv-scores"}
    assert [m.training for m in model.modules()] == flags and model.backbone.patch_embed.input_norm is None
    assert out["cv-scores"].shape == (3, 3) and out["best-alpha"] in ref.ALPHAS

    def feats(batches):
        model.eval()
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            f = torch.cat([model(norm(b)[0]).float() for b in batches])
        return f, torch.cat([b[1] for b in batches])
    Xtr, ytr = feats(train)
    Xev, yev = feats(evalb)
    pipe, best, cv = linear_probe.grid_search(Xtr, ytr, n_splits=3, n_classes=N_LEAVES)
    pred = pipe.predict(Xev)
    assert out["best-alpha"] == best and np.array_equal(out["cv-scores"], cv)
    assert out["acc@1"] == float((pred == yev).double().mean())
    assert out["tree-dist"] == float(tree_dists.cuda()[pred, yev].double().mean())
    cfg.model.variant = "simpleshot"
    with pytest.raises(AssertionError):
        linear_probe.evaluate(cfg, model, train, evalb)
