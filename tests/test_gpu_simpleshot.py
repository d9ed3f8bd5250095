"""hvk_ss_* / hvamd.simpleshot on the GPU against the numpy float64 restatement of
tests/simpleshot_ref.py.

Predictions are compared under the near-tie rule of simpleshot_ref.margin_band: f32 cannot be
asked for a float64 argmin where best and second-best squared distance differ by no more than
1e-5 (||x||^2 + max ||c||^2) -- 30 times the f32 MFMA's error bound of about 1.5e-7 sum |a b| per
dot product, applied twice -- so those rows (at most 2 %, asserted) are excluded and every other
row must agree.  The data follows the tree: every tier-t node adds a normal offset of scale 0.5^t,
samples add normal noise of 0.6, 3 training rows per leaf."""
import functools

import numpy as np
import pytest
import torch

import simpleshot_ref as ref

pytestmark = pytest.mark.gpu

# name -> (tree sizes, D, seed, evaluation rows)
TREES = {"tiny": ((1, 1, 1, 1, 1, 1, 2), 4, 1, 1), "small": ((2, 3, 5, 8, 13, 21, 37), 100, 2, 67),
         "wide": ((3, 6, 12, 24, 48, 96, 400), 768, 3, 300), "wave": ((2, 2, 2, 2, 2, 4, 600), 100, 4, 200),
         "inat": ((3, 13, 51, 273, 1103, 4884, 10000), 768, 5, 256)}
MAX_EXCLUDED = 0.02


class Case:
    """The data of one tree on the host and the device, and the oracle's fit (computed once)."""

    def __init__(self, name):
        self.sizes, self.D, seed, n_eval = TREES[name]
        self.Xtr, self.ytr, self.Xev, self.yev = ref.hierarchical_data(self.sizes, self.D, seed, n_eval=n_eval)
        self.lookups = ref.tree_sizes_lookup(self.sizes)
        self.tiers = ref.fit_tiers_sized(self.Xtr, self.ytr, self.sizes)
        self.max_cnorm = max(float((m * m).sum(1).max()) for m, _ in self.tiers)

    @functools.cached_property
    def tree_oracle(self):
        return ref.predict_tree(self.Xev, self.tiers, self.lookups)

    @functools.cached_property
    def flat_oracle(self):
        return ref.predict_flat(self.Xev, *self.tiers[-1])

    @functools.cached_property
    def dev(self):
        return tuple(torch.from_numpy(a).cuda() for a in (self.Xtr, self.ytr, self.Xev, self.yev))

    @functools.cached_property
    def tree_clf(self):
        from hvamd import simpleshot
        Xtr, ytr, _, _ = self.dev
        return simpleshot.HierarchicalNearestCentroid(self.lookups).fit(Xtr, ytr)

    @functools.cached_property
    def flat_clf(self):
        from hvamd import simpleshot
        Xtr, ytr, _, _ = self.dev
        clf = simpleshot.NearestCentroid(n_classes=self.sizes[-1])
        for i in range(0, len(Xtr), 8192):
            clf.partial_fit(Xtr[i:i + 8192], ytr[i:i + 8192, -1])
        return clf.finalize()


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


def _close(got, want, rtol):
    return bool((np.abs(got - want) <= rtol * np.abs(want)).all())


# --------------------------------------------------------------------------- prepare
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,D", [(1, 4), (67, 100), (5, 768)])
@pytest.mark.parametrize("centered,l2n", [(False, False), (True, False), (False, True), (True, True)])
def test_prepare_matches_float64(centered, l2n, B, D, dtype):
    """rtol 1e-5 = 12 x the (log2 D + 2) 2^-24 bound of a tree-shaped f32 row sum at D = 768;
    positive-mean inputs (1 + 0.3 normal), so the mean has no cancellation; the rows sit in a
    wider buffer (ld > D)."""
    import hvamd.ops as ops
    g = torch.Generator().manual_seed(B * 1000 + D)
    x = (1 + 0.3 * torch.randn(B, D, generator=g)).to(dtype)
    buf = torch.full((B, D + 12), 7e4, dtype=dtype, device="cuda")
    view = buf[:, :D]
    view.copy_(x)
    assert B == 1 or view.stride(0) > D
    got = ops.ss_prepare(view, centered=centered, l2_normalized=l2n)
    assert got.dtype == torch.float32 and got.shape == (B, D) and got.is_contiguous()
    want = ref.prepare(x.float().numpy(), centered, l2n)
    assert _close(got.cpu().numpy().astype(np.float64), want, 1e-5)
    assert torch.equal(got, ops.ss_prepare(x.cuda(), centered=centered, l2_normalized=l2n))  # dense == strided
    if centered and not l2n:
        from hvamd import simpleshot
        assert torch.equal(got, simpleshot.center(view))
    if l2n and not centered:
        from hvamd import simpleshot
        assert torch.equal(got, simpleshot.l2_normalize(view))


def test_prepare_zero_mean_and_zero_norm_follow_ieee():
    import hvamd.ops as ops
    x = torch.tensor([[1.0, -1.0, 2.0, -2.0], [0.0, 0.0, 0.0, 0.0], [1.0, 2.0, 3.0, 4.0]])
    for flags in ((True, False), (False, True), (True, True)):
        got = ops.ss_prepare(x.cuda(), *flags).cpu().numpy()
        want = ref.prepare(x.numpy(), *flags)
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want))
        assert np.array_equal(np.sign(got[np.isinf(got)]), np.sign(want[np.isinf(want)]))
        assert _close(got[2].astype(np.float64), want[2], 1e-5)
    assert ops.ss_prepare(torch.zeros(0, 8, device="cuda"), True, True).shape == (0, 8)


# --------------------------------------------------------------------------- fit
@pytest.mark.parametrize("name", ["small", "wide"])
def test_fit_centroids_counts_and_upper_tiers(name):
    """Every tier's centroids against the per-tier float64 means (each tier averaged by its own
    label column, as the reference does) at rtol 2e-7 -- one f32 rounding of a float64 mean is
    6e-8 -- counts exact, cnorm the squared norm of the f32 centroid (rtol 1e-5, as prepare)."""
    c = case(name)
    clf = c.tree_clf
    assert len(clf.centroids_) == len(clf.counts_) == 7
    for t, (means, counts) in enumerate(c.tiers):
        got = clf.centroids_[t].cpu().numpy()
        assert got.dtype == np.float32 and got.shape == means.shape
        assert _close(got.astype(np.float64), means, 2e-7), t
        assert np.array_equal(clf.counts_[t].cpu().numpy(), counts)
        cn = clf._tier(clf._cnorm, t).cpu().numpy().astype(np.float64)
        assert _close(cn, (got.astype(np.float64) ** 2).sum(1), 1e-5)
    flat = c.flat_clf
    assert torch.equal(flat.centroids_, clf.centroids_[-1]) and torch.equal(flat.counts_, clf.counts_[-1])
    assert flat.invalid_ == 0 and clf.invalid_ == 0


def test_fit_twice_is_bit_identical_and_batch_splits_do_not_matter():
    """300 rows in one call and as batches of 1 + 67 + 232 leave bit-identical sums."""
    from hvamd import simpleshot
    c = case("wide")
    X, y = c.dev[0][:300], c.dev[1][:300]
    a = simpleshot.HierarchicalNearestCentroid(c.lookups).fit(X, y)
    b = simpleshot.HierarchicalNearestCentroid(c.lookups).fit(X, y)
    s = simpleshot.HierarchicalNearestCentroid(c.lookups)
    for lo, hi in ((0, 1), (1, 68), (68, 300)):
        s.partial_fit(X[lo:hi], y[lo:hi])
    s.finalize()
    for other in (b, s):
        assert torch.equal(a._sums, other._sums) and torch.equal(a._counts, other._counts)
        assert torch.equal(a._cent, other._cent) and torch.equal(a._cnorm, other._cnorm)
    assert a._state.tolist() == s._state.tolist() == [300.0, 0.0, 0.0, 0.0]
    f1 = simpleshot.NearestCentroid(n_classes=400).fit(X, y[:, -1])
    f2 = simpleshot.NearestCentroid(n_classes=400)
    for lo, hi in ((0, 1), (1, 68), (68, 300)):
        f2.partial_fit(X[lo:hi], y[lo:hi, -1])
    assert torch.equal(f1._sums, f2._sums) and torch.equal(f1._sums, a._sums[-400:])
    # finalize may be repeated, and more rows added after it
    a.finalize()
    assert torch.equal(a._cent, b._cent)
    # the class count taken from the labels
    g = simpleshot.NearestCentroid().fit(X, y[:, -1])
    assert g.tier_sizes[0] == int(y[:, -1].max()) + 1 and torch.equal(g._sums, f1._sums[:g.tier_sizes[0]])


def test_fit_skips_and_counts_labels_outside_the_range():
    from hvamd import simpleshot
    c = case("small")
    L = c.sizes[-1]
    X, y = c.dev[0], c.dev[1][:, -1].clone()
    bad = [5, 40]
    y[bad[0]], y[bad[1]] = -1, L
    keep = torch.ones(len(y), dtype=torch.bool, device="cuda")
    keep[bad] = False
    got = simpleshot.NearestCentroid(n_classes=L).fit(X, y)
    want = simpleshot.NearestCentroid(n_classes=L).fit(X[keep], y[keep])
    assert got.invalid_ == 2 and want.invalid_ == 0
    assert got._state.tolist() == [len(y) - 2.0, 2.0, 0.0, 0.0]
    assert torch.equal(got._sums, want._sums) and torch.equal(got._counts, want._counts)
    means, counts = ref.class_means(c.Xtr, y.cpu().numpy(), L)
    assert np.array_equal(got.counts_.cpu().numpy(), counts)
    assert _close(got.centroids_.cpu().numpy().astype(np.float64), means, 2e-7)


def test_empty_class_has_infinite_cnorm_and_is_never_predicted():
    from hvamd import simpleshot
    c = case("small")
    L, gone = c.sizes[-1], 11
    X, y, Xev, _ = c.dev
    keep = y[:, -1] != gone
    # the rows of the missing class themselves are the hardest queries
    Q = torch.cat([Xev, X[~keep], torch.zeros(1, c.D, device="cuda")])
    flat = simpleshot.NearestCentroid(n_classes=L).fit(X[keep], y[keep, -1])
    assert flat.counts_[gone] == 0 and torch.isinf(flat._cnorm[gone]) and flat._cnorm[gone] > 0
    assert torch.isfinite(flat._cnorm).sum() == L - 1 and not flat.centroids_[gone].any()
    p = flat.predict(Q)
    assert p.dtype == torch.int64 and not (p == gone).any()
    tree = simpleshot.HierarchicalNearestCentroid(c.lookups).fit(X[keep], y[keep])
    pt = tree.predict(Q)
    assert not (pt[:, -1] == gone).any()
    means, counts = ref.class_means(c.Xtr[keep.cpu().numpy()], c.ytr[keep.cpu().numpy(), -1], L)
    want, best, second = ref.predict_flat(Q.cpu().numpy(), means, counts)
    ok = ~ref.margin_band(Q.cpu().numpy(), best, second, c.max_cnorm)
    assert np.array_equal(p.cpu().numpy()[ok], want[ok])


# --------------------------------------------------------------------------- flat
def _flat_agrees(c, pred):
    want, best, second = c.flat_oracle
    band = ref.margin_band(c.Xev, best, second, float((c.tiers[-1][0] ** 2).sum(1).max()))
    assert band.mean() <= MAX_EXCLUDED, band.mean()
    got = pred.cpu().numpy()
    assert got.min() >= 0 and got.max() < c.sizes[-1]
    assert np.array_equal(got[~band], want[~band]), np.flatnonzero((got != want) & ~band)


@pytest.mark.parametrize("name", ["tiny", "small", "wide", "inat"])
def test_flat_predict_matches_oracle(name):
    """(B, L, D) = (1, 2, 4), (67, 37, 100), (300, 400, 768), (256, 10 000, 768)."""
    c = case(name)
    assert (len(c.Xev), c.sizes[-1], c.D) in ((1, 2, 4), (67, 37, 100), (300, 400, 768), (256, 10000, 768))
    clf = c.flat_clf
    pred = clf.predict(c.dev[2])
    assert pred.dtype == torch.int64 and pred.shape == (len(c.Xev),)
    _flat_agrees(c, pred)
    assert torch.equal(pred, clf.predict(c.dev[2]))  # run to run


def test_flat_lowest_index_wins_between_identical_centroids():
    import hvamd.ops as ops
    c = case("wide")
    clf = c.flat_clf
    cent, cnorm = clf.centroids_.clone(), clf._cnorm.clone()
    # across class splits; neighbouring lanes of one tile; one lane's two accumulators; first / last
    pairs = ((3, 70), (129, 130), (200, 216), (64, 399))
    for j, k in pairs:
        cent[k], cnorm[k] = cent[j], cnorm[j]
    Q = torch.cat([c.dev[2], cent[[j for j, _ in pairs]]])
    pred = ops.ss_predict_flat(Q, cent, cnorm)
    assert pred.dtype == torch.int32
    assert not any((pred == k).any() for _, k in pairs)
    assert pred[-len(pairs):].tolist() == [j for j, _ in pairs]


def test_flat_nan_row_does_not_fault_and_stays_in_range():
    c = case("wide")
    clf = c.flat_clf
    Q = c.dev[2].clone()
    Q[7] = float("nan")
    Q[100, 5] = float("nan")
    Q[200, ::2] = float("inf")
    pred = clf.predict(Q)
    torch.cuda.synchronize()
    assert pred.min() >= 0 and pred.max() < 400
    clean = torch.ones(len(Q), dtype=torch.bool, device="cuda")
    clean[[7, 100, 200]] = False
    assert torch.equal(pred[clean], clf.predict(c.dev[2])[clean])
    assert clf.predict(torch.zeros(0, c.D, device="cuda")).shape == (0,)


# --------------------------------------------------------------------------- tree
def _real_paths(c, pred):
    for t, vec in enumerate(c.lookups):
        assert np.array_equal(vec.astype(np.int64)[pred[:, t + 1]], pred[:, t]), t
    assert (pred >= 0).all() and (pred < np.array(c.sizes)[None, :]).all()


@pytest.mark.parametrize("name", ["tiny", "small", "wide", "wave", "inat"])
def test_tree_predict_matches_oracle(name):
    """Equal to the oracle's path for every row that is outside the band at every tier of the
    oracle's path; a real path (parent(pred[t + 1]) == pred[t]) for every row.  "wave": a tree
    (2, 2, 2, 2, 2, 4, 600) whose last-tier nodes have 150 children, more than a wave's lanes."""
    c = case(name)
    pred = c.tree_clf.predict(c.dev[2])
    assert pred.dtype == torch.int64 and pred.shape == (len(c.Xev), 7)
    got = pred.cpu().numpy()
    _real_paths(c, got)
    want, best, second = c.tree_oracle
    band = ref.margin_band(c.Xev, best, second, c.max_cnorm)
    assert band.mean() <= MAX_EXCLUDED, band.mean()
    assert np.array_equal(got[~band], want[~band]), np.flatnonzero((got != want).any(1) & ~band)
    assert torch.equal(pred, c.tree_clf.predict(c.dev[2]))


def test_tree_nan_row_is_still_a_path():
    c = case("small")
    Q = c.dev[2].clone()
    Q[3] = float("nan")
    pred = c.tree_clf.predict(Q).cpu().numpy()
    _real_paths(c, pred)
    assert c.tree_clf.predict(torch.zeros(0, c.D, device="cuda")).shape == (0, 7)


@pytest.mark.parametrize("name", ["small", "wide"])
def test_golden_predictions(golden, name):
    """The reference's HierarchicalNearestCentroid.fit / predict output and sklearn's flat
    NearestCentroid predictions on the fixture's inputs (no row of which is a near-tie:
    tests/golden/make_simpleshot_golden.py picks the seed so), exactly."""
    from hvamd import hierarchy, simpleshot
    g = golden("simpleshot_golden")
    sizes, D = tuple(int(v) for v in g[f"{name}.sizes"]), int(g[f"{name}.D"])
    Xtr, ytr, Xev, _ = ref.hierarchical_data(sizes, D, int(g[f"{name}.seed"]), n_eval=int(g[f"{name}.n_eval"]))
    Xtr, ytr, Xev = (torch.from_numpy(a).cuda() for a in (Xtr, ytr, Xev))
    clf = hierarchy.HierarchicalNearestCentroid(ref.tree_sizes_lookup(sizes)).fit(Xtr, ytr)
    assert np.array_equal(clf.predict(Xev).cpu().numpy(), g[f"{name}.tree_pred"])
    flat = simpleshot.NearestCentroid().fit(Xtr, ytr[:, -1])
    assert np.array_equal(flat.predict(Xev).cpu().numpy(), g[f"{name}.flat_pred"])
    for t in range(7):
        got = clf.centroids_[t].cpu().numpy().astype(np.float64).reshape(-1)[g[f"{name}.centroids{t}.idx"]]
        assert _close(got, g[f"{name}.centroids{t}"], 2e-7)


# --------------------------------------------------------------------------- end to end
MINI = dict(img_size=32, embed_dim=32, depths=[2, 2], num_heads=[1, 2], window_size=4, drop_path_rate=0.0)
MEAN = [0.463 * 255, 0.480 * 255, 0.376 * 255]
STD = [0.209 * 255, 0.200 * 255, 0.231 * 255]
SIZES = (2, 3, 4, 5, 6, 7, 12)


def _feature_model():
    from hvamd import configs, models
    torch.manual_seed(0)
    cfg = configs.Config()
    cfg.model.name = "swinv2_tiny_window7_224"
    cfg.model.variant = "simpleshot"
    model = models.build_model(cfg, 2, **MINI).cuda()
    assert isinstance(model, models.FeatureOnlyModel)
    # a fresh final LayerNorm makes every feature row's mean 0, which `centered` divides by:
    # a bias as a trained one, so that the row means are ordinary numbers
    with torch.no_grad():
        model.backbone.norm.bias.fill_(0.5)
    return cfg, model


def _u8_batches(sizes, seed):
    """32 x 32 uint8 images that depend on their class: a fixed pattern per leaf under noise."""
    gen = torch.Generator().manual_seed(seed)
    pattern = torch.randint(0, 256, (SIZES[-1], 3, 32, 32), generator=torch.Generator().manual_seed(99)).float()
    paths = torch.from_numpy(ref.leaf_paths(SIZES))
    out = []
    for b in sizes:
        leaf = torch.randint(0, SIZES[-1], (b,), generator=gen)
        noise = torch.randint(0, 256, (b, 3, 32, 32), generator=gen).float()
        x = (0.7 * pattern[leaf] + 0.3 * noise).round().clamp(0, 255).to(torch.uint8)
        out.append((x.cuda(), paths[leaf].cuda()))
    return out


@pytest.mark.parametrize("hier", [False, True], ids=["flat", "hierarchical"])
@pytest.mark.parametrize("centered,l2n", [(True, True), (False, False)], ids=["cl2n", "plain"])
def test_evaluate_mini_swinv2_against_the_oracle(hier, centered, l2n):
    """simpleshot.evaluate on a mini SwinV2 (32 x 32 uint8 images, 2 train batches, 2 eval batches
    with the last one smaller) against the oracle run on the features the same model produced.
    The NormalizationFn is folded into the patch embedding (hierarchical) or applied per batch
    (flat).  The returned numbers are exact sums over the rows, so they may differ from the
    oracle's by the rows inside the near-tie band only."""
    from hvamd import hierarchy, simpleshot
    from hvamd.data import NormalizationFn
    cfg, model = _feature_model()
    cfg.simpleshot.centered, cfg.simpleshot.l2_normalized, cfg.simpleshot.hierarchical = centered, l2n, hier
    norm = NormalizationFn(MEAN, STD)
    train, evalb = _u8_batches((16, 16), 31), _u8_batches((8, 5), 32)
    lookups = ref.tree_sizes_lookup(SIZES)
    tax = hierarchy.Taxonomy.synthetic(SIZES)
    assert np.array_equal(tax.leaf_paths, ref.leaf_paths(SIZES))
    tree_dists = hierarchy.build_tree_dist_matrix([hierarchy.HierarchicalLabel.parse(n) for n in tax.classes])
    model.train()  # found in training mode: left so
    before = [p.detach().clone() for p in model.parameters()]
    flags = [m.training for m in model.modules()]
    out = simpleshot.evaluate(cfg, model, train, evalb, lookup_vecs=lookups if hier else None,
                              tree_dists=tree_dists, device_transforms=norm if hier else (lambda b: norm(b)))
    keys = {"acc@1", "tree-dist"} | ({f"acc@1/tier{t}" for t in range(7)} if hier else set())
    assert set(out) == keys and all(isinstance(v, float) for v in out.values())
    assert [m.training for m in model.modules()] == flags
    assert all(torch.equal(p.detach(), b) for p, b in zip(model.parameters(), before))
    assert not any(p.requires_grad for p in model.parameters())
    assert model.backbone.patch_embed.input_norm is None
    # the oracle on the same features
    def feats(batches):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            f = torch.cat([model(norm(b)[0]) for b in batches])
        return ref.prepare(f.float().cpu().numpy(), centered, l2n), torch.cat([b[1] for b in batches]).cpu().numpy()
    Xtr, ytr = feats(train)
    Xev, yev = feats(evalb)
    n = len(yev)
    assert n == 13
    tiers = ref.fit_tiers_sized(Xtr, ytr, SIZES)
    cn = max(float((m * m).sum(1).max()) for m, _ in tiers)
    if hier:
        pred, best, second = ref.predict_tree(Xev, tiers, lookups)
        leaf = pred[:, -1]
    else:
        leaf, best, second = ref.predict_flat(Xev, *tiers[-1])
    slack = int(ref.margin_band(Xev, best, second, cn).sum())
    td = tree_dists.numpy().astype(np.float64)
    assert abs(out["acc@1"] - np.mean(leaf == yev[:, -1])) <= slack / n
    assert abs(out["tree-dist"] - td[leaf, yev[:, -1]].mean()) <= 7 * slack / n
    if hier:
        for t in range(7):
            assert abs(out[f"acc@1/tier{t}"] - np.mean(pred[:, t] == yev[:, t])) <= slack / n
        assert out["acc@1/tier6"] == out["acc@1"]
    assert slack <= 2, slack  # or the comparison above says little


def test_evaluate_without_tree_dists_or_eval_batches():
    """Flat with the class count unknown in advance (no tree_dists, no lookup_vecs): the labels
    decide it; no eval batches: NaN."""
    from hvamd import simpleshot
    cfg, model = _feature_model()
    norm_free = [(b[0].float() / 255 - 0.5, b[1][:, -1]) for b in _u8_batches((16, 16), 31)]
    out = simpleshot.evaluate(cfg, model, norm_free, [])
    assert set(out) == {"acc@1"} and np.isnan(out["acc@1"])
    out = simpleshot.evaluate(cfg, model, norm_free, norm_free[:1])
    assert 0.0 <= out["acc@1"] <= 1.0
