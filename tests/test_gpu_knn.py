"""hvk_knn_topk / hvk_knn_vote / hvamd.knn on the GPU against the float64 restatement of
tests/knn_ref.py, on the same bf16-rounded inputs.  No row is excluded: every check is a tolerance
statement that holds for every row.  u = 2^-24.
tol (top-k): products of bf16 inputs are exact in f32, so a score's error is that of adding D exact
terms in f32 in some order; each addition rounds a partial sum of magnitude <= sum |q_i b_i| <=
||q|| ||b|| (Cauchy-Schwarz) by at most u of it: |s - s64| <= D u ||q|| ||b||_max, in any order.
tol_v (vote), relative to sum w: a weight is exp(a), a = (s_i - s_0) * (1 / temperature), |a| <=
2 / temperature.  The subtraction, the f32 temperature, its reciprocal and the product each round by
u, so exp(a) is off by 4 u |a| relatively, plus 2 u for expf; a vote of up to k terms summed in f32
adds k u.  A vote is within e = (8 / temperature + 2 + k) u sum w of its float64 value, and the
argmax of the f32 votes has a float64 vote within 2 e sum w of the largest."""
import functools

import numpy as np
import pytest
import torch

import knn_ref as ref
import simpleshot_ref as ss_ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
TEMP = 0.07
SHAPES = [(1, 5, 8, 20), (67, 111, 104, 5), (64, 1800, 104, 200), (130, 2000, 768, 20), (3, 300, 1024, 256)]


class Case:
    """Tree-shaped features as unit bf16 rows, the float64 scores, the kernel's (sims, idx): computed once."""

    def __init__(self, shape):
        import hvamd.ops as ops
        self.B, self.N, self.D, self.k = shape
        leaves = -(-self.N // 3)
        self.sizes = tuple(min(s, leaves) for s in (3, 6, 12, 24, 48, 96)) + (leaves,)
        Xtr, ytr, Xev, _ = ss_ref.hierarchical_data(self.sizes, self.D, sum(shape), n_eval=self.B)
        self.bank, self.q = ref.unit_rows_bf16(Xtr[:self.N]), ref.unit_rows_bf16(Xev)
        self.labels = ytr[:self.N].astype(np.int32)
        self.S = self.q.astype(np.float64) @ self.bank.astype(np.float64).T
        norm = lambda a: np.sqrt((a.astype(np.float64) ** 2).sum(1))  # noqa: E731
        self.tol = self.D * U * norm(self.q) * norm(self.bank).max()  # per row
        self.q_dev = torch.from_numpy(self.q).cuda().bfloat16()
        self.bank_dev = torch.from_numpy(self.bank).cuda().bfloat16()
        self.labels_dev = torch.from_numpy(self.labels).cuda()
        self.sims_dev, self.idx_dev = ops.knn_topk(self.q_dev, self.bank_dev, self.k)
        self.sims, self.idx = self.sims_dev.cpu().numpy(), self.idx_dev.cpu().numpy()


@functools.lru_cache(maxsize=None)
def case(shape):
    return Case(shape)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_topk_every_row_within_the_f32_bound(shape):
    c = case(shape)
    n = min(c.N, c.k)
    assert c.sims.shape == c.idx.shape == (c.B, c.k) and c.sims.dtype == np.float32 and c.idx.dtype == np.int32
    assert np.isneginf(c.sims[:, n:]).all() and (c.idx[:, n:] == -1).all()  # exactly (-inf, -1) past N
    for r in range(c.B):
        s, i = c.sims[r, :n].astype(np.float64), c.idx[r, :n]
        assert i.min() >= 0 and i.max() < c.N and len(set(i.tolist())) == n, r
        assert ((s[:-1] > s[1:]) | ((s[:-1] == s[1:]) & (i[:-1] < i[1:]))).all(), r
        assert (np.abs(s - c.S[r, i]) <= c.tol[r]).all(), (r, np.abs(s - c.S[r, i]).max(), c.tol[r])
        rest = np.delete(c.S[r], i)
        assert rest.size == 0 or rest.max() <= c.S[r, i].min() + 2 * c.tol[r], r


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_any_number_of_splits_gives_the_same_bits(shape):
    import hvamd.ops as ops
    c = case(shape)
    for splits in (1, 3, 7):
        sims, idx = ops.knn_topk(c.q_dev, c.bank_dev, c.k, splits=splits)
        assert torch.equal(sims, c.sims_dev) and torch.equal(idx, c.idx_dev), splits


def test_exact_ties_return_the_lower_indices_first():
    """Bank rows 0 .. 39 (and 50, 56, ..., 284: 80 copies over five tiles) are one vector: a query
    along it gets the lowest indices in order, at one similarity, for any splits."""
    import hvamd.ops as ops
    bank = ref.unit_rows_bf16(np.random.default_rng(7).standard_normal((300, 104)))
    bank[:40] = bank[0]
    bank[50:290:6] = bank[0]
    q = torch.from_numpy(bank[:1]).cuda().bfloat16()
    for splits in (0, 1, 3):
        sims, idx = ops.knn_topk(q, torch.from_numpy(bank).cuda().bfloat16(), 20, splits=splits)
        assert idx[0].tolist() == list(range(20)) and (sims[0] == sims[0, 0]).all(), splits
    sims, idx = ops.knn_topk(q, torch.from_numpy(bank).cuda().bfloat16(), 60, splits=3)
    assert idx[0].tolist() == list(range(40)) + list(range(50, 170, 6))


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_vote_within_the_f32_bound_of_the_largest_vote(shape):
    """From the kernel's own (sims, idx): the leaf and the node chosen at every tier carry a float64 vote within
    tol_v sum w of the largest, every row and k_j; a path of the tree; k_j = 1: the nearest neighbour's labels."""
    import hvamd.ops as ops
    c = case(shape)
    ks = sorted({1, min(c.k, 3), min(c.k, 10), c.k})
    leaf, path = (t.cpu().numpy() for t in ops.knn_vote(c.sims_dev, c.idx_dev, c.labels_dev, ks, TEMP))
    assert leaf.shape == (len(ks), c.B) and path.shape == (len(ks), c.B, 7)
    flat_leaf, flat_path = ops.knn_vote(c.sims_dev, c.idx_dev, c.labels_dev[:, -1].contiguous(), ks, TEMP)
    assert np.array_equal(flat_leaf.cpu().numpy(), leaf) and torch.equal(flat_path[:, :, 0], flat_leaf)  # T = 1
    lookups = ss_ref.tree_sizes_lookup(c.sizes)
    for t, vec in enumerate(lookups):
        assert np.array_equal(vec.astype(np.int64)[path[:, :, t + 1]], path[:, :, t]), t
    assert np.array_equal(leaf[0], c.labels[c.idx[:, 0], -1]) and np.array_equal(path[0], c.labels[c.idx[:, 0]])
    for j, kj in enumerate(ks):
        tol_v = 2 * (8 / TEMP + 2 + kj) * U
        for r in range(c.B):
            w = ref.weights(c.sims[r], c.idx[r], TEMP)[:kj]
            valid = c.idx[r, :kj] >= 0
            lab = np.where(valid[:, None], c.labels[np.where(valid, c.idx[r, :kj], 0)], -1)
            v = ref.votes(w, lab[:, -1])
            assert v[leaf[j, r]] >= max(v.values()) - tol_v * w.sum(), (kj, r)
            mask = np.ones(kj, bool)
            for t in range(7):
                v = ref.votes(w, lab[:, t], mask)
                assert v[path[j, r, t]] >= max(v.values()) - tol_v * w.sum(), (kj, r, t)
                mask = lab[:, t] == path[j, r, t]


def test_evaluate_finds_every_row_as_its_own_nearest_neighbour():
    """knn.evaluate on a mini SwinV2, the evaluation batches also the bank, k = [1]: every row's nearest
    neighbour is itself and every accuracy 1.  The reference checks on the bank that the second
    neighbour is farther than the rounding: S[r, r] beats every other score by more than 2 tol."""
    from hvamd import configs, knn, models
    from hvamd.data import NormalizationFn
    torch.manual_seed(0)
    cfg = configs.Config()
    cfg.model.name, cfg.model.variant, cfg.knn.k = "swinv2_tiny_window7_224", "knn", [1]
    model = models.build_model(cfg, 2, img_size=32, embed_dim=32, depths=[2, 2], num_heads=[1, 2], window_size=4,
                               drop_path_rate=0.0).cuda()
    sizes = (2, 3, 4, 5, 6, 7, 12)
    paths = torch.from_numpy(ss_ref.leaf_paths(sizes))
    gen = torch.Generator().manual_seed(5)
    norm = NormalizationFn([0.463 * 255, 0.480 * 255, 0.376 * 255], [0.209 * 255, 0.200 * 255, 0.231 * 255])
    # 128 coarse 4 x 4 block images; an untrained network maps many to nearly parallel features, and
    # bf16 rounding moves a unit row's squared norm by up to 2^-8: keep 13 whose f32 cosines are < 0.98
    x = torch.randint(0, 256, (128, 3, 4, 4), generator=gen).repeat_interleave(8, 2).repeat_interleave(8, 3)
    x, y = x.to(torch.uint8).cuda(), paths[torch.randint(0, 12, (128,), generator=gen)].cuda()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        cos = torch.nn.functional.normalize(model(norm((x, y))[0]).float(), dim=1)
    cos = (cos @ cos.T).cpu()
    keep = []
    for i in range(128):
        if len(keep) < 13 and all(cos[i, j] < 0.98 for j in keep):
            keep.append(i)
    assert len(keep) == 13, len(keep)
    batches = [(x[keep[:8]], y[keep[:8]]), (x[keep[8:]], y[keep[8:]])]
    model.train()
    flags = [m.training for m in model.modules()]
    out = knn.evaluate(cfg, model, batches, batches, device_transforms=norm)
    assert [m.training for m in model.modules()] == flags and model.backbone.patch_embed.input_norm is None
    keys = {"acc@1"} | {f"acc@1/tier{t}" for t in range(7)}
    assert set(out) == keys | {k.replace("acc@1", "acc@1/k1") for k in keys}
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):  # the reference, on the same bank
        feats = torch.cat([model(norm(b)[0]) for b in batches])
    clf = knn.KNeighbors(k=1).fit(feats, torch.cat([b[1] for b in batches]))
    bank = clf._bank[:clf.n_].float().cpu().numpy().astype(np.float64)
    S = bank @ bank.T
    tol = bank.shape[1] * U * np.sqrt((bank * bank).sum(1)).max() ** 2
    other = S - np.diag(np.full(len(S), np.inf))
    assert (np.diag(S) - other.max(1) > 2 * tol).all(), (np.diag(S) - other.max(1)).min()
    assert all(v == 1.0 for v in out.values()), out
    assert clf.predict(feats).shape == (13, 7) and torch.equal(clf.kneighbors(feats)[1][:, 0].cpu(), torch.arange(13).int())
