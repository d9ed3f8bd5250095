"""hvk_backoff_decode against the float64 restatement of backoff_ref.py, as intervals.

The band, from the kernel's summation order (u = 2^-24):
* a leaf's term fl(expf(fl(z - M))) has relative error <= (|z - M| + 2) u: the subtraction's rounding
  u |z - M| passes through the exponential, expf is within 1 ulp = 2 u.  E = max |z - M| + 2.
* a node of w children puts at most a(w) additions on any term: w for w <= 16 (one lane, serial),
  ceil(w / 64) + 6 above it (a lane's strided partial sum, then the 6-step butterfly).  Every
  addition of non-negatives adds at most u, so the mass of a node has relative error <= (E + A) u,
  A = the sum over the 7 levels (tiers 5 .. 0 and the root) of the largest a(w) of the level.
* prob = S(n) / S(root), one correctly rounded division: (2 E + 2 A + 1) u.
REL is twice that.  Two sibling masses each carry (E + A) u, so the chosen child's true mass is at
least (1 - REL) times the best sibling's, and a depth read from prob lies between the true depths at
tau (1 +- REL).  Measured on an MI355X over all cases: worst |prob - q| at 2.3 % of the band."""
import functools

import numpy as np
import pytest
import torch

import backoff_ref as ref

pytestmark = pytest.mark.gpu

TREES = {"narrow": (1, 2, 3, 5, 9, 17, 131), "wide-leaves": (1, 2, 3, 4, 5, 6, 1000),
         "wide-slots": (1, 1, 2, 3, 3, 200, 1500), "shuffled": (1, 2, 3, 5, 9, 17, 131)}
THRESHOLDS = (0.05, 0.3, 0.5, 0.9)


@functools.lru_cache(maxsize=None)
def _tax(tree):
    from hvamd.hierarchy import Taxonomy
    tax = Taxonomy.synthetic(TREES.get(tree, tree))
    if tree == "shuffled":  # new leading numbers: another sorted() order, so perm is not the identity
        order = np.random.default_rng(7).permutation(tax.num_leaves)
        tax = Taxonomy([f"{order[i]:05d}_" + c.split("_", 1)[1] for i, c in enumerate(tax.classes)])
        assert not tax.identity_perm
    return tax


@functools.lru_cache(maxsize=None)
def _case(tree, dtype, B):
    """(logits rounded to the dtype, targets, the float64 node masses): shared, never written."""
    tax, rng = _tax(tree), np.random.default_rng(B + len(str(tree)))
    z = torch.from_numpy(3 * rng.standard_normal((B, tax.num_leaves))).to(torch.bfloat16 if dtype == "bf16" else torch.float32)
    t = rng.integers(0, tax.num_leaves, B)
    return z, t, ref.node_masses(ref.softmax(z.double().numpy()), tax.leaf_paths)


def _rel(tax, z):
    rank_off, lo, hi = tax.soft_tables()[:3]
    w = hi.astype(np.int64) - lo
    adds = np.where(w <= 16, w, -(-w // 64) + 6)
    A = sum(adds[rank_off[t]:rank_off[t + 1]].max() for t in range(7))
    zf = z[np.isfinite(z)]
    return 2 * (2 * (zf.max() - zf.min() + 2) + 2 * A + 1) * 2.0 ** -24


def _decode(tax, logits, targets, thresholds=THRESHOLDS):
    from hvamd.hierarchy import BackoffMetrics
    m = BackoffMetrics(tax, thresholds).cuda()
    m.update(logits, torch.as_tensor(targets).cuda())
    return m, m.path.cpu().numpy(), m.prob.cpu().numpy(), m.match.cpu().numpy(), m.state.cpu().numpy()


def _check(tax, z, t, masses, out):
    """Checks 1-5 of one batch; returns the worst |prob - q| over its band."""
    _, path, prob, match, state = out
    rel = _rel(tax, z)
    q = np.stack([masses[d][np.arange(len(t)), path[:, d]] for d in range(7)], 1)  # true masses along the path
    for b in range(len(t)):
        for d in range(7):
            kids = ref.children(tax.leaf_paths, tax.perm, d, path[b, d - 1] if d else None)
            top = kids[np.argmax(masses[d][b, kids])]
            assert path[b, d] in kids
            assert path[b, d] == top or q[b, d] >= (1 - rel) * masses[d][b, top], (b, d)  # check 2
    worst = float((np.abs(prob - q) / (rel * q)).max())
    assert worst <= 1, worst  # check 1
    for tau in THRESHOLDS:  # check 3
        D = ref.depth(prob, np.float32(tau))
        assert (ref.depth(q, tau * (1 + rel)) <= D).all() and (D <= ref.depth(q, tau * (1 - rel))).all()
    assert np.array_equal(match, ref.agreement(path, tax.leaf_paths[t]))  # check 5
    assert np.array_equal(state, ref.fold(path, prob, match, THRESHOLDS)) and state[0] == len(t) and state[1] == 0
    return worst


@pytest.mark.parametrize("layout", ["contiguous", "view"])
@pytest.mark.parametrize("B", [1, 37])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("tree", list(TREES))
def test_backoff_matches_float64(tree, dtype, B, layout):
    tax, (z, t, masses) = _tax(tree), _case(tree, dtype, B)
    x = z.cuda()
    if layout == "view":  # ld > L, rows that start off a 16-byte boundary, padding that would win any maximum
        buf = torch.full((B, z.shape[1] + 8), 1e4, dtype=z.dtype, device="cuda")
        x = buf[:, 3:3 + z.shape[1]]
        x.copy_(z)
    worst = _check(tax, z.double().numpy(), t, masses, _decode(tax, x, t))
    print(f"backoff {tree} {dtype} B={B} {layout}: worst |prob - q| / band = {worst:.3f}")


def test_more_slots_than_64_kb_of_lds_and_two_runs_bit_identical():
    """8706 slots are 68 KB of dynamic LDS, and one family of 8700 genera: the widest slot path."""
    sizes = (1, 1, 1, 1, 1, 8700, 8800)
    z, t, masses = _case(sizes, "f32", 1)
    a, b = (_decode(_tax(sizes), z.cuda(), t) for _ in range(2))
    _check(_tax(sizes), z.double().numpy(), t, masses, a)
    assert all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))


def test_uniform_logits_follow_the_largest_subtree():
    tax, L = _tax("narrow"), 131
    want, q = ref.greedy(ref.node_masses(np.full((1, L), 1 / L), tax.leaf_paths), tax.leaf_paths, tax.perm)
    count = np.array([(tax.leaf_paths[:, d] == want[0, d]).sum() for d in range(7)])
    ratios = np.unique(np.r_[0.0, count / L, 1.0])
    th = tuple((ratios[:-1] + ratios[1:]) / 2)  # midway between the masses the path takes, and one below them all
    m, path, prob, match, state = _decode(tax, torch.zeros(2, L).cuda(), [int(want[0, 6]), (int(want[0, 6]) + 1) % L], th)
    assert np.array_equal(path, np.repeat(want, 2, 0)) and match[0] == 7
    assert np.array_equal(prob[0], count.astype(np.float32) / np.float32(L)) and np.array_equal(prob[0], prob[1])
    assert [state[2 + 5 * j] for j in range(len(th))] == [2 * int((count / L >= tau).sum()) for tau in th]
    got = m.compute()  # depth 7 at the lowest threshold; only the first row's target is the greedy leaf
    assert [got[f"backoff/{k}@{th[0]:g}"] for k in ("depth", "acc", "hP", "hR", "leaf-coverage", "leaf-acc")] == [
        7, 0.5, (7 + match[1]) / 14, (7 + match[1]) / 14, 1, 0.5]


def test_one_dominant_leaf_and_invalid_targets():
    """Depth 7 at 0.99 with the leaf's path; targets L and -1 are counted and left out of every sum."""
    tax = _tax("shuffled")
    z = torch.full((3, tax.num_leaves), -30.0)
    z[:, 77] = 0
    m, path, prob, match, state = _decode(tax, z.cuda(), [77, tax.num_leaves, -1], (0.99,))
    assert (path == tax.leaf_paths[77]).all() and match.tolist() == [7, -1, -1] and (prob[:, 6] >= 0.99).all()
    assert state.tolist() == [1, 2, 7, 1, 7, 1, 1]
    from hvamd.hierarchy import backoff_predictions
    pred = backoff_predictions([None, z.cuda()], tax, 0.99)  # a list: its finest tier
    assert pred["depth"].tolist() == [7, 7, 7] and np.array_equal(pred["path"].cpu().numpy(), path)
    with pytest.raises(ValueError, match="2 target"):
        m.compute()


def test_nan_logits_count_as_minus_infinity():
    tax, (z, t, _) = _tax("wide-leaves"), _case("wide-leaves", "f32", 37)
    z = z[:2]
    hole = torch.zeros_like(z, dtype=torch.bool)
    hole[0, z[0].argmax()] = hole[0, ::7] = True
    hole[1] = True  # a row of NaNs alone: no mass anywhere
    a = _decode(tax, z.masked_fill(hole, float("nan")).cuda(), t[:2])
    b = _decode(tax, z.masked_fill(hole, float("-inf")).cuda(), t[:2])
    assert all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:])) and (a[2][0] > 0).all()
    assert not a[2][1].any() and a[4][2] == (a[2][0] >= np.float32(0.05)).sum()  # the NaN row stops at the root


def test_trainer_eval_with_backoff_on_the_mini_hxe_model():
    from test_gpu_eval_metrics import _composer_model, _trainer, _u8_batches, _f32_batch
    model, tax, _ = _composer_model("hxe")
    tr, batches = _trainer(model), [_f32_batch(b) for b in _u8_batches(tax, (8, 8, 5), 21)]
    out = tr.eval(batches, metrics={"eval": model.fused_metrics(), "backoff": model.backoff_metrics()})
    assert out["eval"] == tr.eval(batches, metrics=model.fused_metrics())
    hand = model.eval().backoff_metrics()
    for b in batches:
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            hand.update(model(b), b[1])
    same = lambda d: {k: v for k, v in d.items() if v == v}  # noqa: E731  (NaN: an empty denominator)
    assert hand.state[0] == 21 and len(out["backoff"]) == 42 and same(out["backoff"]) == same(hand.compute())
    with pytest.raises(ValueError, match="taxonomy"):
        type(model)(model.module, {}, {}, None).backoff_metrics()
