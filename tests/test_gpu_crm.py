"""CRM decoding (hvk_tree_dist_matrix, hvk_crm_predict, EvalMetrics(decoding="crm")) on the GPU
against float64 numpy: p = softmax(z), r = p @ D.T, argmin.  A row whose two lowest risks lie
within 1e-5 * D.max() (30 x the f32 MFMA's 1.5e-7 * sum|ab| bound on two compared scores, sum|ab| =
risk <= D.max(); the rule of simpleshot_ref.margin_band) is left out of the prediction check, and
every case asserts that at most 2 % of its rows are."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BAND = 1e-5
SIZES = {17: (2, 3, 5, 7, 11, 13, 17), 333: (2, 3, 5, 9, 30, 100, 333), 400: (2, 4, 8, 20, 50, 150, 400),
         10000: (3, 13, 51, 273, 1103, 4884, 10000)}


def _paths(L):
    """int32 [L, 7] of the synthetic tree: the parent of node i at tier t is i * n_{t-1} // n_t."""
    p = np.zeros((L, 7), np.int64)
    p[:, 6] = np.arange(L)
    for t in range(5, -1, -1):
        p[:, t] = p[:, t + 1] * SIZES[L][t] // SIZES[L][t + 1]
    return p.astype(np.int32)


@functools.lru_cache(maxsize=None)
def _matrix(kind, L):
    if kind == "tree":  # hierarchy.build_tree_dist_matrix's rule on the tier-id columns
        ids = _paths(L)
        d = np.full((L, L), 7, np.uint8)
        for lvl, t in enumerate(range(6, -1, -1)):
            d = np.where((ids[:, None, t] == ids[None, :, t]) & (d == 7), np.uint8(lvl), d)
        return d
    d = np.random.default_rng(L).integers(0, 256, (L, L)).astype(np.uint8)  # asymmetric
    np.fill_diagonal(d, 0)
    return d


def _softmax64(z):
    p = np.exp(z.astype(np.float64) - z.astype(np.float64).max(1, keepdims=True))
    return p / p.sum(1, keepdims=True)


def _check(z_dev, t, D_dev, r, state=None):
    """crm_predict on the device against the float64 risks r [B, L]; returns the count of band rows."""
    import hvamd.ops as ops
    if state is None:
        state = torch.zeros(16, dtype=torch.float64, device="cuda")
    pred, risk, dist = (x.cpu().numpy() for x in ops.crm_predict(z_dev, torch.from_numpy(t).cuda(), D_dev, state))
    dmax = float(D_dev.max())
    two = np.partition(r, 1, axis=1)[:, :2] if r.shape[1] > 1 else np.stack([r[:, 0], r[:, 0] + np.inf], 1)
    band = (two[:, 1] - two[:, 0]) <= BAND * dmax
    print(f"band rows {band.sum()} / {len(band)}, smallest gap {(two[:, 1] - two[:, 0]).min():.3g}, "
          f"risk error {np.abs(risk - r.min(1)).max():.3g} (bound {BAND * dmax:.3g})")
    assert band.mean() <= 0.02
    assert np.array_equal(pred[~band], r.argmin(1)[~band])
    assert np.abs(risk - r.min(1)).max() <= BAND * dmax
    return pred, dist, int(band.sum())


CASES = [(B, kind, L, dtype, False) for B in (1, 37, 130) for kind in ("tree", "random") for L in (17, 333, 400)
         for dtype in ("f32", "bf16")] + [(37, "random", L, "f32", True) for L in (17, 333, 400)]  # ld > L


@pytest.mark.parametrize("B,kind,L,dtype,padded", CASES)
def test_crm_predict_matches_float64(B, kind, L, dtype, padded):
    rng = np.random.default_rng(B + L)
    z = torch.from_numpy((2.0 * rng.standard_normal((B, L))).astype(np.float32))
    if dtype == "bf16":
        z = z.bfloat16()
    t = rng.integers(0, L, B)
    D = _matrix(kind, L)
    z_dev = z.cuda()
    if padded:
        z_dev = torch.full((B, L + 5), 7e4, device="cuda")[:, :L].copy_(z)
    r = _softmax64(z.float().numpy()) @ D.astype(np.float64).T
    pred, dist, _ = _check(z_dev, t, torch.from_numpy(D).cuda(), r)
    assert np.array_equal(dist, D[pred, t].astype(np.int32))


def test_equal_rows_lowest_class_wins():
    """Rows a < b of the matrix are equal and b lies in a later class tile: a wins on every row."""
    import hvamd.ops as ops
    L, B, a, b = 300, 37, 5, 200
    rng = np.random.default_rng(1)
    D = rng.integers(100, 256, (L, L)).astype(np.uint8)
    D[a] = D[b] = rng.integers(0, 20, L)  # risk_a = risk_b < 20 < 100 <= every other risk
    z = torch.from_numpy((2.0 * rng.standard_normal((B, L))).astype(np.float32)).cuda()
    pred = ops.crm_predict(z, torch.zeros(B, dtype=torch.int64, device="cuda"), torch.from_numpy(D).cuda(),
                           torch.zeros(16, dtype=torch.float64, device="cuda"))[0]
    assert (pred == a).all()
    with pytest.raises(ValueError):
        ops.crm_predict(z, torch.zeros(B, dtype=torch.int64, device="cuda"), torch.from_numpy(D).cuda().float(),
                        torch.zeros(16, dtype=torch.float64, device="cuda"))


def test_state_slots():
    from hvamd.hierarchy import EvalMetrics
    L = 333
    D = torch.from_numpy(_matrix("tree", L)).cuda()
    rng = np.random.default_rng(2)
    batches = []
    for B in (37, 130):
        t = torch.from_numpy(rng.integers(0, L, B))
        t[3] = L if B == 37 else -1  # one target outside [0, L) per batch
        batches.append((torch.from_numpy((2.0 * rng.standard_normal((B, L))).astype(np.float32)).cuda(), t.cuda()))
    states = []
    for _ in range(2):
        m = EvalMetrics(tree_dists=D, decoding="crm")
        hits = dsum = 0
        for z, t in batches:
            m.update(z, t)
            ok = (t >= 0) & (t < L)
            assert (m.crm_dist[~ok] == -1).all() and (m.crm_dist[ok] >= 0).all()
            hits += int((m.crm_pred[ok] == t[ok]).sum())
            dsum += int(m.crm_dist[ok].sum())
        assert m.state[13].item() == hits and m.state[14].item() == dsum and m.state[15].item() == 0
        states.append(m.state.clone())
    assert torch.equal(states[0], states[1])  # bit-identical from run to run
    m = EvalMetrics(tree_dists=D)
    m.update(*batches[0])
    assert (m.state[13:] == 0).all()
    with pytest.raises(ValueError):
        EvalMetrics(decoding="crm")


def test_tree_dist_matrix_matches_host_rule():
    import hvamd.ops as ops
    got = ops.tree_dist_matrix(torch.from_numpy(_paths(333)).cuda())
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), _matrix("tree", 333))


def test_workload_width():
    """L = 10 000 (the synthetic iNat21 tree), matrix built on the device.  The oracle is the closed
    form risk_k = 7 - sum_t P(ancestor_t(k)): the distance is the number of tiers at which two
    paths differ."""
    import hvamd.ops as ops
    L, B = 10000, 16
    paths = _paths(L)
    z = (2.0 * np.random.default_rng(5).standard_normal((B, L))).astype(np.float32)
    t = np.random.default_rng(6).integers(0, L, B)
    p = _softmax64(z)
    r = np.full((B, L), 7.0)
    for q in range(7):
        node = np.stack([np.bincount(paths[:, q], weights=p[b], minlength=SIZES[L][q]) for b in range(B)])
        r -= node[:, paths[:, q]]
    D = ops.tree_dist_matrix(torch.from_numpy(paths).cuda())
    pred, dist, n_band = _check(torch.from_numpy(z).cuda(), t, D, r)
    assert n_band == 0 and (pred != z.argmax(1)).any()  # not the argmax in disguise
    assert np.array_equal(dist, (paths[pred] != paths[t]).sum(1))


def test_eval_metrics_crm_end_to_end():
    from hvamd.hierarchy import EvalMetrics, Taxonomy, crm_predictions
    L = 333
    tax = Taxonomy.synthetic(SIZES[L])
    crm, plain = EvalMetrics(taxonomy=tax, decoding="crm"), EvalMetrics(taxonomy=tax)
    D = _matrix("tree", L)
    assert np.array_equal(D, (tax.leaf_paths[:, None] != tax.leaf_paths[None]).sum(2))  # the same tree
    rng = np.random.default_rng(3)
    hits = dsum = slack = n = 0
    for B in (37, 130):
        z = (2.0 * rng.standard_normal((B, L))).astype(np.float32)
        t = rng.integers(0, L, B)
        for m in (crm, plain):
            m.update([torch.zeros(B, 2, device="cuda"), torch.from_numpy(z).cuda()], torch.from_numpy(t).cuda())
        r = _softmax64(z) @ D.astype(np.float64).T
        two = np.partition(r, 1, axis=1)
        slack += int(((two[:, 1] - two[:, 0]) <= BAND * 7).sum())
        hits += int((r.argmin(1) == t).sum())
        dsum += int(D[r.argmin(1), t].sum())
        n += B
        assert torch.equal(crm_predictions(torch.from_numpy(z).cuda(), torch.from_numpy(D).cuda()),
                           crm.crm_pred.long())
    got, old = crm.compute(), plain.compute()
    assert abs(got["acc@1/crm"] - hits / n) <= slack / n and abs(got["tree-dist/crm"] - dsum / n) <= slack / n
    assert set(got) == set(old) | {"acc@1/crm", "tree-dist/crm"}
    assert all(got[k] == old[k] for k in old)
