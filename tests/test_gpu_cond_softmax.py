"""The conditional softmax (hvk_cond_softmax_fwd / _bwd / _decode) on the GPU against the float64
restatement of tests/cond_softmax_ref.py.

Error bands, derived from the kernels' summation orders (csrc/cond_softmax.hip), u = 2^-24, per row
and tier on the reference's magnitudes M = max|z_t|, A = the largest |group LSE| and n = the widest
group of the tier:
 * a group's max-shifted sum S: the loss's wave adds ceil(n / 64) terms a lane and folds 6 butterfly
   levels; the decoder's narrow path adds up to 32 terms in sequence, its wide path is the wave's.
   At most D(n) = 2 (ceil(n / 64) + min(n, 32)) + 6 operations touch a term (the 2: an add may sit
   behind one rescale), each an expf (2u), a product (u) and an add (u): 4 D u relative.  The
   exponents' roundings sum to at most u log n (test_gpu_joint_decode.py).  LSE = max + logf(S):
   logf 1 ulp of |log S| <= A + M, the add u A.  E_lse = u (4 D(n) + log n + 3 (A + M)).
 * loss term (LSE - z_y) + eps (z_y - mean): the differences round by u (A + M) and 2u M, the mean's
   sum (ceil(n / 64) + 6 adds) and quotient by (ceil(n / 64) + 7) u M, the fma by u |term|:
   E_term = E_lse + u (3 + eps (ceil(n / 64) + 10)) (A + M).  A row's loss is 7 fmas over the terms:
   sum_t lam_t E_term_t + 7u sum_t lam_t |term_t|; the f32 batch mean adds at most B u |loss|.
 * gradient lam_t / B ((p - hot) + (eps hot - eps / n)), p = expf(z - LSE): the exponent carries
   E_lse + u (A + M), expf 2u, the sums and products 6u at most, p <= 1:
   E_g = lam_t / B (E_lse + u (A + M) + 8u), plus one bf16 rounding 2^-9 |g| for a bf16 gradient.
 * decoder: c_t = (z - LSE) + c_{t-1}[parent], |c_t| <= C_t = sum_{q <= t} (A_q + M_q):
   e_t = e_{t-1} + E_lse_t + u (A_t + M_t) + u C_t, E_s = e_6.  Its lse over the L scores: a lane
   folds at most T = 32 ceil(n_5 / 256) + sum over the groups wider than 32 of ceil(n / 64) scores,
   then 6 butterfly levels and 3 wave merges: E_J = u (4 (2T + 9) + log L + 4 (|lse| + max|s|)).
Every test uses twice its band."""
import functools

import numpy as np
import pytest
import torch

import cond_softmax_ref as ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
TREES = {"small": (1, 2, 3, 5, 9, 17, 131), "shuffled": (1, 2, 3, 5, 9, 17, 131),
         "wide": (1, 1, 1, 1, 1, 2, 1500), "large": (3, 5, 11, 23, 47, 301, 2500)}
CONFIGS = {"plain": ((1,) * 7, 0.0), "smoothed": ((8, 5.65, 4, 2.82, 2, 1.41, 1), 0.1)}


@functools.lru_cache(maxsize=None)
def _tax(tree):
    from hvamd.hierarchy import Taxonomy
    tax = Taxonomy.synthetic(TREES[tree])
    if tree == "shuffled":  # new leading numbers: another sorted() order, so a non-identity sib_col
        order = np.random.default_rng(7).permutation(tax.num_leaves)
        tax = Taxonomy([f"{order[i]:05d}_" + c.split("_", 1)[1] for i, c in enumerate(tax.classes)])
        tax.sibling_tables()
        assert not tax.identity_siblings
    return tax


@functools.lru_cache(maxsize=None)
def _inputs(tree, dtype, B):
    """(the 7 tier logits rounded to the dtype, leaf targets)."""
    rng = np.random.default_rng(B + len(tree))
    dt = torch.bfloat16 if dtype == "bf16" else torch.float32
    zs = tuple(torch.from_numpy(3 * rng.standard_normal((B, n))).to(dt) for n in _tax(tree).num_classes)
    return zs, rng.integers(0, _tax(tree).num_leaves, B)


@functools.lru_cache(maxsize=None)
def _magnitudes(tree, dtype, B):
    """Per tier: (E_lse [B], A + M [B], the widest group n) of the module docstring."""
    out = []
    for z, par in zip(_inputs(tree, dtype, B)[0], ref.parent_ids(_tax(tree).leaf_paths)):
        z = z.double()
        lse, size = ref.group_lse(z, par)
        n, am = int(size.max()), (lse.abs().max(1).values + z.abs().max(1).values).numpy()
        D = 2 * (-(-n // 64) + min(n, 32)) + 6
        out.append((U * (4 * D + np.log(n) + 3 * am), am, n))
    return out


@functools.lru_cache(maxsize=None)
def _loss_ref(tree, dtype, B, cfg):
    zs, t = _inputs(tree, dtype, B)
    return ref.loss_and_grad([z.double() for z in zs], _tax(tree).leaf_paths, _tax(tree).leaf_paths[t], *CONFIGS[cfg])


@functools.lru_cache(maxsize=None)
def _decode_ref(tree, dtype, B):
    """float64 (log p [B, L], band [B] of scores and of lse / nll on top)."""
    zs, _ = _inputs(tree, dtype, B)
    logp = ref.leaf_logp([z.double() for z in zs], _tax(tree).leaf_paths).numpy()
    e = C = 0.0
    for e_lse, am, _ in _magnitudes(tree, dtype, B):
        C = C + am
        e = e + e_lse + U * am + U * C
    sizes = np.bincount(_tax(tree).leaf_paths[:, 5])
    T = 32 * -(-len(sizes) // 256) + sum(-(-s // 64) for s in sizes if s > 32)
    e_j = U * (4 * (2 * T + 9) + np.log(logp.shape[1]) + 4 * np.abs(logp).max(1))
    return logp, 2 * e, 2 * (e + e_j)


def _device_outputs(zs, layout, grad=False):
    if layout == "separate":
        return [z.cuda().requires_grad_(grad) for z in zs]
    total = sum(z.shape[1] for z in zs)  # column views of one padded buffer, ld > sum n_t
    buf = torch.full((zs[0].shape[0], total + 5), 7e4, dtype=zs[0].dtype, device="cuda")
    off = np.r_[0, np.cumsum([z.shape[1] for z in zs])]
    for z, a in zip(zs, off):
        buf[:, a:a + z.shape[1]] = z
    buf.requires_grad_(grad)
    return [buf[:, a:b] for a, b in zip(off, off[1:])]


def _tables(tree):
    tax = _tax(tree)
    parents, paths = tax.device_parent_tables("cuda")
    return (parents, *tax.device_sibling_tables("cuda")), paths


@pytest.mark.parametrize("B", [1, 37])
@pytest.mark.parametrize("cfg", list(CONFIGS))
@pytest.mark.parametrize("layout", ["separate", "views"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("tree", list(TREES))
def test_loss_and_gradient_match_float64(tree, dtype, layout, cfg, B):
    """Checks 1 and 2: the loss, its per-tier terms, the saved LSEs and the gradient within the
    bands; the gradient bit-exact zero outside the 7 target groups, on the pad columns and on only
    children; every active group's gradient sums to 0.  Measured on an MI355X over all cases, worst
    error / band: LSE 0.036, terms 0.046, mean loss 0.0062, f32 gradient 0.028, group sums 0.72; the
    bf16 gradient 0.97, its band being the bf16 rounding itself (half an ulp is 2^-8 = 2 * 2^-9)."""
    import hvamd.ops as ops
    zs, t = _inputs(tree, dtype, B)
    tax, (coeffs, eps) = _tax(tree), CONFIGS[cfg]
    y = tax.leaf_paths[t]
    outs = _device_outputs(zs, layout, grad=True)
    views = []
    outs[0].register_hook(views.append)  # the tier's gradient as the backward hands it over: a view
    loss, terms, lse = ops.cond_softmax_cross_entropy(outs, torch.from_numpy(y).cuda(), *_tables(tree)[0],
                                                      coeffs=coeffs, smoothing=eps, return_tiers=True)
    loss.backward()
    want, want_lse, want_terms, want_grads = _loss_ref(tree, dtype, B, cfg)
    mags = _magnitudes(tree, dtype, B)
    e_lse = np.stack([m[0] for m in mags], 1)
    e_term = e_lse + U * np.stack([(3 + eps * (-(-m[2] // 64) + 10)) * m[1] for m in mags], 1)
    lam = np.asarray(coeffs, np.float64)
    row_band = (lam * e_term).sum(1) + 7 * U * (lam * want_terms.abs().numpy()).sum(1)
    err = [np.abs(lse.cpu().double().numpy() - want_lse.numpy()) / (2 * e_lse),
           np.abs(terms.cpu().double().numpy() - want_terms.numpy()) / (2 * e_term + 2 * U * want_terms.abs().numpy()),
           np.abs(loss.item() - want.item()) / (2 * (row_band.mean() + B * U * abs(want.item())))]
    # the gradient: one buffer [B, ldg], every tier a column view of it
    full = views[0]._base
    off, n_el = np.r_[0, np.cumsum(tax.num_classes)], 8 if dtype == "bf16" else 4
    assert full.shape == (B, -(-off[7] // n_el) * n_el) and full.dtype == zs[0].dtype
    got = full.cpu().double().numpy()
    assert not got[:, off[7]:].any()  # pad columns
    active = np.concatenate([par[None, :] == (y[:, q - 1:q] if q else np.zeros((B, 1), int))
                             for q, par in enumerate(ref.parent_ids(tax.leaf_paths))], 1)
    assert not got[:, :off[7]][~active].any()  # bit-exact zero outside the target's 7 groups
    ref_g = torch.cat(want_grads, 1).numpy()
    e_g = np.concatenate([np.repeat((lam[t] / B * (m[0] + U * m[1] + 8 * U))[:, None], tax.num_classes[t], 1)
                          for t, m in enumerate(mags)], 1) + (2.0 ** -9 * np.abs(ref_g) if dtype == "bf16" else 0)
    err.append(np.abs(got[:, :off[7]] - ref_g) / (2 * e_g))
    for t in range(7):  # an active group's gradient sums to 0
        a = active[:, off[t]:off[t + 1]]
        err.append(np.abs((got[:, off[t]:off[t + 1]] * a).sum(1)) / (2 * (e_g[:, off[t]:off[t + 1]] * a).sum(1)))
        if a.sum(1).max() == 1:  # only children: log p = 0 and no gradient, exactly
            assert not terms[:, t].any() and not got[:, off[t]:off[t + 1]].any()
    print(f"worst error / band: lse {err[0].max():.3g}, terms {err[1].max():.3g}, loss {err[2]:.3g}, "
          f"gradient {err[3].max():.3g}, group sums {max(e.max() for e in err[4:]):.3g}")
    assert all((e <= 1).all() for e in err)
    for o, g in zip(outs, want_grads) if layout == "separate" else ():
        assert o.grad.shape == g.shape  # each tier received its view


def _decode(tree, dtype, B, layout="separate"):
    import hvamd.ops as ops
    zs, t = _inputs(tree, dtype, B)
    tables, paths = _tables(tree)
    state = torch.zeros(16, dtype=torch.float64, device="cuda")
    out = ops.cond_softmax_decode(_device_outputs(zs, layout), torch.from_numpy(t).cuda(), *tables, paths, state,
                                  topk=5, want_scores=True)
    return {k: v.cpu().numpy() for k, v in out.items()}, state.cpu().numpy(), t


@pytest.mark.parametrize("B", [1, 37])
@pytest.mark.parametrize("layout", ["separate", "views"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("tree", list(TREES))
def test_decode_matches_float64(tree, dtype, layout, B):
    """Check 3: scores, lse and NLL within the bands; prediction, rank and the state's sums as
    intervals under them; dist / tier_hit exact given pred; two runs bitwise equal.  Measured on an
    MI355X over all cases, worst error / band: scores 0.045, lse 0.0038, NLL 0.014."""
    got, state, t = _decode(tree, dtype, B, layout)
    again, state2, _ = _decode(tree, dtype, B, layout)
    assert all(np.array_equal(got[k], again[k], equal_nan=True) for k in got) and np.array_equal(state, state2)
    logp, band_s, band = _decode_ref(tree, dtype, B)
    rows, paths = np.arange(B), _tax(tree).leaf_paths
    err = np.abs(got["scores"].astype(np.float64) - logp).max(1) / band_s
    lse_err, nll_err = np.abs(got["lse"]) / band, np.abs(got["nll"] + logp[rows, t]) / band
    print(f"worst error / band: scores {err.max():.3g}, lse {lse_err.max():.3g}, nll {nll_err.max():.3g}; "
          f"smallest score band {band_s.min():.3g}")
    assert (err <= 1).all() and (lse_err <= 1).all() and (nll_err <= 1).all()
    assert (logp[rows, got["pred"]] >= logp.max(1) - band_s).all()
    st = logp[rows, t][:, None]
    lo, hi = (logp > st + band_s[:, None]).sum(1), (logp >= st - band_s[:, None]).sum(1) - 1
    assert ((lo <= got["rank"]) & (got["rank"] <= hi)).all()
    assert state[0] == B and state[5] == 0 and not state[13:].any()
    for slot, k in ((1, 1), (2, 5)):
        assert (hi < k).sum() <= state[slot] <= (lo < k).sum()
    assert abs(state[3] - got["nll"].astype(np.float64).sum()) <= 1e-12 * max(1.0, abs(state[3]))
    same = paths[got["pred"]] == paths[t]
    assert np.array_equal(got["dist"], 7 - same.sum(1))  # same tiers form a prefix of the path
    assert np.array_equal(got["tier_hit"], (same.astype(int) << np.arange(7)).sum(1))
    assert np.array_equal(state[6:13], same.sum(0)) and state[4] == got["dist"].sum()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("tree", list(TREES))
def test_loss_is_the_decoded_nll(tree, dtype):
    """Check 4: with lam = 1 and eps = 0 a row's loss is the decoder's NLL of its leaf, within the
    sum of both bands."""
    import hvamd.ops as ops
    B = 37
    zs, t = _inputs(tree, dtype, B)
    y = torch.from_numpy(_tax(tree).leaf_paths[t]).cuda()
    terms = ops.cond_softmax_cross_entropy(_device_outputs(zs, "separate"), y, *_tables(tree)[0], return_tiers=True)[1]
    mags = _magnitudes(tree, dtype, B)
    band = 2 * sum(m[0] + 3 * U * m[1] for m in mags) + _decode_ref(tree, dtype, B)[2]
    nll = _decode(tree, dtype, B)[0]["nll"]
    assert (np.abs(terms.cpu().double().numpy().sum(1) - nll) <= band + 8 * U * np.abs(nll)).all()


@pytest.mark.parametrize("tree", list(TREES))
def test_zero_logits_known_answer(tree):
    """Check 5: all-zero logits make every conditional uniform: log p(k) = -sum_t log|g_t(k)| and
    loss = sum_t log|g(y_t)|, exact up to logf (1 ulp = 2u a tier) and the 7 adds: 2 * 9u * the sum."""
    import hvamd.ops as ops
    tax, B = _tax(tree), 5
    zs = [torch.zeros(B, n) for n in tax.num_classes]
    sizes = [np.bincount(par)[par] for par in ref.parent_ids(tax.leaf_paths)]
    want = sum(np.log(s[tax.leaf_paths[:, q]]) for q, s in enumerate(sizes))  # -log p [L]
    t = np.random.default_rng(1).integers(0, tax.num_leaves, B)
    tables, paths = _tables(tree)
    state = torch.zeros(16, dtype=torch.float64, device="cuda")
    out = ops.cond_softmax_decode([z.cuda() for z in zs], torch.from_numpy(t).cuda(), *tables, paths, state, want_scores=True)
    assert (np.abs(out["scores"].cpu().double().numpy() + want) <= 18 * U * want).all()
    loss = ops.cond_softmax_cross_entropy([z.cuda() for z in zs], torch.from_numpy(tax.leaf_paths[t]).cuda(), *tables)
    assert abs(loss.item() - want[t].mean()) <= (18 + B) * U * want[t].mean()


def test_trainer_step_and_eval_end_to_end():
    """Check 6, on the mini SwinV2 of test_gpu_eval_metrics.py with variant cond-softmax."""
    from hvamd.hierarchy import EvalMetrics, backoff_predictions, cond_softmax_scores
    from test_gpu_eval_metrics import _composer_model, _trainer, _u8_batches, _f32_batch
    model, tax, _ = _composer_model("cond-softmax")
    batches = [_f32_batch(b) for b in _u8_batches(tax, (8, 8, 5), 21)]
    with torch.autocast("cuda", dtype=torch.bfloat16):
        outputs = model(batches[0])
    model.loss(outputs, batches[0]).backward()
    torch.cuda.synchronize()
    y = batches[0][1].cpu().numpy()
    for q, par in enumerate(ref.parent_ids(tax.leaf_paths)):  # head rows outside the batch's target groups
        idle = ~np.isin(par, y[:, q - 1]) if q else np.zeros(len(par), bool)
        g = model.module.head.heads[q].weight.grad
        assert g is not None and not g[torch.from_numpy(idle).cuda()].any()
        assert q == 0 or idle.any() or len(par) <= 8
    tr = _trainer(model)
    assert torch.isfinite(tr.train_step(batches[0])).item()
    out = tr.eval(batches, metrics=model.fused_metrics(decoding="cond-crm"))
    assert model.fused_metrics().decoding == "cond"
    model.eval()
    hand = EvalMetrics(taxonomy=tax, decoding="cond-crm").cuda()
    for b in batches:
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            outputs = model(b)
        hand.update(outputs, b[1])
    want = hand.compute()
    keys = ["acc@1", "acc@5", "cross-entropy", "tree-dist", "acc@1/crm", "tree-dist/crm"] + [f"acc@1/tier{q}" for q in range(7)]
    assert set(keys) == set(out) and all(out[k] == want[k] for k in keys)
    scores = cond_softmax_scores(outputs, tax)
    assert scores.shape == (5, tax.num_leaves) and torch.allclose(scores.exp().sum(1), torch.ones(5, device="cuda"), atol=1e-5)
    assert backoff_predictions(scores, tax)["path"].shape == (5, 7)
