"""Joint path decoding (hvk_joint_decode, EvalMetrics(decoding="joint" | "joint-crm")) on the GPU
against float64 numpy: seven log-softmaxes, a gather by leaf_paths, a weighted sum.

The error band, from the kernel's summation order (csrc/joint.hip), u = 2^-24, per row, on the
float64 reference's magnitudes M_t = max|z_t|, LSE_t, C_t = sum_{q<=t} w_q (M_q + |LSE_q|) >= |c_t|:
 * a max-shifted sum S over n entries: a thread adds ceil(n / 256) terms in sequence, each add
   possibly behind one rescale of the running sum, then 6 butterfly levels and 3 wave merges fold
   the partial sums: at most D(n) = 2 ceil(n / 256) + 9 operations touch a term, each an expf
   (1 ulp = 2u), a product (u) and an add (u): 4 D u relative.  The roundings of the exponents
   telescope to u (max - z_k) for term k, and sum_k p_k (max - z_k) <= the entropy <= log n.
   LSE = max + logf(S): logf 1 ulp on |log S| <= |LSE| + M, the add u |LSE|.  Together
   E_lse(n, M, LSE) = u (4 D(n) + log n + 3 (|LSE| + M)).
 * prefix, tiers 0-5: c_t = w_t (z - LSE_t) + c_{t-1}[parent]: the difference rounds by
   u (M_t + |LSE_t|), the product by as much times w_t, the add by u C_t:
   e_t = e_{t-1} + w_t (E_lse_t + 2 u (M_t + |LSE_t|)) + u C_t.
 * leaves: s_k = fma(w_6, z_6[k], c_5[parent]): one rounding of |s_k| <= w_6 M_6 + C_5, so
   E_s = e_5 + u (w_6 M_6 + C_5).
 * joint lse over the L scores: E_J = u (4 D(L) + log L + 4 (|lse| + max|s|)) (the 4th u covers
   nll = lse - s_t), on top of the scores' own E_s.
|scores - lse - ref| <= 2 E_s + E_J; the tests use band = 2 (2 E_s + E_J), a margin of 2 x."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
TREES = {"small": (1, 2, 3, 5, 9, 17, 131), "large": (3, 5, 11, 23, 47, 301, 2500), "shuffled": (1, 2, 3, 5, 9, 17, 131)}
WEIGHTS = {"uniform": (1,) * 7, "coeffs": (8, 5.65, 4, 2.82, 2, 1.41, 1), "species": (0, 0, 0, 0, 0, 0, 1)}


@functools.lru_cache(maxsize=None)
def _tax(tree):
    from hvamd.hierarchy import Taxonomy
    tax = Taxonomy.synthetic(TREES[tree])
    if tree == "shuffled":  # new leading numbers: another sorted() order, so non-monotone parents
        order = np.random.default_rng(7).permutation(tax.num_leaves)
        tax = Taxonomy([f"{order[i]:05d}_" + c.split("_", 1)[1] for i, c in enumerate(tax.classes)])
        assert not tax.identity_perm
    return tax


@functools.lru_cache(maxsize=None)
def _inputs(tree, dtype, B):
    """(7 tier logits as float64 numpy, rounded to the dtype; targets)."""
    rng = np.random.default_rng(B + len(tree))
    dt = torch.bfloat16 if dtype == "bf16" else torch.float32
    zs = tuple(torch.from_numpy(3 * rng.standard_normal((B, n))).to(dt) for n in _tax(tree).num_classes)
    return zs, rng.integers(0, _tax(tree).num_leaves, B)


def _lse(x):
    m = x.max(1, keepdims=True)
    return (m + np.log(np.exp(x - m).sum(1, keepdims=True)))[:, 0]


@functools.lru_cache(maxsize=None)
def _ref(tree, dtype, B, wname):
    """float64: (s = the kernel's scores, without the row constant w_6 LSE_6; log p; band [B])."""
    zs = [z.double().numpy() for z in _inputs(tree, dtype, B)[0]]
    paths, w = _tax(tree).leaf_paths, WEIGHTS[wname]
    lses = [_lse(z) for z in zs]
    logp = sum(w[t] * (zs[t] - lses[t][:, None])[:, paths[:, t]] for t in range(7))
    s = logp + w[6] * lses[6][:, None]
    logp = logp - _lse(logp)[:, None]
    D = lambda n: 2 * -(-n // 256) + 9  # noqa: E731
    e = C = 0.0
    for t in range(6):
        M, n = np.abs(zs[t]).max(1), zs[t].shape[1]
        C = C + w[t] * (M + np.abs(lses[t]))
        e = e + w[t] * U * (4 * D(n) + np.log(n) + 3 * (np.abs(lses[t]) + M) + 2 * (M + np.abs(lses[t]))) + U * C
    L = s.shape[1]
    e_s = e + U * (w[6] * np.abs(zs[6]).max(1) + C)
    e_j = U * (4 * D(L) + np.log(L) + 4 * (np.abs(_lse(s)) + np.abs(s).max(1)))
    return s, logp, 2 * (2 * e_s + e_j)


def _device_outputs(zs, layout):
    if layout == "separate":
        return [z.cuda() for z in zs]
    total = sum(z.shape[1] for z in zs)  # column views of one padded buffer, ld > sum n_t
    buf = torch.full((zs[0].shape[0], total + 5), 7e4, dtype=zs[0].dtype, device="cuda")
    outs, off = [], 0
    for z in zs:
        outs.append(buf[:, off:off + z.shape[1]].copy_(z))
        off += z.shape[1]
    return outs


def _decode(tree, dtype, B, wname, layout="separate"):
    import hvamd.ops as ops
    zs, t = _inputs(tree, dtype, B)
    parents, paths = _tax(tree).device_parent_tables("cuda")
    state = torch.zeros(16, dtype=torch.float64, device="cuda")
    out = ops.joint_decode(_device_outputs(zs, layout), torch.from_numpy(t).cuda(), parents, paths, WEIGHTS[wname],
                           state, topk=5, want_scores=True)
    return {k: v.cpu().numpy() for k, v in out.items()}, state.cpu().numpy(), t


@pytest.mark.parametrize("B", [1, 37])
@pytest.mark.parametrize("wname", ["uniform", "coeffs"])
@pytest.mark.parametrize("layout", ["separate", "views"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("tree", list(TREES))
def test_joint_decode_matches_float64(tree, dtype, layout, wname, B):
    """Checks 1 and 2: scores, NLL, and prediction / rank / state sums as intervals under the band
    of the module docstring.  Measured on an MI355X over all cases: worst score error 3.1e-5, worst
    NLL error 2.5e-5, at most 3.3 % of the row's band."""
    got, state, t = _decode(tree, dtype, B, wname, layout)
    s, logp, band = _ref(tree, dtype, B, wname)
    rows, paths = np.arange(B), _tax(tree).leaf_paths
    err = np.abs(got["scores"].astype(np.float64) - got["lse"][:, None] - logp).max(1)
    nll_err = np.abs(got["nll"] + logp[rows, t])
    print(f"score error {err.max():.3g}, nll error {nll_err.max():.3g}, smallest band {band.min():.3g}, "
          f"worst error / band {max((err / band).max(), (nll_err / band).max()):.3g}")
    assert (err <= band).all() and (nll_err <= band).all()
    assert (s[rows, got["pred"]] >= s.max(1) - band).all()
    st = s[rows, t][:, None]
    lo, hi = (s > st + band[:, None]).sum(1), (s >= st - band[:, None]).sum(1) - 1
    assert ((lo <= got["rank"]) & (got["rank"] <= hi)).all()
    assert state[0] == B and state[5] == 0
    for slot, k in ((1, 1), (2, 5)):
        assert (hi < k).sum() <= state[slot] <= (lo < k).sum()
    same = paths[got["pred"]] == paths[t]
    assert np.array_equal(got["dist"], 7 - same.sum(1))  # same tiers form a prefix of the path
    assert np.array_equal(got["tier_hit"], (same.astype(int) << np.arange(7)).sum(1))
    assert np.array_equal(state[6:13], same.sum(0)) and state[4] == got["dist"].sum()
    assert np.array_equal(got["head_pred"], np.stack([z.float().numpy().argmax(1) for z in _inputs(tree, dtype, B)[0]], 1))
    cons = np.all([paths[got["head_pred"][:, 6], q] == got["head_pred"][:, q] for q in range(7)], 0)
    assert np.array_equal(got["consistent"], cons) and state[15] == cons.sum()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("tree", list(TREES))
def test_species_weight_alone_is_eval_metrics(tree, dtype):
    """Check 3: weights (0, ..., 0, 1) leave the species logits, so prediction and rank equal
    hvk_eval_metrics' bit for bit (bf16 ties included)."""
    import hvamd.ops as ops
    got, _, t = _decode(tree, dtype, 37, "species")
    z = _inputs(tree, dtype, 37)[0][6].cuda()
    pred, rank = ops.eval_metrics(z, torch.from_numpy(t).cuda(), torch.zeros(16, dtype=torch.float64, device="cuda"))[:2]
    assert np.array_equal(got["pred"], pred.cpu().numpy()) and np.array_equal(got["rank"], rank.cpu().numpy())
    assert np.array_equal(got["head_pred"][:, 6], got["pred"])


def test_known_answer():
    """Check 4: the species head prefers leaf A by 0.5 over X, the best leaf under B's genus, and
    every coarser head prefers B's branch by 2: the joint prediction is X, the species head's is A
    and the row is path-inconsistent.  With every head's argmax on A's path it is consistent."""
    from hvamd.hierarchy import EvalMetrics
    tax = _tax("small")
    paths = tax.leaf_paths
    A, B_ = 3, 120
    X = int(np.flatnonzero(paths[:, 5] == paths[B_, 5])[-1])
    assert paths[A, 5] != paths[B_, 5]
    m = EvalMetrics(taxonomy=tax, decoding="joint").cuda()
    for lead, joint_pred, consistent in ((B_, X, 0.0), (A, A, 1.0)):
        zs = [torch.zeros(1, n) for n in tax.num_classes]
        zs[6][0, A], zs[6][0, X] = 1.0, 0.5
        for q in range(6):
            zs[q][0, paths[lead, q]] = 2.0
        m.reset()
        m.update([z.cuda() for z in zs], torch.tensor([A]).cuda())
        assert m.pred.item() == A and m.joint_pred.item() == joint_pred
        assert m.head_pred[0].tolist() == list(paths[lead, :6]) + [A]
        assert m.consistent.item() == consistent and m.compute()["path-consistency"] == consistent


def test_trainer_eval_joint_crm_end_to_end():
    """Check 5, on the mini multitask SwinV2 of test_gpu_eval_metrics.py, three ragged batches."""
    import hvamd.ops as ops
    from hvamd.hierarchy import EvalMetrics, joint_scores
    from test_gpu_eval_metrics import _composer_model, _trainer, _u8_batches, _f32_batch
    model, tax, info = _composer_model("multitask")
    tr = _trainer(model)
    batches = [_f32_batch(b) for b in _u8_batches(tax, (8, 8, 5), 21)]
    out = tr.eval(batches, metrics=model.fused_metrics(decoding="joint-crm"))
    plain = tr.eval(batches, metrics=model.fused_metrics())
    assert all(out[k] == plain[k] for k in ("acc@1", "acc@5", "cross-entropy", "tree-dist"))
    model.eval()
    hand, D = EvalMetrics(taxonomy=tax, decoding="joint").cuda(), info.tree_dists.cuda()
    crm_state = torch.zeros(16, dtype=torch.float64, device="cuda")
    states = []
    for _ in range(2):
        m = model.fused_metrics(decoding="joint-crm")
        for b in batches:
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                outputs = model(b)
            m.update(outputs, b[1])
            if not states:
                hand.update(outputs, b[1])
                ops.crm_predict(joint_scores(outputs, tax)[0], b[1], D, crm_state)
        states.append(m.joint_state.clone())
    assert torch.equal(states[0], states[1])
    want = hand.compute()
    joint_keys = [k for k in want if "joint" in k or k == "path-consistency"]
    assert len(joint_keys) == 12 and all(out[k] == want[k] for k in joint_keys)
    assert out["acc@1/joint-crm"] == crm_state[13].item() / 21 and out["tree-dist/joint-crm"] == crm_state[14].item() / 21
