"""tests/wmsa_ref.py on the CPU: the float64 restatement of the W-MSA core against the oracle
(oracle/swinv2_ref.py::wmsa_core_ref under autograd, in double), the honest-bf16 baseline of every
case of tests/test_gpu_wmsa_blocks.py, the separation of the geometry pin, and the sensitivity of
the per-block / per-entry comparison: four deliberate defects that the whole-tensor figures of
tests/test_gpu_wmsa.py let through."""
import numpy as np
import pytest
import torch

import wmsa_ref as R
from oracle import index_ref, swinv2_ref

ORACLE_CASES = [(2, 14, 14, 2, 7, 3), (1, 21, 14, 3, 7, 3), (1, 16, 16, 2, 8, 4), (1, 24, 24, 2, 12, 6)]
PIN_CASES = [(1, 14, 14, 1, 7, 3), (1, 14, 14, 3, 7, 3), (1, 21, 14, 3, 7, 3), (1, 16, 16, 2, 8, 4),
             (1, 24, 24, 2, 12, 6)]


@pytest.mark.parametrize("B,H,W,nh,win,shift", ORACLE_CASES)
def test_core_matches_oracle_in_double(B, H, W, nh, win, shift):
    """out and the four gradients equal the oracle's, element by element, to 1e-12 of the larger
    of the two values.  Two float64 evaluations that sum in a different order cannot agree better
    than a few ulp of the terms they add, so an element that cancels to nearly 0 gets the float64
    floor on top: 1e-14 of the tensor's largest magnitude (measured: <= 2.1e-15)."""
    qkv, tab, scale = R.inputs(B, H, W, nh, win, 1)
    gout = R.grad_out(B, H, W, nh, 2)
    mine = R.core(qkv, tab, scale, H, W, nh, win, shift, gout)
    q, t, s = (torch.from_numpy(x).double().requires_grad_(True) for x in (qkv, tab, scale))
    out = swinv2_ref.wmsa_core_ref(q, t, s, H, W, nh, win, shift)
    out.backward(torch.from_numpy(gout))
    C = 32 * nh
    pairs = [("out", mine["out"], out.detach().numpy()), ("dqkv", mine["dqkv"], q.grad.numpy()),
             ("dbias", mine["dbias"], t.grad.numpy()), ("dscale", mine["dscale"], s.grad.numpy()),
             ("dq_bias", mine["dq_bias"], q.grad[..., :C].sum((0, 1)).numpy())]
    for name, a, b in pairs:
        assert a.shape == b.shape and a.dtype == np.float64 == b.dtype, name
        big = np.maximum(np.abs(a), np.abs(b))
        excess = np.abs(a - b) - (1e-12 * big + 1e-14 * big.max())
        assert (excess <= 0).all(), (name, float(excess.max()), float(np.abs(a - b).max() / big.max()))
    # the sizes bound what they normalise
    assert (np.abs(mine["dbias"]) <= mine["size_dbias"]).all()
    assert (np.abs(mine["dscale"]) <= mine["size_dscale"]).all()
    assert (np.abs(mine["dq_bias"]) <= mine["size_dq_bias"] * (1 + 1e-12)).all()
    assert (mine["size_dbias"] > 0).all() and (mine["size_dscale"] > 0).all() and (mine["size_dq_bias"] > 0).all()
    assert np.array_equal(mine["g"], index_ref.window_gather_map(H, W, win, shift))


def test_bf16_rounding_is_nearest_even():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -0.3, 0.0, 3.0e-40])
    want = torch.from_numpy(x).float().bfloat16().double().numpy()
    assert np.array_equal(R.bf16(x), want)
    rng = np.random.default_rng(0)
    y = rng.standard_normal(10000) * np.exp(5 * rng.standard_normal(10000))
    assert np.array_equal(R.bf16(y), torch.from_numpy(y).float().bfloat16().double().numpy())


@pytest.mark.parametrize("group,geom,form", R.BLOCK_CASES, ids=[R.case_id(g, c) for g, c, _ in R.BLOCK_CASES])
def test_baseline_table(group, geom, form):
    """The honest-bf16 baseline (round_ops=True against round_ops=False) of every GPU block case:
    the worst normalised error per class, printed (tools/wmsa_baseline_blocks.py writes the same
    rows to profiles/wmsa/baseline_blocks.txt).  It is a property of the reference alone; a bf16
    operand rounding is 2^-9 relative, so each class must sit between 1e-7 and 0.5 -- a baseline
    of 0 (or one near 1) would make the GPU bound 2 x baseline meaningless."""
    rows = R.baseline_rows(group, geom, form)
    for name, v, where in rows:
        print(f"{R.case_id(group, geom):<34s} {name:<8s} baseline {v:.3e}  worst: {where}")
    for name, v, _ in rows:
        assert 1e-7 < v < 0.5, (name, v)
    # the baseline sits at exactly its own level and passes its own bound
    _, _, _, _, ref, base = R.block_case(group, geom, form)
    table, bad = R.check_units(base, ref, base, geom[3], geom[1:3] + geom[4:])
    assert not bad and all(r[3] == 1.0 for r in table)


def test_rounding_forms_differ_where_the_kernels_do():
    """form selects what the backward rounds: the three forms give three different dqkv on the
    same inputs, and the same forward (one q image in every form)."""
    B, H, W, nh, win, shift = 1, 16, 16, 2, 8, 4
    qkv, tab, scale = R.inputs(B, H, W, nh, win, 3)
    gout = R.grad_out(B, H, W, nh, 4)
    res = {f: R.core(qkv, tab, scale, H, W, nh, win, shift, gout, round_ops=True, form=f) for f in R.FORMS}
    for f in R.FORMS[1:]:
        assert np.array_equal(res[f]["out"], res["small"]["out"])
        assert not np.array_equal(res[f]["dqkv"], res["small"]["dqkv"])
    assert not np.array_equal(res["large"]["dqkv"], res["normed"]["dqkv"])
    for f in R.FORMS:  # outputs are bf16 values
        assert np.array_equal(R.bf16(res[f]["out"]), res[f]["out"])
        assert np.array_equal(R.bf16(res[f]["dqkv"]), res[f]["dqkv"])


# --------------------------------------------------------------------------- geometry pin
def _regions(H, W, win, shift):
    """[nW, n] label of the attention region (window, mask class) of every window position."""
    g = index_ref.window_gather_map(H, W, win, shift)
    nW, n = g.shape
    m = index_ref.shift_mask(H, W, win, shift)
    lab = np.zeros((nW, n), np.int64)
    for k in range(nW):
        same = np.ones((n, n), bool) if m is None else m[k] == 0
        # the first member of each position's region names it
        lab[k] = k * n + same.argmax(1)
    return g, lab


def _swap_pair(H, W, win, shift, diagonal=True):
    """Two tokens of the last (row- and column-edge) window on either side of both of its mask
    boundaries, or (diagonal False) neighbours in one row across the column boundary."""
    g, lab = _regions(H, W, win, shift)
    c = win - shift
    a, b = (c - 1) * win + (c - 1), (c if diagonal else c - 1) * win + c
    assert lab[-1, a] != lab[-1, b]
    return int(g[-1, a]), int(g[-1, b])


def _swap_rows(qkv, gout, ta, tb):
    """The v rows and the gout rows of tokens ta and tb exchanged (q and k stay: they are random
    and nearly without effect here).  This is the mildest misplacement: both tokens' output rows
    stay where they are and only the two regions' means move, by one code step over the region's
    size; a token moved with its output row changes that whole row as well."""
    C = gout.shape[-1]
    qkv, gout = qkv.copy(), gout.copy()
    qkv[0, [ta, tb], 2 * C:] = qkv[0, [tb, ta], 2 * C:]  # image 0 only
    gout[0, [ta, tb]] = gout[0, [tb, ta]]
    return qkv, gout


@pytest.mark.parametrize("B,H,W,nh,win,shift", PIN_CASES)
def test_pin_tolerance_separates_a_swapped_token(B, H, W, nh, win, shift):
    """The pin's inputs make out and dv region means of a two-level code.  (a) The softmax is
    uniform to 2e-3.  (b) Any two tokens differ by the full code step 2 amp in some channel of
    every head, so a token taken from another region moves that channel of a region of n members by
    2 amp / n: above the tolerance 2^-6 amp whenever n < 128.  Every region here has at most 72
    members except the one unmasked 144-token window of the w12 case, and a swap across two
    regions is seen in the smaller one.  (c) Shown on the restatement: the v and gout rows of two tokens swapped across
    the mask boundaries of the edge window exceed the tolerance in out and in dv."""
    qkv, tab, scale, gout = R.pin_inputs(B, H, W, nh, win, 5)
    C = 32 * nh
    ref = R.core(qkv, tab, scale, H, W, nh, win, shift, gout)
    assert R.pin_excess(ref["out"], ref["dqkv"], ref) == (0.0, 0.0)
    # (a) uniform attention: out is the mean of v over the region, to 2e-3 of max |v|
    g, lab = _regions(H, W, win, shift)
    v = qkv[0][:, 2 * C:]
    mean = np.empty_like(v)
    sizes = []
    for r in np.unique(lab):
        tok = g[lab == r]
        mean[tok] = v[tok].mean(0)
        sizes.append(len(tok))
    assert np.abs(ref["out"][0] - mean).max() <= 2e-3 * R.PIN_V
    # (b) the code names every token in every head, and at most one region reaches 128 members
    for code in (v, gout[0]):
        for h in range(nh):
            signs = code[:, 32 * h:32 * h + 32] > 0
            assert len(np.unique(signs, axis=0)) == H * W
        assert set(np.unique(np.abs(code))) == {np.abs(code).max()}
    assert sorted(sizes)[-2] < 128 and 2.0 / sorted(sizes)[-2] > R.PIN_TOL
    # (c) the swap
    ta, tb = _swap_pair(H, W, win, shift)
    q2, g2 = _swap_rows(qkv, gout, ta, tb)
    bad = R.core(q2, tab, scale, H, W, nh, win, shift, g2)
    eo, ev = R.pin_excess(bad["out"], bad["dqkv"], ref)
    print(f"swap of tokens {ta} and {tb}: out {eo:.2f} x tolerance, dv {ev:.2f} x tolerance")
    assert eo > 1 and ev > 1
    # ... and the honest bf16 rounding stays well inside it
    base = R.core(qkv, tab, scale, H, W, nh, win, shift, gout, round_ops=True)
    bo, bv = R.pin_excess(base["out"], base["dqkv"], ref)
    assert bo < 0.5 and bv < 0.5, (bo, bv)


# --------------------------------------------------------------------------- sensitivity
def _old_figures_pass(got, ref):
    rel = R.whole_tensor_rel(got, ref)
    return all(rel[k] < R.WHOLE_BOUNDS[k] for k in rel), rel


def _copy(res):
    return {k: np.array(v, copy=True) for k, v in res.items()}


def test_block_comparison_catches_what_the_whole_tensor_norm_misses():
    """Four float64 results with one deliberate defect each.  Every one passes the whole-tensor
    figures of tests/test_gpu_wmsa.py (1e-2 forward, 2e-2 gradients, 5e-2 dscale) and trips the
    per-unit bound (2 x baseline) in the class, and at the unit, of the defect."""
    geom = (1, 21, 14, 3, 7, 3)
    B, H, W, nh, win, shift = geom
    _, _, _, _, ref, base = R.block_case("mask", geom, "small")
    g4 = (H, W, win, shift)
    ok, rel = _old_figures_pass(base, ref)
    assert ok and not R.check_units(base, ref, base, nh, g4)[1], rel

    # 1. one corner entry of the CPB-table gradient dropped: offset (-(w-1), -(w-1)) of head 1 of 24
    #    (one (query, key) pair per window against the 49 of offset (0, 0))
    geom24 = (2, 7, 7, 24, 7, 0)
    _, _, _, _, ref24, base24 = R.block_case("mask", geom24, "small")
    got = _copy(base24)
    got["dbias"][1, 0] = 0.0
    ok, rel = _old_figures_pass(got, ref24)
    bad = R.check_units(got, ref24, base24, 24, (7, 7, 7, 0))[1]
    assert ok, rel
    assert [r[0] for r in bad] == ["dbias"] and bad[0][4] == "head 1 offset (-6, -6)", bad

    # 2. dk of one block of the last (row- and column-edge) window 10 % too large
    got = _copy(base)
    C = 32 * nh
    k_last = ref["g"].shape[0] - 1
    got["dqkv"][0][np.ix_(ref["g"][k_last], np.arange(C + 64, C + 96))] *= 1.1
    ok, rel = _old_figures_pass(got, ref)
    bad = R.check_units(got, ref, base, nh, g4)[1]
    assert ok, rel
    assert [r[0] for r in bad] == ["dk"] and bad[0][4].startswith(f"image 0 window {k_last} (row 2, col 1, mask rc) head 2")

    # 3. one head's dscale 10 % too large, among 24
    B, H, W, nh, win, shift = geom24
    ref, base = ref24, base24
    head = int(np.argsort(np.abs(ref["dscale"]))[nh // 2])  # a head of median |dscale|
    got = _copy(base)
    got["dscale"][head] *= 1.1
    ok, rel = _old_figures_pass(got, ref)
    bad = R.check_units(got, ref, base, nh, (H, W, win, shift))[1]
    assert ok, rel
    assert [r[0] for r in bad] == ["dscale"] and bad[0][4] == f"head {head}", bad

    # 4. two tokens swapped (row neighbours across the column seam of image 0's last window), under
    #    the geometry pin's inputs at the largest shape of tests/test_gpu_wmsa.py
    B, H, W, nh, win, shift = 3, 56, 56, 3, 7, 3
    qkv, tab, scale, gout = R.pin_inputs(B, H, W, nh, win, 5)
    ref = R.core(qkv, tab, scale, H, W, nh, win, shift, gout)
    ta, tb = _swap_pair(H, W, win, shift, diagonal=False)
    q2, g2 = _swap_rows(qkv, gout, ta, tb)
    got = R.core(q2, tab, scale, H, W, nh, win, shift, g2)
    rel = R.whole_tensor_rel({"out": got["out"], "dqkv": got["dqkv"]}, ref)
    eo, ev = R.pin_excess(got["out"], got["dqkv"], ref)
    print("swap:", rel, eo, ev)
    assert rel["out"] < R.WHOLE_BOUNDS["out"] and rel["dqkv"] < R.WHOLE_BOUNDS["dqkv"], rel
    assert eo > 1 and ev > 1
