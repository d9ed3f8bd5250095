"""W-MSA HIP kernels against the float64 restatement tests/wmsa_ref.py, unit by unit: every
(image, window, head) block of out / dq / dk / dv, every CPB-table entry of every head, every
head's logit-scale gradient and every q_bias channel is normalised by its own size and must stay
within 2 x the honest-bf16 baseline of the same case (the same float64 math with the kernels' bf16
operand roundings, computed here at run time; tests/test_wmsa_ref_cpu.py shows on the CPU that this
catches a dropped table corner, one window's dk or one head's dscale 10 % off, and a swapped token,
all of which pass the whole-tensor norms of tests/test_gpu_wmsa.py).  Plus a geometry pin on
near-uniform attention and the zero-workspace contract of the backward.

Each comparison prints a "blocks|" row, observed / baseline per class; the rows of a run on an
MI355X are kept in profiles/wmsa/gpu_blocks.txt."""
import numpy as np
import pytest
import torch

import wmsa_ref as R

pytestmark = pytest.mark.gpu

IDS = [R.case_id(g, c) for g, c, _ in R.BLOCK_CASES]
RAW_CASES = [c for c in R.BLOCK_CASES if c[0] != "normed"]
NORMED_CASES = [c for c in R.BLOCK_CASES if c[0] == "normed"]
PIN_CASES = [(1, 14, 14, 1, 7, 3), (1, 14, 14, 3, 7, 3), (1, 21, 14, 3, 7, 3), (1, 16, 16, 2, 8, 4),
             (1, 24, 24, 2, 12, 6)]


@pytest.fixture(autouse=True)
def _reset_options():
    yield
    import hvamd._lib as lib
    for name, v in (("wmsa_fwd_form", 0), ("wmsa_bwd_nt", 0), ("wmsa_bwd_slice_bytes", 1 << 31)):
        lib.set_option(name, v)


def _dev(x, bf=False):
    t = torch.from_numpy(np.ascontiguousarray(x)).float().cuda()
    return t.bfloat16() if bf else t


def _image_bytes(H, W, nh):
    return H * W * 3 * 32 * nh * 2


def _run(qkv, tab, scale, gout, geom):
    """Forward + backward through ops.window_attention_core; float64 numpy results."""
    import hvamd.ops as ops
    B, H, W, nh, win, shift = geom
    q = _dev(qkv, bf=True).requires_grad_(True)
    t, s = _dev(tab).requires_grad_(True), _dev(scale).requires_grad_(True)
    qb = torch.zeros(32 * nh, device="cuda", requires_grad=True)
    out = ops.window_attention_core(q, t, s, H, W, nh, win, shift, q_bias=qb)
    out.backward(_dev(gout, bf=True))
    torch.cuda.synchronize()
    return {"out": out.detach().double().cpu().numpy(), "dqkv": q.grad.double().cpu().numpy(),
            "dbias": t.grad.double().cpu().numpy(), "dscale": s.grad.double().cpu().numpy(),
            "dq_bias": qb.grad.double().cpu().numpy()}


def _judge(label, got, ref, base, geom):
    B, H, W, nh, win, shift = geom
    for k, v in got.items():
        assert np.isfinite(v).all(), (label, k)
    rows, bad = R.check_units(got, ref, base, nh, (H, W, win, shift))
    for line in R.format_rows(label, rows):
        print("blocks| " + line)
    assert not bad, "\n".join(R.format_rows(label, bad))


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("group,geom,form", RAW_CASES, ids=IDS[:len(RAW_CASES)])
def test_wmsa_blocks_within_twice_bf16_baseline(monkeypatch, group, geom, form, variant):
    """ops.window_attention_core forward + backward.  Windows <= 8: variant 0 / 1 is the forward
    form (wmsa_fwd_form 0: wmsa_win.hip, 1: wmsa_ring.hip).  Large windows: variant 0 keeps the
    forward's row constants for the backward (wmsa_large_lse), variant 1 recomputes them.  The
    "slices" case runs the backward in batch slices of two images + 17 bytes."""
    import hvamd._lib as lib
    import hvamd.ops as ops
    B, H, W, nh, win, shift = geom
    qkv, tab, scale, gout, ref, base = R.block_case(group, geom, form)
    if win <= 8:
        lib.set_option("wmsa_fwd_form", variant)
        label = R.case_id(group, geom) + ("/ring" if variant else "/win")
    else:
        monkeypatch.setattr(ops.OPTIONS, "wmsa_large_lse", variant == 0)
        label = R.case_id(group, geom) + ("/recompute" if variant else "/lse")
    if group == "slices":
        lib.set_option("wmsa_bwd_slice_bytes", 2 * _image_bytes(H, W, nh) + 17)
    _judge(label, _run(qkv, tab, scale, gout, geom), ref, base, geom)


@pytest.mark.parametrize("fwd_form", [0, 1])
@pytest.mark.parametrize("group,geom,form", NORMED_CASES, ids=IDS[len(RAW_CASES):])
def test_wmsa_normed_blocks_within_twice_bf16_baseline(group, geom, form, fwd_form):
    """hvk_wmsa_fwd_normed / hvk_wmsa_bwd_normed on (q^ scale log2e, k^, v) from hvk_qk_normalize,
    as tests/test_gpu_qknorm.py reaches them; the gradients are those of the un-normalised qkv."""
    import hvamd._lib as lib
    B, H, W, nh, win, shift = geom
    C, T = 32 * nh, B * H * W
    qkv, tab, scale, gout, ref, base = R.block_case(group, geom, form)
    qn = _dev(qkv.reshape(T, 3 * C), bf=True)
    t, s, do = _dev(tab), _dev(scale), _dev(gout.reshape(T, C), bf=True)
    rn = torch.empty(T, 2 * nh, device="cuda")
    lib.call("hvk_qk_normalize", lib.ptr(qn), lib.ptr(rn), lib.ptr(s), T, C, lib.stream())
    out = torch.empty(T, C, device="cuda", dtype=torch.bfloat16)
    nb = lib.load().hvk_wmsa_bwd_workspace_bytes(nh, win)
    ws = torch.zeros(nb // 4, device="cuda")
    dqkv = torch.empty(T, 3 * C, device="cuda", dtype=torch.bfloat16)
    dqb, dtab, dsc = torch.empty(C, device="cuda"), torch.empty_like(t), torch.empty_like(s)
    with lib.option("wmsa_fwd_form", fwd_form):
        lib.call("hvk_wmsa_fwd_normed", lib.ptr(qn), lib.ptr(out), lib.ptr(t), lib.ptr(s), B, H, W, C, nh, win,
                 shift, lib.stream())
        lib.call("hvk_wmsa_bwd_normed", lib.ptr(qn), lib.ptr(rn), lib.ptr(do), lib.ptr(dqkv), lib.ptr(dqb),
                 lib.ptr(t), lib.ptr(s), lib.ptr(dtab), lib.ptr(dsc), lib.ptr(ws), nb, B, H, W, C, nh, win, shift,
                 lib.stream())
        torch.cuda.synchronize()
    got = {"out": out.double().cpu().numpy().reshape(B, H * W, C),
           "dqkv": dqkv.double().cpu().numpy().reshape(B, H * W, 3 * C), "dbias": dtab.double().cpu().numpy(),
           "dscale": dsc.double().cpu().numpy(), "dq_bias": dqb.double().cpu().numpy()}
    _judge(R.case_id(group, geom) + ("/ring" if fwd_form else "/win"), got, ref, base, geom)
    assert not ws.view(torch.int32).any().item(), "the backward must leave its workspace zero"


@pytest.mark.parametrize("B,H,W,nh,win,shift", PIN_CASES)
def test_wmsa_near_uniform_attention_pins_geometry(B, H, W, nh, win, shift):
    """Table 0, scale 1e-3, random q / k, and v / gout two-level codes of the token position
    (wmsa_ref.pin_inputs): the softmax is uniform over the unmasked members of a window to 2e-3, so
    out and dv are region means of the codes -- exactly what partition, roll and mask decide.
    Elementwise |out - out64| <= 2^-6 max|v| and |dv - dv64| <= 2^-6 max|gout|: P rounded to bf16
    contributes 2^-9, the bf16 output 2^-9, the 2e-3 non-uniformity is in the float64 answer
    itself; together below 2^-7, with a margin of 2.  A token from another region moves an element
    by 2 max|v| / n >= 2^-6 max|v| * 1.7 (n <= 72; tests/test_wmsa_ref_cpu.py)."""
    import hvamd._lib as lib
    geom = (B, H, W, nh, win, shift)
    qkv, tab, scale, gout = R.pin_inputs(B, H, W, nh, win, 5)
    ref = R.core(qkv, tab, scale, H, W, nh, win, shift, gout)
    for fwd_form in ((0, 1) if win <= 8 else (0,)):
        lib.set_option("wmsa_fwd_form", fwd_form)
        got = _run(qkv, tab, scale, gout, geom)
        eo, ev = R.pin_excess(got["out"], got["dqkv"], ref)
        print(f"blocks| pin-{'x'.join(map(str, geom))}/form{fwd_form}  out {eo:.3f}  dv {ev:.3f}  (x tolerance)")
        assert eo <= 1 and ev <= 1, (fwd_form, eo, ev)


def _wmsa_workspaces():
    import hvamd.ops as ops
    return {k: v for k, v in ops._WORKSPACES.items() if k[0] == "wmsa"}


def _param_grads(geom, seed):
    B, H, W, nh, win, shift = geom
    qkv, tab, scale = R.inputs(B, H, W, nh, win, seed)
    got = _run(qkv, tab, scale, R.grad_out(B, H, W, nh, seed + 1), geom)
    return [torch.from_numpy(got[k]).float() for k in ("dbias", "dscale", "dq_bias")]


def test_wmsa_backward_leaves_workspace_zero():
    """ops._workspace("wmsa", ..., zero=True) is zero-filled once; every backward must hand it back
    with every slot zero (finalize_slots, wmsa_common.h), whatever B, H, W came before.  After a w7,
    a w8, a batch-sliced and a w12 backward no "wmsa" workspace holds a nonzero bit (as int32: -0.0
    and NaN count), and a following run with another B on the same (heads, window) gives the bits
    of a run on a freshly zero-filled workspace."""
    import hvamd._lib as lib
    import hvamd.ops as ops
    runs = [((1, 14, 14, 3, 7, 3), None, (3, 14, 14, 3, 7, 3)), ((1, 16, 16, 2, 8, 4), None, (3, 16, 16, 2, 8, 4)),
            ((5, 14, 14, 2, 7, 3), 2 * _image_bytes(14, 14, 2) + 17, (2, 28, 14, 2, 7, 3)),
            ((1, 24, 24, 2, 12, 6), None, (2, 12, 12, 2, 12, 0))]
    for first, slice_bytes, second in runs:
        with lib.option("wmsa_bwd_slice_bytes", slice_bytes if slice_bytes else 1 << 31):
            _param_grads(first, 31)
        held = _wmsa_workspaces()
        assert held, "the backward took no wmsa workspace"
        for key, ws in held.items():
            assert not ws.view(torch.int32).any().item(), (first, key)
        after = _param_grads(second, 33)
        assert set(_wmsa_workspaces()) == set(held), "same (heads, window): the same workspace"
        for key in held:
            del ops._WORKSPACES[key]
        fresh = _param_grads(second, 33)
        for name, a, b in zip(("dbias", "dscale", "dq_bias"), after, fresh):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (first, second, name)
        for key, ws in _wmsa_workspaces().items():
            assert not ws.view(torch.int32).any().item(), (second, key)
