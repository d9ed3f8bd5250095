"""The complete kernel-routing table of hvamd.ops on the CPU: which hvk_* entry points each
GEMM-family op launches, forward and backward, for every SwinV2 width, token count around a
threshold and routing-option combination, against tests/golden/routes_golden.json (recorded from
the parent of the commit that moved the decisions into hvamd/routes.py; see
tests/golden/make_routes_golden.py), and hvamd.routes' answers against those launches."""
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN

# keys where the recording raised (a gate passed and the chooser found no kernel): the ops must
# take the unfused route there.  Named here so that none can be added silently.
RAISED = ()


def _load_generator():
    spec = importlib.util.spec_from_file_location("make_routes_golden", os.path.join(GOLDEN, "make_routes_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def tables():
    from hvamd import ops, options
    gen = _load_generator()
    with open(os.path.join(GOLDEN, "routes_golden.json")) as f:
        golden = gen.unpack(json.load(f))
    return gen, golden, gen.record(ops, options)


def test_routes_match_golden(tables):
    gen, (gold, gold_merge), (new, new_merge) = tables
    assert set(new) == set(gold) and len(gold) == 19200
    raised = sorted(k for k, v in gold.items() if v[0].startswith("raise"))
    assert raised == sorted(RAISED) and len(raised) == 0
    bad = {k: (gold[k], new[k]) for k in gold if new[k] != gold[k] and k not in RAISED}
    assert not bad, f"{len(bad)} routes differ, e.g. {sorted(bad.items())[:3]}"
    for k in RAISED:  # the working unfused route: GEMM + activation kernel
        assert "hvk_bias_gelu_fwd" in new[k] and not new[k][0].startswith("raise"), (k, new[k])
    assert new_merge == gold_merge and len(gold_merge) == 384


def test_routes_agree_with_launches(tables):
    """routes.* asked directly, under the same options, names the kernel family the op launched."""
    from hvamd import ops, options, routes
    gen, _, (new, new_merge) = tables
    with gen.recording(ops):  # the same libhvk answers as the recording
        _check_routes(gen, options, routes, new, new_merge)


def _check_routes(gen, options, routes, new, new_merge):
    fwd = {"hvk_gemm_fwd": "tile", "hvk_linear_fwd": "skinny", "fb:mm_nt": None}
    qkv = {"hvk_gemm_qkv_fwd": "tile", "hvk_linear_qkv_fwd": "skinny"}
    gelu = {"hvk_gemm_gelu_fwd": "tile", "hvk_linear_gelu_fwd": "skinny"}
    mlp_first = {"hvk_mlp_fwd": "fused", "hvk_gemm_gelu_fwd": "chain", "hvk_linear_gelu_fwd": "chain"}
    checked = 0
    for op, (names, _) in gen.OPS.items():
        for combo in gen.combos(names):
            with options.override(**combo, **gen.FIXED):
                for C in gen.WIDTHS:
                    for M in gen.TOKENS:
                        k = gen.key(op, C, M, combo)
                        seq = new[k]
                        if op.startswith("linear:"):
                            K, N = gen.LINEAR_KN[op[7:]](C)
                            assert routes.nt(M, K, N) == fwd[seq[0]], k
                            assert (routes.nt(M, N, K) is None) == ("fb:dgrad" in seq), k
                            assert bool(routes.dw(M, N, K)) == ("fb:weight_grad" not in seq), k
                        elif op == "linear_qkv":
                            assert routes.qkv(M, C, 3 * C) == qkv.get(seq[0], "normalize"), k
                        elif op == "linear_gelu":
                            assert routes.gelu_fwd(M, C, 4 * C) == gelu.get(seq[0]), k
                        elif op.startswith("mlp_ln"):
                            plan = routes.mlp_ln(M, C, 4 * C, C)
                            want = None if seq == gen.GATED_OFF else "fused" if seq[0] == "hvk_mlp_ln_fwd" else "chain"
                            assert plan == want, k
                        elif op.startswith("mlp"):
                            plan = routes.mlp(M, C, 4 * C, C)
                            if "hvk_linear_gelu_in_fwd" in seq:
                                assert plan == "recompute", k
                            else:
                                assert plan == mlp_first.get(seq[0]), k
                            if plan is not None and "hvk_mlp_bwd" not in seq:
                                tile = "hvk_gemm_gelu_bwd" in seq
                                assert tile != ("hvk_linear_gelu_bwd" in seq), k
                                assert routes.gelu_bwd(M, C, 4 * C) == ("tile" if tile else "skinny"), k
                        elif op.startswith("linear_ln:"):
                            K, N = gen.LINEAR_KN[op[10:]](C)
                            assert (routes.linear_ln(M, K, N) is None) == (seq == gen.GATED_OFF), k
                        checked += 1
    assert checked == len(new)
    for combo in gen.combos(gen.MERGE):
        with options.override(**combo, **gen.FIXED):
            for C in gen.WIDTHS:
                for hw in gen.MERGE_HW:
                    for B in gen.MERGE_B:
                        got = new_merge[gen.key(f"merge B={B} H={hw}", C, B * hw * hw // 4, combo)]
                        r = routes.merge(B, hw, hw, C, 2 * C)
                        assert got == (r is not None, r == "ln"), (B, hw, C, combo)
