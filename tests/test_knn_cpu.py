"""CPU-only checks of the k-NN evaluation: the hvk_knn_* exports and their validation (before any HIP call),
the config and model surface, and tests/knn_ref.py against a brute-force loop on an example worked by hand."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import knn_ref as ref

HVK_OK, HVK_EINVAL, HVK_EUNSUPPORTED = 0, 1, 2
P = ctypes.c_void_p
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args(name, **over):
    a = {"hvk_knn_topk": dict(q=P(0x1000), B=4, bank=P(0x2000), N=100, D=64, k=5, splits=0, sims=P(0x3000),
                              idx=P(0x4000), workspace=P(0x10000), workspace_bytes=1 << 30, stream=None),
         "hvk_knn_vote": dict(sims=P(0x1000), idx=P(0x2000), B=4, k=5, labels=P(0x3000), N=100, T=7,
                              ks=(ctypes.c_int * 2)(1, 5), n_k=2, temperature=0.07, leaf=P(0x4000), path=P(0x5000),
                              stream=None)}[name]
    assert set(over) <= set(a), (name, over)
    a.update(over)
    return list(a.values())


def test_abi_symbols_support_and_workspace():
    from hvamd import _lib
    hdr = open(os.path.join(ROOT, "include", "hvk.h")).read()
    assert int(re.search(r"#define\s+HVK_ABI_VERSION\s+(\d+)", hdr).group(1)) >= 26
    lib = _lib.load()
    assert _lib.ABI_VERSION >= 26 and lib.hvk_abi_version() == _lib.ABI_VERSION
    for name in ("hvk_knn_supported", "hvk_knn_workspace", "hvk_knn_topk", "hvk_knn_vote"):
        assert name in _lib.SIGNATURES and hasattr(ctypes.CDLL(_lib.LIB_PATH), name), name
        assert name[8:] in ("supported", "workspace") or len(_lib.SIGNATURES[name][1]) == len(_args(name))
    assert [lib.hvk_knn_supported(D, k) for D, k in ((768, 200), (1024, 256), (8, 1))] == [1, 1, 1]
    assert [lib.hvk_knn_supported(D, k) for D, k in ((1032, 20), (100, 20), (768, 257), (768, 0), (0, 5))] == [0] * 5
    assert lib.hvk_knn_workspace(130, 2000, 20, 7) == 7 * 130 * 20 * 8  # a (key, index) list per (split, row)
    assert lib.hvk_knn_workspace(130, 100, 20, 7) == 2 * 130 * 20 * 8  # never more splits than 64-row tiles
    assert lib.hvk_knn_workspace(0, 100, 20, 0) == 0 and lib.hvk_knn_workspace(4, 100, 257, 0) == 0


BAD = [("hvk_knn_topk", {k: None}, HVK_EINVAL, b"null") for k in ("q", "bank", "sims", "idx")]
BAD += [("hvk_knn_vote", {k: None}, HVK_EINVAL, b"null") for k in ("sims", "idx", "labels", "ks", "leaf", "path")]
BAD += [("hvk_knn_topk", dict(B=-1), HVK_EINVAL, b"shape"), ("hvk_knn_topk", dict(N=0), HVK_EINVAL, b"shape"),
        ("hvk_knn_topk", dict(k=0), HVK_EINVAL, b"shape"), ("hvk_knn_topk", dict(N=0x7fffffff), HVK_EINVAL, b"shape"),
        ("hvk_knn_topk", dict(q=P(0x1008)), HVK_EINVAL, b"aligned"),
        ("hvk_knn_topk", dict(workspace=None), HVK_EINVAL, b"workspace"),
        ("hvk_knn_topk", dict(workspace_bytes=4 * 5 * 8 - 1), HVK_EINVAL, b"workspace"),
        ("hvk_knn_vote", dict(T=3), HVK_EINVAL, b"shape"), ("hvk_knn_vote", dict(n_k=9), HVK_EINVAL, b"shape"),
        ("hvk_knn_vote", dict(ks=(ctypes.c_int * 2)(1, 6)), HVK_EINVAL, b"shape"),
        ("hvk_knn_vote", dict(temperature=0.0), HVK_EINVAL, b"temperature")]
BAD += [(n, o, HVK_EUNSUPPORTED, b"unsupported") for n, o in (("hvk_knn_topk", dict(D=100)), ("hvk_knn_topk", dict(D=1032)),
                                                               ("hvk_knn_topk", dict(k=257)), ("hvk_knn_vote", dict(k=257)))]


@pytest.mark.parametrize("name,over,code,word", BAD, ids=[f"{b[0][8:]}-{'-'.join(b[1])}-{i}" for i, b in enumerate(BAD)])
def test_invalid_arguments_refused_before_any_launch(name, over, code, word):
    from hvamd import _lib
    lib = _lib.load()
    assert getattr(lib, name)(*_args(name, **over)) == code
    msg = lib.hvk_last_error_string()
    assert name.encode() in msg and word in msg, msg
    assert getattr(lib, name)(*_args(name, B=0)) == HVK_OK  # an empty batch: no launch


def test_config_model_and_wrappers():
    import hvamd.ops as ops
    from hvamd import configs, knn, models
    cfg = configs.Config()
    assert (cfg.knn.k, cfg.knn.temperature, cfg.knn.centered) == ([10, 20, 100, 200], 0.07, False)
    configs.merge(cfg, {"knn": {"k": [1, 5]}, "model": {"variant": "knn", "name": "swinv2_tiny_window7_224"}},
                  {"knn": {"temperature": 0.1}})
    assert (cfg.knn.k, cfg.knn.temperature, cfg.knn.centered) == ([1, 5], 0.1, False)
    model = models.build_model(cfg, 2, img_size=32, embed_dim=32, depths=[2, 2], num_heads=[1, 2], window_size=4)
    assert isinstance(model, models.FeatureOnlyModel)
    with pytest.raises(ValueError, match="FeatureOnlyModel"):
        knn.evaluate(cfg, torch.nn.Identity(), [], [])
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.knn_topk(torch.zeros(2, 8, dtype=torch.bfloat16), torch.zeros(4, 8, dtype=torch.bfloat16), 3)


def test_reference_against_a_brute_force_loop_by_hand():
    """Six bf16-exact bank rows, k = 4, temperature 0.5.  q0 = (1, 0): similarities 1, 0, .5, 1, -1, .5 -> rows
    0, 3, 2, 5; q1 = (0, 1): 0, 1, .5, 0, 0, -.5 -> rows 1, 2, 0, 3 (0, 3, 4 tie at 0: the lower indices).
    Leaves 2, 1, 1, 2, 0, 1: q0 votes leaf 2 with 2 against 2 / e; q1 leaf 1 with 1 + 1 / e against 2 / e^2."""
    bank = np.array([[1, 0], [0, 1], [.5, .5], [1, 0], [-1, 0], [.5, -.5]], np.float32)
    q = np.array([[1, 0], [0, 1]], np.float64)
    assert np.array_equal(ref.bf16_round(bank), bank)
    leaves = np.array([2, 1, 1, 2, 0, 1])
    labels = np.stack([leaves // 2 ** (6 - t) for t in range(7)], 1)  # a binary tree's paths
    sims, idx = ref.topk(q @ bank.T.astype(np.float64), 4)
    assert idx.tolist() == [[0, 3, 2, 5], [1, 2, 0, 3]] and sims.tolist() == [[1, 1, .5, .5], [1, .5, 0, 0]]
    for r, (leaf, vote) in enumerate([(2, 2.0), (1, 1 + 1 / math.e)]):
        tally = {}  # brute force: a plain loop over the neighbours
        for i in range(4):
            c = leaves[idx[r][i]]
            tally[c] = tally.get(c, 0.0) + math.exp((sims[r][i] - sims[r][0]) / 0.5)
        assert max(tally, key=lambda c: (tally[c], -c)) == leaf and abs(tally[leaf] - vote) < 1e-12
        got_leaf, got_path = ref.predict(sims[r], idx[r], labels, 4, 0.5)
        assert got_leaf == leaf and ref.predict(sims[r], idx[r], leaves, 4, 0.5)[0] == leaf
        assert got_path.tolist() == [leaf // 2 ** (6 - t) for t in range(7)]  # here the walk ends at that leaf
    s5, i5 = ref.topk(q @ bank[:3].T.astype(np.float64), 5)  # N < k; leaf 2: 1; leaf 1: 1 / e + 1 / e^2; pads: 0
    assert i5[0].tolist() == [0, 2, 1, -1, -1] and ref.predict(s5[0], i5[0], leaves[:3], 5, 0.5)[0] == 2
