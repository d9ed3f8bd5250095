"""CPU-only checks of SimpleShot: the float64 restatement against the reference's recorded
predictions and centroids (tests/golden/simpleshot_golden.npz), the hvk_ss_* exports and their
argument validation (which runs before any HIP call), the CSR children lists, and the Python
surface's refusals."""
import ctypes

import numpy as np
import pytest
import torch

import simpleshot_ref as ref

HVK_OK, HVK_EINVAL = 0, 1
CASES = ("small", "wide")


# --------------------------------------------------------------------------- restatement vs golden
@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_the_reference(golden, case):
    g = golden("simpleshot_golden")
    sizes, D, seed = tuple(int(v) for v in g[f"{case}.sizes"]), int(g[f"{case}.D"]), int(g[f"{case}.seed"])
    Xtr, ytr, Xev, yev = ref.hierarchical_data(sizes, D, seed, n_eval=int(g[f"{case}.n_eval"]))
    assert np.array_equal(ytr, g[f"{case}.ytrain"]) and np.array_equal(yev, g[f"{case}.yeval"])
    tiers = ref.fit_tiers(Xtr, ytr)
    assert [len(c) for _, c in tiers] == list(sizes)
    for t, (means, counts) in enumerate(tiers):
        assert counts.min() > 0  # every class occurs: LabelEncoder positions are the tier ids
        got = means.reshape(-1)[g[f"{case}.centroids{t}.idx"]]
        assert np.abs(got - g[f"{case}.centroids{t}"]).max() <= 1e-12
    pred, tb, ts = ref.predict_tree(Xev, tiers, ref.tree_sizes_lookup(sizes))
    assert np.array_equal(pred, g[f"{case}.tree_pred"])
    flat, fb, fs = ref.predict_flat(Xev, *tiers[-1])
    assert np.array_equal(flat, g[f"{case}.flat_pred"])
    # the fixture's seed was chosen so that no row is a near-tie (the GPU test asks for equality)
    cn = max(float((m * m).sum(1).max()) for m, _ in tiers)
    assert not ref.margin_band(Xev, tb, ts, cn).any() and not ref.margin_band(Xev, fb, fs, cn).any()
    # the expanded form the large flat case uses picks the same classes here
    assert np.array_equal(ref.predict_flat(Xev, *tiers[-1], expanded=True)[0], flat)
    # the tree's means of an upper tier are the means over the rows under the node
    up, _ = ref.class_means(Xtr, ref.leaf_paths(sizes)[ytr[:, -1], 3], sizes[3])
    assert np.array_equal(up, tiers[3][0])


def test_prepare_restatement_and_margin_band():
    x = np.array([[1.0, 2.0, 3.0, 6.0], [0.0, 0.0, 0.0, 0.0]])
    c = ref.prepare(x, centered=True)
    assert np.allclose(c[0], x[0] / 3.0) and np.isnan(c[1]).all()
    n = ref.prepare(x, l2_normalized=True)
    assert np.allclose(n[0], x[0] / np.sqrt(50.0)) and np.isnan(n[1]).all()
    both = ref.prepare(x, centered=True, l2_normalized=True)
    assert np.allclose(both[0], (x[0] / 3.0) / np.linalg.norm(x[0] / 3.0))
    X = np.array([[3.0, 4.0]])  # ||x||^2 25, max cnorm 75: tolerance 1e-3
    assert ref.margin_band(X, np.array([1.0]), np.array([1.0009]), 75.0).tolist() == [True]
    assert ref.margin_band(X, np.array([1.0]), np.array([1.0011]), 75.0).tolist() == [False]
    assert ref.margin_band(X, np.array([[1.0, 1.0]]), np.array([[2.0, 1.0005]]), 75.0).tolist() == [True]
    assert ref.margin_band(X, np.array([[1.0, 1.0]]), np.array([[2.0, np.inf]]), 75.0).tolist() == [False]


# --------------------------------------------------------------------------- C ABI
P = ctypes.c_void_p
ENTRY = ("hvk_ss_prepare", "hvk_ss_accumulate", "hvk_ss_finalize", "hvk_ss_predict_flat", "hvk_ss_predict_tree")
TB1 = (ctypes.c_int * 2)(0, 10)
TB3 = (ctypes.c_int * 4)(0, 2, 5, 15)


def _args(name, **over):
    """A valid argument list of entry point `name` (device addresses never dereferenced before a
    launch; tier_base is a real host array)."""
    a = {
        "hvk_ss_prepare": dict(x=P(0x1000), dtype=0, B=4, D=8, ld=8, centered=1, l2n=1, out=P(0x2000), stream=None),
        "hvk_ss_accumulate": dict(x=P(0x1000), B=4, D=8, labels=P(0x2000), t_stride=7, t_off=6, order=P(0x3000),
                                  L=10, sums=P(0x4000), counts=P(0x5000), state=P(0x6000), stream=None),
        "hvk_ss_finalize": dict(sums=P(0x4000), counts=P(0x5000), D=8, n_tiers=3, tier_base=TB3,
                                child_ptr=P(0x7000), child_idx=P(0x8000), centroids=P(0x9000), cnorm=P(0xa000),
                                stream=None),
        "hvk_ss_predict_flat": dict(x=P(0x1000), B=4, D=8, centroids=P(0x9000), cnorm=P(0xa000), L=10,
                                    pred=P(0xb000), workspace=P(0xc000), workspace_bytes=1 << 20, stream=None),
        "hvk_ss_predict_tree": dict(x=P(0x1000), B=4, D=8, centroids=P(0x9000), counts=P(0x5000), n_tiers=3,
                                    tier_base=TB3, child_ptr=P(0x7000), child_idx=P(0x8000), pred=P(0xb000),
                                    stream=None),
    }[name]
    assert set(over) <= set(a), (name, over)
    a.update(over)
    return list(a.values())


def test_symbols_exported_and_bound():
    from hvamd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY + ("hvk_ss_predict_flat_workspace",):
        assert name in _lib.SIGNATURES and hasattr(raw, name), name
        assert len(_lib.SIGNATURES[name][1]) == (2 if name.endswith("workspace") else len(_args(name)))
    assert _lib.ABI_VERSION >= 18 and _lib.load().hvk_abi_version() == _lib.ABI_VERSION


_NULLS = {"hvk_ss_prepare": ("x", "out"),
          "hvk_ss_accumulate": ("x", "labels", "order", "sums", "counts", "state"),
          "hvk_ss_finalize": ("sums", "counts", "tier_base", "child_ptr", "child_idx", "centroids", "cnorm"),
          "hvk_ss_predict_flat": ("x", "centroids", "cnorm", "pred", "workspace"),
          "hvk_ss_predict_tree": ("x", "centroids", "counts", "tier_base", "child_ptr", "child_idx", "pred")}
BAD = [(n, {k: None}, b"null") for n, ks in _NULLS.items() for k in ks]
BAD += [(n, dict(B=-1), b"shape") for n in ENTRY if n != "hvk_ss_finalize"]
BAD += [(n, dict(D=0), b"shape") for n in ENTRY]
BAD += [("hvk_ss_accumulate", dict(L=0), b"shape"), ("hvk_ss_predict_flat", dict(L=0), b"shape"),
        ("hvk_ss_predict_flat", dict(D=6), b"multiple of 4"), ("hvk_ss_predict_flat", dict(D=1), b"multiple of 4"),
        ("hvk_ss_predict_flat", dict(x=P(0x1004)), b"aligned"),
        ("hvk_ss_predict_flat", dict(workspace_bytes=8), b"workspace"),
        ("hvk_ss_prepare", dict(ld=7), b"shape"), ("hvk_ss_prepare", dict(dtype=2), b"dtype"),
        ("hvk_ss_prepare", dict(dtype=-1), b"dtype"),
        ("hvk_ss_accumulate", dict(t_off=7), b"stride"), ("hvk_ss_accumulate", dict(t_stride=0, t_off=0), b"stride"),
        ("hvk_ss_accumulate", dict(t_off=-1), b"stride"),
        ("hvk_ss_finalize", dict(n_tiers=0), b"n_tiers"), ("hvk_ss_predict_tree", dict(n_tiers=9), b"n_tiers"),
        ("hvk_ss_finalize", dict(tier_base=(ctypes.c_int * 4)(0, 2, 2, 15)), b"tier_base"),
        ("hvk_ss_predict_tree", dict(tier_base=(ctypes.c_int * 4)(1, 2, 5, 15)), b"tier_base")]


@pytest.mark.parametrize("name,over,word", BAD, ids=[f"{b[0][7:]}-{'-'.join(b[1])}-{i}" for i, b in enumerate(BAD)])
def test_invalid_arguments_refused_before_any_launch(name, over, word):
    from hvamd import _lib
    lib = _lib.load()
    assert getattr(lib, name)(*_args(name, **over)) == HVK_EINVAL
    msg = lib.hvk_last_error_string()
    assert name.encode() in msg and word in msg, msg


def test_empty_batch_is_ok_without_a_launch():
    from hvamd import _lib
    lib = _lib.load()
    for name in ENTRY:
        if name != "hvk_ss_finalize":
            assert getattr(lib, name)(*_args(name, B=0)) == HVK_OK, name
    assert lib.hvk_ss_predict_flat(*_args("hvk_ss_predict_flat", B=0, workspace=None, workspace_bytes=0)) == HVK_OK
    assert lib.hvk_ss_predict_flat(*_args("hvk_ss_predict_flat", B=0, D=6)) == HVK_EINVAL  # still validated
    assert lib.hvk_ss_predict_tree(*_args("hvk_ss_predict_tree", B=0, n_tiers=1, tier_base=TB1, child_ptr=None,
                                          child_idx=None)) == HVK_OK


def test_flat_workspace_arithmetic():
    """8 bytes per (split, row); the splits cover the 64-class tiles, about 512 workgroups in all."""
    from hvamd import _lib
    ws = _lib.load().hvk_ss_predict_flat_workspace
    assert ws(0, 10) == 0 and ws(4, 0) == 0 and ws(-1, 10) == 0
    assert ws(1, 2) == 8 and ws(67, 37) == 67 * 8
    assert ws(300, 400) == 300 * 8 * 7      # 7 class tiles, 5 row tiles: one tile per split
    assert ws(256, 10000) == 256 * 8 * 79   # 157 tiles over 128 wanted splits: 2 per split, 79 splits
    for B, L in ((1, 1), (64, 64), (65, 65), (1000, 100000)):
        n = ws(B, L)
        assert n % (8 * B) == 0 and 1 <= n // (8 * B) <= (L + 63) // 64


# --------------------------------------------------------------------------- CSR children lists
@pytest.mark.parametrize("sizes", [(2, 3, 4, 5, 6, 7, 12), (3, 13, 51, 273, 1103, 4884, 10000)])
def test_children_csr_matches_parent_vectors(sizes):
    from hvamd import hierarchy, simpleshot
    tax = hierarchy.Taxonomy.synthetic(sizes)
    vecs = hierarchy.parent_vectors([hierarchy.HierarchicalLabel.parse(c) for c in tax.classes])
    got_sizes, tier_base, child_ptr, child_idx = simpleshot.children_csr(vecs)
    assert got_sizes == tuple(tax.num_classes) and tier_base.tolist() == [0, *np.cumsum(sizes)]
    assert child_ptr.dtype == child_idx.dtype == tier_base.dtype == np.int32
    assert len(child_ptr) == sum(sizes[:-1]) + 1 and len(child_idx) == sum(sizes[1:])
    assert child_ptr[0] == 0 and child_ptr[-1] == len(child_idx) and (np.diff(child_ptr) >= 1).all()
    for t, vec in enumerate(vecs):
        for i in range(sizes[t]):
            kids = child_idx[child_ptr[tier_base[t] + i]:child_ptr[tier_base[t] + i + 1]]
            assert kids.tolist() == np.flatnonzero(vec == i).tolist()
    # and the leaf paths the taxonomy holds climb through the same parents
    for t, vec in enumerate(vecs):
        assert np.array_equal(vec[tax.leaf_paths[:, t + 1]], tax.leaf_paths[:, t])


def test_children_csr_non_contiguous_children_and_bad_parents():
    from hvamd import simpleshot
    sizes, tier_base, child_ptr, child_idx = simpleshot.children_csr([np.array([1, 0, 1, 0, 1], np.uint16)])
    assert sizes == (2, 5) and tier_base.tolist() == [0, 2, 7]
    assert child_ptr.tolist() == [0, 2, 5] and child_idx.tolist() == [1, 3, 0, 2, 4]
    with pytest.raises(ValueError):
        simpleshot.children_csr([])
    with pytest.raises(ValueError):
        simpleshot.children_csr([np.array([0, 1]), np.array([0, 2, 1])])


# --------------------------------------------------------------------------- Python surface
def test_wrappers_refuse_cpu_tensors():
    import hvamd.ops as ops
    from hvamd import simpleshot
    x, y = torch.zeros(4, 8), torch.zeros(4, dtype=torch.int64)
    calls = [lambda: ops.ss_prepare(x), lambda: simpleshot.center(x), lambda: simpleshot.l2_normalize(x),
             lambda: ops.ss_accumulate(x, y, torch.zeros(3, 8, dtype=torch.float64),
                                       torch.zeros(3, dtype=torch.int64), torch.zeros(4, dtype=torch.float64)),
             lambda: ops.ss_finalize(torch.zeros(3, 8, dtype=torch.float64), torch.zeros(3, dtype=torch.int64),
                                     [0, 3], None, None),
             lambda: ops.ss_predict_flat(x, torch.zeros(3, 8), torch.zeros(3)),
             lambda: ops.ss_predict_tree(x, torch.zeros(3, 8), torch.zeros(3, dtype=torch.int64), [0, 3], None, None),
             lambda: simpleshot.NearestCentroid().fit(x, y),
             lambda: simpleshot.NearestCentroid(n_classes=3).partial_fit(x, y),
             lambda: simpleshot.HierarchicalNearestCentroid(ref.tree_sizes_lookup((2, 3, 4, 5, 6, 7, 12))).fit(
                 x, torch.zeros(4, 7, dtype=torch.int64))]
    for i, c in enumerate(calls):
        with pytest.raises(RuntimeError, match="GPU only"):
            c()
            pytest.fail(f"call {i} accepted a CPU tensor")


def test_classifier_state_errors():
    from hvamd import simpleshot
    clf = simpleshot.NearestCentroid(n_classes=3)
    with pytest.raises(RuntimeError, match="not fitted"):
        clf.predict(torch.zeros(1, 4))
    with pytest.raises(RuntimeError, match="finalize"):
        clf.finalize()
    with pytest.raises(ValueError, match="n_classes"):
        simpleshot.NearestCentroid().partial_fit(torch.zeros(1, 4), torch.zeros(1, dtype=torch.int64))
    h = simpleshot.HierarchicalNearestCentroid(ref.tree_sizes_lookup((2, 3, 4, 5, 6, 7, 12)))
    assert h.tier_sizes == (2, 3, 4, 5, 6, 7, 12)
    with pytest.raises(RuntimeError, match="not fitted"):
        h.centroids_


def test_evaluate_refuses_a_non_feature_model():
    from hvamd import configs, simpleshot
    cfg = configs.Config()
    with pytest.raises(ValueError, match="FeatureOnlyModel"):
        simpleshot.evaluate(cfg, torch.nn.Linear(4, 4), [], [])


def test_evaluate_hierarchical_needs_lookup_vectors():
    from hvamd import configs, models, simpleshot
    cfg = configs.Config()
    cfg.simpleshot.hierarchical = True

    class Backbone(torch.nn.Module):
        pass

    with pytest.raises(ValueError, match="lookup_vecs"):
        simpleshot.evaluate(cfg, models.FeatureOnlyModel(Backbone()), [], [])


def test_hierarchy_exposes_the_same_class_without_an_import_cycle():
    """hierarchy resolves the name on first use (simpleshot imports ops only), whichever of the two
    modules was loaded first."""
    import importlib
    import sys
    saved = {k: sys.modules.pop(k) for k in ("hvamd.hierarchy", "hvamd.simpleshot") if k in sys.modules}
    try:
        for first in ("hvamd.simpleshot", "hvamd.hierarchy"):
            for k in ("hvamd.hierarchy", "hvamd.simpleshot"):
                sys.modules.pop(k, None)
            importlib.import_module(first)
            h, s = importlib.import_module("hvamd.hierarchy"), importlib.import_module("hvamd.simpleshot")
            assert h.HierarchicalNearestCentroid is s.HierarchicalNearestCentroid
            with pytest.raises(AttributeError):
                h.no_such_name
    finally:
        for k in ("hvamd.hierarchy", "hvamd.simpleshot"):
            sys.modules.pop(k, None)
        sys.modules.update(saved)
