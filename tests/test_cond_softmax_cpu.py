"""The conditional softmax without a GPU: the ABI-25 symbols, the decoder's LDS limit, the sibling
tables, the config / model wiring and the float64 restatement's normalisation."""
import os
import re

import numpy as np
import pytest
import torch

import cond_softmax_ref as ref
from hvamd import _lib, configs, hierarchy, models, ops
from hvamd.hierarchy import Taxonomy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = (1, 2, 3, 5, 9, 17, 131)


def _shuffled():
    tax = Taxonomy.synthetic(SMALL)
    order = np.random.default_rng(7).permutation(tax.num_leaves)
    return Taxonomy([f"{order[i]:05d}_" + c.split("_", 1)[1] for i, c in enumerate(tax.classes)])


def test_symbols_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "hvk.h")).read()
    assert int(re.search(r"#define\s+HVK_ABI_VERSION\s+(\d+)", hdr).group(1)) >= 25
    lib = _lib.load()
    assert _lib.ABI_VERSION >= 25 and lib.hvk_abi_version() == _lib.ABI_VERSION
    for name, n_args in (("hvk_cond_softmax_supported", 1), ("hvk_cond_softmax_fwd", 15),
                         ("hvk_cond_softmax_bwd", 16), ("hvk_cond_softmax_decode", 22)):
        decl = re.sub(r"/\*.*?\*/", "", re.search(r"\nint " + name + r"\(([^;]*)\);", hdr).group(1))
        assert len(decl.split(",")) == n_args == len(_lib.SIGNATURES[name][1]) and hasattr(lib, name)
    assert ops.cond_softmax_supported((3, 13, 51, 273, 1103, 4884, 10000))
    assert ops.cond_softmax_supported((1, 1, 1, 1, 1, 15355, 7))  # tiers 0-5: 15360 nodes
    assert not ops.cond_softmax_supported((1, 1, 1, 1, 1, 15356, 7))
    assert not ops.cond_softmax_supported((1, 1, 0, 1, 1, 5, 7)) and not ops.cond_softmax_supported((1, 2, 3))


@pytest.mark.parametrize("tree", ["identity", "shuffled"])
def test_sibling_tables_against_brute_force(tree):
    tax = Taxonomy.synthetic(SMALL) if tree == "identity" else _shuffled()
    sib_ptr, sib_col = tax.sibling_tables()
    off, paths = tax.parent_tables()[0], tax.leaf_paths
    assert sib_ptr.dtype == sib_col.dtype == np.int32 and len(sib_ptr) == off[6] + 2 and len(sib_col) == off[7]
    assert tax.sibling_tables() is tax.sibling_tables()  # cached
    groups = [np.arange(off[1])]  # the root's children, then by (parent tier, parent id)
    for t in range(1, 7):
        groups += [off[t] + np.unique(paths[paths[:, t - 1] == p, t]) for p in range(off[t] - off[t - 1])]
    assert np.array_equal(sib_ptr, np.r_[0, np.cumsum([len(g) for g in groups])])
    assert np.array_equal(sib_col, np.concatenate(groups))
    assert all(sib_ptr[1 + off[t]] == off[t + 1] for t in range(6))  # tier t = positions [off[t], off[t + 1])
    dev_ptr, dev_col = tax.device_sibling_tables("cpu")
    assert np.array_equal(dev_ptr.numpy(), sib_ptr)
    if tree == "identity":
        assert tax.identity_siblings and dev_col is None
    else:
        assert not tax.identity_siblings and np.array_equal(dev_col.numpy(), sib_col)


def test_config_and_model_wiring():
    tax = Taxonomy.synthetic((2, 3, 4, 5, 6, 7, 12))
    cfg = configs.Config()
    assert cfg.hierarchy.cond_softmax_smoothing == 0.0
    cfg.model.name = "swinv2_tiny_window7_224"
    cfg.hierarchy.variant, cfg.hierarchy.cond_softmax_smoothing = "cond-softmax", 0.1
    cfg.hierarchy.multitask_coeffs = [8, 5.65, 4, 2.82, 2, 1.41, 1]
    info = models.DatasetInfo(num_classes=tax.num_leaves, taxonomy=tax)
    m = models.build_composer_model(cfg, info, img_size=56, embed_dim=32, depths=[2, 2], num_heads=[1, 2], window_size=7)
    assert isinstance(m.module.head, hierarchy.MultitaskHead) and m.module.head.num_classes == tuple(tax.num_classes)
    assert isinstance(m.loss_fn, hierarchy.ConditionalSoftmaxCrossEntropy)
    assert m.loss_fn.coeffs == (8, 5.65, 4, 2.82, 2, 1.41, 1) and m.loss_fn.smoothing == 0.1
    assert set(m.train_metrics) == {"cross-entropy", "acc@1", "acc@5"} == set(m.val_metrics)
    assert m.fused_metrics().decoding == "cond" and m.fused_metrics(decoding="cond-crm").taxonomy is tax
    assert hierarchy.ConditionalSoftmaxCrossEntropy(tax, coeffs=[]).coeffs == (1.0,) * 7
    with pytest.raises(ValueError):
        models.build_composer_model(cfg, models.DatasetInfo(num_classes=12))


@pytest.mark.parametrize("kind", ["float", "list"])
def test_probability_targets_are_refused(kind):
    tax = Taxonomy.synthetic(SMALL)
    outputs = [torch.zeros(2, n) for n in tax.num_classes]
    soft = [torch.full((2, n), 1.0 / n) for n in tax.num_classes]
    with pytest.raises(ValueError, match="smoothing="):
        hierarchy.ConditionalSoftmaxCrossEntropy(tax)(outputs, soft if kind == "list" else soft[-1])


@pytest.mark.parametrize("tree", ["identity", "shuffled"])
def test_reference_is_normalised(tree):
    tax = Taxonomy.synthetic(SMALL) if tree == "identity" else _shuffled()
    rng = np.random.default_rng(3)
    zs = [torch.from_numpy(3 * rng.standard_normal((4, n))) for n in tax.num_classes]
    logp = ref.leaf_logp(zs, tax.leaf_paths)
    assert torch.allclose(torch.exp(logp).sum(1), torch.ones(4, dtype=torch.float64), rtol=0, atol=1e-13)
    y = tax.leaf_paths[[5, 77, 130, 0]]
    total, _, terms = ref.loss(zs, tax.leaf_paths, y, (1,) * 7, 0.0)  # eps = 0: the loss is -log p(leaf)
    assert torch.allclose(terms.sum(1), -logp[torch.arange(4), torch.as_tensor(y[:, 6])], rtol=0, atol=1e-12)
