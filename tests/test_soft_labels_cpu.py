"""Host side of the soft-labels loss: the normalisers against the restatement
(tests/soft_labels_ref.py), the ABI symbols and the config wiring."""
import ctypes

import numpy as np
import pytest
import torch

import soft_labels_ref as S
from hxe_soft_ref import shuffled_tree


@pytest.mark.parametrize("tree", ["small", "shuffled40", "chain"])
@pytest.mark.parametrize("beta", [4.0, 15.0])
def test_soft_label_norms_vs_restatement(tree, beta):
    from hvamd.hierarchy import Taxonomy
    tax = {"small": lambda: Taxonomy.synthetic((2, 3, 4, 5, 6, 7, 12)),
           "shuffled40": lambda: shuffled_tree(40),
           "chain": lambda: Taxonomy.synthetic((1, 1, 1, 1, 1, 2, 33))}[tree]()
    w = S.level_weights64(beta)
    inv = tax.soft_label_norms(w)
    assert inv.dtype == torch.float32 and inv.shape == (tax.num_leaves,)
    _, Z = S.effective_targets(tax, np.zeros((1, tax.num_leaves)), w)
    assert np.abs(inv.numpy() * Z - 1).max() < 1e-6
    assert tax.soft_label_norms(w) is inv  # cached per weights
    with pytest.raises(ValueError):
        tax.soft_label_norms([0.0] + [1.0] * 7)


def test_level_weights_beta_zero_is_uniform():
    from hvamd.hierarchy import soft_label_level_weights
    assert torch.equal(soft_label_level_weights(0), torch.ones(8))
    assert np.allclose(soft_label_level_weights(15.0).numpy(), S.level_weights64(15.0), rtol=1e-6)


@pytest.mark.parametrize("name", ["hvk_soft_labels_fwd", "hvk_soft_labels_bwd",
                                  "hvk_soft_labels_dense_fwd", "hvk_soft_labels_dense_bwd"])
def test_symbols_declared_and_exported(name):
    from hvamd import _lib
    assert name in _lib.SIGNATURES
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)


def test_composer_model_soft_labels_wiring():
    from hvamd import configs, models
    hierarchy = models.hierarchy  # the module object models.py builds from, whatever reloaded since
    cfg = configs.Config()
    assert cfg.hierarchy.soft_labels_beta == 15.0
    cfg.model.name = "swinv2_tiny_window7_224"
    cfg.hierarchy.variant = "soft-labels"
    cfg.hierarchy.soft_labels_beta = 6.0
    tax = hierarchy.Taxonomy.synthetic((2, 3, 4, 5, 6, 7, 12))
    m = models.build_composer_model(cfg, models.DatasetInfo(num_classes=tax.num_classes, taxonomy=tax))
    assert isinstance(m.loss_fn, hierarchy.SoftLabelsCrossEntropy) and m.loss_fn.beta == 6.0
    assert torch.equal(m.loss_fn.level_weight, hierarchy.soft_label_level_weights(6.0))
    assert m.module.head.out_features == 12
    assert list(m.get_metrics(is_train=True)) == ["cross-entropy", "acc@1", "acc@5"]
    assert m.fused_metrics().taxonomy is tax
    with pytest.raises(NotImplementedError, match="per-tier list"):
        m.loss_fn(torch.zeros(2, 12), [torch.zeros(2, 2)] * 7)
    with pytest.raises(ValueError, match="soft-labels needs DatasetInfo.taxonomy"):
        models.build_composer_model(cfg, models.DatasetInfo(num_classes=12))
    cfg.hierarchy.variant = "soft_labels"  # unknown spellings still raise
    with pytest.raises(ValueError):
        models.build_composer_model(cfg, models.DatasetInfo(num_classes=12, taxonomy=tax))
