"""Back-off decoding without a GPU: the ABI-24 symbols, the slot limit, the device tables, the
threshold rules and the float64 restatement on a hand-computed row."""
import os
import re

import numpy as np
import pytest
import torch

import backoff_ref as ref
from hvamd import _lib, ops
from hvamd.hierarchy import BackoffMetrics, Taxonomy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "hvk.h")).read()
    assert int(re.search(r"#define\s+HVK_ABI_VERSION\s+(\d+)", hdr).group(1)) >= 24
    lib = _lib.load()
    assert _lib.ABI_VERSION >= 24 and lib.hvk_abi_version() == _lib.ABI_VERSION
    for name, n_args in (("hvk_backoff_supported", 1), ("hvk_backoff_decode", 21)):
        decl = re.sub(r"/\*.*?\*/", "", re.search(r"\nint " + name + r"\(([^;]*)\);", hdr).group(1))
        assert len(decl.split(",")) == n_args == len(_lib.SIGNATURES[name][1]) and hasattr(lib, name)
    assert ops.backoff_supported((0, 3, 16, 67, 340, 1443, 6327, 6328)) and ops.backoff_supported((0, 1, 2, 3, 4, 5, 15359, 15360))
    assert not any(ops.backoff_supported(o) for o in ((0, 1, 2, 3, 4, 5, 15360, 15361), (0, 1, 2, 2, 4, 5, 9, 10),
                                                      (0, 1, 2, 3, 4, 5, 9, 11)))


def test_device_backoff_tables_are_the_soft_tables():
    tax = Taxonomy.synthetic((1, 2, 3, 5, 9, 17, 131))
    assert tax.device_backoff_tables("cpu")[0] is None  # the identity
    order = np.random.default_rng(7).permutation(tax.num_leaves)
    tax = Taxonomy([f"{order[i]:05d}_" + c.split("_", 1)[1] for i, c in enumerate(tax.classes)])
    perm, *tables = tax.device_backoff_tables("cpu")
    soft = tax.soft_tables()
    assert not tax.identity_perm and np.array_equal(perm.numpy(), tax.perm)
    for got, want in zip(tables, (soft[0], soft[1], soft[2], soft[4])):
        assert got.dtype == torch.int32 and np.array_equal(got.numpy(), want)
    assert tax.device_backoff_tables("cpu") is tax.device_backoff_tables("cpu")  # cached
    assert len(tax.device_soft_tables("cpu")) == 5 and tax.device_soft_tables("cpu")[4].shape == (131, 6)


@pytest.mark.parametrize("bad", [(), (0.0, 0.5), (0.5, 1.5), (0.5, 0.5), (0.6, 0.5), (float("nan"),),
                                 (0.5, 0.5 + 1e-9), tuple(np.linspace(0.1, 0.9, 33)), 0.5])
def test_threshold_validation(bad):
    with pytest.raises(ValueError):
        BackoffMetrics(Taxonomy.synthetic((1, 2, 3, 5, 9, 17, 131)), thresholds=bad)


def test_reference_on_a_hand_computed_row():
    """Two families, genera (a: 2 leaves, b: 1 | c: 1): p = (.3, .3, .05 | .35).  The walk takes family 0
    (.65), genus a (.6), the first of its equal leaves (.3): not the argmax leaf (.35, the other family)."""
    tax = Taxonomy(["0_k_p_c_o_f0_a_s0", "1_k_p_c_o_f0_a_s1", "2_k_p_c_o_f0_b_s2", "3_k_p_c_o_f1_c_s3"])
    p = np.array([[0.3, 0.3, 0.05, 0.35]])
    assert np.allclose(ref.softmax(np.log(p)), p)
    masses = ref.node_masses(p, tax.leaf_paths)
    assert np.allclose(masses[4], [[0.65, 0.35]]) and np.allclose(masses[5], [[0.6, 0.05, 0.35]])
    path, q = ref.greedy(masses, tax.leaf_paths, tax.perm)
    assert path.tolist() == [[0, 0, 0, 0, 0, 0, 0]] and np.allclose(q, [[1, 1, 1, 1, 0.65, 0.6, 0.3]])
    assert [int(ref.depth(q, t)[0]) for t in (0.2, 0.5, 0.62, 0.7)] == [7, 6, 5, 4]
    assert ref.agreement(path, tax.leaf_paths[[1, 3]]).tolist() == [6, 4]
    s = ref.fold(np.repeat(path, 3, 0), np.repeat(q, 3, 0).astype(np.float32), np.array([6, 4, -1]), (0.2, 0.62))
    assert s.tolist() == [2, 1, 14, 0, 10, 2, 0, 10, 1, 9, 0, 0]
