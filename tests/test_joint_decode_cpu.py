"""Joint path decoding without a GPU: the ABI-22 symbols, the LDS limit, the parent tables and the
EvalMetrics surface of decoding="joint" / "joint-crm"."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from hvamd import _lib
from hvamd.hierarchy import EvalMetrics, Taxonomy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INAT21 = (3, 13, 51, 273, 1103, 4884, 10000)


def _offsets(sizes):
    return (ctypes.c_int * 8)(*np.r_[0, np.cumsum(sizes)].tolist())


def test_symbols_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "hvk.h")).read()
    assert int(re.search(r"#define\s+HVK_ABI_VERSION\s+(\d+)", hdr).group(1)) >= 22
    lib = _lib.load()
    assert _lib.ABI_VERSION >= 22 and lib.hvk_abi_version() == _lib.ABI_VERSION
    for name, n_args in (("hvk_joint_supported", 1), ("hvk_joint_decode", 23)):
        decl = re.search(r"\nint " + name + r"\(([^;]*)\);", hdr).group(1)
        decl = re.sub(r"/\*.*?\*/", "", decl)
        assert len(decl.split(",")) == n_args == len(_lib.SIGNATURES[name][1]) and hasattr(lib, name)


@pytest.mark.parametrize("sizes,ok", [(INAT21, 1), ((3, 13, 51, 273, 1103, 13917, 10000), 1),
                                      ((3, 13, 51, 273, 1103, 13918, 10000), 0), ((3, 13, 0, 273, 1103, 4884, 10000), 0)])
def test_joint_supported_is_the_lds_limit(sizes, ok):
    """Tiers 0-5 hold at most 15360 nodes; hvk_joint_decode refuses more before any launch."""
    lib = _lib.load()
    assert lib.hvk_joint_supported(_offsets(sizes)) == ok
    if not ok and min(sizes) > 0:
        args = [ctypes.c_void_p(16), 0, 1, 1 << 20, _offsets(sizes), None, 1, 0, None, None, None, 5] + [None] * 11
        rc = lib.hvk_joint_decode(*args)
        assert rc == 2 and b"15360" in lib.hvk_last_error_string()


@pytest.mark.parametrize("shuffled", [False, True])
def test_parent_tables_agree_with_leaf_paths(shuffled):
    tax = Taxonomy.synthetic((1, 2, 3, 5, 9, 17, 131))
    if shuffled:
        order = np.random.default_rng(7).permutation(tax.num_leaves)
        tax = Taxonomy([f"{order[i]:05d}_" + c.split("_", 1)[1] for i, c in enumerate(tax.classes)])
        assert not tax.identity_perm
    off, parents = tax.parent_tables()
    assert off.dtype == parents.dtype == np.int32 and off.tolist() == np.r_[0, np.cumsum(tax.num_classes)].tolist()
    assert parents.shape == (off[7] - off[1],) and tax.parent_tables()[1] is parents  # cached
    for t in range(1, 7):
        assert np.array_equal(parents[off[t] - off[1] + tax.leaf_paths[:, t]], tax.leaf_paths[:, t - 1])
        assert parents[off[t] - off[1]:off[t + 1] - off[1]].max() < tax.num_classes[t - 1]


@pytest.mark.parametrize("decoding", ["joint", "joint-crm"])
def test_eval_metrics_joint_surface(decoding):
    tax = Taxonomy.synthetic((1, 2, 3, 5, 9, 17, 131))
    with pytest.raises(ValueError, match="taxonomy"):
        EvalMetrics(decoding=decoding)
    m = EvalMetrics(taxonomy=tax, decoding=decoding, topk=3)
    with pytest.raises(ValueError, match="7 tier"):
        m.update(torch.zeros(2, 131), torch.zeros(2, dtype=torch.int64))
    assert list(EvalMetrics().state_dict()) == ["state"]
    assert list(EvalMetrics(taxonomy=tax, decoding="crm").state_dict()) == ["state"]
    assert list(m.state_dict()) == ["state", "joint_state"]
    m.state[0] = m.joint_state[0] = 8
    m.joint_state[1:5] = torch.tensor([4.0, 6.0, 16.0, 12.0], dtype=torch.float64)
    m.joint_state[6:16] = torch.tensor([8, 8, 7, 6, 5, 4, 4, 2, 20, 6], dtype=torch.float64)
    got = m.compute()
    want = {"acc@1/joint": 0.5, "acc@3/joint": 0.75, "cross-entropy/joint": 2.0, "tree-dist/joint": 1.5,
            "path-consistency": 0.75, **{f"acc@1/joint/tier{t}": v / 8 for t, v in enumerate((8, 8, 7, 6, 5, 4, 4))}}
    if decoding == "joint-crm":
        want.update({"acc@1/joint-crm": 0.25, "tree-dist/joint-crm": 2.5})
    assert {k: got[k] for k in got if "joint" in k or k == "path-consistency"} == want
    m.reset()
    assert not m.joint_state.any()
