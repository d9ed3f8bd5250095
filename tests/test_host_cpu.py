"""CPU-only checks: C-ABI exports, host-side taxonomy logic (bit-exact vs the reference's
goldens), config layering, algorithms, model surface and state-dict parity."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    hdr = open(os.path.join(ROOT, "include", "hvk.h")).read()
    return sorted(set(re.findall(r"\b(hvk_[a-z0-9_]+)\s*\(", hdr)))


def test_library_exports_every_declared_symbol():
    from hvamd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    declared = _declared_symbols()
    assert len(declared) >= 15
    for name in declared:
        assert hasattr(lib, name), name
    assert set(declared) == set(_lib.SIGNATURES), set(declared) ^ set(_lib.SIGNATURES)
    # and nothing else: internal helpers are hidden, so the export table IS the ABI
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True)
    if nm.returncode == 0:
        exported = {ln.split()[-1] for ln in nm.stdout.splitlines() if " T hvk_" in ln}
        assert exported == set(declared), exported ^ set(declared)
    lib = _lib.load()
    assert lib.hvk_abi_version() == _lib.ABI_VERSION
    # [accumulators][dscale nH][dq_bias 32 nH] floats
    # [heads][slots: 512 / heads][R*R CPB bins, d scale, 32 d q_bias] f32 (deterministic reduction)
    assert lib.hvk_wmsa_bwd_workspace_bytes(3, 7) == 3 * (512 // 3) * (13 * 13 + 33) * 4
    assert lib.hvk_wmsa_bwd_workspace_bytes(4, 24) == 4 * 64 * (47 * 47 + 33) * 4
    # weight-gradient plan: one tile, 256 token chunks of [dW | db] partials
    assert lib.hvk_weight_grad_supported(802816, 288, 96) == 1
    assert lib.hvk_weight_grad_workspace(802816, 288, 96) == 256 * (288 * 96 + 288) * 4
    assert lib.hvk_weight_grad_supported(802816 + 16, 288, 96) == 0  # M % 32
    assert lib.hvk_weight_grad_supported(4096, 100, 96) == 0


def test_abi_version_agrees_everywhere():
    """include/hvk.h's HVK_ABI_VERSION, the library's hvk_abi_version(), the Python binding's
    ABI_VERSION and the version INTEGRATION.md's binding example asserts are one number."""
    from hvamd import _lib
    hdr = open(os.path.join(ROOT, "include", "hvk.h")).read()
    m = re.search(r"#define\s+HVK_ABI_VERSION\s+(\d+)", hdr)
    assert m, "include/hvk.h defines no HVK_ABI_VERSION"
    v = int(m.group(1))
    assert _lib.ABI_VERSION == v
    assert _lib.load().hvk_abi_version() == v
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    asserted = [int(x) for x in re.findall(r"hvk_abi_version\(\)\s*==\s*(\d+)", doc)]
    assert asserted and all(a == v for a in asserted), (asserted, v)


def test_product_modules_read_no_environment():
    """Routing switches live in hvamd.options (printed by bench.py), not in the environment:
    no product module reads os.environ / os.getenv except _lib.py's HVK_LIB_PATH."""
    pkg = os.path.join(ROOT, "hierarchical-vision_amd")
    for fn in sorted(os.listdir(pkg)):
        if not fn.endswith(".py"):
            continue
        for ln in open(os.path.join(pkg, fn)):
            if "os.environ" in ln or "getenv(" in ln:
                assert fn == "_lib.py" and "HVK_LIB_PATH" in ln, (fn, ln)


def test_bounds_build_not_broken():
    """__graft_entry__.build() keeps the bounds-checking debug build optional for the product,
    but records its failure; W-MSA memory-safety coverage (tests/test_gpu_wmsa.py) must not
    disappear silently."""
    marker = os.path.join(ROOT, "hierarchical-vision_amd", "BOUNDS_BUILD_FAILED.txt")
    assert not os.path.exists(marker), open(marker).read()


def test_host_options_object():
    from hvamd import options
    assert options.non_default() == {}
    with options.override(qk_epilogue=False, mlp_fused=0):
        assert options.OPTIONS.qk_epilogue is False and options.OPTIONS.mlp_fused is False
        assert set(options.non_default()) == {"qk_epilogue", "mlp_fused"}
    assert options.non_default() == {}
    assert options.parse("head_gemm=false") == {"head_gemm": 0}
    with pytest.raises(KeyError):
        options.set(no_such_option=1)


def test_library_rejects_bad_arguments_without_gpu():
    """Argument validation runs on the host before any launch."""
    from hvamd import _lib
    lib = _lib.load()
    rc = lib.hvk_wmsa_fwd(None, None, None, None, None, 1, 7, 7, 96, 3, 7, 0, None)
    assert rc == 1 and b"null" in lib.hvk_last_error_string()
    rc = lib.hvk_patch_merge_gather(ctypes.c_void_p(16), ctypes.c_void_p(16), 1, 7, 7, 32, None)
    assert rc == 1  # odd H
    rc = lib.hvk_bias_gelu_fwd(ctypes.c_void_p(16), None, ctypes.c_void_p(16), 4, 12, None)
    assert rc == 2  # N % 8


def test_library_options_table():
    """libhvk reads no environment variable: its selectable forms are named options with a
    range, set and read through the C ABI (include/hvk.h); unknown names and out-of-range
    values are refused."""
    from hvamd import _lib
    defaults = {"wmsa_fwd_form": 0, "wmsa_bwd_nt": 0, "wmsa_bwd_slice_bytes": 1 << 31,
                "tile_wide": -1, "dw_tile": 5, "wmsa_fwd_hg": 0, "dw_chunks": 256}
    for name, v in defaults.items():
        assert _lib.get_option(name) == v, name
    with _lib.option("wmsa_fwd_form", 1):
        assert _lib.get_option("wmsa_fwd_form") == 1
    assert _lib.get_option("wmsa_fwd_form") == 0
    for name, bad in [("wmsa_fwd_form", 2), ("dw_tile", 3), ("no_such_option", 0)]:
        with pytest.raises(RuntimeError):
            _lib.set_option(name, bad)
    for gone in ("gemm_pp", "gemm_xr", "gemm_wide"):  # the measured-slower GEMM forms were removed (round 6)
        with pytest.raises(RuntimeError):
            _lib.get_option(gone)
    src = os.path.join(ROOT, "hierarchical-vision_amd", "csrc")
    for f in os.listdir(src):
        if f.endswith((".hip", ".h")):
            assert "getenv" not in open(os.path.join(src, f)).read(), f


def test_ops_refuse_cpu_tensors():
    import hvamd.ops as ops
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.patch_merge_gather(torch.zeros(1, 16, 8, dtype=torch.bfloat16), 4, 4)


def test_taxonomy_tables_match_reference_assignment(golden):
    from hvamd import hierarchy
    g = golden("taxonomy_golden")
    names = list(g["synthetic.classes"])
    tax = hierarchy.Taxonomy(names)
    assert tax.num_classes == tuple(g["synthetic.num_classes"])
    assert np.array_equal(tax.leaf_paths, g["synthetic.ids"])
    # every node is one contiguous range of permuted leaves holding exactly its leaves
    ordered = tax.leaf_paths[tax.perm]
    for t in range(7):
        for node in np.random.default_rng(t).integers(0, tax.num_classes[t], 20):
            k = tax.tier_base[t] + node
            seg = ordered[tax.node_start[k]:tax.node_end[k], t]
            assert (seg == node).all() and len(seg) == (tax.leaf_paths[:, t] == node).sum()


def test_hand_labels_and_parent_lookup_bit_exact(golden):
    from hvamd import hierarchy
    g = golden("taxonomy_golden")
    classes, c2i, nc = hierarchy.assign_tier_ids(list(g["hand.classes"]))
    assert np.array_equal(np.stack([c2i[c].numpy() for c in classes]), g["hand.ids"])
    labels = [hierarchy.HierarchicalLabel.parse(c) for c in classes]
    assert [lb.clean_tiers for lb in labels] == [list(t) for t in g["hand.tiers"]]
    assert np.array_equal(np.array([[a.dist(b) for b in labels] for a in labels]), g["hand.dist"])
    dm = hierarchy.build_tree_dist_matrix(labels).numpy()
    assert np.array_equal(dm, g["hand.dist"])
    labels = [hierarchy.HierarchicalLabel.parse(n) for n in sorted(g["parent.names"])]
    for i, v in enumerate(hierarchy.parent_vectors(labels)):
        assert np.array_equal(v, g[f"parent.vec{i}"])


def test_hxe_level_coefficients_telescope():
    """uniform weights: HXE == flat CE on the leaf (only c_0 = -1 and c_7 = +1 survive)."""
    from hvamd.hierarchy import hxe_level_coeffs
    c = hxe_level_coeffs("uniform")
    assert torch.equal(c, torch.tensor([-1, 0, 0, 0, 0, 0, 0, 1.0]))
    c = hxe_level_coeffs("exponential", 0.1)
    assert abs(c.sum().item()) < 1e-6  # coefficients of a sum of differences sum to 0


def test_hxe_oracle_closed_form_known_answers():
    """PARITY UNPINNED by the reference (hierarchy.py:183-185): pin the oracle on a
    2-leaf-per-node toy tree where every term has a closed form."""
    from oracle import hierarchy_ref as H
    # 4 leaves: kingdom 0 -> {0,1}, kingdom 1 -> {2,3}; all lower tiers = leaf itself
    paths = np.array([[0, 0, 0, 0, 0, 0, 0], [0, 1, 1, 1, 1, 1, 1],
                      [1, 2, 2, 2, 2, 2, 2], [1, 3, 3, 3, 3, 3, 3]])
    z = np.array([[1.0, 2.0, 0.5, -1.0]])
    lam = H.hxe_level_weights("exponential", 0.1)
    lse = lambda v: np.log(np.exp(v).sum())  # noqa: E731
    # target leaf 1: levels 0..5 are the leaf itself, level 6 = kingdom {0,1}, level 7 = all
    p_king = lse(z[0, :2]) - lse(z[0])
    p_leaf = z[0, 1] - lse(z[0])
    want = -(lam[5] * (p_leaf - p_king) + lam[6] * (p_king - 0.0))
    got = H.hxe_loss(z, paths, np.array([1]), lam)
    assert abs(got - want) < 1e-12
    # uniform: exactly the flat CE of the leaf
    u = H.hxe_loss(z, paths, np.array([2]), H.hxe_level_weights("uniform", 0))
    assert abs(u - (lse(z[0]) - z[0, 2])) < 1e-12


def test_config_layering_and_reference_yaml():
    from hvamd import configs
    # the reference's configs/pretrain/r50_multitask_base.yaml, stored with the goldens
    ref_yaml = os.path.join(ROOT, "tests", "golden", "r50_multitask_base.yaml")
    cfg = configs.load_config(ref_yaml, overrides={"model": {"name": "swinv2_tiny_window7_224"},
                                                   "hierarchy": {"variant": "hxe"}})
    assert cfg.model.name == "swinv2_tiny_window7_224" and cfg.hierarchy.variant == "hxe"
    assert cfg.optim.name == "DecoupledSGDW" and cfg.seed == 42
    assert cfg.hierarchy.multitask_coeffs == [8, 5.65, 4, 2.82, 2, 1.41, 1]
    with pytest.raises(KeyError):
        configs.merge(configs.Config(), {"model": {"loss_name": "x"}})
    cfg = configs.merge(configs.Config(), {"algorithms": [{"cls": "LabelSmoothing",
                                                            "args": {"smoothing": 0.08}}]})
    assert cfg.algorithms[0].cls == "LabelSmoothing" and cfg.algorithms[0].args["smoothing"] == 0.08


def test_label_smoothing_list_semantics():
    from hvamd.algorithmic import Event, LabelSmoothing, State
    st = State(model=None)
    st.batch = (torch.zeros(2, 3), torch.tensor([[0, 1], [1, 2]]))
    st.outputs = [torch.zeros(2, 2), torch.zeros(2, 3)]
    ls = LabelSmoothing(smoothing=0.1)
    ls.apply(Event.BEFORE_LOSS, st)
    sm = st.batch[1]
    assert isinstance(sm, list) and len(sm) == 2
    assert torch.allclose(sm[1][1], torch.tensor([0.1 / 3, 0.1 / 3, 0.9 + 0.1 / 3]))
    ls.apply(Event.AFTER_LOSS, st)
    assert torch.equal(st.batch[1], torch.tensor([[0, 1], [1, 2]]))


def test_model_registry_state_dict_matches_reference(golden):
    from hvamd import models
    ref_keys = list(golden("model_golden")["tiny.state_keys"])
    net = models.create_model("swinv2_tiny_window7_224", num_classes=1000)
    assert list(net.state_dict().keys()) == ref_keys
    assert net.flops() == float(golden("model_golden")["tiny.macs"])
    with pytest.raises(ValueError, match="hot path"):
        models.create_model("resnet50")


def test_build_model_multitask_surgery_and_weight_init():
    from hvamd import configs, hierarchy, models
    cfg = configs.Config()
    cfg.model.name = "swinv2_tiny_window7_224"
    with pytest.raises(AssertionError):
        models.build_model(cfg, (3, 4))
    cfg.hierarchy.variant = "multitask"
    m = models.build_model(cfg, (3, 13, 51))
    assert isinstance(m.head, hierarchy.MultitaskHead)
    assert [h.out_features for h in m.head.heads] == [3, 13, 51]
    std = m.layers[0].blocks[0].mlp.fc1.weight.std().item()
    assert abs(std - (2 / 96) ** 0.5) < 0.02  # kaiming-normal fan_in (models.py:208-213)


def test_composer_model_surface_and_hxe_wiring():
    from hvamd import configs, hierarchy, models
    cfg = configs.Config()
    cfg.model.name = "swinv2_tiny_window7_224"
    cfg.hierarchy.variant = "hxe"
    tax = hierarchy.Taxonomy.synthetic((2, 3, 4, 5, 6, 7, 12))
    m = models.build_composer_model(cfg, models.DatasetInfo(num_classes=12, taxonomy=tax))
    assert isinstance(m.loss_fn, hierarchy.HierarchicalCrossEntropy)
    assert m.module.head.out_features == 12
    for name in ("forward", "loss", "get_metrics", "update_metric"):
        assert callable(getattr(m, name))
    cfg.hierarchy.variant = "bogus"
    with pytest.raises(ValueError):
        models.build_composer_model(cfg, models.DatasetInfo(num_classes=12))


def test_metric_dicts_match_reference_and_topk_known_answer():
    """models.py:61-101: the metric keys per variant and is_train, and acc@1 / acc@5 on a
    hand-made batch (torchmetrics multiclass micro accuracy: target among the top-k)."""
    from hvamd import configs, hierarchy, models
    tax = hierarchy.Taxonomy.synthetic((2, 3, 4, 5, 6, 7, 12))
    dists = torch.zeros(12, 12, dtype=torch.uint8)
    flat, fg = ["cross-entropy", "acc@1", "acc@5"], ["cross-entropy", "acc@1", "acc@5"]
    for variant, is_train, train_keys, val_keys in [
            ("", True, flat, flat), ("", False, flat + ["tree-dist"], flat + ["tree-dist"]),
            ("hxe", True, flat, flat), ("hxe", False, flat + ["tree-dist"], flat + ["tree-dist"]),
            ("multitask", True, fg, fg + ["tree-dist"]),
            ("multitask", False, fg + ["tree-dist"], fg + ["tree-dist"])]:
        cfg = configs.Config()
        cfg.model.name = "swinv2_tiny_window7_224"
        cfg.hierarchy.variant = variant
        cfg.is_train = is_train
        nc = tuple(tax.num_classes) if variant == "multitask" else 12
        m = models.build_composer_model(cfg, models.DatasetInfo(num_classes=nc, tree_dists=dists,
                                                                taxonomy=tax))
        assert list(m.get_metrics(is_train=True)) == train_keys, (variant, is_train)
        assert list(m.get_metrics(is_train=False)) == val_keys, (variant, is_train)
        assert m.get_metrics(is_train=True)["acc@1"] is not m.get_metrics(is_train=False)["acc@1"]
    # known answer: 4 samples over 6 classes
    logits = torch.tensor([[0.0, 5, 4, 3, 2, 1],    # target 1: top-1 hit
                           [9.0, 0, 1, 2, 3, 4],    # target 5: 2nd -> top-5 hit only
                           [0.0, 1, 2, 3, 4, 5],    # target 0: rank 6 -> miss both
                           [1.0, 2, 3, 4, 5, 6]])   # target 1: rank 5 -> top-5 hit
    tgt = torch.tensor([1, 5, 0, 1])
    a1, a5 = hierarchy.Accuracy(6), hierarchy.Accuracy(6, top_k=5)
    a1.update(logits, tgt)
    a5.update(logits, tgt)
    assert a1.compute().item() == pytest.approx(0.25)
    assert a5.compute().item() == pytest.approx(0.75)
    a5.update(logits, torch.stack([tgt] * 7, dim=1))  # [B, tiers] taxonomy targets: leaf column
    assert a5.compute().item() == pytest.approx(0.75)


def test_optimizer_groups_follow_reference_rule():
    from hvamd import configs, models, optim
    cfg = configs.Config()
    cfg.model.name = "swinv2_tiny_window7_224"
    m = models.build_composer_model(cfg, models.DatasetInfo(num_classes=10))
    opt = optim.build_optimizer(cfg, m)
    decay, no_decay = opt.param_groups
    names = {id(p): n for n, p in m.named_parameters()}
    assert all(names[id(p)].endswith("weight") or "logit_scale" in names[id(p)] for p in decay["params"])
    assert any("logit_scale" in names[id(p)] for p in decay["params"])  # optim.py:9-14 quirk
    assert no_decay["weight_decay"] == 0.0


def test_decoupled_sgdw_matches_closed_form():
    from hvamd.optim import DecoupledSGDW
    p = torch.nn.Parameter(torch.tensor([1.0, -2.0]))
    opt = DecoupledSGDW([p], lr=0.1, momentum=0.9, weight_decay=0.01)
    p.grad = torch.tensor([0.5, 0.5])
    opt.step()
    want = torch.tensor([1.0, -2.0]) * (1 - 0.01) - 0.1 * torch.tensor([0.5, 0.5])
    assert torch.allclose(p.detach(), want)
    p.grad = torch.tensor([0.5, 0.5])
    opt.step()
    want = want * (1 - 0.01) - 0.1 * (0.9 * 0.5 + 0.5)
    assert torch.allclose(p.detach(), want)


def test_checkpoint_uri_and_filter():
    from hvamd.swinv2 import Checkpoint
    ck = Checkpoint.parse("swin://ckpts/swinv2_tiny.pth")
    assert ck.path == "ckpts/swinv2_tiny.pth"
    with pytest.raises(ValueError):
        Checkpoint.parse("wandb://x")
    d = Checkpoint.filter({"a.relative_position_index": 1, "b.weight": 2, "c.logit_clamp_max": 3})
    assert d == {"b.weight": 2}


def test_normalization_fn_cpu_and_channel_stats():
    """data.channel_stats scales configs.py's 0-1 means / stds to 0-255 as build_dataspec does
    (data.py:128-133); NormalizationFn on a CPU batch is composer's f32 (x - mean) / std."""
    import types
    from hvamd.data import NormalizationFn, channel_stats
    cfg = types.SimpleNamespace(channel_mean=(0.463, 0.480, 0.376), channel_std=(0.238, 0.229, 0.247))
    mean, std = channel_stats(cfg)
    assert mean == [0.463 * 255, 0.480 * 255, 0.376 * 255] and std[2] == 0.247 * 255
    x = torch.randint(0, 256, (2, 3, 8, 8), dtype=torch.uint8)
    y, t = NormalizationFn(mean, std)((x, "t"))
    ref = (x.float() - torch.tensor(mean).view(1, 3, 1, 1)) / torch.tensor(std).view(1, 3, 1, 1)
    assert t == "t" and torch.equal(y, ref)


def test_composer_and_swin_checkpoints_round_trip(tmp_path):
    """A composer checkpoint (["state"]["model"], DDP "module." prefix; algorithmic.py:136-147)
    and an official-Swin one (["model"] with the non-persistent buffers; swinv2.py:870-895)
    both load weights-only into the 262-key SwinV2-T; the head is left alone (PretrainedBackbone
    drops head keys, algorithmic.py:67-80)."""
    from hvamd.algorithmic import PretrainedBackbone, State, WandbCheckpoint, parse_checkpoint
    from hvamd.models import create_model
    from hvamd.swinv2 import Checkpoint
    torch.manual_seed(0)
    src = create_model("swinv2_tiny_window7_224", num_classes=1000)
    sd = src.state_dict()
    assert len(sd) >= 262
    wb = WandbCheckpoint.parse("wandb://team/proj/run-1:v3?ep10.pt")
    path = wb.local_path(str(tmp_path))
    os.makedirs(os.path.dirname(path))
    torch.save({"state": {"model": {"module." + k: v for k, v in sd.items()}}}, path)
    torch.save({"model": sd}, str(tmp_path / "swin.pth"))
    for uri in ("wandb://team/proj/run-1:v3?ep10.pt", f"swin://{tmp_path}/swin.pth"):
        dst = create_model("swinv2_tiny_window7_224", num_classes=10)
        head = dst.head.weight.detach().clone()
        algo = PretrainedBackbone(uri, str(tmp_path / "cache"), strict=True)
        if isinstance(algo.checkpoint, WandbCheckpoint):
            algo.local_cache = str(tmp_path)
        algo.apply(None, State(dst))
        for k, v in dst.state_dict().items():
            if "head." in k:
                continue
            assert torch.equal(v, sd[k]), (uri, k)
        assert torch.equal(dst.head.weight, head)
    assert isinstance(parse_checkpoint(f"swin://{tmp_path}/swin.pth"), Checkpoint)
    with pytest.raises(RuntimeError, match="network"):
        WandbCheckpoint.parse("wandb://a/b/c:v0?x.pt").load_model_dict(str(tmp_path / "empty"))
    with pytest.raises(ValueError):
        parse_checkpoint("s3://bucket/x.pt")


def test_host_side_validation_under_asan():
    """SURVEY.md §5 debug build: libhvk's host code compiled with AddressSanitizer
    (-Xarch_host -fsanitize=address) and driven by tests/asan/host_checks.cpp through every
    entry point's argument validation, the workspace / support arithmetic and the error text,
    without a GPU.  Any ASan report or failed expectation fails the run."""
    import subprocess
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "hierarchical-vision_amd", "csrc"),
                        f"-j{min(8, os.cpu_count() or 2)}", "asan"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "host checks ok" in r.stdout
    assert "AddressSanitizer" not in r.stderr
