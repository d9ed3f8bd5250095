"""Host side of the device transforms (data.py: RaggedImages, ragged_image_collate,
RandomResizedCropFlip, ResizeCenterCrop, DeviceTransforms, build_device_transforms) and the
numpy restatement of PIL's bilinear resize the GPU tests compare against.  No GPU."""
import os

import numpy as np
import pytest
import torch

import resample_ref

HERE = os.path.dirname(os.path.abspath(__file__))
MEAN = [0.463 * 255, 0.480 * 255, 0.376 * 255]
STD = [0.238 * 255, 0.229 * 255, 0.247 * 255]


def _golden():
    return np.load(os.path.join(HERE, "golden", "resample_golden.npz"))


def _meta(sizes):
    off, rows = 0, []
    for H, W in sizes:
        rows.append([off, H, W])
        off += 3 * H * W
    return torch.tensor(rows, dtype=torch.int64)


def test_resample_ref_equals_pil_golden():
    """The restatement equals PIL's crop().resize(BILINEAR) (and resize + centre slice) byte for
    byte on every stored case."""
    g = _golden()
    assert int(g["n_crop"]) >= 16 and int(g["n_resize_center"]) == 3
    for prefix, n in (("c", int(g["n_crop"])), ("r", int(g["n_resize_center"]))):
        for k in range(n):
            want = g[f"{prefix}{k}_out"]
            got = resample_ref.resized_crop_ref(g[f"{prefix}{k}_img"], g[f"{prefix}{k}_box"], want.shape[1:])
            assert got.dtype == np.uint8 and np.array_equal(got, want), (prefix, k)


def test_golden_resize_center_boxes_are_what_the_transform_samples():
    from hvamd.data import ResizeCenterCrop
    g = _golden()
    for k in range(int(g["n_resize_center"])):
        H, W = g[f"r{k}_img"].shape[:2]
        out = g[f"r{k}_out"]
        vh, vw = g[f"r{k}_box"][4:6]
        t = ResizeCenterCrop(int(min(vh, vw)), out.shape[1])
        assert t.sample(_meta([(H, W)]))[0].tolist() == g[f"r{k}_box"].tolist()


def _mixed_sizes(n, seed):
    rng = np.random.default_rng(seed)
    sizes = [(int(h), int(w)) for h, w in zip(rng.integers(1, 600, n), rng.integers(1, 600, n))]
    sizes[:6] = [(1, 1), (1, 500), (500, 1), (8, 400), (400, 8), (375, 500)]
    return sizes


def test_sample_equals_scalar_loop_and_stays_inside():
    from hvamd.data import RandomResizedCropFlip
    sizes = _mixed_sizes(64, 3)
    meta = _meta(sizes)
    a, b = RandomResizedCropFlip(224, seed=11), RandomResizedCropFlip(224, seed=11)
    box = a.sample(meta)
    assert box.dtype == torch.int32 and tuple(box.shape) == (64, 9) and box.device.type == "cpu"
    frac, aspect, corner, uflip = b.draw(64)
    assert frac.shape == (64, 10) and aspect.shape == (64, 10) and corner.shape == (64, 2) and uflip.shape == (64,)
    assert frac.min() >= 0.08 and frac.max() <= 1.0 and aspect.min() >= 0.75 and aspect.max() <= 4.0 / 3.0
    n_fallback = 0
    for n, (H, W) in enumerate(sizes):
        want = resample_ref.get_params_ref(H, W, frac[n], aspect[n], corner[n])
        i, j, h, w, vh, vw, oy, ox, flip = box[n].tolist()
        assert (i, j, h, w) == want, (n, H, W)
        assert (vh, vw, oy, ox) == (224, 224, 0, 0) and flip == int(uflip[n] < 0.5)
        assert 0 <= i and 0 <= j and h >= 1 and w >= 1 and i + h <= H and j + w <= W
        n_fallback += all(not (0 < int(round(np.sqrt(H * W * f * r))) <= W and 0 < int(round(np.sqrt(H * W * f / r))) <= H)
                          for f, r in zip(frac[n], aspect[n]))
    assert 0 < n_fallback < 64  # both branches were compared
    assert 0 < int(box[:, 8].sum()) < 64
    # the same seed draws the same table; the next batch differs
    assert torch.equal(RandomResizedCropFlip(224, seed=11).sample(meta), box)
    assert not torch.equal(a.sample(meta), box)


def test_first_valid_attempt_wins():
    """Attempt 0 does not fit (a 4:3 box of the whole area in a square image is too wide), attempts
    1 and 2 both do: the box is attempt 1's."""
    from hvamd.data import RandomResizedCropFlip
    t = RandomResizedCropFlip(32, seed=0)
    H = W = 100
    frac = np.full((1, 10), 0.25)
    frac[0, 0] = 1.0
    frac[0, 2] = 0.5
    aspect = np.full((1, 10), 1.0)
    aspect[0, 0] = 4.0 / 3.0
    corner = np.array([[0.5, 0.999]])
    box = t.boxes(_meta([(H, W)]), frac, aspect, corner, np.array([0.9]))
    assert int(round(np.sqrt(H * W * 1.0 * 4.0 / 3.0))) > W  # attempt 0 is invalid
    assert box[0].tolist() == [25, 50, 50, 50, 32, 32, 0, 0, 0]
    assert resample_ref.get_params_ref(H, W, frac[0], aspect[0], corner[0]) == (25, 50, 50, 50)


def test_sliver_always_falls_back():
    from hvamd.data import RandomResizedCropFlip
    t = RandomResizedCropFlip(224, scale=(0.9, 1.0), seed=5)
    meta = _meta([(8, 400)] * 32)
    for _ in range(4):
        box = t.sample(meta)
        assert (box[:, :4] == torch.tensor([0, 194, 8, 11], dtype=torch.int32)).all()
    tall = RandomResizedCropFlip(224, scale=(0.9, 1.0), seed=5).sample(_meta([(400, 8)]))
    assert tall[0, :4].tolist() == [194, 0, 11, 8]


def test_p_flip_extremes():
    from hvamd.data import RandomResizedCropFlip
    meta = _meta([(40, 50)] * 50)
    assert int(RandomResizedCropFlip(16, p_flip=0.0, seed=1).sample(meta)[:, 8].sum()) == 0
    assert int(RandomResizedCropFlip(16, p_flip=1.0, seed=1).sample(meta)[:, 8].sum()) == 50


def test_resize_center_crop_geometry():
    from hvamd.data import ResizeCenterCrop
    box = ResizeCenterCrop(256, 224).sample(_meta([(300, 200), (200, 300), (256, 256)]))
    assert box.dtype == torch.int32
    assert box[0].tolist() == [0, 0, 300, 200, 384, 256, 80, 16, 0]
    assert box[1].tolist() == [0, 0, 200, 300, 256, 384, 16, 80, 0]
    assert box[2].tolist() == [0, 0, 256, 256, 256, 256, 16, 16, 0]
    # Resize truncates the long side: int(256 * 301 / 200) = int(385.28)
    assert ResizeCenterCrop(256, 224).sample(_meta([(301, 200)]))[0, 4:6].tolist() == [385, 256]
    # Python's round goes to even: (vh - crop) / 2 = 0.5 -> 0, 1.5 -> 2, 2.5 -> 2
    b = ResizeCenterCrop(-1, 224).sample(_meta([(225, 227), (229, 224)]))
    assert b[0].tolist() == [0, 0, 225, 227, 225, 227, 0, 2, 0]
    assert b[1].tolist() == [0, 0, 229, 224, 229, 224, 2, 0, 0]
    with pytest.raises(ValueError, match="smaller than"):
        ResizeCenterCrop(32, 40).sample(_meta([(300, 200)]))
    with pytest.raises(ValueError, match="smaller than"):
        ResizeCenterCrop(-1, 224).sample(_meta([(300, 200)]))


def test_ragged_image_collate():
    from hvamd.data import RaggedImages, ragged_image_collate
    rng = np.random.default_rng(0)
    a = rng.integers(0, 256, (5, 7, 3), dtype=np.uint8)
    grey = rng.integers(0, 256, (4, 6), dtype=np.uint8)
    t = torch.from_numpy(rng.integers(0, 256, (3, 2, 3), dtype=np.uint8))
    grey1 = rng.integers(0, 256, (2, 9, 1), dtype=np.uint8)
    ragged, targets = ragged_image_collate([(a, 3), (grey, 1), (t, 4), (grey1, 0)])
    assert isinstance(ragged, RaggedImages) and len(ragged) == 4
    assert ragged.data.dtype == torch.uint8 and ragged.data.ndim == 1 and ragged.data.is_contiguous()
    assert ragged.meta.dtype == torch.int64 and ragged.meta.device.type == "cpu"
    assert ragged.meta.tolist() == [[0, 5, 7], [105, 4, 6], [177, 3, 2], [195, 2, 9]]
    assert ragged.data.numel() == 195 + 54
    flat = ragged.data.numpy()
    assert np.array_equal(flat[:105].reshape(5, 7, 3), a)
    assert np.array_equal(flat[105:177].reshape(4, 6, 3), np.repeat(grey[:, :, None], 3, 2))
    assert np.array_equal(flat[177:195].reshape(3, 2, 3), t.numpy())
    assert np.array_equal(flat[195:].reshape(2, 9, 3), np.repeat(grey1, 3, 2))
    assert targets.dtype == torch.int64 and targets.tolist() == [3, 1, 4, 0]
    # [7] tier targets stack to [B, 7]
    tiers = [torch.arange(7) + n for n in range(2)]
    _, y = ragged_image_collate([(a, tiers[0]), (grey, tiers[1])])
    assert y.dtype == torch.int64 and torch.equal(y, torch.stack(tiers))
    # .to moves data only
    moved = ragged.to("cpu")
    assert moved.meta is ragged.meta and torch.equal(moved.data, ragged.data)
    with pytest.raises(TypeError):
        ragged_image_collate([(a.astype(np.float32), 0)])
    with pytest.raises(ValueError):
        ragged_image_collate([(np.zeros((4, 4, 4), np.uint8), 0)])


def test_ragged_image_collate_pil():
    Image = pytest.importorskip("PIL.Image")
    from hvamd.data import ragged_image_collate
    rng = np.random.default_rng(1)
    rgb = rng.integers(0, 256, (6, 5, 3), dtype=np.uint8)
    grey = rng.integers(0, 256, (3, 8), dtype=np.uint8)
    ragged, targets = ragged_image_collate([(Image.fromarray(rgb), 0), (Image.fromarray(grey), 1)])
    assert ragged.meta.tolist() == [[0, 6, 5], [90, 3, 8]]
    assert np.array_equal(ragged.data.numpy()[:90].reshape(6, 5, 3), rgb)
    assert np.array_equal(ragged.data.numpy()[90:].reshape(3, 8, 3), np.repeat(grey[:, :, None], 3, 2))
    assert targets.tolist() == [0, 1]


class _PatchEmbed:
    input_norm = None

    def set_input_normalization(self, mean, std):
        self.input_norm = (mean, std)


class _Net:
    def __init__(self):
        self.patch_embed = _PatchEmbed()


def test_device_transforms_fuse_into():
    from hvamd.data import DeviceTransforms, NormalizationFn, RandomResizedCropFlip, ResizeCenterCrop
    for crop in (RandomResizedCropFlip(56, seed=0), ResizeCenterCrop(64, 56)):
        net = _Net()
        comp = DeviceTransforms([crop, NormalizationFn(MEAN, STD)])
        assert comp.fuse_into(net) is False
        assert net.patch_embed.input_norm is not None and comp.stages == [crop]
    net = _Net()
    assert DeviceTransforms([NormalizationFn(MEAN, STD)]).fuse_into(net) is True
    assert net.patch_embed.input_norm is not None
    # a model without the entry point keeps every stage
    comp = DeviceTransforms([NormalizationFn(MEAN, STD)])
    assert comp.fuse_into(object()) is False and len(comp.stages) == 1
    # stages run in order
    order = DeviceTransforms([lambda b: (b[0] + 1, b[1]), lambda b: (b[0] * 2, b[1])])
    assert order((1, "y")) == (4, "y")


def test_crop_stages_refuse_graph_capture(monkeypatch):
    from hvamd.data import RaggedImages, RandomResizedCropFlip, ResizeCenterCrop
    ragged = RaggedImages(torch.zeros(3 * 20 * 30, dtype=torch.uint8), _meta([(20, 30)]))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    for stage in (RandomResizedCropFlip(8, seed=0), ResizeCenterCrop(16, 8)):
        with pytest.raises(RuntimeError, match="capture"):
            stage((ragged, None))


def test_build_device_transforms():
    from hvamd import configs
    from hvamd.data import (NormalizationFn, RandomResizedCropFlip, ResizeCenterCrop, build_device_transforms,
                            channel_stats)
    cfg = configs.Config()
    cfg.eval_dataset.resize_size, cfg.eval_dataset.crop_size = 256, 224
    train = build_device_transforms(cfg, is_train=True)
    assert isinstance(train.stages[0], RandomResizedCropFlip) and train.stages[0].size == (224, 224)
    assert isinstance(train.stages[1], NormalizationFn)
    assert train.stages[1].mean == channel_stats(cfg.train_dataset)[0]
    meta = _meta([(300, 200)] * 4)
    again = build_device_transforms(cfg, is_train=True)
    assert torch.equal(train.stages[0].sample(meta), again.stages[0].sample(meta))  # seeded by config.seed
    ev = build_device_transforms(cfg, is_train=False)
    assert isinstance(ev.stages[0], ResizeCenterCrop) and isinstance(ev.stages[1], NormalizationFn)
    assert ev.stages[0].sample(meta)[0].tolist() == [0, 0, 300, 200, 384, 256, 80, 16, 0]
    cfg.train_dataset.resize_size = 256
    with pytest.raises(NotImplementedError, match="twice"):
        build_device_transforms(cfg, is_train=True)


def test_abi_20_exports_resized_crop():
    import re

    from hvamd import _lib
    root = os.path.dirname(HERE)
    hdr = open(os.path.join(root, "include", "hvk.h")).read()
    assert int(re.search(r"#define\s+HVK_ABI_VERSION\s+(\d+)", hdr).group(1)) >= 20
    assert re.search(r"\bint\s+hvk_resized_crop_u8\(", hdr)
    assert _lib.ABI_VERSION >= 20 and "hvk_resized_crop_u8" in _lib.SIGNATURES
    lib = _lib.load()
    assert lib.hvk_abi_version() >= 20 and hasattr(lib, "hvk_resized_crop_u8")


def test_host_validation_refuses_before_any_launch():
    """Every refusal comes from the host copies of the tables: the data tensor is on the CPU, so a
    call that got as far as the launch would raise RuntimeError (libhvk takes no CPU tensor)."""
    import hvamd.ops as ops
    from hvamd.data import RaggedImages
    ragged = RaggedImages(torch.zeros(3 * 100 * 80 + 3 * 700 * 8, dtype=torch.uint8), _meta([(100, 80), (700, 8)]))

    def box(rows):
        return torch.tensor(rows, dtype=torch.int32)

    ok = [0, 0, 100, 80, 32, 32, 0, 0, 0]
    ok1 = [0, 0, 320, 8, 32, 32, 0, 0, 0]
    bad = {
        "box outside the image": [[10, 0, 100, 80, 32, 32, 0, 0, 0], [0, 1, 100, 80, 32, 32, 0, 0, 0],
                                  [-1, 0, 50, 50, 32, 32, 0, 0, 0], [0, 0, 0, 80, 32, 32, 0, 0, 0]],
        "window outside the virtual image": [[0, 0, 100, 80, 32, 32, 1, 0, 0], [0, 0, 100, 80, 31, 40, 0, 0, 0],
                                             [0, 0, 100, 80, 40, 40, 0, 9, 0], [0, 0, 100, 80, 40, 40, -1, 0, 0]],
    }
    for what, rows in bad.items():
        for row in rows:
            with pytest.raises(ValueError, match=what):
                ops.resized_crop_u8(ragged, box([row, ok1]), (32, 32))
    with pytest.raises(ValueError, match="scale above 64"):  # 700 rows -> 10: scale 70
        ops.resized_crop_u8(ragged, box([ok, [0, 0, 700, 8, 10, 10, 0, 0, 0]]), (10, 10))
    with pytest.raises(ValueError, match="image 1"):
        ops.resized_crop_u8(ragged, box([ok, [0, 0, 700, 9, 32, 32, 0, 0, 0]]), (32, 32))
    with pytest.raises(ValueError, match="output"):
        ops.resized_crop_u8(ragged, box([ok, ok1]), (32, 1025))
    with pytest.raises(ValueError, match="output"):
        ops.resized_crop_u8(ragged, box([ok, ok1]), (0, 32))
    with pytest.raises(ValueError, match="int32"):
        ops.resized_crop_u8(ragged, box([ok, ok1]).long(), (32, 32))
    with pytest.raises(ValueError, match="int32"):
        ops.resized_crop_u8(ragged, box([ok]), (32, 32))
    short = RaggedImages(ragged.data[:-1], ragged.meta)
    with pytest.raises(ValueError, match="packed buffer"):
        ops.resized_crop_u8(short, box([ok, ok1]), (32, 32))
    big = RaggedImages(torch.zeros(3 * 8193, dtype=torch.uint8), _meta([(1, 8193)]))
    with pytest.raises(ValueError, match="source side"):
        ops.resized_crop_u8(big, box([[0, 0, 1, 8193, 200, 200, 0, 0, 0]]), (200, 200))
    # a valid table passes validation and only then meets the missing GPU
    with pytest.raises(RuntimeError, match="GPU"):
        ops.resized_crop_u8(ragged, box([ok, ok1]), (32, 32))
