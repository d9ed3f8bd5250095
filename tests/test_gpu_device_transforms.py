"""hvk_resized_crop_u8 and the device transforms built on it (data.py): every comparison is
torch.equal against PIL's own bytes (tests/golden/resample_golden.npz) or the numpy restatement of
PIL's arithmetic (tests/resample_ref.py), which the CPU tests pin to PIL byte for byte."""
import os

import numpy as np
import pytest
import torch

import resample_ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MEAN = [0.463 * 255, 0.480 * 255, 0.376 * 255]
STD = [0.238 * 255, 0.229 * 255, 0.247 * 255]


def _images(sizes, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for H, W in sizes]


def _ragged(images):
    from hvamd.data import ragged_image_collate
    ragged, _ = ragged_image_collate([(im, 0) for im in images])
    return ragged.to("cuda")


def _run(images, boxes, out_hw):
    import hvamd.ops as ops
    return ops.resized_crop_u8(_ragged(images), torch.tensor(boxes, dtype=torch.int32).reshape(-1, 9), out_hw)


def _check(images, boxes, out_hw):
    got = _run(images, boxes, out_hw)
    want = torch.from_numpy(resample_ref.batch_ref(images, boxes, out_hw))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (len(images), 3) + tuple(out_hw)
    assert torch.equal(got.cpu(), want)
    return got


def test_golden_cases_are_pils_bytes():
    """Each stored case alone, and all cases of one output size in one ragged launch."""
    g = np.load(os.path.join(HERE, "golden", "resample_golden.npz"))
    cases = [(g[f"{p}{k}_img"], g[f"{p}{k}_box"], g[f"{p}{k}_out"])
             for p, n in (("c", int(g["n_crop"])), ("r", int(g["n_resize_center"]))) for k in range(n)]
    assert len(cases) >= 19
    by_size = {}
    for img, box, out in cases:
        got = _run([img], [box.tolist()], out.shape[1:])
        assert torch.equal(got[0].cpu(), torch.from_numpy(out)), box.tolist()
        by_size.setdefault(out.shape[1:], []).append((img, box, out))
    for out_hw, group in by_size.items():
        got = _run([c[0] for c in group], [c[1].tolist() for c in group], out_hw)
        assert torch.equal(got.cpu(), torch.from_numpy(np.stack([c[2] for c in group])))


def test_ragged_batch_one_launch():
    sizes = [(37, 53), (64, 64), (1, 50), (50, 1), (120, 9), (96, 128)]
    images = _images(sizes, 1)
    boxes = [[3, 5, 30, 41, 32, 32, 0, 0, 1], [0, 0, 64, 64, 32, 32, 0, 0, 0], [0, 7, 1, 40, 32, 32, 0, 0, 1],
             [11, 0, 33, 1, 32, 32, 0, 0, 0], [20, 1, 99, 7, 32, 32, 0, 0, 1], [9, 30, 80, 61, 32, 32, 0, 0, 0]]
    _check(images, boxes, (32, 32))


EDGES = {
    "1x1 crop -> 8": ((5, 6), [2, 3, 1, 1, 8, 8, 0, 0, 0], (8, 8)),
    "2x3 -> 56": ((2, 3), [0, 0, 2, 3, 56, 56, 0, 0, 0], (56, 56)),
    "8x8 -> 224": ((8, 8), [0, 0, 8, 8, 224, 224, 0, 0, 0], (224, 224)),
    "320x320 -> 8": ((320, 320), [0, 0, 320, 320, 8, 8, 0, 0, 0], (8, 8)),
    "224x100 -> 224": ((224, 100), [0, 0, 224, 100, 224, 224, 0, 0, 0], (224, 224)),
    "box on all four borders": ((45, 61), [0, 0, 45, 61, 24, 24, 0, 0, 0], (24, 24)),
    "interior box": ((80, 90), [21, 33, 30, 27, 24, 24, 0, 0, 0], (24, 24)),
    "W = 37": ((41, 37), [2, 1, 36, 35, 24, 24, 0, 0, 1], (24, 24)),
    # the paths the tiling adds: scale 64 with one output row per sub-band pass (129 source rows
    # each), a sub-band split inside a 16-row tile (scale 14: 16 rows need 14 * 17 > 192 source rows),
    # a partial last tile in both directions (33 = 32 + 1 columns, 17 = 16 + 1 rows)
    "scale 64": ((1100, 40), [3, 0, 1088, 33, 17, 33, 0, 0, 1], (17, 33)),
    "sub-band split": ((480, 20), [0, 0, 476, 20, 34, 20, 0, 0, 0], (34, 20)),
    "non-square window": ((70, 50), [0, 0, 70, 50, 60, 47, 9, 5, 1], (40, 37)),
}


@pytest.mark.parametrize("name", list(EDGES))
def test_edges(name):
    size, box, out_hw = EDGES[name]
    images = _images([size], 2)
    if name == "interior box":
        # a neighbour's pixels must not leak in: the crop sits in a constant frame of another colour
        images[0][:] = 255
        i, j, h, w = box[:4]
        images[0][i:i + h, j:j + w] = np.random.default_rng(3).integers(0, 100, (h, w, 3), dtype=np.uint8)
    got = _check(images, [box], out_hw)
    if name == "interior box":
        assert int(got.max()) < 100


def test_resize_center_crop():
    from hvamd.data import ResizeCenterCrop
    images = _images([(90, 120), (301, 97)], 4)
    t = ResizeCenterCrop(32, 24)
    ragged = _ragged(images)
    boxes = t.sample(ragged.meta)
    assert boxes[0].tolist() == [0, 0, 90, 120, 32, 42, 4, 9, 0]
    assert boxes[1].tolist() == [0, 0, 301, 97, 99, 32, 38, 4, 0]
    y = torch.tensor([1, 2], device="cuda")
    got, targets = t((ragged, y))
    assert targets is y and got.is_cuda
    assert torch.equal(got.cpu(), torch.from_numpy(resample_ref.batch_ref(images, boxes.numpy(), (24, 24))))


def test_flip_is_torch_flip_and_calls_repeat():
    images = _images([(37, 53), (64, 40)], 5)
    boxes = [[3, 5, 30, 41, 32, 40, 0, 3, 0], [0, 0, 64, 40, 33, 70, 1, 0, 0]]
    plain = _run(images, boxes, (32, 37))
    flipped = _run(images, [b[:8] + [1] for b in boxes], (32, 37))
    assert torch.equal(flipped, torch.flip(plain, dims=[3]))
    assert torch.equal(_run(images, boxes, (32, 37)), plain)


def _mini_swin(num_classes=10):
    from hvamd import swinv2
    torch.manual_seed(0)
    return swinv2.SwinTransformerV2(img_size=56, embed_dim=32, depths=[2, 2], num_heads=[1, 2], window_size=7,
                                    num_classes=num_classes, drop_path_rate=0.0).cuda()


def test_trainer_takes_ragged_batches_end_to_end():
    """Trainer with [RandomResizedCropFlip, NormalizationFn]: the normalisation goes into the patch
    gather, the crop stage stays; the logits equal, bit for bit, those of feeding the same boxes'
    reference crops through the existing uint8 path."""
    from hvamd import hierarchy, models, optim
    from hvamd.data import DeviceTransforms, NormalizationFn, RandomResizedCropFlip, ragged_image_collate
    from hvamd.trainer import Trainer
    net = _mini_swin()
    model = models.Model(net, None, None, hierarchy.soft_cross_entropy)
    opt = optim.DecoupledSGDW(optim.set_weight_decay(model), lr=0.0, momentum=0.9)
    comp = DeviceTransforms([RandomResizedCropFlip(56, seed=0), NormalizationFn(MEAN, STD)])
    t = Trainer(model, opt, device_transforms=comp)
    assert t.device_transforms is comp and len(comp.stages) == 1 and net.patch_embed.input_norm is not None
    images = _images([(90, 120), (75, 64)], 7)
    ragged, targets = ragged_image_collate([(images[0], 1), (images[1], 2)])
    ragged, targets = ragged.to("cuda"), targets.cuda()

    boxes = RandomResizedCropFlip(56, seed=0).sample(ragged.meta)  # the table the composite draws first
    x, y = comp((ragged, targets))
    assert y is targets and x.dtype == torch.uint8 and tuple(x.shape) == (2, 3, 56, 56)
    ref = torch.from_numpy(resample_ref.batch_ref(images, boxes.numpy(), (56, 56))).cuda()
    assert torch.equal(x, ref)
    net.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        assert torch.equal(net(x), net(ref))
    loss = t.train_step((ragged, targets))
    assert torch.isfinite(loss)


def test_trainer_eval_with_the_evaluation_composite():
    from hvamd import hierarchy, models, optim
    from hvamd.data import DeviceTransforms, NormalizationFn, ResizeCenterCrop, ragged_image_collate
    from hvamd.trainer import Trainer
    net = _mini_swin()
    model = models.Model(net, None, None, hierarchy.soft_cross_entropy)
    opt = optim.DecoupledSGDW(optim.set_weight_decay(model), lr=0.0, momentum=0.9)
    t = Trainer(model, opt, device_transforms=DeviceTransforms([ResizeCenterCrop(64, 56), NormalizationFn(MEAN, STD)]))
    batches = []
    for seed, sizes in ((8, [(90, 120), (75, 64), (64, 200)]), (9, [(301, 97), (56, 56)])):
        ragged, targets = ragged_image_collate([(im, n) for n, im in enumerate(_images(sizes, seed))])
        batches.append((ragged.to("cuda"), targets.cuda()))
    metrics = t.eval(batches)
    assert metrics and all(np.isfinite(float(v)) for v in metrics.values())
