"""Device-side input transforms -- the data.py slice on the hot path.

Normalisation.  The reference normalises each uint8 batch from pil_image_collate (data.py:36-76)
on the device with composer's NormalizationFn (data.py:130-136, :154-164 DataSpec
device_transforms): f32 (x - mean) / std with mean / std in the 0-255 scale (data.py:128-133).
Here that is one HIP kernel (hvk_normalize_u8), or -- when the model's PatchEmbed takes it
(fuse_into) -- no separate pass at all: the normalisation runs inside the patch gather that feeds
the patch-embedding GEMM (hvk_patchify_u8_bf16), so the f32 image batch is never written.
composer's NormalizationFn is third-party (mosaicml 0.13.1, not vendored): its arithmetic is
restated from the published source and pinned against torch's own sub_ / div_ (parity unpinned by
the reference, which has no tests).

Crop and resample.  Everything before the normalisation runs in the reference's CPU workers on
PIL through torchvision: RandomResizedCrop + RandomHorizontalFlip for training (data.py:118-124),
Resize + CenterCrop for evaluation (data.py:114-126).  Here the workers only decode:
ragged_image_collate packs the decoded images of a batch, at their own sizes, into one uint8 buffer
(RaggedImages); RandomResizedCropFlip / ResizeCenterCrop turn it into the uint8 [B, 3, S, S] batch
pil_image_collate would have returned with ONE library call (hvk_resized_crop_u8), which resamples
with PIL's 8-bit fixed-point bilinear arithmetic and so equals PIL byte for byte.  The boxes are
sampled on the host (a few vectorised numpy operations per batch).  DeviceTransforms chains the
stages; build_device_transforms is the device half of build_dataspec.
"""
import numpy as np
import torch

from . import ops

try:  # the workers' decoder; arrays and tensors collate without it
    from PIL import Image as _PILImage
except ImportError:  # pragma: no cover
    _PILImage = None


def channel_stats(data_cfg):
    """(mean, std) in the 0-255 scale, as build_dataspec scales them (data.py:128-133)."""
    mean, std = list(data_cfg.channel_mean), list(data_cfg.channel_std)
    if all(m < 1 for m in mean):
        mean = [m * 255 for m in mean]
    if all(s < 1 for s in std):
        std = [s * 255 for s in std]
    return mean, std


class NormalizationFn:
    """composer.datasets.utils.NormalizationFn surface: called on a (images, targets) batch,
    returns the batch with images normalised to f32 (uint8 CUDA images: hvk_normalize_u8)."""

    def __init__(self, mean, std, ignore_background=False):
        if ignore_background:
            raise NotImplementedError("ignore_background is a segmentation option (ADE20k)")
        self.mean = mean
        self.std = std
        self._dev = {}

    def _stats(self, device):
        if device not in self._dev:
            self._dev[device] = (torch.tensor(self.mean, dtype=torch.float32, device=device),
                                 torch.tensor(self.std, dtype=torch.float32, device=device))
        return self._dev[device]

    def __call__(self, batch):
        xs, ys = batch
        if xs.is_cuda and xs.dtype == torch.uint8:
            m, s = self._stats(xs.device)
            return ops.normalize_u8(xs, m, s), ys
        m, s = (t.view(1, -1, 1, 1) for t in self._stats(xs.device))
        return xs.float().sub_(m).div_(s), ys

    def fuse_into(self, model):
        """Move the normalisation into the model's PatchEmbed (uint8 batches then go straight to
        the model); False when the model has no such entry point (the trainer keeps calling
        this transform)."""
        net = getattr(model, "module", model)
        pe = getattr(net, "patch_embed", None)
        if pe is None or not hasattr(pe, "set_input_normalization"):
            return False
        pe.set_input_normalization(self.mean, self.std)
        return True


class RaggedImages:
    """A batch of decoded images of different sizes in one buffer: data, a 1-D uint8 tensor on any
    device holding each image HWC, RGB-interleaved, row-major (np.asarray(pil_image)); meta, int64
    [B, 3] = (byte offset, H, W), always on the host (the box sampler and the launch's validation
    read it there)."""

    def __init__(self, data, meta):
        if data.dtype != torch.uint8 or data.ndim != 1:
            raise TypeError("RaggedImages.data is a 1-D uint8 tensor")
        if meta.dtype != torch.int64 or meta.ndim != 2 or meta.shape[1] != 3 or meta.device.type != "cpu":
            raise TypeError("RaggedImages.meta is a host int64 [B, 3] tensor")
        self.data = data
        self.meta = meta

    def __len__(self):
        return self.meta.shape[0]

    @property
    def device(self):
        return self.data.device

    def to(self, device, non_blocking=False):
        return RaggedImages(self.data.to(device, non_blocking=non_blocking), self.meta)

    def pin_memory(self):
        return RaggedImages(self.data.pin_memory(), self.meta)


def _hwc_u8(img):
    """One sample's image as a contiguous HWC uint8 array with three channels (a grey image is
    replicated, as pil_image_collate does, data.py:62-70)."""
    if isinstance(img, torch.Tensor):
        a = img.numpy()
    elif _PILImage is not None and isinstance(img, _PILImage.Image):
        a = np.asarray(img, dtype=np.uint8)
    else:
        a = np.asarray(img)
    if a.dtype != np.uint8:
        raise TypeError(f"ragged_image_collate takes uint8 images, got {a.dtype}")
    if a.ndim == 2:
        a = a[:, :, None]
    if a.ndim != 3 or a.shape[2] not in (1, 3) or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"ragged_image_collate takes HWC images with 1 or 3 channels, got shape {a.shape}")
    if a.shape[2] == 1:
        a = np.repeat(a, 3, axis=2)
    return np.ascontiguousarray(a)


def ragged_image_collate(batch):
    """collate_fn for a DataLoader whose dataset decodes but does not transform: samples are
    (image, target) with the image a PIL image, an HWC uint8 numpy array or an HWC uint8 tensor.
    Returns (RaggedImages, targets): the images packed back to back in one contiguous host buffer,
    the targets stacked to int64 as pil_image_collate stacks them (data.py:49-60, 74: ints -> [B],
    [7] tensors -> [B, 7])."""
    arrays = [_hwc_u8(sample[0]) for sample in batch]
    sizes = [a.size for a in arrays]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    data = torch.empty(int(offsets[-1]), dtype=torch.uint8)
    flat = data.numpy()
    for a, o in zip(arrays, offsets):
        flat[o:o + a.size] = a.reshape(-1)
    meta = torch.tensor([[int(o), a.shape[0], a.shape[1]] for a, o in zip(arrays, offsets)],
                        dtype=torch.int64).reshape(len(arrays), 3)
    targets = torch.from_numpy(np.stack([
        (sample[1].numpy() if isinstance(sample[1], torch.Tensor) else np.asarray(sample[1])).astype(np.int64)
        for sample in batch]))
    return RaggedImages(data, meta), targets


def _no_capture(what):
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        raise RuntimeError(f"{what} takes a ragged batch, which a graph cannot capture (sizes and boxes "
                           "change per batch): crop before copying into the graph's static tensors")


class RandomResizedCropFlip:
    """torchvision's RandomResizedCrop(size, scale, ratio) + RandomHorizontalFlip(p_flip)
    (data.py:118-124) on a ragged device batch: sample(meta) draws every image's box on the host,
    one hvk_resized_crop_u8 call crops, resamples (bilinear, PIL's arithmetic) and flips.

    sample() is RandomResizedCrop.get_params vectorised over the batch from a
    numpy.random.Generator: ten area fractions and ten log-uniform aspect ratios per image
    ([B, 10]), two uniforms for the corner, one for the flip; the first attempt with 0 < w <= W
    and 0 < h <= H wins, else get_params' centre-crop fallback.  It draws from torchvision's
    DISTRIBUTION but not its random stream (torchvision draws per attempt from torch's generator
    and stops at the first success).  torchvision is third-party and not vendored: the sampler is
    restated from its published source, parity unpinned (tests/resample_ref.py holds the scalar
    loop it is checked against)."""

    def __init__(self, size, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), p_flip=0.5, seed=None):
        self.size = (size, size) if isinstance(size, int) else tuple(int(v) for v in size)
        self.scale = tuple(float(v) for v in scale)
        self.ratio = tuple(float(v) for v in ratio)
        self.p_flip = float(p_flip)
        self.rng = np.random.default_rng(seed)

    def draw(self, B):
        """The uniforms of one batch: (area fractions [B, 10], aspect ratios [B, 10], corner
        uniforms [B, 2], flip uniforms [B])."""
        frac = self.rng.uniform(self.scale[0], self.scale[1], (B, 10))
        aspect = np.exp(self.rng.uniform(np.log(self.ratio[0]), np.log(self.ratio[1]), (B, 10)))
        return frac, aspect, self.rng.random((B, 2)), self.rng.random(B)

    def boxes(self, meta, frac, aspect, corner, uflip):
        """The box table of given uniforms (sample() = boxes(meta, *draw(B)))."""
        H = meta[:, 1].numpy().astype(np.int64)
        W = meta[:, 2].numpy().astype(np.int64)
        B = len(H)
        area = (H * W).astype(np.float64)[:, None]
        w = np.round(np.sqrt(area * frac * aspect)).astype(np.int64)
        h = np.round(np.sqrt(area * frac / aspect)).astype(np.int64)
        valid = (w > 0) & (w <= W[:, None]) & (h > 0) & (h <= H[:, None])
        found = valid.any(1)
        rows = np.arange(B)
        first = valid.argmax(1)
        w, h = w[rows, first], h[rows, first]
        i = np.floor(corner[:, 0] * (H - h + 1)).astype(np.int64)
        j = np.floor(corner[:, 1] * (W - w + 1)).astype(np.int64)
        # get_params' fallback: the central crop at the nearest allowed ratio
        in_ratio = W.astype(np.float64) / H.astype(np.float64)
        lo, hi = min(self.ratio), max(self.ratio)
        fw = np.where(in_ratio > hi, np.round(H * hi).astype(np.int64), W)
        fh = np.where(in_ratio < lo, np.round(W / lo).astype(np.int64), H)
        w, h = np.where(found, w, fw), np.where(found, h, fh)
        i, j = np.where(found, i, (H - h) // 2), np.where(found, j, (W - w) // 2)
        oh, ow = self.size
        box = np.stack([i, j, h, w, np.full(B, oh), np.full(B, ow), np.zeros(B, np.int64), np.zeros(B, np.int64),
                        (uflip < self.p_flip).astype(np.int64)], 1)
        return torch.from_numpy(box.astype(np.int32)).reshape(B, 9)

    def sample(self, meta):
        """Host int32 [B, 9] box table (i, j, h, w, vh, vw, oy, ox, flip) for meta int64 [B, 3]."""
        return self.boxes(meta, *self.draw(meta.shape[0]))

    def __call__(self, batch):
        ragged, targets = batch
        _no_capture("RandomResizedCropFlip")
        return ops.resized_crop_u8(ragged, self.sample(ragged.meta), self.size), targets


class ResizeCenterCrop:
    """torchvision's Resize(resize_size) + CenterCrop(crop_size) (data.py:114-126) on a ragged
    device batch, one hvk_resized_crop_u8 call.  Resize(int): the shorter side goes to
    resize_size, the longer to int(resize_size * long / short); skipped when resize_size <= 0.
    CenterCrop: top = int(round((vh - crop) / 2.0)), left likewise (Python's round, to even).
    Deviation: torchvision zero-pads an image smaller than the crop; here that raises ValueError."""

    def __init__(self, resize_size, crop_size):
        self.resize_size = int(resize_size)
        self.size = (crop_size, crop_size) if isinstance(crop_size, int) else tuple(int(v) for v in crop_size)

    def sample(self, meta):
        """Host int32 [B, 9] box table: the whole image, the resized size, the centre-crop corner."""
        ch, cw = self.size
        rows = []
        for _, H, W in meta.tolist():
            vh, vw = H, W
            if self.resize_size > 0:
                if W <= H:
                    vw, vh = self.resize_size, int(self.resize_size * H / W)
                else:
                    vh, vw = self.resize_size, int(self.resize_size * W / H)
            if vh < ch or vw < cw:
                raise ValueError(f"ResizeCenterCrop: a {H}x{W} image resized to {vh}x{vw} is smaller than the "
                                 f"{ch}x{cw} crop (torchvision would zero-pad; not supported)")
            rows.append([0, 0, H, W, vh, vw, int(round((vh - ch) / 2.0)), int(round((vw - cw) / 2.0)), 0])
        return torch.tensor(rows, dtype=torch.int32).reshape(len(rows), 9)

    def __call__(self, batch):
        ragged, targets = batch
        _no_capture("ResizeCenterCrop")
        return ops.resized_crop_u8(ragged, self.sample(ragged.meta), self.size), targets


class DeviceTransforms:
    """The stages of a device transform, called in order on the (inputs, targets) batch."""

    def __init__(self, stages):
        self.stages = list(stages)

    def __call__(self, batch):
        for stage in self.stages:
            batch = stage(batch)
        return batch

    def fuse_into(self, model):
        """Hand a trailing NormalizationFn to the model's PatchEmbed (NormalizationFn.fuse_into);
        True only if no stage remains, so that a Trainer given a crop stage keeps calling this
        composite and the model takes the uint8 crops."""
        if self.stages and isinstance(self.stages[-1], NormalizationFn) and self.stages[-1].fuse_into(model):
            self.stages.pop()
        return not self.stages


def build_device_transforms(config, is_train=True):
    """The device half of build_dataspec (data.py:98-136): RandomResizedCropFlip(crop_size,
    seed=config.seed) for training, ResizeCenterCrop(resize_size, crop_size) for evaluation, then
    NormalizationFn.  A training config with resize_size > 0 is refused: the reference then
    resamples twice (Resize, then the crop's resize), which one launch does not reproduce."""
    data_cfg = config.train_dataset if is_train else config.eval_dataset
    norm = NormalizationFn(*channel_stats(data_cfg))
    if not is_train:
        return DeviceTransforms([ResizeCenterCrop(data_cfg.resize_size, data_cfg.crop_size), norm])
    if data_cfg.resize_size > 0:
        raise NotImplementedError("train_dataset.resize_size > 0: the reference resamples twice (Resize, then "
                                  "RandomResizedCrop's resize); the device transform resamples once")
    return DeviceTransforms([RandomResizedCropFlip(data_cfg.crop_size, seed=config.seed), norm])
