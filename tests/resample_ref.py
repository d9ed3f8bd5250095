"""Reference restatements for the device transforms (not a test).

resized_crop_ref: PIL's 8-bit bilinear resize (Resample.c: precompute_coeffs,
normalize_coeffs_8bpc, ImagingResampleHorizontal_8bpc / Vertical_8bpc, PRECISION_BITS = 22) of a
crop, in numpy: coefficients in float64 with a scalar loop for ww, accumulation in integers, the
intermediate rounded to uint8 between the horizontal and the vertical pass, a pass whose sizes
agree skipped.  tests/golden/resample_golden.npz pins it to Image.crop(...).resize(..., BILINEAR)
byte for byte (tests/test_device_transforms_cpu.py), so the GPU tests need no PIL.

get_params_ref: torchvision's RandomResizedCrop.get_params as a scalar loop over given uniforms
(the arrays data.RandomResizedCropFlip.draw returns), restated from the published source.
"""
import math

import numpy as np

PRECISION_BITS = 22


def axis_coefs(n_in, n_out):
    """[(xmin, int coefficients)] per output index of one axis n_in -> n_out."""
    scale = float(n_in) / float(n_out)
    fs = max(scale, 1.0)
    support = fs
    ss = 1.0 / fs
    table = []
    for x in range(n_out):
        center = (x + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in)
        ws = []
        ww = 0.0
        for t in range(xmax - xmin):
            w = max(0.0, 1.0 - abs((t + xmin - center + 0.5) * ss))
            ws.append(w)
            ww += w
        ks = [int(0.5 + (w / ww if ww != 0.0 else w) * (1 << PRECISION_BITS)) for w in ws]
        table.append((xmin, np.array(ks, dtype=np.int64)))
    return table


def _resample_axis0(a, n_out):
    """a uint8 [n_in, ...] -> uint8 [n_out, ...] along axis 0."""
    n_in = a.shape[0]
    if n_in == n_out:
        return a
    out = np.empty((n_out,) + a.shape[1:], dtype=np.uint8)
    wide = a.astype(np.int64)
    for x, (xmin, ks) in enumerate(axis_coefs(n_in, n_out)):
        acc = np.tensordot(ks, wide[xmin:xmin + len(ks)], axes=(0, 0)) + (1 << (PRECISION_BITS - 1))
        assert acc.max(initial=0) < 2 ** 31
        out[x] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return out


def resize_ref(img, vh, vw):
    """HWC uint8 -> [vh, vw, C] uint8: horizontal pass first, then vertical."""
    a = _resample_axis0(np.ascontiguousarray(img).transpose(1, 0, 2), vw).transpose(1, 0, 2)
    return _resample_axis0(a, vh)


def resized_crop_ref(img, box, out_hw):
    """hvk_resized_crop_u8 for one image: img HWC uint8 (grey: HW), box = (i, j, h, w, vh, vw, oy,
    ox, flip), out_hw = (out_h, out_w) -> uint8 [3, out_h, out_w]."""
    img = np.asarray(img)
    if img.ndim == 2:
        img = np.repeat(img[:, :, None], 3, axis=2)
    i, j, h, w, vh, vw, oy, ox, flip = (int(v) for v in box)
    oh, ow = out_hw
    assert 0 <= i and 0 <= j and h >= 1 and w >= 1 and i + h <= img.shape[0] and j + w <= img.shape[1]
    assert 0 <= oy and 0 <= ox and oy + oh <= vh and ox + ow <= vw
    v = resize_ref(img[i:i + h, j:j + w], vh, vw)[oy:oy + oh, ox:ox + ow]
    if flip:
        v = v[:, ::-1]
    return np.ascontiguousarray(v.transpose(2, 0, 1))


def batch_ref(images, boxes, out_hw):
    """uint8 [B, 3, out_h, out_w] of a list of images and a [B, 9] box table."""
    return np.stack([resized_crop_ref(im, bx, out_hw) for im, bx in zip(images, np.asarray(boxes))])


def get_params_ref(H, W, frac, aspect, corner, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0)):
    """(i, j, h, w) of one H x W image from its ten area fractions, ten aspect ratios and two
    corner uniforms: the first attempt that fits, else the central crop at the nearest ratio."""
    area = float(H * W)
    for f, r in zip(frac, aspect):
        w = int(round(math.sqrt(area * f * r)))
        h = int(round(math.sqrt(area * f / r)))
        if 0 < w <= W and 0 < h <= H:
            return (int(math.floor(corner[0] * (H - h + 1))), int(math.floor(corner[1] * (W - w + 1))), h, w)
    in_ratio = float(W) / float(H)
    if in_ratio < min(ratio):
        w = W
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = H
        w = int(round(h * max(ratio)))
    else:
        w, h = W, H
    return (H - h) // 2, (W - w) // 2, h, w
