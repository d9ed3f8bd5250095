"""Writes tests/golden/resample_golden.npz: PIL's own output for the device transforms.

Run once where PIL is installed (this fixture was made with Pillow 12.2.0):
    python tests/golden/make_resample_golden.py
Every case stores the seeded source image, the box table row (i, j, h, w, vh, vw, oy, ox, flip) and
what PIL returns for it.  Crop cases ("c"): Image.crop((j, i, j + w, i + h)).resize((vw, vh),
BILINEAR), mirrored with Image.transpose(FLIP_LEFT_RIGHT) where flip is set -- crop THEN resize, as
torchvision's resized_crop does (Image.resize(box=...) reads pixels outside the box and is a
different function).  Resize + CenterCrop cases ("r"): Image.resize((vw, vh), BILINEAR) followed by
the centre slice.  Outputs are stored CHW like the kernel's; a grey (mode "L") source is stored
[H, W] and its output replicated to three channels, as pil_image_collate does.
"""
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))

# (H, W, (i, j, h, w), (vh, vw), flip, grey)
CROPS = [
    (37, 53, (0, 0, 37, 53), (8, 8), 0, False),        # whole image, both axes down
    (48, 48, (5, 7, 40, 30), (32, 32), 1, False),      # interior box, flipped
    (1, 50, (0, 0, 1, 50), (8, 8), 0, False),          # one source row
    (50, 1, (0, 0, 50, 1), (8, 8), 1, False),          # one source column
    (120, 9, (10, 2, 100, 5), (32, 32), 0, False),     # tall sliver: down by 3.1, up by 6.4
    (48, 64, (3, 9, 44, 50), (40, 40), 1, False),      # scales just above 1
    (8, 8, (0, 0, 8, 8), (40, 40), 0, False),          # x5 upscaling
    (2, 3, (0, 0, 2, 3), (56, 56), 0, False),          # clamped taps everywhere
    (5, 5, (2, 3, 1, 1), (8, 8), 0, False),            # 1 x 1 crop
    (128, 8, (0, 0, 128, 8), (8, 4), 0, False),        # scale 16 vertically (33 taps)
    (40, 37, (0, 0, 40, 37), (32, 32), 1, False),      # odd row stride
    (40, 40, (4, 4, 32, 32), (32, 32), 1, False),      # both passes skipped: a plain crop
    (40, 32, (5, 7, 32, 20), (32, 32), 0, False),      # vertical pass skipped
    (20, 64, (0, 0, 20, 64), (40, 16), 0, False),      # up vertically, down horizontally, non-square
    (33, 45, (4, 6, 25, 31), (16, 16), 1, True),       # grey source
    (31, 29, (30, 0, 1, 29), (8, 32), 0, False),       # last row only, non-square output
]
# (H, W, resize_size, crop_size)
RESIZE_CENTER = [(45, 60, 32, 24), (70, 42, 32, 24), (24, 64, 40, 32)]


def resize_center_box(H, W, resize_size, crop):
    if W <= H:
        vw, vh = resize_size, int(resize_size * H / W)
    else:
        vh, vw = resize_size, int(resize_size * W / H)
    return [0, 0, H, W, vh, vw, int(round((vh - crop) / 2.0)), int(round((vw - crop) / 2.0)), 0]


def chw(pil):
    a = np.asarray(pil, dtype=np.uint8)
    if a.ndim == 2:
        a = np.repeat(a[:, :, None], 3, axis=2)
    return np.ascontiguousarray(a.transpose(2, 0, 1))


def main():
    rng = np.random.default_rng(20)
    out = {"n_crop": np.int64(len(CROPS)), "n_resize_center": np.int64(len(RESIZE_CENTER))}
    for n, (H, W, (i, j, h, w), (vh, vw), flip, grey) in enumerate(CROPS):
        img = rng.integers(0, 256, (H, W) if grey else (H, W, 3), dtype=np.uint8)
        res = Image.fromarray(img).crop((j, i, j + w, i + h)).resize((vw, vh), Image.BILINEAR)
        if flip:
            res = res.transpose(Image.FLIP_LEFT_RIGHT)
        out[f"c{n}_img"] = img
        out[f"c{n}_box"] = np.array([i, j, h, w, vh, vw, 0, 0, flip], dtype=np.int32)
        out[f"c{n}_out"] = chw(res)
    for n, (H, W, rs, crop) in enumerate(RESIZE_CENTER):
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        box = resize_center_box(H, W, rs, crop)
        vh, vw, oy, ox = box[4:8]
        res = np.asarray(Image.fromarray(img).resize((vw, vh), Image.BILINEAR))[oy:oy + crop, ox:ox + crop]
        out[f"r{n}_img"] = img
        out[f"r{n}_box"] = np.array(box, dtype=np.int32)
        out[f"r{n}_out"] = np.ascontiguousarray(res.transpose(2, 0, 1))
    path = os.path.join(HERE, "resample_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
