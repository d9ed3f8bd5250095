"""hvk_resized_crop_u8 at the training shape: a ragged batch of 256 synthetic 500 x 375 (W x H)
decoded images, RandomResizedCrop boxes from the project's sampler, output 224 x 224.

Two figures, both between device events with the window closed by a device synchronise:
  kernel    `--launches` back-to-back launches of the entry point on tables already on the device
            (the launches queue up behind each other, so the mean is the kernel's execution once it
            exceeds the enqueue cost of a few microseconds), with the rate over the bytes the
            launch needs: every crop's h * w * 3 source bytes read once plus the 3 * S * S output
            bytes per image written once;
  transform RandomResizedCropFlip.__call__ per batch as the Trainer calls it: the host sampler,
            the validation, the two table copies and the launch.
The sides repeat for `--rounds` rounds; the median is reported with the min-max spread.  The result
is checked against tests/resample_ref.py on the first four images before anything is timed.

    python tools/bench_device_transforms.py [--batch 256] [--height 375] [--width 500] [--size 224] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _window_us(fn, n):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--height", type=int, default=375)
    ap.add_argument("--width", type=int, default=500)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_device_transforms needs a GPU: nothing here is measurable on the CPU")
    import resample_ref
    from hvamd import _lib
    from hvamd.data import RandomResizedCropFlip, ragged_image_collate
    B, H, W, S = a.batch, a.height, a.width, a.size
    rng = np.random.default_rng(0)
    images = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(B)]
    ragged, targets = ragged_image_collate([(im, 0) for im in images])
    ragged = ragged.to("cuda")
    stage = RandomResizedCropFlip(S, seed=0)
    box = stage.sample(ragged.meta)
    meta_d, box_d = ragged.meta.cuda(), box.cuda()
    out = torch.empty((B, 3, S, S), dtype=torch.uint8, device="cuda")

    def kernel():
        _lib.call("hvk_resized_crop_u8", _lib.ptr(ragged.data), _lib.ptr(meta_d), _lib.ptr(box_d), B, S, S,
                  _lib.ptr(out), _lib.stream())

    def transform():
        stage((ragged, targets))

    kernel()
    torch.cuda.synchronize()
    n_ref = min(4, B)
    want = torch.from_numpy(resample_ref.batch_ref(images[:n_ref], box[:n_ref].numpy(), (S, S)))
    assert torch.equal(out[:n_ref].cpu(), want), "kernel output differs from the reference"
    for fn in (kernel, transform):  # warm both
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    times = {"kernel": [], "transform": []}
    for _ in range(a.rounds):
        times["kernel"].append(_window_us(kernel, a.launches))
        times["transform"].append(_window_us(transform, max(1, a.launches // 4)))
    read = int((box[:, 2].long() * box[:, 3].long()).sum()) * 3
    written = B * 3 * S * S
    med = {k: statistics.median(v) for k, v in times.items()}
    report = {"batch": B, "source_hw": [H, W], "size": S, "launches": a.launches, "rounds": a.rounds,
              "bytes_read": read, "bytes_written": written, "source_bytes_resident": int(ragged.data.numel()),
              "us": {k: {"median": round(med[k], 2), "min": round(min(v), 2), "max": round(max(v), 2)}
                     for k, v in times.items()},
              "kernel_GB_per_s": round((read + written) / med["kernel"] / 1e3, 1)}
    lines = [f"hvk_resized_crop_u8: B {B}, sources {H} x {W}, output {S} x {S}; crops read {read / 1e6:.1f} MB "
             f"(of {ragged.data.numel() / 1e6:.1f} MB resident), {written / 1e6:.1f} MB written"]
    for k, v in times.items():
        lines.append(f"  {k:10s} median {med[k]:9.2f} us  (min {min(v):9.2f}, max {max(v):9.2f}, {a.rounds} rounds)")
    lines.append(f"  kernel rate over read + written bytes: {report['kernel_GB_per_s']:.1f} GB/s")
    text = "\n".join(lines)
    print(text, flush=True)
    print(json.dumps(report))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n" + json.dumps(report) + "\n")


if __name__ == "__main__":
    main()
