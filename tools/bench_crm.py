"""EvalMetrics.update with decoding="crm" (hvk_eval_metrics + hvk_crm_predict) beside the same
update with the default argmax decoding, and beside the eager route to the CRM prediction,
`(softmax(z).float() @ D.float().T).argmin(1)` with the f32 copy of the distance matrix made up
front (4 L^2 bytes that the fused path never needs), at the evaluation shape: B = 256 logit rows
over L = 10 000 leaves, f32 logits.

Timing: `--updates` calls between two device events, the window closed by a device synchronise,
so a figure is what an evaluation loop pays per batch (launches and host enqueue included).  The
sides alternate for `--rounds` rounds; the median is reported with the min-max spread.  The
difference crm - argmax is the cost of hvk_crm_predict's three kernels; 2 B L^2 flop over it is
the rate given beside it.

    python tools/bench_crm.py [--batch 256] [--leaves 10000] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _eager_us(fn, updates):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(updates):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / updates


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--leaves", type=int, default=10000)
    ap.add_argument("--updates", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_crm needs a GPU: nothing here is measurable on the CPU")
    from hvamd import hierarchy, ops
    dev = torch.device("cuda:0")
    B, L = a.batch, a.leaves
    sizes = tuple(min(s, L) for s in (3, 13, 51, 273, 1103, 4884, L))
    paths = np.zeros((L, 7), np.int64)
    paths[:, 6] = np.arange(L)
    for q in range(5, -1, -1):  # Taxonomy.synthetic's tree
        paths[:, q] = paths[:, q + 1] * sizes[q] // sizes[q + 1]
    g = torch.Generator(device=dev).manual_seed(0)
    z = 2 * torch.randn(B, L, device=dev, generator=g)
    t = torch.randint(0, L, (B,), device=dev, generator=g)
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    td = ops.tree_dist_matrix(torch.from_numpy(paths.astype(np.int32)).to(dev))
    e.record()
    torch.cuda.synchronize()
    build_ms = s.elapsed_time(e)  # one call, first launch included
    td32 = td.float()
    crm = hierarchy.EvalMetrics(tree_dists=td, decoding="crm").to(dev)
    argmax = hierarchy.EvalMetrics(tree_dists=td).to(dev)
    sides = {"argmax": lambda: argmax.update(z, t), "crm": lambda: crm.update(z, t),
             "eager_crm": lambda: (torch.softmax(z, 1).float() @ td32.T).argmin(1)}
    for fn in sides.values():  # warm every shape the timed windows use
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    # the two routes agree before either is timed (rows whose two lowest risks nearly tie may differ)
    differ = int((crm.crm_pred.long() != sides["eager_crm"]()).sum())
    moved = int((crm.crm_pred != crm.pred).sum())
    assert differ <= B // 50, differ
    times = {k: [] for k in sides}
    for _ in range(a.rounds):
        for k, fn in sides.items():  # alternating
            times[k].append(_eager_us(fn, a.updates))
    med = {k: statistics.median(v) for k, v in times.items()}
    crm_us = med["crm"] - med["argmax"]
    flop = 2.0 * B * L * L
    report = {"batch": B, "leaves": L, "updates": a.updates, "rounds": a.rounds,
              "update_us": {k: {"median": round(med[k], 1), "min": round(min(v), 1), "max": round(max(v), 1)}
                            for k, v in times.items()},
              "crm_predict_us": round(crm_us, 1), "crm_predict_TFLOPs": round(flop / crm_us / 1e6, 1),
              "eager_over_crm_predict": round(med["eager_crm"] / crm_us, 2), "tree_dist_matrix_ms": round(build_ms, 2),
              "rows_differing_from_eager": differ, "rows_crm_differs_from_argmax": moved}
    lines = [f"f32 logits, B {B}, L {L}: uint8 matrix {L * L / 1e6:.0f} MB (its f32 copy for the eager route "
             f"{4 * L * L / 1e6:.0f} MB), 2 B L^2 = {flop / 1e9:.1f} GFLOP per batch"]
    for k, v in times.items():
        lines.append(f"  {k:10s} median {med[k]:9.1f} us  (min {min(v):9.1f}, max {max(v):9.1f}, "
                     f"{a.rounds} rounds x {a.updates} calls)")
    lines.append(f"  crm - argmax = hvk_crm_predict: {crm_us:.1f} us = {flop / crm_us / 1e6:.1f} TFLOP/s; "
                 f"eager route / hvk_crm_predict: {med['eager_crm'] / crm_us:.2f} x")
    lines.append(f"  ops.tree_dist_matrix (one call, first launch included): {build_ms:.2f} ms")
    lines.append(f"  CRM differs from the argmax on {moved} of {B} rows; fused and eager CRM differ on {differ}")
    text = "\n".join(lines)
    print(text, flush=True)
    print(json.dumps(report))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n" + json.dumps(report) + "\n")


if __name__ == "__main__":
    main()
