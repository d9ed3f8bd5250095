"""EvalMetrics.update (one hvk_eval_metrics call) beside the four metric classes it stands in
for (Accuracy top-1, Accuracy top-5, CrossEntropyMetric, TreeDistance: their update calls) at
the evaluation shape, B = 256 logit rows over L = 10 000 leaves, f32 and bf16.

Timing: `--updates` eager update calls between two device events, the window closed by a device
synchronise, so the figure is what a caller's evaluation loop pays per batch (launches and host
enqueue included).  The two sides alternate for `--rounds` rounds; the median is reported with
the min-max spread.  The fused update is also captured 50 times into a HIP graph and replayed:
its device time with no enqueue gap, given with the rate against the B * ld * elemsize bytes of
one read of the logits.  (The classes are not captured: their cross-entropy builds a host tensor
per call.)

    python tools/bench_eval_metrics.py [--batch 256] [--leaves 10000] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PER_GRAPH = 50


def _eager_us(fn, updates):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(updates):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / updates


def _graph_us(fn, replays):
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(PER_GRAPH):
            fn()
    graph.replay()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(replays):
        graph.replay()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / (PER_GRAPH * replays)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--leaves", type=int, default=10000)
    ap.add_argument("--updates", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--replays", type=int, default=40)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval_metrics needs a GPU: nothing here is measurable on the CPU")
    from hvamd import hierarchy
    dev = torch.device("cuda:0")
    B, L = a.batch, a.leaves
    tax = hierarchy.Taxonomy.synthetic(tuple(min(s, L) for s in (3, 13, 51, 273, 1103, 4884, L)))
    g = torch.Generator(device=dev).manual_seed(0)
    z32 = 3 * torch.randn(B, L, device=dev, generator=g)
    t = torch.randint(0, L, (B,), device=dev, generator=g)
    # the L x L uint8 matrix both sides read one entry per row of
    paths = torch.from_numpy(tax.leaf_paths).to(dev)
    td = torch.full((L, L), 7, dtype=torch.uint8, device=dev)
    for lvl, q in enumerate(range(6, -1, -1)):
        same = paths[:, None, q] == paths[None, :, q]
        td = torch.where(same & (td == 7), torch.tensor(lvl, dtype=torch.uint8, device=dev), td)
        del same
    lines, report = [], {"batch": B, "leaves": L, "updates": a.updates, "rounds": a.rounds}
    for name, z in (("f32", z32), ("bf16", z32.bfloat16())):
        fused = hierarchy.EvalMetrics(tree_dists=td).to(dev)
        fused_paths = hierarchy.EvalMetrics(taxonomy=tax).to(dev)
        classes = [hierarchy.Accuracy(L).to(dev), hierarchy.Accuracy(L, top_k=5).to(dev),
                   hierarchy.CrossEntropyMetric().to(dev), hierarchy.TreeDistance(td).to(dev)]

        def run_classes():
            for m in classes:
                m.update(z, t)

        sides = {"fused": lambda: fused.update(z, t), "fused_paths": lambda: fused_paths.update(z, t),
                 "classes": run_classes}
        for fn in sides.values():  # warm every shape the timed windows use
            for _ in range(20):
                fn()
        torch.cuda.synchronize()
        # both agree before either is timed
        fused.reset()
        for m in classes:
            m.reset()
        sides["fused"]()
        sides["classes"]()
        got = fused.compute()
        want = [m.compute().item() for m in classes]
        for k, w in zip(("acc@1", "acc@5", "cross-entropy", "tree-dist"), want):
            assert abs(got[k] - w) <= 1e-5 * max(1.0, abs(w)), (k, got[k], w)
        times = {k: [] for k in sides}
        for _ in range(a.rounds):
            for k, fn in sides.items():  # alternating
                times[k].append(_eager_us(fn, a.updates))
        nbytes = B * z.stride(0) * z.element_size()
        gus = _graph_us(sides["fused"], a.replays)
        med = {k: statistics.median(v) for k, v in times.items()}
        report[name] = {"eager_us": {k: {"median": round(med[k], 2), "min": round(min(v), 2), "max": round(max(v), 2)}
                                     for k, v in times.items()},
                        "classes_over_fused": round(med["classes"] / med["fused"], 2),
                        "fused_graph_us": round(gus, 2), "logit_bytes": nbytes,
                        "fused_graph_TB_per_s": round(nbytes / gus / 1e6, 3)}
        lines.append(f"{name} logits, B {B}, L {L} ({nbytes / 1e6:.2f} MB per read of the logits)")
        for k, v in times.items():
            lines.append(f"  eager update  {k:12s} median {med[k]:8.2f} us  (min {min(v):8.2f}, max {max(v):8.2f}, "
                         f"{a.rounds} rounds x {a.updates} updates)")
        lines.append(f"  classes / fused (eager medians): {med['classes'] / med['fused']:.2f} x")
        lines.append(f"  fused update in a HIP graph (rows + accumulate kernels, no enqueue gap): {gus:.2f} us  "
                     f"= {nbytes / gus / 1e6:.3f} TB/s of logits")
    text = "\n".join(lines)
    print(text, flush=True)
    print(json.dumps(report))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n" + json.dumps(report) + "\n")


if __name__ == "__main__":
    main()
