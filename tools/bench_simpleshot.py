"""SimpleShot's four device steps at the evaluation shape, B = 256 feature rows against the
L = 10 000 leaves of Taxonomy.synthetic(), D = 768 (SwinV2-T) and 1024 (SwinV2-B): predict_flat
(hvk_ss_predict_flat: the f32-MFMA GEMM with its running row argmin), predict_tree
(hvk_ss_predict_tree: one walk down the tree), one partial_fit batch (a stable argsort by torch,
then hvk_ss_accumulate) and finalize (hvk_ss_finalize over the 16 327 nodes), next to the torch
f32 expression `(cnorm - 2 * x @ c.T).argmin(1)` the flat prediction stands in for.

Timing: `--calls` eager calls between two device events, the window closed by a device
synchronise: what a caller's loop pays per call, launches and host enqueue included.  The sides
alternate for `--rounds` rounds; the median is reported with the min-max spread.  The two
predictions are also captured `PER_GRAPH` times into a HIP graph and replayed: device time with
no enqueue gap, given with the rate against the algorithmic bytes

    flat  4 (B * splits_read + L) * D + 4 L   every centroid once, the 64-row X tiles once per
                                              class split that reads them (splits = workspace
                                              bytes / 8 B), and cnorm
    tree  4 (1 + rows on the path) * D        per sample: its row and the centroid rows of the
                                              candidates it compares (counted from the tree and
                                              the predicted paths)

and, for flat, the f32 matrix rate 2 B L D / t.  Before anything is timed the flat prediction
is checked against the torch expression (rows where they differ are counted and printed: both
are f32, so near-ties may fall either way).

    python tools/bench_simpleshot.py [--batch 256] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PER_GRAPH = 20


def _eager_us(fn, calls):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(calls):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / calls


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
    ap.add_argument("--dims", type=int, nargs="+", default=[768, 1024])
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_simpleshot needs a GPU: nothing here is measurable on the CPU")
    from hvamd import _lib, hierarchy, ops, simpleshot
    dev = torch.device("cuda:0")
    B = a.batch
    tax = hierarchy.Taxonomy.synthetic()
    L = tax.num_leaves
    vecs = hierarchy.parent_vectors([hierarchy.HierarchicalLabel.parse(c) for c in tax.classes])
    paths = torch.from_numpy(tax.leaf_paths).to(dev)
    sizes, tier_base, child_ptr, _ = simpleshot.children_csr(vecs)
    n_children = [np.ones(1, np.int64) * sizes[0]] + [
        np.diff(child_ptr[tier_base[t]:tier_base[t + 1] + 1]).astype(np.int64) for t in range(len(sizes) - 1)]
    lines, report = [], {"batch": B, "leaves": L, "calls": a.calls, "rounds": a.rounds}
    for D in a.dims:
        g = torch.Generator(device=dev).manual_seed(D)
        # class means that follow the tree, 3 training rows per leaf, as the tests build them
        mean = torch.zeros(L, D, device=dev)
        for t, n in enumerate(sizes):
            mean += 0.5 ** t * torch.randn(n, D, device=dev, generator=g)[paths[:, t]]
        leaf = torch.randperm(3 * L, device=dev, generator=g) % L
        clf = simpleshot.HierarchicalNearestCentroid(vecs)
        for i in range(0, 3 * L, 4096):
            rows = leaf[i:i + 4096]
            clf.partial_fit(mean[rows] + 0.6 * torch.randn(len(rows), D, device=dev, generator=g), paths[rows])
        clf.finalize()
        q = torch.randint(0, L, (B,), device=dev, generator=g)
        x = mean[q] + 0.6 * torch.randn(B, D, device=dev, generator=g)
        y = paths[q]
        cent, cnorm = clf.centroids_[-1], clf._tier(clf._cnorm, 6)
        tb, cptr, cidx = clf._device_csr(dev)
        # a scratch classifier the timed partial_fit / finalize work on (their sums keep growing)
        fit = simpleshot.HierarchicalNearestCentroid(vecs)
        fit.partial_fit(x, y)

        sides = {
            "predict_flat": lambda: ops.ss_predict_flat(x, cent, cnorm),
            "torch_argmin": lambda: (cnorm - 2 * x @ cent.T).argmin(1),
            "predict_tree": lambda: ops.ss_predict_tree(x, clf._cent, clf._counts, tb, cptr, cidx),
            "partial_fit": lambda: fit.partial_fit(x, y),
            "finalize": lambda: fit.finalize(),
        }
        for fn in sides.values():  # warm every shape the timed windows use
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        ours, theirs = sides["predict_flat"]().long(), sides["torch_argmin"]()
        differ = int((ours != theirs).sum())
        tree_pred = sides["predict_tree"]().cpu().numpy()
        # centroid rows a sample compares: all of tier 0, then the children of each chosen node
        path_rows = float(np.mean(sum(n_children[t][tree_pred[:, t - 1]] if t else
                                      np.full(B, n_children[0][0]) for t in range(len(sizes)))))
        times = {k: [] for k in sides}
        for _ in range(a.rounds):
            for k, fn in sides.items():  # alternating
                times[k].append(_eager_us(fn, a.calls))
        med = {k: statistics.median(v) for k, v in times.items()}
        splits = _lib.load().hvk_ss_predict_flat_workspace(B, L) // (8 * B)
        flat_bytes = 4 * (B * splits + L) * D + 4 * L
        tree_bytes = 4 * B * (1 + path_rows) * D
        gf, gt, gm = (_graph_us(sides[k], a.replays) for k in ("predict_flat", "predict_tree", "torch_argmin"))
        report[str(D)] = {
            "eager_us": {k: {"median": round(med[k], 2), "min": round(min(v), 2), "max": round(max(v), 2)}
                         for k, v in times.items()},
            "torch_over_flat": round(med["torch_argmin"] / med["predict_flat"], 2),
            "flat_vs_torch_rows_differing": differ, "class_splits": int(splits),
            "graph_us": {"predict_flat": round(gf, 2), "torch_argmin": round(gm, 2), "predict_tree": round(gt, 2)},
            "flat_bytes": flat_bytes, "flat_TB_per_s": round(flat_bytes / gf / 1e6, 3),
            "flat_TFLOP_per_s": round(2.0 * B * L * D / gf / 1e6, 2),
            "tree_rows_per_sample": round(path_rows, 1), "tree_bytes": int(tree_bytes),
            "tree_TB_per_s": round(tree_bytes / gt / 1e6, 3)}
        lines.append(f"D {D}, B {B}, L {L} ({sum(sizes)} nodes); flat and torch argmin differ in {differ} of {B} rows")
        for k, v in times.items():
            lines.append(f"  eager  {k:13s} median {med[k]:9.2f} us  (min {min(v):9.2f}, max {max(v):9.2f}, "
                         f"{a.rounds} rounds x {a.calls} calls)")
        word = "faster" if med["torch_argmin"] >= med["predict_flat"] else "SLOWER"
        lines.append(f"  predict_flat is {word} than the torch f32 expression: torch / flat = "
                     f"{med['torch_argmin'] / med['predict_flat']:.2f} x (eager medians)")
        lines.append(f"  HIP graph, no enqueue gap: predict_flat {gf:.2f} us = {2.0 * B * L * D / gf / 1e6:.2f} TFLOP/s f32, "
                     f"{flat_bytes / 1e6:.2f} MB algorithmic ({splits} class splits) = {flat_bytes / gf / 1e6:.3f} TB/s; "
                     f"torch expression {gm:.2f} us")
        lines.append(f"  HIP graph: predict_tree {gt:.2f} us, {path_rows:.1f} centroid rows per sample, "
                     f"{tree_bytes / 1e6:.2f} MB algorithmic = {tree_bytes / gt / 1e6:.3f} TB/s "
                     f"(the reference's route compares every one of the {sum(sizes)} rows with every sample)")
    text = "\n".join(lines)
    print(text, flush=True)
    print(json.dumps(report))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n" + json.dumps(report) + "\n")


if __name__ == "__main__":
    main()
