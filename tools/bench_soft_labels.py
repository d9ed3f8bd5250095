"""Soft-labels loss at the bench shape (B = 256, the 10 000-leaf iNat21-shaped tree): the four
kernels (hvk_soft_labels_fwd / _bwd, hvk_soft_labels_dense_fwd / _bwd), each captured 50 times
into a HIP graph and replayed (time per launch without the host enqueue gap, and the rate
against the algorithmic bytes), then loss + backward through the public interface next to the
route a user had without the kernels: targets gathered from a precomputed [L, L] f32 matrix
into hierarchy.soft_cross_entropy.

    python tools/bench_soft_labels.py [--batch 256] [--replays 100]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PER_GRAPH = 50


def timed(fn, n):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--replays", type=int, default=100)
    a = ap.parse_args()
    from hvamd import _lib, hierarchy
    from hvamd.algorithmic import smooth_labels
    P, st = _lib.ptr, _lib.stream
    dev = torch.device("cuda:0")
    tax = hierarchy.Taxonomy.synthetic()
    B, L = a.batch, tax.num_leaves
    g = torch.Generator(device=dev).manual_seed(0)
    z = (3 * torch.randn(B, L, device=dev, generator=g)).requires_grad_(True)
    leaves = torch.randint(0, L, (B,), device=dev, generator=g)
    perm, start, end, base, paths = tax.device_tables(dev)
    _, rank_off, lo, hi, anc = tax.device_soft_tables(dev)
    n_nodes = lo.numel() - 1
    tgt = paths[leaves].contiguous()
    q = smooth_labels(z.detach(), leaves, 0.08).contiguous()
    loss_fn = hierarchy.SoftLabelsCrossEntropy(tax, beta=15.0).to(dev)
    w, inv = loss_fn.level_weight, tax.soft_label_norms(loss_fn.level_weight.tolist(), dev)
    row, lse, ts = (torch.empty(B, device=dev) for _ in range(3))
    nr = torch.empty(B, n_nodes + 1, device=dev)
    gout, dz = torch.ones(1, device=dev), torch.empty(B, L, device=dev)
    kernels = {
        "soft_labels_fwd": (lambda: _lib.call("hvk_soft_labels_fwd", P(z), B, L, P(perm), P(tgt), P(start), P(end),
                                              P(base), P(w), P(row), P(lse), st()), 4 * B * L),
        "soft_labels_bwd": (lambda: _lib.call("hvk_soft_labels_bwd", P(z), B, L, P(perm), P(tgt), P(start), P(end),
                                              P(base), P(w), P(lse), P(gout), P(dz), st()), 8 * B * L),
        "soft_labels_dense_fwd": (lambda: _lib.call("hvk_soft_labels_dense_fwd", P(z), P(q), P(inv), B, L, P(perm),
                                                    n_nodes, P(rank_off), P(lo), P(hi), P(anc), P(w), P(row), P(lse),
                                                    P(ts), P(nr), st()), 8 * B * L + 4 * B * (n_nodes + 1)),
        "soft_labels_dense_bwd": (lambda: _lib.call("hvk_soft_labels_dense_bwd", P(z), P(q), P(inv), B, L, P(perm),
                                                    n_nodes, P(anc), P(w), P(lse), P(ts), P(nr), P(gout), P(dz), st()),
                                  12 * B * L + 4 * B * (n_nodes + 1)),
    }
    out = {"batch": B, "leaves": L, "n_nodes": n_nodes, "launches": PER_GRAPH * a.replays}
    for name, (fn, nbytes) in kernels.items():
        with torch.cuda.stream(torch.cuda.Stream()):
            fn()  # warm-up: code object load
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(PER_GRAPH):
                fn()
        graph.replay()
        torch.cuda.synchronize()
        us = timed(graph.replay, a.replays) / (PER_GRAPH * a.replays)
        out[name] = {"us": round(us, 2), "bytes": nbytes, "TB_per_s": round(nbytes / us / 1e6, 3)}
        print(f"{name:22s} {us:8.2f} us  {nbytes / 1e6:7.2f} MB  {nbytes / us / 1e6:6.3f} TB/s", flush=True)

    # the [L, L] f32 target matrix of the route without the kernels: T[c] = w[d(c, .)] / Z_c
    T = torch.empty(L, L, device=dev)
    for c0 in range(0, L, 1000):  # equal tier ids are the shared ancestors: d = 7 - their number
        d = 7 - (paths[c0:c0 + 1000, None, :] == paths[None, :, :]).sum(-1)
        T[c0:c0 + 1000] = w[d] * inv[c0:c0 + 1000, None]

    def step(loss):
        z.grad = None
        loss().backward()
    routes = {"kernels_hard": lambda: loss_fn(z, tgt), "kernels_dense": lambda: loss_fn(z, q),
              "gather_soft_ce": lambda: hierarchy.soft_cross_entropy(z, T[leaves])}
    for name, loss in routes.items():  # loss + backward, host enqueue included, alternating repeats below
        step(loss)
    torch.cuda.synchronize()
    for rep in range(3):
        for name, loss in routes.items():
            us = timed(lambda: step(loss), 200) / 200
            out.setdefault(name, []).append(round(us, 1))
            print(f"{name:22s} {us:8.1f} us per loss + backward (repeat {rep})", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
