"""HXE loss kernels at the bench shape (B = 256, the 10 000-leaf iNat21-shaped tree): the hard
pair (hvk_hxe_fwd / _bwd) next to the soft-target pair (hvk_hxe_soft_fwd / _bwd, dense
LabelSmoothing(0.08) targets).  Each kernel is captured 50 times into a HIP graph and the graph
replayed, so the time per launch has no host enqueue gap in it; reported with the rate against
the algorithmic bytes.

    python tools/bench_hxe.py [--batch 256] [--replays 100]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PER_GRAPH = 50


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
    z = 3 * torch.randn(B, L, device=dev, generator=g)
    leaves = torch.randint(0, L, (B,), device=dev, generator=g)
    perm, start, end, base, paths = tax.device_tables(dev)
    _, rank_off, lo, hi, anc = tax.device_soft_tables(dev)
    n_nodes = lo.numel() - 1
    tgt = paths[leaves].contiguous()
    soft = smooth_labels(z, leaves, 0.08).contiguous()
    coeff = hierarchy.hxe_level_coeffs("exponential").to(dev)
    row, lse = torch.empty(B, device=dev), torch.empty(B, 8, device=dev)
    nl, nt = (torch.empty(B, n_nodes + 1, device=dev) for _ in range(2))
    gout, dz = torch.ones(1, device=dev), torch.empty_like(z)
    kernels = {
        "hxe_fwd": (lambda: _lib.call("hvk_hxe_fwd", P(z), B, L, P(perm), P(tgt), P(start), P(end), P(base),
                                      P(coeff), P(row), P(lse), st()), 4 * B * L),
        "hxe_bwd": (lambda: _lib.call("hvk_hxe_bwd", P(z), B, L, P(perm), P(tgt), P(start), P(end), P(base),
                                      P(coeff), P(lse), P(gout), P(dz), st()), 8 * B * L),
        "hxe_soft_fwd": (lambda: _lib.call("hvk_hxe_soft_fwd", P(z), P(soft), B, L, P(perm), n_nodes,
                                           P(rank_off), P(lo), P(hi), P(coeff), P(row), P(nl), P(nt), st()),
                         8 * B * L + 8 * B * (n_nodes + 1)),
        "hxe_soft_bwd": (lambda: _lib.call("hvk_hxe_soft_bwd", P(z), P(soft), B, L, P(perm), n_nodes, P(anc),
                                           P(coeff), P(nl), P(nt), P(gout), P(dz), st()),
                         12 * B * L + 8 * B * (n_nodes + 1)),
    }
    out = {"batch": B, "leaves": L, "n_nodes": n_nodes, "launches": PER_GRAPH * a.replays}
    for name, (fn, nbytes) in kernels.items():
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            fn()  # warm-up: code object load
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(PER_GRAPH):
                fn()
        graph.replay()
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(a.replays):
            graph.replay()
        e.record()
        torch.cuda.synchronize()
        us = s.elapsed_time(e) * 1e3 / (PER_GRAPH * a.replays)
        out[name] = {"us": round(us, 2), "bytes": nbytes, "TB_per_s": round(nbytes / us / 1e6, 3)}
        print(f"{name:13s} {us:8.2f} us  {nbytes / 1e6:7.2f} MB  {nbytes / us / 1e6:6.3f} TB/s", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
