"""ops.backoff_decode (hvk_backoff_decode: the greedy walk down the taxonomy by node mass, every
node's mass in LDS) beside the eager route to the same numbers -- a softmax, six segment sums by
index_add, seven masked argmaxes with their gathers, and the per-threshold counts -- at the
evaluation shape: B = 256 rows over the synthetic iNat21 tree (10 000 leaves, 6 328 node slots), f32
and bf16 logits, BackoffMetrics' seven default thresholds.

Timing: `--calls` calls between two device events, the window closed by a device synchronise, so a
figure is what an evaluation loop pays per batch (launches, output allocation and host enqueue
included).  The sides alternate for `--rounds` rounds; the median is reported with the min-max
spread.  The rate is two reads of the logits (the second from L2) over the median.

    python tools/bench_backoff.py [--batch 256] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _us(fn, calls):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(calls):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_backoff needs a GPU: nothing here is measurable on the CPU")
    from hvamd import hierarchy, ops
    dev = torch.device("cuda:0")
    tax = hierarchy.Taxonomy.synthetic()
    B, L, sizes = a.batch, tax.num_leaves, tax.num_classes
    tables = tax.device_backoff_tables(dev)
    parents, paths = tax.device_parent_tables(dev)
    off = tax.parent_tables()[0]
    anc = paths.long()
    # the parent of every node of tier t >= 1, and a rank that orders a tier's nodes by node_start
    parent = [None] + [parents[off[t] - off[1]:off[t + 1] - off[1]].long() for t in range(1, 7)]
    start = [torch.from_numpy(tax.node_start[tax.tier_base[t]:tax.tier_base[t] + sizes[t]].copy()).to(dev) for t in range(7)]
    thresholds = hierarchy.BackoffMetrics(tax).thresholds
    th = torch.tensor(thresholds, device=dev)
    g = torch.Generator(device=dev).manual_seed(0)
    t = torch.randint(0, L, (B,), device=dev, generator=g)
    state = torch.zeros(2 + 5 * len(thresholds), device=dev, dtype=torch.float64)
    lines, report = [], {"batch": B, "sizes": list(sizes), "calls": a.calls, "rounds": a.rounds}
    for name, dt in (("f32", torch.float32), ("bf16", torch.bfloat16)):
        z = (3 * torch.randn(B, L, device=dev, generator=g)).to(dt)

        def eager():
            p = torch.softmax(z.float(), 1)
            path, prob, cur = [], [], None
            for d in range(7):
                mass = p if d == 6 else torch.zeros(B, sizes[d], device=dev).index_add_(1, anc[:, d], p)
                if d > 0:  # only the children of the node the walk stands on compete
                    mass = mass.masked_fill(parent[d][None, :] != cur[:, None], -1.0)
                # the largest mass, the lowest node_start among equals
                best = mass.max(1, keepdim=True)[0]
                cur = torch.where(mass == best, start[d][None, :], L).argmin(1)
                path.append(cur)
                prob.append(best[:, 0])
            path, prob = torch.stack(path, 1), torch.stack(prob, 1)
            m = (path == anc[t]).long().cumprod(1).sum(1)
            D = (prob[:, None, :] >= th[None, :, None]).sum(2)  # [B, T]
            mm = m[:, None]
            sums = torch.stack([x.long() for x in (D, D <= mm, torch.minimum(D, mm), D == 7, (D == 7) & (mm == 7))], 2).sum(0)
            return path, prob, m, sums

        sides = {"backoff": lambda: ops.backoff_decode(z, t, *tables, paths, thresholds, state), "eager": eager}
        for fn in sides.values():  # warm every shape the timed windows use
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        state.zero_()
        got, ref = sides["backoff"](), eager()
        differ = int((got["path"].long() != ref[0]).any(1).sum())  # near-ties of f32 masses may differ
        same = (got["path"].long() == ref[0]).all(1)
        err = float((got["prob"] - ref[1])[same].abs().max())
        counts_equal = bool(differ) or torch.equal(state[2:].view(-1, 5), ref[3].double())
        assert differ <= B // 50 and err < 1e-5 and counts_equal, (differ, err, counts_equal)
        times = {k: [] for k in sides}
        for _ in range(a.rounds):
            for k, fn in sides.items():  # alternating
                times[k].append(_us(fn, a.calls))
        med = {k: statistics.median(v) for k, v in times.items()}
        rd = 2 * B * L * z.element_size()
        report[name] = {"us": {k: {"median": round(med[k], 1), "min": round(min(v), 1), "max": round(max(v), 1)}
                               for k, v in times.items()},
                        "GBps": round(rd / med["backoff"] / 1e3, 1),
                        "eager_over_backoff": round(med["eager"] / med["backoff"], 2),
                        "rows_differing_from_eager": differ, "max_prob_difference": err}
        lines.append(f"{name} logits, B {B}, tiers {tuple(sizes)}, {len(thresholds)} thresholds: {rd / 1e6:.1f} MB read")
        for k, v in times.items():
            lines.append(f"  {k:8s} median {med[k]:8.1f} us  (min {min(v):8.1f}, max {max(v):8.1f}, "
                         f"{a.rounds} rounds x {a.calls} calls)" + (f"  {rd / med[k] / 1e3:7.1f} GB/s" if k == "backoff" else ""))
        lines.append(f"  eager / backoff {med['eager'] / med['backoff']:.2f} x; paths differing from eager {differ} of {B}, "
                     f"largest |prob| difference {err:.3g}")
    text = "\n".join(lines)
    print(text, flush=True)
    print(json.dumps(report))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n" + json.dumps(report) + "\n")


if __name__ == "__main__":
    main()
