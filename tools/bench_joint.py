"""ops.joint_decode (hvk_joint_decode: the seven multitask heads combined along every leaf's path,
one read of the logits) beside the eager route to the same numbers -- seven log_softmax calls, six
[B, L] gathers by the ancestor columns, a weighted sum, a topk and an argmax -- at the evaluation
shape: B = 256 rows over the iNat21 tier sizes (16 327 logits a row, column views of one buffer as
the head GEMM leaves them), f32 and bf16 logits, with and without the stored [B, L] scores.

Timing: `--calls` calls between two device events, the window closed by a device synchronise, so a
figure is what an evaluation loop pays per batch (launches, output allocation and host enqueue
included).  The sides alternate for `--rounds` rounds; the median is reported with the min-max
spread.  The rate is one read of the logits plus one write of the scores over the median.

    python tools/bench_joint.py [--batch 256] [--out FILE]
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
        raise SystemExit("bench_joint needs a GPU: nothing here is measurable on the CPU")
    from hvamd import hierarchy, ops
    dev = torch.device("cuda:0")
    tax = hierarchy.Taxonomy.synthetic()
    sizes, B, L = tax.num_classes, a.batch, tax.num_leaves
    parents, paths = tax.device_parent_tables(dev)
    anc = paths.long()
    total = sum(sizes)
    ld = (total + 7) // 8 * 8
    g = torch.Generator(device=dev).manual_seed(0)
    t = torch.randint(0, L, (B,), device=dev, generator=g)
    w = (8, 5.65, 4, 2.82, 2, 1.41, 1)
    wt = torch.tensor(w, device=dev)
    state = torch.zeros(16, device=dev, dtype=torch.float64)
    lines, report = [], {"batch": B, "sizes": list(sizes), "calls": a.calls, "rounds": a.rounds}
    for name, dt in (("f32", torch.float32), ("bf16", torch.bfloat16)):
        buf = (3 * torch.randn(B, ld, device=dev, generator=g)).to(dt)
        outs, off = [], 0
        for n in sizes:
            outs.append(buf[:, off:off + n])
            off += n

        def eager():
            lp = [torch.log_softmax(o.float(), 1) for o in outs]
            s = wt[6] * lp[6]
            for q in range(6):
                s = s + wt[q] * lp[q].gather(1, anc[:, q].expand(B, L))
            return s, s.topk(5, dim=1)[1], s.argmax(1)

        sides = {"joint": lambda: ops.joint_decode(outs, t, parents, paths, w, state),
                 "joint+scores": lambda: ops.joint_decode(outs, t, parents, paths, w, state, want_scores=True),
                 "eager": eager}
        for fn in sides.values():  # warm every shape the timed windows use
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        got, ref = sides["joint+scores"](), eager()
        differ = int((got["pred"].long() != ref[2]).sum())  # near-ties of f32 scores may differ
        err = float((got["scores"] - got["lse"][:, None] - torch.log_softmax(ref[0].double(), 1)).abs().max())
        assert differ <= B // 50 and err < 1e-2, (differ, err)
        times = {k: [] for k in sides}
        for _ in range(a.rounds):
            for k, fn in sides.items():  # alternating
                times[k].append(_us(fn, a.calls))
        med = {k: statistics.median(v) for k, v in times.items()}
        rd, wr = B * total * buf.element_size(), 4 * B * L
        gbs = {"joint": rd / med["joint"] / 1e3, "joint+scores": (rd + wr) / med["joint+scores"] / 1e3}
        report[name] = {"us": {k: {"median": round(med[k], 1), "min": round(min(v), 1), "max": round(max(v), 1)}
                               for k, v in times.items()},
                        "GBps": {k: round(v, 1) for k, v in gbs.items()},
                        "eager_over_joint": round(med["eager"] / med["joint"], 2),
                        "eager_over_joint_scores": round(med["eager"] / med["joint+scores"], 2),
                        "rows_differing_from_eager": differ, "max_logp_difference": err}
        lines.append(f"{name} logits, B {B}, tiers {tuple(sizes)}: {rd / 1e6:.1f} MB read, {wr / 1e6:.1f} MB of scores")
        for k, v in times.items():
            lines.append(f"  {k:13s} median {med[k]:8.1f} us  (min {min(v):8.1f}, max {max(v):8.1f}, "
                         f"{a.rounds} rounds x {a.calls} calls)" + (f"  {gbs[k]:7.1f} GB/s" if k in gbs else ""))
        lines.append(f"  eager / joint {med['eager'] / med['joint']:.2f} x, eager / joint+scores "
                     f"{med['eager'] / med['joint+scores']:.2f} x; predictions differing from eager {differ} of {B}, "
                     f"largest |log p| difference {err:.3g}")
    text = "\n".join(lines)
    print(text, flush=True)
    print(json.dumps(report))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n" + json.dumps(report) + "\n")


if __name__ == "__main__":
    main()
