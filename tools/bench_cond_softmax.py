"""The conditional-softmax head (hvk_cond_softmax_fwd / _bwd / _decode) beside the eager route to
the same numbers on the device -- per tier a segment log-sum-exp over the sibling groups
(scatter_reduce amax, index_add of the shifted exponentials), a gather back to the nodes, and for
the leaf distribution seven [B, L] gathers by leaf_paths -- at B = 256 rows over the iNat21 tier
sizes (16 327 node logits a row, column views of one buffer as the head GEMM leaves them), f32 and
bf16 logits: the loss's forward + backward, and the decoder with and without the stored scores.

Timing: `--calls` calls between two device events, the window closed by a device synchronise, so a
figure is what a training / evaluation loop pays per batch (launches, output allocation and host
enqueue included).  The sides alternate for `--rounds` rounds; the median is reported with the
min-max spread.

    python tools/bench_cond_softmax.py [--batch 256] [--out FILE]
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
        raise SystemExit("bench_cond_softmax needs a GPU: nothing here is measurable on the CPU")
    from hvamd import hierarchy, ops
    dev = torch.device("cuda:0")
    tax = hierarchy.Taxonomy.synthetic()
    sizes, B, L = tax.num_classes, a.batch, tax.num_leaves
    parents, paths = tax.device_parent_tables(dev)
    sib_ptr, sib_col = tax.device_sibling_tables(dev)
    off, par = tax.parent_tables()
    # eager tables: per tier the group of every node (0-based within the tier) and the group count
    group = [torch.zeros(sizes[0], dtype=torch.long, device=dev)] + [
        torch.from_numpy(par[off[t] - off[1]:off[t + 1] - off[1]]).long().to(dev) for t in range(1, 7)]
    n_groups = [1] + list(sizes[:6])
    anc = paths.long()
    total = sum(sizes)
    ld = (total + 7) // 8 * 8
    g = torch.Generator(device=dev).manual_seed(0)
    t = torch.randint(0, L, (B,), device=dev, generator=g)
    y = anc[t]
    rows = torch.arange(B, device=dev)
    state = torch.zeros(16, device=dev, dtype=torch.float64)
    lines, report = [], {"batch": B, "sizes": list(sizes), "calls": a.calls, "rounds": a.rounds}

    def log_cond(outs):
        res = []
        for q, o in enumerate(outs):
            z, idx = o.float(), group[q].expand(B, -1)
            m = torch.full((B, n_groups[q]), -torch.inf, device=dev).scatter_reduce(1, idx, z.detach(), "amax")
            s = torch.zeros(B, n_groups[q], device=dev).scatter_add(1, idx, torch.exp(z - m.gather(1, idx)))
            res.append(z - (m + torch.log(s)).gather(1, idx))
        return res

    for name, dt in (("f32", torch.float32), ("bf16", torch.bfloat16)):
        buf = (3 * torch.randn(B, ld, device=dev, generator=g)).to(dt).requires_grad_()
        outs = [buf[:, a_:b_] for a_, b_ in zip(off[:-1].tolist(), off[1:].tolist())]
        plain = [o.detach() for o in outs]

        def fused_loss():
            buf.grad = None
            ops.cond_softmax_cross_entropy(outs, y, parents, sib_ptr, sib_col).backward()
            return buf.grad

        def eager_loss():
            buf.grad = None
            sum(-lc[rows, y[:, q]] for q, lc in enumerate(log_cond(outs))).mean().backward()
            return buf.grad

        def eager_decode():
            s = sum(lc.gather(1, anc[:, q].expand(B, L)) for q, lc in enumerate(log_cond(plain)))
            return s, s.topk(5, dim=1)[1], s.argmax(1)

        sides = {"loss fwd+bwd": fused_loss, "eager loss fwd+bwd": eager_loss,
                 "decode": lambda: ops.cond_softmax_decode(plain, t, parents, sib_ptr, sib_col, paths, state),
                 "decode+scores": lambda: ops.cond_softmax_decode(plain, t, parents, sib_ptr, sib_col, paths, state,
                                                                  want_scores=True),
                 "eager decode": eager_decode}
        for fn in sides.values():  # warm every shape the timed windows use
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        gerr = float((fused_loss().float() - eager_loss().float()).abs().max())
        got, ref = sides["decode+scores"](), eager_decode()
        differ = int((got["pred"].long() != ref[2]).sum())  # near-ties of f32 scores may differ
        err = float((got["scores"] - ref[0]).abs().max())
        assert differ <= B // 50 and err < 1e-2 and gerr < (1e-4 if dt == torch.float32 else 1e-2) / B, (differ, err, gerr)
        times = {k: [] for k in sides}
        for _ in range(a.rounds):
            for k, fn in sides.items():  # alternating
                times[k].append(_us(fn, a.calls))
        med = {k: statistics.median(v) for k, v in times.items()}
        ratios = {"eager_over_fused_loss": med["eager loss fwd+bwd"] / med["loss fwd+bwd"],
                  "eager_over_decode": med["eager decode"] / med["decode"],
                  "eager_over_decode_scores": med["eager decode"] / med["decode+scores"]}
        report[name] = {"us": {k: {"median": round(med[k], 1), "min": round(min(v), 1), "max": round(max(v), 1)}
                               for k, v in times.items()},
                        **{k: round(v, 2) for k, v in ratios.items()},
                        "rows_differing_from_eager": differ, "max_logp_difference": err, "max_gradient_difference": gerr}
        lines.append(f"{name} logits, B {B}, tiers {tuple(sizes)}: {B * total * buf.element_size() / 1e6:.1f} MB of logits, "
                     f"{4 * B * L / 1e6:.1f} MB of scores")
        for k, v in times.items():
            lines.append(f"  {k:19s} median {med[k]:8.1f} us  (min {min(v):8.1f}, max {max(v):8.1f}, "
                         f"{a.rounds} rounds x {a.calls} calls)")
        lines.append("  " + ", ".join(f"{k.replace('_', ' ')} {v:.2f} x" for k, v in ratios.items())
                     + f"; predictions differing from eager {differ} of {B}, largest |log p| difference {err:.3g}, "
                     f"largest gradient difference {gerr:.3g}")
    text = "\n".join(lines)
    print(text, flush=True)
    print(json.dumps(report))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n" + json.dumps(report) + "\n")


if __name__ == "__main__":
    main()
