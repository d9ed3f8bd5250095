"""The optimizer step on the SwinV2-T + HXE parameter list (shapes only, random data): the fused
AdamW step (hvk_adamw_step) next to the torch sequences it replaces, and the fused SGDW step
(hvk_sgdw_step) on the same list as the yardstick for streaming rate.

  (a) hvamd.optim.AdamW.step() with the clip and the EMA handed over      (40 B / element)
  (b) clip_grad_norm_(foreach) + torch.optim.AdamW(foreach=True).step() + the two EMA foreach ops
  (a0) hvamd.optim.AdamW.step() alone                                      (28 B / element)
  (c) torch.optim.AdamW(fused=True).step() alone                           (context only)
  (s) / (s0) hvamd.optim.DecoupledSGDW.step() with / without clip and EMA  (32 / 20 B / element)

Every arm has its own tensors.  "eager": device events around STEPS back-to-back steps issued from
Python (the larger of host enqueue and device time, what a training loop sees), arms interleaved
over ROUNDS rounds, median.  "graph" (libhvk arms): the step captured PER_GRAPH times into a HIP
graph and replayed, so no host enqueue gap is in it.  Rates are the algorithmic bytes over the
time, as a fraction of 8 TB/s.

    python tools/bench_optim.py [--out FILE]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
STEPS, ROUNDS, PER_GRAPH, REPLAYS = 20, 5, 10, 10
PEAK = 8e12  # B / s


def shapes_and_groups():
    """[(shape, group)] of SwinV2-T with the 10 000-leaf HXE head; group 1 = no decay
    (optim.set_weight_decay's rule)."""
    from hvamd import hierarchy, swinv2
    tax = hierarchy.Taxonomy.synthetic()
    net = swinv2.SwinTransformerV2(num_classes=tax.num_leaves)  # on the host: only its shapes are used
    return [(tuple(p.shape), int(p.dim() == 1 or n.endswith(".bias")))
            for n, p in net.named_parameters() if p.requires_grad]


class Arm:
    def __init__(self, name, table, dev, seed):
        g = torch.Generator(device=dev).manual_seed(seed)
        self.name = name
        self.ps = [torch.nn.Parameter(0.02 * torch.randn(s, device=dev, generator=g)) for s, _ in table]
        for p in self.ps:
            p.grad = 0.1 * torch.randn(p.shape, device=dev, generator=g)
        self.emas = [p.detach().clone() for p in self.ps]
        self.groups = [{"params": [p for p, (_, k) in zip(self.ps, table) if k == 0]},
                       {"params": [p for p, (_, k) in zip(self.ps, table) if k == 1], "weight_decay": 0.0}]
        self.bytes_per_el = None  # algorithmic bytes per element, where the arm has a count
        self.graphable = False

    def handover(self):
        self.opt.pending_clip = 2.0
        self.opt.pending_ema = ([(id(p), e) for p, e in zip(self.ps, self.emas)], 0.99)


def build_arms(table, dev):
    from hvamd.optim import AdamW, DecoupledSGDW
    arms = []

    def add(name, make, step, nbytes=None, graphable=False):
        a = Arm(name, table, dev, len(arms))
        a.opt = make(a)
        a.step = lambda a=a: step(a)
        a.bytes_per_el, a.graphable = nbytes, graphable
        arms.append(a)

    def fused_full(a):
        a.handover()
        a.opt.step()

    def torch_sequence(a):
        torch.nn.utils.clip_grad_norm_(a.ps, 2.0, foreach=True)
        a.opt.step()
        torch._foreach_mul_(a.emas, 0.99)
        torch._foreach_add_(a.emas, [p.detach() for p in a.ps], alpha=0.01)

    adamw = lambda a: AdamW(a.groups, lr=1e-4, weight_decay=0.05)  # noqa: E731
    sgdw = lambda a: DecoupledSGDW(a.groups, lr=1e-4, momentum=0.9, weight_decay=5e-4)  # noqa: E731
    add("a  hvk adamw + clip + ema", adamw, fused_full, 40, True)
    add("b  torch clip + adamw(foreach) + ema", lambda a: torch.optim.AdamW(
        a.groups, lr=1e-4, weight_decay=0.05, foreach=True), torch_sequence)
    add("a0 hvk adamw alone", adamw, lambda a: a.opt.step(), 28, True)
    add("c  torch adamw(fused) alone", lambda a: torch.optim.AdamW(
        a.groups, lr=1e-4, weight_decay=0.05, fused=True), lambda a: a.opt.step())
    add("s  hvk sgdw + clip + ema", sgdw, fused_full, 32, True)
    add("s0 hvk sgdw alone", sgdw, lambda a: a.opt.step(), 20, True)
    return arms


def eager_us(arm):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(STEPS):
        arm.step()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / STEPS


def graph_us(arm, dev):
    arm.opt.enable_device_hyper(dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        arm.step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(PER_GRAPH):
            arm.step()
    graph.replay()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(REPLAYS):
        graph.replay()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / (PER_GRAPH * REPLAYS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    table = shapes_and_groups()
    numel = sum(torch.Size(s).numel() for s, _ in table)
    arms = build_arms(table, dev)
    for arm in arms:  # state init, code object loads
        arm.step()
        arm.step()
    times = {arm.name: [] for arm in arms}
    for _ in range(ROUNDS):
        for arm in arms:
            times[arm.name].append(eager_us(arm))
    lines = [f"SwinV2-T + HXE head: {len(table)} tensors, {numel} elements ({4 * numel / 1e6:.1f} MB f32)",
             f"eager: median of {ROUNDS} interleaved rounds of {STEPS} back-to-back steps; "
             f"graph: {PER_GRAPH} steps per HIP graph, {REPLAYS} replays; rate = algorithmic bytes / time",
             f"{'arm':38s} {'eager us':>9s} {'min..max':>17s} {'B/el':>5s} {'of 8 TB/s':>9s} "
             f"{'graph us':>9s} {'of 8 TB/s':>9s}"]
    med = {}
    for arm in arms:
        t = times[arm.name]
        med[arm.name] = m = statistics.median(t)
        row = f"{arm.name:38s} {m:9.1f} {min(t):8.1f}..{max(t):<8.1f}"
        if arm.bytes_per_el:
            nbytes = arm.bytes_per_el * numel
            row += f" {arm.bytes_per_el:5d} {nbytes / (m * 1e-6) / PEAK:9.3f}"
        if arm.graphable:
            g = graph_us(arm, dev)
            row += f" {g:9.1f} {arm.bytes_per_el * numel / (g * 1e-6) / PEAK:9.3f}"
        lines.append(row)
    fa, fb = med[arms[0].name], med[arms[1].name]
    lines.append(f"(a) / (b) = {fa / fb:.3f}  ((a) must be below 1: (b) makes over ten times the passes)")
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    if not fa < fb:
        sys.exit("defect: the fused step (a) is not faster than the sequence it replaces (b)")


if __name__ == "__main__":
    main()
