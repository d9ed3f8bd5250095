"""Run-to-run spread of twin AdamW trainers on the mini SwinV2 + HXE of tests/test_gpu_adamw.py:
RUNS trainers on the FOREACH path from the same start, every pair compared per tensor class with
that test's twin_errors().  The backward's f32 atomics sum in a run-dependent order and Adam's
normalised update amplifies that noise in the zero-initialised 1-D tensors; the largest
foreach-against-foreach figure of a class times 4 is that class's bound in the test where the
project's 1e-2 does not hold (no reading of the fused path enters it).  The fused path against
the foreach path is printed next to it for information.

    python tools/adamw_twin_spread.py [--out FILE]
"""
import argparse
import copy
import itertools
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
RUNS = 5
# the step sequences of the test's trainer cases: (lr per step, decoupled)
SCENARIOS = {"4 steps": ([1e-3] * 4, False), "5 steps": ([1e-3] * 5, False), "6 steps": ([1e-3] * 6, False),
             "lr schedule, 7 steps": ([1e-3] * 4 + [3e-3, 0.0, 0.0], True)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import test_gpu_adamw as T
    from hvamd import options

    def run(model0, batch, lrs, decoupled, fused):
        model = copy.deepcopy(model0)
        with options.override(fused_optim=fused):
            t = T._trainer(model, decoupled=decoupled)
            for lr in lrs:
                for g in t.optimizer.param_groups:
                    g["lr"] = lr
                t.train_step(batch)
        torch.cuda.synchronize()
        return model, T._ema(t)

    def worst_of(pairs, init):
        worst = {}
        for (ma, ea), (mb, eb) in pairs:
            for cls, (err, _) in T.twin_errors(ma, mb, init, ea, eb).items():
                worst[cls] = max(worst.get(cls, 0.0), err)
        return worst

    lines = [f"{RUNS} foreach runs per case, all {RUNS * (RUNS - 1) // 2} pairs; fused: one run against each; "
             "worst tensor of each class"]
    total = {}
    for name, (lrs, dec) in SCENARIOS.items():
        model0, batch = T._setup()
        init = {n: p.detach().clone() for n, p in model0.named_parameters()}
        foreach = [run(model0, batch, lrs, dec, False) for _ in range(RUNS)]
        fused = run(model0, batch, lrs, dec, True)
        spread = worst_of(itertools.combinations(foreach, 2), init)
        against = worst_of([(fused, f) for f in foreach], init)
        for cls in sorted(spread):
            total[cls] = max(total.get(cls, 0.0), spread[cls])
            lines.append(f"{name:22s} {cls:18s} foreach-vs-foreach {spread[cls]:.3e}   "
                         f"fused-vs-foreach {against[cls]:.3e}")
    lines.append("largest foreach-vs-foreach figure per class (x 4 = the bound where 1e-2 does not hold):")
    for cls in sorted(total):
        lines.append(f"  {cls:18s} {total[cls]:.3e}   x4 = {4 * total[cls]:.3e}")
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
