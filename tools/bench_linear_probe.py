"""The linear probe's solver at the evaluation shapes: one accelerated-gradient iteration
(hvk_lp_loss_grad + hvk_lp_step over all R = 3 L binary problems of one cross-validation fold) and
a whole `grid_search`, on 10 rows per class of Gaussian blobs: N = 20 000 / L = 2 000 and
N = 100 000 / L = 10 000, D = 768 (SwinV2-T) and 1024 (SwinV2-B), next to the same iteration
written in torch eager f32 on the same device (which materialises the [N, R] scores).

Timing: `--calls` iterations between two device events, the window closed by a device
synchronise; the sides alternate for `--rounds` rounds and the median is reported with the
min-max spread.  The iteration's rate is given against its algorithmic work

    flops  4 N R D               the two products (forward scores, residual^T . xs)
    bytes  4 (N D + 3 R D + N)   xs once, W read and dW written and W read again, the labels

as the fraction of the f32-input MFMA peak (157.3 TFLOP/s).  There is no threshold: the numbers
go to DESIGN.md as measured.  A grid search is run for the shapes named by `--grid` only (the
largest one takes many minutes); its iteration counts per fold are printed.

    python tools/bench_linear_probe.py [--shapes 20000x2000 100000x10000] [--grid 20000x2000x768] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
F32_MFMA_PEAK = 157.3e12
ALPHAS = (1e-4, 1e-2, 1.0)


def _window_us(fn, calls):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(calls):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / calls


def _blobs(N, L, D, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    means = 0.4 * torch.randn(L, D, device=dev, generator=g)
    y = torch.randperm(N, device=dev, generator=g) % L
    return means[y] + torch.randn(N, D, device=dev, generator=g) + 3.0, y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=["20000x2000", "100000x10000"], help="NxL of the iteration")
    ap.add_argument("--dims", type=int, nargs="+", default=[768, 1024])
    ap.add_argument("--grid", nargs="*", default=["20000x2000x768", "20000x2000x1024", "100000x10000x768",
                                                  "100000x10000x1024"], help="NxLxD of the grid searches")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_linear_probe needs a GPU: nothing here is measurable on the CPU")
    from hvamd import linear_probe, ops
    dev = torch.device("cuda:0")
    lines, report = [], {"calls": a.calls, "rounds": a.rounds}
    for shape in a.shapes:
        N, L = (int(v) for v in shape.split("x"))
        for D in a.dims:
            X, y = _blobs(N, L, D, dev, D)
            fold = torch.from_numpy(linear_probe.stratified_folds(y.cpu().numpy(), 5)).to(dev)
            xs = linear_probe.StandardScaler().fit(X).transform(X)
            del X
            R = 3 * L
            target = torch.arange(L, dtype=torch.int32, device=dev).repeat(3)
            alpha = torch.tensor(ALPHAS, device=dev).repeat_interleave(L)
            keep = fold != 0
            n_eff = int(keep.sum())
            step = 1.0 / (0.25 * linear_probe._lipschitz_lambda(xs, keep.float(), n_eff) + max(ALPHAS))
            st = [torch.zeros(R, D, device=dev), torch.zeros(R, device=dev), torch.zeros(R, D, device=dev),
                  torch.zeros(R, device=dev), torch.ones(R, device=dev)]
            gmax, conv = torch.zeros(R, device=dev), torch.zeros(R, dtype=torch.uint8, device=dev)
            grads = (torch.empty(R, D, device=dev), torch.empty(R, device=dev),
                     torch.empty(R, dtype=torch.float64, device=dev))

            def ours():
                ops.lp_loss_grad(xs, y, st[2], st[3], target, alpha, fold=fold, skip_fold=0, out=grads,
                                 check_labels=False)
                ops.lp_step(st[0], st[1], st[2], st[3], grads[0], grads[1], st[4], step, 1e-4, gmax, conv)

            tw = [torch.zeros(R, D, device=dev), torch.zeros(R, device=dev), torch.zeros(R, D, device=dev),
                  torch.zeros(R, device=dev), torch.ones(R, device=dev)]
            xk = xs * keep[:, None]  # the masked rows as zero rows (their residuals are zeroed below)
            rows = torch.arange(N, device=dev)
            keepf = keep.float()[:, None]

            def theirs():
                W, b, Yw, Yb, t = tw
                r = torch.sigmoid(torch.addmm(Yb, xs, Yw.t()))
                r.view(N, 3, L)[rows, :, y] -= 1.0
                r *= keepf
                gW = torch.addmm(alpha[:, None] * Yw, r.t(), xk, alpha=1.0 / n_eff)
                gb = r.sum(0) / n_eff
                xw, xb = Yw - step * gW, Yb - step * gb
                restart = ((gW * (xw - W)).sum(1) + gb * (xb - b)) > 0
                t1 = torch.where(restart, torch.ones_like(t), 0.5 * (1 + torch.sqrt(1 + 4 * t * t)))
                beta = torch.where(restart, torch.zeros_like(t), (t - 1) / t1)
                tw[2], tw[3] = xw + beta[:, None] * (xw - W), xb + beta * (xb - b)
                tw[0], tw[1], tw[4] = xw, xb, t1

            for fn in (ours, theirs):
                for _ in range(2):
                    fn()
            torch.cuda.synchronize()
            agree = float((st[0] - tw[0]).abs().max() / tw[0].abs().max())
            times = {"hvk": [], "torch": []}
            for _ in range(a.rounds):
                times["hvk"].append(_window_us(ours, a.calls))
                times["torch"].append(_window_us(theirs, a.calls))
            med = {k: statistics.median(v) for k, v in times.items()}
            flops = 4.0 * n_eff * R * D
            nbytes = 4.0 * (N * D + 3 * R * D + N)
            key = f"iter {N}x{L}x{D}"
            report[key] = {"us": {k: {"median": round(med[k], 1), "min": round(min(v), 1), "max": round(max(v), 1)}
                                  for k, v in times.items()},
                           "torch_over_hvk": round(med["torch"] / med["hvk"], 2), "flops": flops, "bytes": nbytes,
                           "hvk_TFLOP_per_s": round(flops / med["hvk"] / 1e6, 2),
                           "hvk_f32_mfma_fraction": round(flops / (med["hvk"] * 1e-6) / F32_MFMA_PEAK, 3),
                           "torch_TFLOP_per_s": round(flops / med["torch"] / 1e6, 2),
                           "iterates_max_rel_difference_after_2": agree}
            word = "faster" if med["torch"] >= med["hvk"] else "SLOWER"
            lines.append(f"{key} (R {R}, {n_eff} rows in the fold): loss_grad + step {med['hvk']:.0f} us "
                         f"(min {min(times['hvk']):.0f}, max {max(times['hvk']):.0f}) = "
                         f"{flops / med['hvk'] / 1e6:.1f} TFLOP/s, {flops / (med['hvk'] * 1e-6) / F32_MFMA_PEAK:.1%} of "
                         f"the f32 MFMA peak; torch eager {med['torch']:.0f} us (min {min(times['torch']):.0f}, max "
                         f"{max(times['torch']):.0f}): hvk is {word}, torch / hvk = {med['torch'] / med['hvk']:.2f} x")
            print(lines[-1], flush=True)
            del xs, xk, st, tw, grads
            torch.cuda.empty_cache()
    for shape in a.grid:
        N, L, D = (int(v) for v in shape.split("x"))
        X, y = _blobs(N, L, D, dev, D)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pipe, best, cv = linear_probe.grid_search(X, y, n_classes=L)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        report[f"grid_search {shape}"] = {"seconds": round(dt, 2), "iterations_per_fold": pipe.cv_n_iter_,
                                          "refit_iterations": pipe.clf.n_iter_, "best_alpha": best,
                                          "cv_mean": [round(float(v), 4) for v in cv.mean(1)],
                                          "all_converged": bool(pipe.clf.converged_.all())}
        lines.append(f"grid_search {shape}: {dt:.1f} s, iterations per fold {pipe.cv_n_iter_} + refit "
                     f"{pipe.clf.n_iter_}, best alpha {best}, cv means {cv.mean(1).round(4).tolist()}")
        print(lines[-1], flush=True)
        del X, pipe
        torch.cuda.empty_cache()
    print(json.dumps(report))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n" + json.dumps(report) + "\n")


if __name__ == "__main__":
    main()
