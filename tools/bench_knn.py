"""The k-NN search and vote at the evaluation shape: B = 256 query rows against a bank of N
L2-normalised bf16 rows (iNat21's 2.7 M training images and a smaller bank), D = 768 (SwinV2-T)
and 1024 (SwinV2-B), k = 200:

    knn_topk      hvk_knn_topk: the bf16-MFMA sweep with its running top-k, and the merge
    knn_vote      hvk_knn_vote on its result, [N, 7] tier ids, k = 10, 20, 100, 200
    torch_topk    the eager route it replaces: (q @ chunk.T).topk(k) in bf16 over chunks of
                  `--chunk` bank rows, the running best merged by a second topk per chunk
    f32_tile      (--f32) hvk_ss_predict_flat over the same rows as f32 "centroids": the f32-MFMA
                  tile that is the only other matrix sweep with a running selection in libhvk (an
                  argmin, k = 1), to put a measured time where DESIGN.md §3 had an estimate

Timing: `--calls` eager calls between two device events, the window closed by a device
synchronise; the sides alternate for `--rounds` rounds; the median is reported with the min-max
spread.  Rates are against the algorithmic work: 2 B N D flop (of the 2.5 PFLOP/s dense bf16 MFMA
peak) and N D 2 bytes, the bank read once (of the 8 TB/s HBM peak; the row tiles that share a bank
split are expected to meet in the Infinity Cache); the bound is the larger of the two least times.
Before anything is timed the two searches are compared: rows whose index lists differ are counted
(torch rounds its scores to bf16, so it orders near-equal scores differently).

    python tools/bench_knn.py [--banks 2700000 200000] [--dims 768 1024] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
MFMA_PEAK = 2.5e15  # dense bf16, flop/s
HBM_PEAK = 8e12     # bytes/s


def _eager_us(fn, calls):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(calls):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / calls


def torch_topk(q, bank, k, chunk):
    best_s = best_i = None
    for lo in range(0, bank.shape[0], chunk):
        s, i = (q @ bank[lo:lo + chunk].T).topk(min(k, bank.shape[0] - lo), dim=1)
        i = i + lo
        if best_s is not None:
            s, i = torch.cat([best_s, s], 1), torch.cat([best_i, i], 1)
            s, pos = s.topk(k, dim=1)
            i = i.gather(1, pos)
        best_s, best_i = s, i
    return best_s, best_i


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--banks", type=int, nargs="+", default=[2_700_000, 200_000])
    ap.add_argument("--dims", type=int, nargs="+", default=[768, 1024])
    ap.add_argument("--k", type=int, default=200)
    ap.add_argument("--chunk", type=int, default=1 << 17)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--f32", action="store_true", help="also time the f32-MFMA argmin tile over the same rows")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_knn needs a GPU: nothing here is measurable on the CPU")
    from hvamd import _lib, ops
    dev = torch.device("cuda:0")
    B, k = a.batch, a.k
    ks = [v for v in (10, 20, 100, 200) if v <= k] or [k]
    lines, report = [], {"batch": B, "k": k, "calls": a.calls, "rounds": a.rounds, "chunk": a.chunk}
    for D in a.dims:
        for N in a.banks:
            g = torch.Generator(device=dev).manual_seed(D + N)
            # 1000 class directions under noise: neighbourhoods with structure, as real features have
            centres = torch.randn(1000, D, device=dev, generator=g)
            bank = torch.empty(N, D, device=dev, dtype=torch.bfloat16)
            labels = torch.empty(N, 7, device=dev, dtype=torch.int32)
            for lo in range(0, N, 1 << 18):
                n = min(1 << 18, N - lo)
                c = torch.randint(0, 1000, (n,), device=dev, generator=g)
                x = centres[c] + 1.5 * torch.randn(n, D, device=dev, generator=g)
                bank[lo:lo + n] = ops.ss_prepare(x, l2_normalized=True).bfloat16()
                labels[lo:lo + n] = torch.stack([c // 2 ** (6 - t) for t in range(7)], 1).int()
            cq = torch.randint(0, 1000, (B,), device=dev, generator=g)
            q = ops.ss_prepare(centres[cq] + 1.5 * torch.randn(B, D, device=dev, generator=g),
                               l2_normalized=True).bfloat16()
            sims, idx = ops.knn_topk(q, bank, k)
            sides = {"knn_topk": lambda: ops.knn_topk(q, bank, k),
                     "knn_vote": lambda: ops.knn_vote(sims, idx, labels, ks),
                     "torch_topk": lambda: torch_topk(q, bank, k, a.chunk)}
            if a.f32:
                bank32, q32 = bank.float(), q.float()
                cnorm = torch.ones(N, device=dev)
                sides["f32_tile"] = lambda: ops.ss_predict_flat(q32, bank32, cnorm)
            for fn in sides.values():  # warm every shape the timed windows use
                for _ in range(2):
                    fn()
            torch.cuda.synchronize()
            differ = int((idx.long().sort(1).values != torch_topk(q, bank, k, a.chunk)[1].sort(1).values).any(1).sum())
            times = {name: [] for name in sides}
            for _ in range(a.rounds):
                for name, fn in sides.items():  # alternating
                    times[name].append(_eager_us(fn, a.calls))
            med = {name: statistics.median(v) for name, v in times.items()}
            flop, nbytes = 2.0 * B * N * D, 2.0 * N * D
            least = max(flop / MFMA_PEAK, nbytes / HBM_PEAK) * 1e6
            bound = "MFMA" if flop / MFMA_PEAK >= nbytes / HBM_PEAK else "HBM"
            t = med["knn_topk"]
            splits = _lib.load().hvk_knn_workspace(B, N, k, 0) // (8 * B * k)
            report[f"{D}x{N}"] = {
                "us": {n_: {"median": round(med[n_], 1), "min": round(min(v), 1), "max": round(max(v), 1)}
                       for n_, v in times.items()},
                "torch_over_knn": round(med["torch_topk"] / t, 2), "rows_differing_from_torch": differ,
                "splits": int(splits), "TFLOP_per_s": round(flop / t / 1e6, 1),
                "frac_mfma_peak": round(flop / t / 1e-6 / MFMA_PEAK, 4), "TB_per_s": round(nbytes / t / 1e6, 3),
                "frac_hbm_peak": round(nbytes / t / 1e-6 / HBM_PEAK, 4), "bound": bound,
                "least_us": round(least, 1), "frac_of_bound": round(least / t, 4)}
            lines.append(f"D {D}, N {N}, B {B}, k {k} ({splits} bank splits); index sets differ from torch's in "
                         f"{differ} of {B} rows")
            for n_, v in times.items():
                lines.append(f"  {n_:11s} median {med[n_]:10.1f} us  (min {min(v):10.1f}, max {max(v):10.1f}, "
                             f"{a.rounds} rounds x {a.calls} calls)")
            word = "faster" if med["torch_topk"] >= t else "SLOWER"
            lines.append(f"  knn_topk is {word} than torch's chunked bf16 topk: torch / knn = {med['torch_topk'] / t:.2f} x")
            lines.append(f"  knn_topk: {flop / t / 1e6:.1f} TFLOP/s = {flop / t / 1e-6 / MFMA_PEAK:.3f} of the bf16 MFMA "
                         f"peak, {nbytes / t / 1e6:.3f} TB/s = {nbytes / t / 1e-6 / HBM_PEAK:.3f} of the HBM peak; "
                         f"{bound}-bound, least time {least:.1f} us = {least / t:.3f} of the measured")
            del bank, labels
    text = "\n".join(lines)
    print(text, flush=True)
    print(json.dumps(report))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n" + json.dumps(report) + "\n")


if __name__ == "__main__":
    main()
