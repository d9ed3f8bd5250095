// The per-row accumulator of the evaluation sweeps (metrics.hip, joint.hip): running maximum with
// its lowest index, online max-shifted sum of exponentials, entries ranked ahead of the target.
#pragma once
#include <math.h>

#include "eval_common.h"

namespace hvk_eval {

struct RowAcc {
  float m;   // running maximum (never NaN: a NaN compares false and is skipped here)
  int mi;    // lowest index holding m; kNoIdx while nothing compared equal or above
  float s;   // sum of exp(z - m) over the entries seen
  int cnt;   // entries ranked ahead of the target
};

// exp(a - b) as a factor of a sum shifted to b >= a: an entry (or a partial maximum) of -inf
// contributes nothing, also where b is -inf too (-inf - -inf would be NaN)
__device__ __forceinline__ float shifted_exp(float a, float b) { return a == -INFINITY ? 0.f : expf(a - b); }

// N consecutive entries x[e] = z[j0 + e]; a thread's groups arrive in ascending j
template <int N>
__device__ __forceinline__ RowAcc push_group(RowAcc a, const float (&x)[N], int j0, float zt, int t) {
  float cm = x[0];
#pragma unroll
  for (int e = 1; e < N; ++e) cm = fmaxf(cm, x[e]);  // fmaxf drops NaNs
  if (cm > a.m) {  // a new maximum: one rescale per group, its index found below
    a.s *= shifted_exp(a.m, cm);
    a.m = cm;
    a.mi = kNoIdx;
  }
#pragma unroll
  for (int e = 0; e < N; ++e) {
    const int j = j0 + e;
    a.s += shifted_exp(x[e], a.m);
    // float compares: -0.0 and +0.0 tie; the first entry equal to the maximum keeps the index
    if (x[e] == a.m && j < a.mi) a.mi = j;
    a.cnt += (x[e] > zt || (x[e] == zt && j < t)) ? 1 : 0;
  }
  return a;
}

// (`c ? a.mi : b.mi` on two struct members is an lvalue, a select between two ADDRESSES, which
// sends the structs to scratch memory: the fields are copied to scalars first, here and below)
__device__ __forceinline__ RowAcc merge(RowAcc a, RowAcc b) {
  const float am = a.m, bm = b.m, as = a.s, bs = b.s;
  const int ai = a.mi, bi = b.mi;
  const float m = fmaxf(am, bm);
  const bool take_a = am > bm || (am == bm && ai < bi);
  return RowAcc{m, take_a ? ai : bi, as * shifted_exp(am, m) + bs * shifted_exp(bm, m), a.cnt + b.cnt};
}

// wave butterfly: every lane ends with the same bits
__device__ __forceinline__ RowAcc wave_merge(RowAcc acc, int tid) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    RowAcc w{__shfl_xor(acc.m, o), __shfl_xor(acc.mi, o), __shfl_xor(acc.s, o), __shfl_xor(acc.cnt, o)};
    // both lanes of a pair must reach the same bits: merge in lane order (selects on scalar
    // copies, see merge)
    const bool up = (tid & o) != 0;
    const float am = acc.m, as = acc.s, wm = w.m, ws = w.s;
    const int ai = acc.mi, ac = acc.cnt, wi = w.mi, wc = w.cnt;
    const RowAcc lo{up ? wm : am, up ? wi : ai, up ? ws : as, up ? wc : ac};
    const RowAcc hi{up ? am : wm, up ? ai : wi, up ? as : ws, up ? ac : wc};
    acc = merge(lo, hi);
  }
  return acc;
}

}  // namespace hvk_eval

// hvk_eval_metrics' accumulate step (metrics.hip): folds the per-row results of a batch into a
// double[16] state, slots [0, 13), in an order that depends on B only
__attribute__((visibility("hidden"))) void hvk_eval_accumulate_launch(int B, int kmax, const int* rank,
                                                                      const float* nll, const int* dist,
                                                                      const unsigned char* tier_hit,
                                                                      double* state, hipStream_t st);
