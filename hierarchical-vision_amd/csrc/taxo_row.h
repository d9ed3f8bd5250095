// Row helpers shared by the taxonomy losses (losses.hip, soft_labels.hip): the online
// log-sum-exp pair with its wave merge, and the leaf range of a target's ancestor.
#pragma once
#include "hvk_common.h"

namespace {

constexpr int kTiers = 7;
constexpr int kLevels = 8;  // 7 tiers + root

struct Lse {
  float m, s;
};
__device__ __forceinline__ Lse lse_push(Lse a, float x) {
  if (x > a.m) {
    a.s = a.s * __expf(a.m - x) + 1.f;
    a.m = x;
  } else {
    a.s += __expf(x - a.m);
  }
  return a;
}
__device__ __forceinline__ Lse lse_merge(Lse a, Lse b) {
  if (b.m == -INFINITY) return a;
  if (a.m == -INFINITY) return b;
  const float m = fmaxf(a.m, b.m);
  return Lse{m, a.s * __expf(a.m - m) + b.s * __expf(b.m - m)};
}
__device__ __forceinline__ Lse wave_lse(Lse v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    Lse w{__shfl_xor(v.m, o), __shfl_xor(v.s, o)};
    v = lse_merge(v, w);
  }
  return v;
}

// segment [lo, hi) in permuted positions of the target's node at level l (l = 7: all); Args has
// L, tgt [B, 7], tbase, nstart, nend (include/hvk.h, HXE)
template <class Args>
__device__ __forceinline__ void level_range(const Args& a, int b, int l, int& lo, int& hi) {
  if (l == kLevels - 1) { lo = 0; hi = a.L; return; }
  const int tier = kTiers - 1 - l;
  const int64_t node = a.tgt[(size_t)b * kTiers + tier];
  const int n_nodes = tier + 1 < kTiers ? a.tbase[tier + 1] - a.tbase[tier] : a.L;
  if (node < 0 || node >= n_nodes) {  // out-of-range target: an empty segment (NaN loss), no OOB read
    lo = 0;
    hi = -1;
    return;
  }
  lo = a.nstart[a.tbase[tier] + (int)node];
  hi = a.nend[a.tbase[tier] + (int)node];
}

}  // namespace
