// Evaluation metrics on gfx950 (hierarchy.py:97-180, models.py:61-101): acc@1, acc@k,
// cross-entropy and tree distance of a batch of leaf logits from ONE read of every logit row.
//
// * eval_rows_kernel -- one workgroup (4 waves) per sample.  A single sweep over the row keeps,
//   per thread, the running maximum with its lowest index, an online max-shifted sum of
//   exponentials, and the number of entries ranked ahead of the target (z_j > z_t, or z_j == z_t
//   with j < t: the target's position in a stable descending sort).  Waves reduce by shuffles,
//   the four waves through one LDS exchange; thread 0 then reads the one tree-distance entry (or
//   compares the two 7-tier paths) and writes the row's results.
// * eval_accumulate_kernel -- one workgroup folds the per-row results into a persistent
//   double[16] state.  Thread i sums rows i, i + 256, ... in order, waves reduce by a fixed
//   butterfly, thread 0 adds the four wave totals in order: the summation order depends on B only
//   and there is no atomic anywhere, so equal inputs leave bit-identical state.
#include <math.h>

#include "hvk_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTiers = 7;
constexpr int kState = 16;
constexpr int kSums = 13;  // state entries [0, 13) are written; the rest reserved
static_assert(kSums == 6 + kTiers && kSums <= kState, "state layout of include/hvk.h");

struct RowAcc {
  float m;   // running maximum (never NaN: a NaN compares false and is skipped here)
  int mi;    // lowest index holding m; INT_MAX while nothing compared equal or above
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
    a.mi = 0x7fffffff;
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

// One thread's share of `groups` groups of N entries, group g holding z[first + g N ...]: groups
// tid, tid + 256, ... in ascending order, UN of them per round with every load of the round issued
// before the first value is used (a dependent load per group would leave the sweep waiting one
// memory latency per 16 B).  A round's groups past the end reload the last group and are skipped.
template <int N, int UN, typename Load>
__device__ __forceinline__ RowAcc sweep(RowAcc acc, int first, int groups, int tid, float zt, int t, Load load) {
  for (int g0 = tid; g0 < groups; g0 += kThreads * UN) {
    float x[UN][N];
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int g = g0 + u * kThreads;
      load((int)HVK_BCHECK(g < groups ? g : groups - 1, groups), x[u]);
    }
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int g = g0 + u * kThreads;
      if (g < groups) acc = push_group<N>(acc, x[u], first + g * N, zt, t);
    }
  }
  return acc;
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

struct RowArgs {
  const void* logits;
  int bf16, B, L, ld;
  const int64_t* targets;
  int t_stride, t_off;
  const void* tree_dists;
  int dist_f32;
  const int* leaf_paths;
  const int64_t* target_paths;
  int* pred;
  int* rank;
  float* nll;
  int* dist;
  unsigned char* tier_hit;
};

__device__ __forceinline__ float load1(const void* row, int bf16, int j) {
  if (bf16) return __uint_as_float((uint32_t) static_cast<const hvk_bf16*>(row)[j] << 16);
  return static_cast<const float*>(row)[j];
}

// The whole row of one sample, the element type fixed at compile time so that the loads of a
// round are straight-line code.
template <bool BF16>
__device__ __forceinline__ RowAcc sweep_row(const char* row, int L, int tid, float zt, int t) {
  RowAcc acc{-INFINITY, 0x7fffffff, 0.f, 0};
  constexpr int N = BF16 ? 8 : 4;  // entries per 16 B
  const auto one = [row](int j, float (&x)[1]) { x[0] = load1(row, BF16, j); };
  if (((uintptr_t)row & 15) == 0) {
    // 16-B loads over the row's whole vectors, element loads over the tail
    const int nv = L / N, done = nv * N;
    acc = sweep<N, 4>(acc, 0, nv, tid, zt, t, [row](int v, float (&x)[N]) {
      const uint4 w = hvk_ld16(row + (size_t)v * 16);
      if constexpr (BF16) {
        hvk_unpack8(w, x);
      } else {
        x[0] = __uint_as_float(w.x), x[1] = __uint_as_float(w.y), x[2] = __uint_as_float(w.z),
        x[3] = __uint_as_float(w.w);
      }
    });
    return sweep<1, 1>(acc, done, L - done, tid, zt, t, [&](int j, float (&x)[1]) { one(done + j, x); });
  }
  {
    // a row that does not start on a 16-B boundary (a column slice, an odd leading dimension)
    return sweep<1, 8>(acc, 0, L, tid, zt, t, one);
  }
}

__global__ __launch_bounds__(kThreads) void eval_rows_kernel(RowArgs a) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const int L = a.L;
  const size_t esz = a.bf16 ? 2 : 4;
  const char* row = static_cast<const char*>(a.logits) + (size_t)b * a.ld * esz;
  const int64_t t64 = a.targets[(size_t)b * a.t_stride + a.t_off];
  const bool valid = t64 >= 0 && t64 < L;
  const int t = valid ? (int)t64 : -1;
  // the target's logit: the one element read besides the sweep (NaN for an invalid target, so no
  // comparison below counts anything)
  const float zt = valid ? load1(row, a.bf16, HVK_BCHECK(t, L)) : __builtin_nanf("");

  RowAcc acc = a.bf16 ? sweep_row<true>(row, L, tid, zt, t) : sweep_row<false>(row, L, tid, zt, t);

  // wave butterfly, then one LDS exchange across the four waves
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
  __shared__ RowAcc part[kWaves];
  if ((tid & 63) == 0) part[tid >> 6] = acc;
  __syncthreads();
  if (tid != 0) return;
  acc = part[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) acc = merge(acc, part[w]);

  // every entry NaN: nothing compared, the index is still the sentinel
  const int pred = (acc.mi >= 0 && acc.mi < L) ? acc.mi : 0;
  a.pred[b] = pred;
  a.rank[b] = valid ? acc.cnt : -1;
  // LSE(z) - z_t = log(sum exp(z - m)) + (m - z_t)
  a.nll[b] = valid ? logf(acc.s) + (acc.m - zt) : __builtin_nanf("");
  int dist = -1;
  unsigned hit = 0;
  if (valid) {
    if (a.tree_dists) {
      const size_t i = (size_t)HVK_BCHECK(pred, L) * L + t;
      dist = a.dist_f32 ? (int)static_cast<const float*>(a.tree_dists)[i]
                        : (int)static_cast<const unsigned char*>(a.tree_dists)[i];
    } else if (a.leaf_paths) {
      dist = kTiers;
#pragma unroll
      for (int q = 0; q < kTiers; ++q) {  // coarse to fine: the finest matching tier sets dist last
        const bool same = (int64_t)a.leaf_paths[(size_t)HVK_BCHECK(pred, L) * kTiers + q] ==
                          a.target_paths[(size_t)b * kTiers + q];
        if (same) {
          hit |= 1u << q;
          dist = kTiers - 1 - q;
        }
      }
    }
  }
  a.dist[b] = dist;
  if (a.tier_hit) a.tier_hit[b] = (unsigned char)hit;
}

__global__ __launch_bounds__(kThreads) void eval_accumulate_kernel(int B, int kmax, const int* __restrict__ rank,
                                                                  const float* __restrict__ nll,
                                                                  const int* __restrict__ dist,
                                                                  const unsigned char* __restrict__ tier_hit,
                                                                  double* state) {
  const int tid = threadIdx.x;
  double v[kSums];
#pragma unroll
  for (int i = 0; i < kSums; ++i) v[i] = 0.0;
  for (int b = tid; b < B; b += kThreads) {
    const int r = rank[HVK_BCHECK(b, B)];
    if (r < 0) {
      v[5] += 1.0;
      continue;
    }
    v[0] += 1.0;
    v[1] += r < 1 ? 1.0 : 0.0;
    v[2] += r < kmax ? 1.0 : 0.0;
    v[3] += (double)nll[b];
    const int d = dist[b];
    v[4] += d >= 0 ? (double)d : 0.0;
    const unsigned h = tier_hit ? tier_hit[b] : 0u;
#pragma unroll
    for (int q = 0; q < kTiers; ++q) v[6 + q] += (double)((h >> q) & 1u);
  }
  __shared__ double part[kWaves][kSums];
#pragma unroll
  for (int i = 0; i < kSums; ++i) {
    double x = v[i];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const double y = __shfl_xor(x, o);
      x = (tid & o) ? y + x : x + y;  // the same operand order in both lanes of a pair
    }
    if ((tid & 63) == 0) part[tid >> 6][i] = x;
  }
  __syncthreads();
  if (tid < kSums) {
    double x = part[0][tid];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) x += part[w][tid];
    state[tid] += x;
  }
}

}  // namespace

extern "C" {

int hvk_eval_metrics(const void* logits, int logits_dtype, int B, int L, int ld, const int64_t* targets,
                     int t_stride, int t_off, const void* tree_dists, int dist_dtype, const int* leaf_paths,
                     const int64_t* target_paths, int topk, int* pred, int* rank, float* nll, int* dist,
                     unsigned char* tier_hit, double* state, void* stream) {
  // L + 4096 must stay an int: the sweep's loop counters step past L by up to 8 workgroup widths
  if (B < 0 || L < 1 || ld < L || L > 0x7ffff000)
    return hvk_set_error(HVK_EINVAL,
                         "hvk_eval_metrics: bad shape (B %d, L %d, ld %d: B >= 0, 1 <= L <= 2^31 - 4096, ld >= L)", B,
                         L, ld);
  if (topk < 1) return hvk_set_error(HVK_EINVAL, "hvk_eval_metrics: topk %d < 1", topk);
  if (t_stride < 1 || t_off < 0 || t_off >= t_stride)
    return hvk_set_error(HVK_EINVAL, "hvk_eval_metrics: target stride %d / offset %d", t_stride, t_off);
  if (logits_dtype != 0 && logits_dtype != 1)
    return hvk_set_error(HVK_EINVAL, "hvk_eval_metrics: unknown logits dtype %d (0 f32, 1 bf16)", logits_dtype);
  if (tree_dists && dist_dtype != 0 && dist_dtype != 1)
    return hvk_set_error(HVK_EINVAL, "hvk_eval_metrics: unknown tree_dists dtype %d (0 u8, 1 f32)", dist_dtype);
  if (!logits || !targets || !pred || !rank || !nll || !dist || !state)
    return hvk_set_error(HVK_EINVAL, "hvk_eval_metrics: null pointer");
  if (tree_dists && leaf_paths)
    return hvk_set_error(HVK_EINVAL, "hvk_eval_metrics: tree_dists and leaf_paths are alternatives, both given");
  if (leaf_paths && !target_paths)
    return hvk_set_error(HVK_EINVAL, "hvk_eval_metrics: leaf_paths given without target_paths");
  if (tier_hit && !leaf_paths)
    return hvk_set_error(HVK_EINVAL, "hvk_eval_metrics: tier_hit needs leaf_paths");
  if (B == 0) return HVK_OK;
  RowArgs a{logits, logits_dtype, B, L, ld, targets, t_stride, t_off, tree_dists, dist_dtype,
            leaf_paths, target_paths, pred, rank, nll, dist, tier_hit};
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(eval_rows_kernel, dim3(B), dim3(kThreads), 0, st, a);
  HVK_CHECK_LAUNCH("eval_rows");
  hipLaunchKernelGGL(eval_accumulate_kernel, dim3(1), dim3(kThreads), 0, st, B, topk < L ? topk : L,
                     static_cast<const int*>(rank), static_cast<const float*>(nll), static_cast<const int*>(dist),
                     static_cast<const unsigned char*>(tier_hit), state);
  HVK_CHECK_LAUNCH("eval_accumulate");
  return HVK_OK;
}

}  // extern "C"
