// Joint path decoding of the seven multitask heads on gfx950 (hierarchy.py: EvalMetrics
// decoding="joint"): the product of experts along every leaf's root-to-leaf path,
//   s_k = sum_t w_t log softmax(z_t)[anc_t(k)]  (+ the constant w_6 LSE_6, dropped),
// with its argmax, the target's rank, the joint NLL, tree distance and the heads' own argmaxes from
// ONE read of the row's logits (all tiers side by side in one buffer, as the head GEMM leaves them).
//
// * joint_rows_kernel -- one workgroup (4 waves) per sample, three phases:
//   1. the logits of tiers 0-5 go to LDS as f32 while they are loaded (16-B loads over the aligned
//      body of the span, element loads at its ragged ends); per tier, from LDS, an online
//      (max, lowest index, max-shifted sum) per thread, a wave butterfly and one LDS exchange give
//      LSE_t and the head's own argmax -- all six tiers behind ONE barrier;
//   2. top-down prefix in place: c_t[n] = w_t (z_t[n] - LSE_t) + c_{t-1}[parent_t[n]], one barrier
//      per tier; afterwards the score of a leaf's whole coarse path is one LDS read away;
//   3. one sweep over the leaf tier: s_k = fma(w_6, z_6[k], c_5[parent_6[k]]), kept in registers
//      for the running max / online sum / rank count of metrics.hip's sweep (eval_row.h), the
//      species head's own argmax beside it, and optionally stored as scores[b, k] (16-B stores).
//   Thread 0 finishes the row: tree distance and tier hits of the joint prediction, head_pred and
//   the path-consistency bit.
// * the batch is folded into the state by metrics.hip's accumulate kernel (slots 0-12) and
//   joint_consistency_kernel (slot 15, an integer count): fixed order, no atomics.
#include <math.h>
#include <stdio.h>

#include "eval_row.h"
#include "../../include/hvk.h"

using namespace hvk_eval;

namespace {

constexpr int kTiers = 7;
constexpr int kCoarse = kTiers - 1;
// f32 coarse logits a workgroup keeps in LDS: 60 KB of the 64 KB one workgroup may take, the rest
// for the alignment pad and the reduction exchange
constexpr int kMaxCoarse = 15360;
constexpr int kMaxLeaves = 1 << 24;

// 16-B vectors at 4-B alignment: a global dwordx4 access needs dword alignment only
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef int i32x4_t __attribute__((ext_vector_type(4)));
typedef f32x4_t f32x4u __attribute__((aligned(4)));
typedef i32x4_t i32x4u __attribute__((aligned(4)));

struct JointArgs {
  const void* logits;
  int bf16, B, ld;
  int off[kTiers + 1];  // tier t = columns [off[t], off[t + 1])
  float w[kTiers];
  const int64_t* targets;
  int t_stride, t_off;
  const int* parents;     // [off[7] - off[1]]: parent (tier t - 1 id) of node n of tier t at off[t] - off[1] + n
  const int* leaf_paths;  // [L, 7]
  int* pred;
  int* rank;
  float* nll;
  float* lse;
  int* dist;
  unsigned char* tier_hit;
  int* head_pred;  // [B, 7]
  unsigned char* consistent;
  float* scores;  // [B, L] or null
};

template <bool BF16>
__device__ __forceinline__ void unpack(const uint4& w, float (&x)[BF16 ? 8 : 4]) {
  if constexpr (BF16) {
    hvk_unpack8(w, x);
  } else {
    x[0] = __uint_as_float(w.x), x[1] = __uint_as_float(w.y), x[2] = __uint_as_float(w.z), x[3] = __uint_as_float(w.w);
  }
}

// A span of n elements from `p`: `head` elements up to the first 16-B boundary, nv whole vectors,
// the rest as a tail (a pointer that is not even element-aligned: everything by element loads)
template <bool BF16>
__device__ __forceinline__ void split_span(const char* p, int n, int& head, int& nv) {
  constexpr int esz = BF16 ? 2 : 4, N = 16 / esz;
  const uintptr_t a = (uintptr_t)p;
  head = (a & (esz - 1)) ? n : (int)(((16 - (a & 15)) & 15) / esz);
  head = head < n ? head : n;
  nv = (n - head) / N;
}

// a parent id as an index into the tier above: a table entry outside it is clamped, never followed
__device__ __forceinline__ int parent_in(int p, int n_above) { return p < 0 ? 0 : (p < n_above ? p : n_above - 1); }

template <bool BF16, bool SCORES>
__global__ __launch_bounds__(kThreads) void joint_rows_kernel(JointArgs a) {
  constexpr int esz = BF16 ? 2 : 4, N = 16 / esz;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  __shared__ RowAcc tier_part[kCoarse][kWaves];
  __shared__ RowAcc leaf_part[2][kWaves];
  const int b = blockIdx.x, tid = threadIdx.x;
  const char* row = static_cast<const char*>(a.logits) + (size_t)b * a.ld * esz;
  const int nc = a.off[kCoarse], L = a.off[kTiers] - nc;
  const float nanf_ = __builtin_nanf("");

  // ---- phase 1: tiers 0-5 -> LDS (f32), one HBM read per logit --------------------------------
  int head, nv;
  split_span<BF16>(row, nc, head, nv);
  float* c = lds + ((4 - (head & 3)) & 3);  // c[head + v N] is 16-B aligned in LDS
  {
    const int done = head + nv * N;
    for (int j = tid; j < head; j += kThreads) c[j] = load1(row, BF16, HVK_BCHECK(j, nc));
    for (int j = done + tid; j < nc; j += kThreads) c[j] = load1(row, BF16, HVK_BCHECK(j, nc));
    const char* body = row + (size_t)head * esz;
    constexpr int UN = 4;  // every load of a round issued before the first value is used
    for (int v0 = tid; v0 < nv; v0 += kThreads * UN) {
      uint4 w[UN];
#pragma unroll
      for (int u = 0; u < UN; ++u) {
        const int v = v0 + u * kThreads;
        w[u] = hvk_ld16(body + (size_t)HVK_BCHECK(v < nv ? v : nv - 1, nv) * 16);
      }
#pragma unroll
      for (int u = 0; u < UN; ++u) {
        const int v = v0 + u * kThreads;
        if (v >= nv) continue;
        float x[N];
        unpack<BF16>(w[u], x);
        float4* dst = reinterpret_cast<float4*>(c + head + v * N);
#pragma unroll
        for (int q = 0; q < N / 4; ++q) dst[q] = make_float4(x[4 * q], x[4 * q + 1], x[4 * q + 2], x[4 * q + 3]);
      }
    }
  }
  __syncthreads();

  // per tier: (max, lowest index, sum exp(z - max)) from LDS; all six tiers behind one barrier
#pragma unroll
  for (int t = 0; t < kCoarse; ++t) {
    const float* z = c + a.off[t];
    const int n = a.off[t + 1] - a.off[t];
    RowAcc acc{-INFINITY, kNoIdx, 0.f, 0};
    for (int j = tid; j < n; j += kThreads) {
      const float x[1] = {z[j]};
      acc = push_group<1>(acc, x, j, nanf_, -1);
    }
    acc = wave_merge(acc, tid);
    if ((tid & 63) == 0) tier_part[t][tid >> 6] = acc;
  }
  __syncthreads();
  float lse_t[kCoarse];
  int hp[kTiers];
#pragma unroll
  for (int t = 0; t < kCoarse; ++t) {  // every thread folds the four waves in the same order
    RowAcc acc = tier_part[t][0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) acc = merge(acc, tier_part[t][w]);
    lse_t[t] = acc.m + logf(acc.s);
    hp[t] = (acc.mi >= 0 && acc.mi < a.off[t + 1] - a.off[t]) ? acc.mi : 0;  // all NaN: nothing compared
  }

  // ---- phase 2: top-down prefix in place, c_t[n] = w_t (z_t[n] - LSE_t) + c_{t-1}[parent] -------
#pragma unroll
  for (int t = 0; t < kCoarse; ++t) {
    float* z = c + a.off[t];
    const int n = a.off[t + 1] - a.off[t];
    for (int j = tid; j < n; j += kThreads) {
      float base = 0.f;
      if (t > 0) {
        const int p = a.parents[HVK_BCHECK(a.off[t] - a.off[1] + j, a.off[kTiers] - a.off[1])];
        base = c[a.off[t - 1] + parent_in(p, a.off[t] - a.off[t - 1])];
      }
      z[j] = __builtin_fmaf(a.w[t], z[j] - lse_t[t], base);
    }
    __syncthreads();
  }

  // ---- phase 3: one sweep over the leaves --------------------------------------------------------
  const char* lrow = row + (size_t)nc * esz;
  const int* par = a.parents + (nc - a.off[1]);
  const float* c5 = c + a.off[kCoarse - 1];
  const int n5 = nc - a.off[kCoarse - 1];
  const float w6 = a.w[kCoarse];
  const int64_t t64 = a.targets[(size_t)b * a.t_stride + a.t_off];
  const bool valid = t64 >= 0 && t64 < L;
  const int t = valid ? (int)t64 : -1;
  // the target's score by the sweep's own expression: bitwise the s_k met at k == t
  const float st = valid ? __builtin_fmaf(w6, load1(lrow, BF16, HVK_BCHECK(t, L)), c5[parent_in(par[HVK_BCHECK(t, L)], n5)])
                         : nanf_;
  float* srow = SCORES ? a.scores + (size_t)b * L : nullptr;

  RowAcc acc{-INFINITY, kNoIdx, 0.f, 0};  // the joint scores
  RowAcc sp{-INFINITY, kNoIdx, 0.f, 0};   // the species head's own maximum (s, cnt unused)
  split_span<BF16>(lrow, L, head, nv);
  const auto one = [&](int k) {
    const float z = load1(lrow, BF16, HVK_BCHECK(k, L));
    const float s[1] = {__builtin_fmaf(w6, z, c5[parent_in(par[k], n5)])};
    if constexpr (SCORES) srow[k] = s[0];
    acc = push_group<1>(acc, s, k, st, t);
    if (z > sp.m) sp.m = z, sp.mi = k;
    else if (z == sp.m && k < sp.mi) sp.mi = k;
  };
  for (int k = tid; k < head; k += kThreads) one(k);
  for (int k = head + nv * N + tid; k < L; k += kThreads) one(k);
  {
    const char* body = lrow + (size_t)head * esz;
    constexpr int UN = 2;
    for (int v0 = tid; v0 < nv; v0 += kThreads * UN) {
      uint4 w[UN];
      i32x4u pv[UN][N / 4];
#pragma unroll
      for (int u = 0; u < UN; ++u) {
        const int v = (int)HVK_BCHECK(v0 + u * kThreads < nv ? v0 + u * kThreads : nv - 1, nv);
        w[u] = hvk_ld16(body + (size_t)v * 16);
#pragma unroll
        for (int q = 0; q < N / 4; ++q) pv[u][q] = *reinterpret_cast<const i32x4u*>(par + head + v * N + 4 * q);
      }
#pragma unroll
      for (int u = 0; u < UN; ++u) {
        const int v = v0 + u * kThreads;
        if (v >= nv) continue;
        const int k0 = head + v * N;
        float z[N], s[N];
        unpack<BF16>(w[u], z);
#pragma unroll
        for (int e = 0; e < N; ++e) s[e] = __builtin_fmaf(w6, z[e], c5[parent_in(pv[u][e / 4][e % 4], n5)]);
        if constexpr (SCORES) {
#pragma unroll
          for (int q = 0; q < N / 4; ++q)
            *reinterpret_cast<f32x4u*>(srow + k0 + 4 * q) = f32x4_t{s[4 * q], s[4 * q + 1], s[4 * q + 2], s[4 * q + 3]};
        }
        acc = push_group<N>(acc, s, k0, st, t);
        float cm = z[0];
#pragma unroll
        for (int e = 1; e < N; ++e) cm = fmaxf(cm, z[e]);
        if (cm > sp.m) sp.m = cm, sp.mi = kNoIdx;
#pragma unroll
        for (int e = 0; e < N; ++e)
          if (z[e] == sp.m && k0 + e < sp.mi) sp.mi = k0 + e;
      }
    }
  }
  acc = wave_merge(acc, tid);
  sp = wave_merge(sp, tid);
  if ((tid & 63) == 0) leaf_part[0][tid >> 6] = acc, leaf_part[1][tid >> 6] = sp;
  __syncthreads();
  if (tid != 0) return;
  acc = leaf_part[0][0], sp = leaf_part[1][0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) acc = merge(acc, leaf_part[0][w]), sp = merge(sp, leaf_part[1][w]);

  // ---- the row's results --------------------------------------------------------------------------
  const int pred = (acc.mi >= 0 && acc.mi < L) ? acc.mi : 0;
  hp[kCoarse] = (sp.mi >= 0 && sp.mi < L) ? sp.mi : 0;
  const float lse = acc.m + logf(acc.s);
  a.pred[b] = pred;
  a.rank[b] = valid ? acc.cnt : -1;
  a.lse[b] = lse;
  a.nll[b] = valid ? lse - st : nanf_;
  int dist = -1;
  unsigned hit = 0;
  if (valid) {
    dist = kTiers;
#pragma unroll
    for (int q = 0; q < kTiers; ++q) {  // coarse to fine: the finest matching tier sets dist last
      if (a.leaf_paths[(size_t)HVK_BCHECK(pred, L) * kTiers + q] == a.leaf_paths[(size_t)HVK_BCHECK(t, L) * kTiers + q]) {
        hit |= 1u << q;
        dist = kTiers - 1 - q;
      }
    }
  }
  a.dist[b] = dist;
  a.tier_hit[b] = (unsigned char)hit;
  bool cons = true;
#pragma unroll
  for (int q = 0; q < kTiers; ++q) {
    a.head_pred[(size_t)b * kTiers + q] = hp[q];
    if (q > 0) cons = cons && a.parents[HVK_BCHECK(a.off[q] - a.off[1] + hp[q], a.off[kTiers] - a.off[1])] == hp[q - 1];
  }
  a.consistent[b] = cons ? 1 : 0;
}

// state[15] += valid rows whose heads are path-consistent: an integer count, exact in any order
__global__ __launch_bounds__(kThreads) void joint_consistency_kernel(int B, const int* __restrict__ rank,
                                                                    const unsigned char* __restrict__ consistent,
                                                                    double* state) {
  const int tid = threadIdx.x;
  int n = 0;
  for (int b = tid; b < B; b += kThreads) n += (rank[HVK_BCHECK(b, B)] >= 0 && consistent[b]) ? 1 : 0;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) n += __shfl_xor(n, o);
  __shared__ int part[kWaves];
  if ((tid & 63) == 0) part[tid >> 6] = n;
  __syncthreads();
  if (tid == 0) state[15] += (double)(part[0] + part[1] + part[2] + part[3]);
}

// null: supported; else what is wrong with the tier offsets
const char* check_offsets(const int* off, char* buf, size_t cap) {
  if (!off) return "null tier_off";
  if (off[0] != 0) return "tier_off[0] must be 0";
  for (int t = 0; t < kTiers; ++t)
    if (off[t + 1] <= off[t]) return "tier_off must grow strictly (every tier holds a node)";
  if (off[kCoarse] > kMaxCoarse) {
    snprintf(buf, cap, "tiers 0-5 hold %d nodes, above the %d f32 values (60 KB) one workgroup keeps in LDS",
             off[kCoarse], kMaxCoarse);
    return buf;
  }
  if (off[kTiers] - off[kCoarse] > kMaxLeaves) return "more than 2^24 leaves";
  return nullptr;
}

}  // namespace

extern "C" {

int hvk_joint_supported(const int* tier_off) {
  char buf[160];
  return check_offsets(tier_off, buf, sizeof(buf)) == nullptr;
}

int hvk_joint_decode(const void* logits, int logits_dtype, int B, int ld, const int* tier_off,
                     const int64_t* targets, int t_stride, int t_off, const int* parents, const int* leaf_paths,
                     const float* weights, int topk, int* pred, int* rank, float* nll, float* lse, int* dist,
                     unsigned char* tier_hit, int* head_pred, unsigned char* consistent, float* scores,
                     double* state, void* stream) {
  char buf[160];
  if (const char* why = check_offsets(tier_off, buf, sizeof(buf)))
    return hvk_set_error(tier_off && tier_off[0] == 0 && tier_off[kCoarse] > kMaxCoarse ? HVK_EUNSUPPORTED : HVK_EINVAL,
                         "hvk_joint_decode: %s", why);
  if (B < 0 || ld < tier_off[kTiers])
    return hvk_set_error(HVK_EINVAL, "hvk_joint_decode: bad shape (B %d, ld %d < %d columns)", B, ld, tier_off[kTiers]);
  if (topk < 1) return hvk_set_error(HVK_EINVAL, "hvk_joint_decode: topk %d < 1", topk);
  if (t_stride < 1 || t_off < 0 || t_off >= t_stride)
    return hvk_set_error(HVK_EINVAL, "hvk_joint_decode: target stride %d / offset %d", t_stride, t_off);
  if (logits_dtype != 0 && logits_dtype != 1)
    return hvk_set_error(HVK_EINVAL, "hvk_joint_decode: unknown logits dtype %d (0 f32, 1 bf16)", logits_dtype);
  if (!logits || !targets || !parents || !leaf_paths || !weights || !pred || !rank || !nll || !lse || !dist ||
      !tier_hit || !head_pred || !consistent || !state)
    return hvk_set_error(HVK_EINVAL, "hvk_joint_decode: null pointer");
  for (int t = 0; t < kTiers; ++t)
    if (!(weights[t] >= 0.f) || isinf(weights[t]))
      return hvk_set_error(HVK_EINVAL, "hvk_joint_decode: weight %d = %g (finite, >= 0)", t, (double)weights[t]);
  if (B == 0) return HVK_OK;
  JointArgs a{};
  a.logits = logits, a.bf16 = logits_dtype, a.B = B, a.ld = ld;
  for (int t = 0; t <= kTiers; ++t) a.off[t] = tier_off[t];
  for (int t = 0; t < kTiers; ++t) a.w[t] = weights[t];
  a.targets = targets, a.t_stride = t_stride, a.t_off = t_off, a.parents = parents, a.leaf_paths = leaf_paths;
  a.pred = pred, a.rank = rank, a.nll = nll, a.lse = lse, a.dist = dist, a.tier_hit = tier_hit;
  a.head_pred = head_pred, a.consistent = consistent, a.scores = scores;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t lds = (size_t)(tier_off[kCoarse] + 4) * sizeof(float);
  const int L = tier_off[kTiers] - tier_off[kCoarse];
  if (logits_dtype) {
    if (scores) hipLaunchKernelGGL((joint_rows_kernel<true, true>), dim3(B), dim3(kThreads), lds, st, a);
    else hipLaunchKernelGGL((joint_rows_kernel<true, false>), dim3(B), dim3(kThreads), lds, st, a);
  } else {
    if (scores) hipLaunchKernelGGL((joint_rows_kernel<false, true>), dim3(B), dim3(kThreads), lds, st, a);
    else hipLaunchKernelGGL((joint_rows_kernel<false, false>), dim3(B), dim3(kThreads), lds, st, a);
  }
  HVK_CHECK_LAUNCH("joint_rows");
  hvk_eval_accumulate_launch(B, topk < L ? topk : L, rank, nll, dist, tier_hit, state, st);
  HVK_CHECK_LAUNCH("eval_accumulate");
  hipLaunchKernelGGL(joint_consistency_kernel, dim3(1), dim3(kThreads), 0, st, B, static_cast<const int*>(rank),
                     static_cast<const unsigned char*>(consistent), state);
  HVK_CHECK_LAUNCH("joint_consistency");
  return HVK_OK;
}

}  // extern "C"
