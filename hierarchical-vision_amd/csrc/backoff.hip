// Back-off decoding on gfx950 (hierarchy.py: backoff_predictions, BackoffMetrics): the greedy walk
// down the taxonomy by node mass P(n) = sum of softmax(z) over the leaves of n, stopped at the first
// depth whose mass falls below a threshold (Deng et al., CVPR 2012; Valmadre, NeurIPS 2022).
// Definition and tables: include/hvk.h.
//
// * backoff_rows_kernel -- one workgroup (4 waves) per row; the whole tree's per-row state, one f32
//   mass S(n) = sum exp(z_k - M) and one int (the best child) per node slot, lives in dynamic LDS
//   sized from the taxonomy and never touches HBM:
//   1. a coalesced sweep (16-B loads over the aligned body of the row) finds the row maximum M;
//   2. bottom-up over the rank-ordered node slots of Taxonomy.soft_tables(): tier 5 reads its leaf
//      ranges from global memory (the row was just read: L2), coarser tiers and the root their child
//      slots from LDS, a barrier between tiers.  A node sums its children and records the largest
//      in the same visit: a lane per narrow node (adjacent lanes own adjacent ranges), the whole
//      wave strided over a wide one, then a butterfly.  One shared M makes these plain sums of
//      non-negatives, so S(parent) >= S(child) holds in f32 (round-to-nearest is monotone);
//   3. thread 0 follows best[] seven times from LDS and writes path, prob = S(n_d) / S(root) and
//      the agreement with the target's path.
// * backoff_accumulate_kernel -- one workgroup per threshold folds the rows into the state: integer
//   counts in a fixed order.
// No atomics anywhere; equal inputs give bit-identical outputs and state.  No matrix instruction:
// the work is ragged segmented sums and a seven-step dependent walk.
#include <math.h>
#include <stdio.h>

#include "eval_common.h"
#include "../../include/hvk.h"

using namespace hvk_eval;

namespace {

constexpr int kTiers = 7;
constexpr int kCoarse = kTiers - 1;
// node slots (tiers 0-5 and the root) a workgroup keeps in LDS, 8 bytes each: joint.hip's kMaxCoarse,
// 120 KB of gfx950's 160 KB
constexpr int kMaxSlots = 15360;
constexpr int kMaxLeaves = 1 << 24;
constexpr int kMaxThresholds = 32;
// a node with at most this many children is summed by one lane, a wider one by its whole wave
constexpr int kSerialWidth = 16;
constexpr int kSums = 5;  // per threshold: depth, correct, common, at-leaf, leaf-hit

struct BackoffArgs {
  const void* logits;
  int B, L, ld;
  const int64_t* targets;
  int t_stride, t_off;
  const int* perm;      // [L] or null (identity)
  int rank_off[kTiers + 1];
  const int* child_lo;  // [n_slots]
  const int* child_hi;
  const int* slot_node;   // [n_slots - 1]
  const int* leaf_paths;  // [L, 7]
  int* path;              // [B, 7]
  float* prob;            // [B, 7]
  int* match;             // [B]
};

// exp(z - M) as a term of a sum shifted to the row maximum: the maximum itself is exactly 1 (also
// +inf), a NaN or -inf entry contributes nothing (also in a row that holds nothing else)
__device__ __forceinline__ float term(float z, float M) { return z > -INFINITY ? (z == M ? 1.f : expf(z - M)) : 0.f; }

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// a larger mass wins; among equal masses the lower index
__device__ __forceinline__ void take_max(float& m, int& mi, float v, int vi) {
  const bool t = v > m || (v == m && vi < mi);
  m = t ? v : m;
  mi = t ? vi : mi;
}

// children first, first + step, ... < hi of one node: their sum, the largest and its index (the
// first among equals: c ascends).  LEAVES: c is a permuted leaf position, its mass formed from the
// row; else c is a slot whose mass is in LDS.
template <bool BF16, bool LEAVES>
__device__ __forceinline__ void visit(const BackoffArgs& a, const char* row, const float* S, float M, int first,
                                      int hi, int step, float& sum, float& bv, int& bi) {
  for (int c = first; c < hi; c += step) {
    float v;
    if constexpr (LEAVES) {
      const int k = a.perm ? clampi(a.perm[HVK_BCHECK(c, a.L)], 0, a.L - 1) : c;
      v = term(load1(row, BF16, HVK_BCHECK(k, a.L)), M);
    } else {
      v = S[c];
    }
    sum += v;
    if (v > bv) bv = v, bi = c;
  }
}

template <bool BF16>
__global__ __launch_bounds__(kThreads) void backoff_rows_kernel(BackoffArgs a) {
  constexpr int esz = BF16 ? 2 : 4, N = 16 / esz;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  __shared__ float part[kWaves];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int n_slots = a.rank_off[kTiers], L = a.L;
  float* S = lds;                                      // [n_slots] masses
  int* best = reinterpret_cast<int*>(lds + n_slots);   // [n_slots] best child
  const char* row = static_cast<const char*>(a.logits) + (size_t)b * a.ld * esz;

  // ---- pass 1: the row maximum (fmaxf drops NaNs) ----------------------------------------------
  float M = -INFINITY;
  {
    const uintptr_t addr = (uintptr_t)row;
    int head = (addr & (esz - 1)) ? L : (int)(((16 - (addr & 15)) & 15) / esz);
    head = head < L ? head : L;
    const int nv = (L - head) / N;
    for (int j = tid; j < head; j += kThreads) M = fmaxf(M, load1(row, BF16, HVK_BCHECK(j, L)));
    for (int j = head + nv * N + tid; j < L; j += kThreads) M = fmaxf(M, load1(row, BF16, HVK_BCHECK(j, L)));
    const char* body = row + (size_t)head * esz;
    constexpr int UN = 4;  // every load of a round issued before the first value is used
    for (int v0 = tid; v0 < nv; v0 += kThreads * UN) {
      uint4 w[UN];
#pragma unroll
      for (int u = 0; u < UN; ++u) {
        const int v = v0 + u * kThreads;
        w[u] = hvk_ld16(body + (size_t)HVK_BCHECK(v < nv ? v : nv - 1, nv) * 16);  // a repeat moves no maximum
      }
#pragma unroll
      for (int u = 0; u < UN; ++u) {
        float x[N];
        if constexpr (BF16) {
          hvk_unpack8(w[u], x);
        } else {
          x[0] = __uint_as_float(w[u].x), x[1] = __uint_as_float(w[u].y), x[2] = __uint_as_float(w[u].z),
          x[3] = __uint_as_float(w[u].w);
        }
#pragma unroll
        for (int e = 0; e < N; ++e) M = fmaxf(M, x[e]);
      }
    }
    M = block_reduce_ordered(M, part, tid, [](float x, float y) { return fmaxf(x, y); });
  }

  // ---- pass 2: masses and best children of tiers 5 .. 0, then the root ---------------------------
  for (int s = 0; s < kTiers; ++s) {
    const int t = s < kCoarse ? kCoarse - 1 - s : kCoarse;  // t = 6: the root's slot
    const bool leaves = s == 0;
    const int n0 = a.rank_off[t], n1 = a.rank_off[t + 1];
    // where this tier's children live: leaf positions, or the slots of the next finer tier
    const int c0 = leaves ? 0 : (t == kCoarse ? a.rank_off[0] : a.rank_off[t + 1]);
    const int c1 = leaves ? L : (t == kCoarse ? a.rank_off[1] : a.rank_off[t + 2]);
    for (int base = n0 + wv * 64; base < n1; base += kThreads) {  // wave-uniform: 64 slots per wave
      const int i = base + lane;
      int lo = c0, hi = c0;
      if (i < n1) {  // a table entry outside the children's range is clamped into it, never followed
        lo = clampi(a.child_lo[HVK_BCHECK(i, n_slots)], c0, c1);
        hi = clampi(a.child_hi[i], c0, c1);
      }
      const bool wide = hi - lo > kSerialWidth;
      if (i < n1 && !wide) {
        float sum = 0.f, bv = -1.f;
        int bi = lo < c1 ? lo : c1 - 1;  // a node without children: mass 0, a child that exists
        if (leaves) visit<BF16, true>(a, row, S, M, lo, hi, 1, sum, bv, bi);
        else visit<BF16, false>(a, row, S, M, lo, hi, 1, sum, bv, bi);
        S[i] = sum;
        best[i] = bi;
      }
      unsigned long long m = __ballot(wide);
      while (m) {  // the wave's wide nodes, one after the other, 64 lanes strided over the children
        const int j = __ffsll(m) - 1;
        m &= m - 1;
        const int jlo = __shfl(lo, j), jhi = __shfl(hi, j);
        float sum = 0.f, bv = -1.f;
        int bi = kNoIdx;
        if (leaves) visit<BF16, true>(a, row, S, M, jlo + lane, jhi, 64, sum, bv, bi);
        else visit<BF16, false>(a, row, S, M, jlo + lane, jhi, 64, sum, bv, bi);
        sum = wave_sum_ordered(sum, lane);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
          const float v = __shfl_xor(bv, o);
          const int vi = __shfl_xor(bi, o);
          take_max(bv, bi, v, vi);
        }
        if (lane == 0) {
          S[base + j] = sum;
          best[base + j] = bi;  // more than kSerialWidth children: lane 0 had one, bi is set
        }
      }
    }
    __syncthreads();  // the next tier reads these masses back
  }
  if (tid != 0) return;

  // ---- the walk: seven dependent steps from LDS ---------------------------------------------------
  const int root = n_slots - 1;
  const float tot = S[root];
  const int64_t t64 = a.targets[(size_t)b * a.t_stride + a.t_off];
  const bool valid = t64 >= 0 && t64 < L;
  const int* tp = a.leaf_paths + (size_t)(valid ? t64 : 0) * kTiers;
  int slot = root, m = 0;
  bool agree = true;
#pragma unroll
  for (int d = 0; d < kTiers; ++d) {
    const int c = best[slot];
    int id;
    float mass;
    if (d < kCoarse) {
      const int cs = clampi(c, 0, root - 1);
      id = a.slot_node[HVK_BCHECK(cs, root)];
      mass = S[cs];
      slot = cs;
    } else {  // the leaf: its mass by the sum's own expression, bitwise the term tier 5 added
      const int pos = clampi(c, 0, L - 1);
      id = a.perm ? clampi(a.perm[pos], 0, L - 1) : pos;
      mass = term(load1(row, BF16, id), M);
    }
    a.path[(size_t)b * kTiers + d] = id;
    // an IEEE division is monotone in its numerator, so prob descends as the masses do and never
    // exceeds 1; every entry NaN: no mass anywhere, prob 0
    a.prob[(size_t)b * kTiers + d] = tot > 0.f ? mass / tot : 0.f;
    agree = agree && valid && tp[d] == id;
    m += agree ? 1 : 0;
  }
  a.match[b] = valid ? m : -1;
}

struct AccumulateArgs {
  int B;
  float thr[kMaxThresholds];
  const float* prob;
  const int* match;
  double* state;
};

// workgroup j: threshold j (workgroup 0 also the valid / invalid row counts).  Integer sums, exact
// in any order; the order is fixed all the same.
__global__ __launch_bounds__(kThreads) void backoff_accumulate_kernel(AccumulateArgs a) {
  const int tid = threadIdx.x, j = blockIdx.x;
  const float thr = a.thr[j];
  long long v[kSums + 2];
#pragma unroll
  for (int i = 0; i < kSums + 2; ++i) v[i] = 0;
  for (int b = tid; b < a.B; b += kThreads) {
    const int m = a.match[HVK_BCHECK(b, a.B)];
    if (m < 0) {
      v[kSums + 1] += 1;
      continue;
    }
    int D = 0;  // prob descends along the path: the count is the last depth at or above thr
#pragma unroll
    for (int d = 0; d < kTiers; ++d) D += a.prob[(size_t)b * kTiers + d] >= thr ? 1 : 0;
    v[0] += D;
    v[1] += D <= m ? 1 : 0;
    v[2] += D < m ? D : m;
    v[3] += D == kTiers ? 1 : 0;
    v[4] += (D == kTiers && m == kTiers) ? 1 : 0;
    v[kSums] += 1;
  }
  __shared__ long long part[kWaves][kSums + 2];
#pragma unroll
  for (int i = 0; i < kSums + 2; ++i) {
    const long long x = wave_sum_ordered(v[i], tid);
    if ((tid & 63) == 0) part[tid >> 6][i] = x;
  }
  __syncthreads();
  if (tid < kSums + 2) {
    const long long x = (part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid]);
    if (tid < kSums) a.state[2 + j * kSums + tid] += (double)x;
    else if (j == 0) a.state[tid - kSums] += (double)x;
  }
}

// null: supported; else what is wrong with the slot offsets
const char* check_offsets(const int* off, char* buf, size_t cap) {
  if (!off) return "null rank_off";
  if (off[0] != 0) return "rank_off[0] must be 0";
  for (int t = 0; t < kCoarse; ++t)
    if (off[t + 1] <= off[t]) return "rank_off must grow strictly (every tier holds a node)";
  if (off[kTiers] != off[kCoarse] + 1) return "rank_off[7] must be rank_off[6] + 1 (the root's slot)";
  if (off[kTiers] > kMaxSlots) {
    snprintf(buf, cap, "%d node slots, above the %d (8 bytes each, 120 KB) one workgroup keeps in LDS", off[kTiers],
             kMaxSlots);
    return buf;
  }
  return nullptr;
}

}  // namespace

extern "C" {

int hvk_backoff_supported(const int* rank_off) {
  char buf[160];
  return check_offsets(rank_off, buf, sizeof(buf)) == nullptr;
}

int hvk_backoff_decode(const void* logits, int logits_dtype, int B, int L, int ld, const int64_t* targets,
                       int t_stride, int t_off, const int* perm, const int* rank_off, const int* child_lo,
                       const int* child_hi, const int* slot_node, const int* leaf_paths, const float* thresholds,
                       int n_thresholds, int* path, float* prob, int* match, double* state, void* stream) {
  char buf[160];
  if (const char* why = check_offsets(rank_off, buf, sizeof(buf)))
    return hvk_set_error(why == buf ? HVK_EUNSUPPORTED : HVK_EINVAL, "hvk_backoff_decode: %s", why);
  if (B < 0 || L < 1 || ld < L || L > kMaxLeaves)
    return hvk_set_error(HVK_EINVAL, "hvk_backoff_decode: bad shape (B %d, L %d, ld %d: B >= 0, 1 <= L <= 2^24, ld >= L)",
                         B, L, ld);
  if (rank_off[kCoarse] - rank_off[kCoarse - 1] > L)
    return hvk_set_error(HVK_EINVAL, "hvk_backoff_decode: %d tier-5 nodes over %d leaves",
                         rank_off[kCoarse] - rank_off[kCoarse - 1], L);
  if (t_stride < 1 || t_off < 0 || t_off >= t_stride)
    return hvk_set_error(HVK_EINVAL, "hvk_backoff_decode: target stride %d / offset %d", t_stride, t_off);
  if (logits_dtype != 0 && logits_dtype != 1)
    return hvk_set_error(HVK_EINVAL, "hvk_backoff_decode: unknown logits dtype %d (0 f32, 1 bf16)", logits_dtype);
  if (!logits || !targets || !child_lo || !child_hi || !slot_node || !leaf_paths || !thresholds || !path || !prob ||
      !match || !state)
    return hvk_set_error(HVK_EINVAL, "hvk_backoff_decode: null pointer");
  if (n_thresholds < 1 || n_thresholds > kMaxThresholds)
    return hvk_set_error(HVK_EINVAL, "hvk_backoff_decode: %d thresholds (1 .. %d)", n_thresholds, kMaxThresholds);
  for (int j = 0; j < n_thresholds; ++j)
    if (!(thresholds[j] > 0.f && thresholds[j] <= 1.f) || (j > 0 && !(thresholds[j] > thresholds[j - 1])))
      return hvk_set_error(HVK_EINVAL, "hvk_backoff_decode: threshold %d = %g (each in (0, 1], strictly ascending)", j,
                           (double)thresholds[j]);
  if (B == 0) return HVK_OK;
  BackoffArgs a{};
  a.logits = logits, a.B = B, a.L = L, a.ld = ld, a.targets = targets, a.t_stride = t_stride, a.t_off = t_off;
  a.perm = perm, a.child_lo = child_lo, a.child_hi = child_hi, a.slot_node = slot_node, a.leaf_paths = leaf_paths;
  a.path = path, a.prob = prob, a.match = match;
  for (int t = 0; t <= kTiers; ++t) a.rank_off[t] = rank_off[t];
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t lds = (size_t)rank_off[kTiers] * (sizeof(float) + sizeof(int));
  const auto kernel = logits_dtype ? backoff_rows_kernel<true> : backoff_rows_kernel<false>;
  if (lds > 64 * 1024) {  // above the 64 KB a launch may take unasked: ask for it (no stream work)
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess)
      return hvk_set_error(HVK_EHIP, "hvk_backoff_decode: %zu bytes of LDS: %s", lds, hipGetErrorString(e));
  }
  hipLaunchKernelGGL(kernel, dim3(B), dim3(kThreads), lds, st, a);
  HVK_CHECK_LAUNCH("backoff_rows");
  AccumulateArgs acc{};
  acc.B = B, acc.prob = prob, acc.match = match, acc.state = state;
  for (int j = 0; j < n_thresholds; ++j) acc.thr[j] = thresholds[j];
  hipLaunchKernelGGL(backoff_accumulate_kernel, dim3(n_thresholds), dim3(kThreads), 0, st, acc);
  HVK_CHECK_LAUNCH("backoff_accumulate");
  return HVK_OK;
}

}  // extern "C"
