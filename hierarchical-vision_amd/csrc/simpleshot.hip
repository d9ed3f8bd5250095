// SimpleShot evaluation on gfx950 (simpleshot.py:139-203, hierarchy.py:488-597): feature
// conditioning, the nearest-centroid fit with float64 sums, and the flat / top-down predictions.
//
// * ss_prepare_kernel -- one wave per row: x / mean(x) and / or x / ||x||, f32, each row sum a
//   per-lane partial followed by a fixed butterfly.
// * ss_accumulate_kernel -- one workgroup per position p of the stable label order.  The
//   workgroup whose position starts a run of equal labels owns that class for this batch: thread k
//   adds the run's rows to sums[class][k] one at a time in ascending row index, so a (class, k)
//   cell has a single writer and the order of its additions depends on the rows alone: N rows in
//   one call or in consecutive batches leave the same bits.  One extra workgroup counts the rows
//   whose label is outside [0, L).
// * ss_tier_sum_kernel / ss_centroid_kernel -- finalize: the sums and counts of tier t from its
//   CSR children of tier t + 1 in ascending child id, bottom-up, then f32 centroids (the float64
//   mean rounded once) and their squared norms.
// * ss_flat_kernel / ss_flat_reduce_kernel -- argmin_c (cnorm[c] - 2 x . c) on the f32-input MFMA
//   (16x16x4): a workgroup holds 64 rows against a range of 64-class tiles, both staged through
//   LDS in 32-column chunks; the scores live in accumulators only and every lane keeps a running
//   (min, index) per row.  The class range is split over workgroups; a second kernel folds the
//   splits' partial pairs in ascending split order.
// * ss_tree_kernel -- one wave per sample with its row in LDS: at each tier the candidates (all
//   tier-0 nodes, then the CSR children of the node just chosen) are scored one after another by
//   sum_k (x_k - c_k)^2 across the wave's lanes.
// No atomics anywhere: equal inputs give bit-identical outputs.
#include <math.h>

#include "hvk_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxTiers = 8;

// ceil(a / b) for a >= 0 without the a + b - 1 that overflows next to 2^31
constexpr int ceil_div(int a, int b) { return a / b + (a % b != 0 ? 1 : 0); }

// the same operand order in both lanes of a pair: every lane ends with the same bits
__device__ __forceinline__ float wave_sum_ordered(float v, int lane) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const float w = __shfl_xor(v, o);
    v = (lane & o) ? w + v : v + w;
  }
  return v;
}

// ---------------------------------------------------------------------------------- prepare
__device__ __forceinline__ float ss_load(const void* row, int bf16, int k) {
  if (bf16) return __uint_as_float((uint32_t) static_cast<const hvk_bf16*>(row)[k] << 16);
  return static_cast<const float*>(row)[k];
}

__global__ __launch_bounds__(kThreads) void ss_prepare_kernel(const void* x, int bf16, int B, int D, int ld,
                                                             int centered, int l2n, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (b >= B) return;  // whole waves leave: the shuffles below stay wave-complete
  const char* row = static_cast<const char*>(x) + (size_t)b * ld * (bf16 ? 2 : 4);
  float* o = out + (size_t)b * D;
  float mean = 1.f;
  if (centered) {
    float s = 0.f;
    for (int k = lane; k < D; k += 64) s += ss_load(row, bf16, HVK_BCHECK(k, D));
    mean = wave_sum_ordered(s, lane) / (float)D;
  }
  float norm = 1.f;
  if (l2n) {
    float ss = 0.f;
    for (int k = lane; k < D; k += 64) {
      float v = ss_load(row, bf16, k);
      if (centered) v = v / mean;
      ss = __builtin_fmaf(v, v, ss);
    }
    norm = sqrtf(wave_sum_ordered(ss, lane));
  }
  for (int k = lane; k < D; k += 64) {
    float v = ss_load(row, bf16, k);
    if (centered) v = v / mean;
    if (l2n) v = v / norm;
    o[HVK_BCHECK(k, D)] = v;
  }
}

// ---------------------------------------------------------------------------------- fit
__global__ __launch_bounds__(kThreads) void ss_accumulate_kernel(const float* __restrict__ x, int B, int D,
                                                                const int64_t* __restrict__ labels, int t_stride,
                                                                int t_off, const int64_t* __restrict__ order, int L,
                                                                double* sums, long long* counts, double* state) {
  const int tid = threadIdx.x;
  const int p = blockIdx.x;
  if (p == B) {
    // the rows that are skipped: a label outside [0, L), or an order entry that names no row
    int bad = 0;
    for (int q = tid; q < B; q += kThreads) {
      const int64_t r = order[q];
      bool ok = r >= 0 && r < B;
      if (ok) {
        const int64_t c = labels[(size_t)r * t_stride + t_off];
        ok = c >= 0 && c < L;
      }
      bad += ok ? 0 : 1;
    }
    __shared__ int part[kWaves];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) bad += __shfl_xor(bad, o);
    if ((tid & 63) == 0) part[tid >> 6] = bad;
    __syncthreads();
    if (tid == 0) {
      int n = 0;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) n += part[w];
      state[0] += (double)(B - n);
      state[1] += (double)n;
    }
    return;
  }
  const int64_t r0 = order[p];
  if (r0 < 0 || r0 >= B) return;
  const int64_t c = labels[(size_t)r0 * t_stride + t_off];
  if (c < 0 || c >= L) return;
  if (p > 0) {  // not the start of its run: the run's first workgroup adds this row
    const int64_t rp = order[p - 1];
    if (rp >= 0 && rp < B && labels[(size_t)rp * t_stride + t_off] == c) return;
  }
  // the run [p, e): every thread walks it (the same scalar loads in every lane)
  int e = p + 1;
  for (; e < B; ++e) {
    const int64_t r = order[e];
    if (r < 0 || r >= B || labels[(size_t)r * t_stride + t_off] != c) break;
  }
  double* srow = sums + (size_t)HVK_BCHECK(c, L) * D;
  for (int k = tid; k < D; k += kThreads) {
    double s = srow[k];
    for (int q = p; q < e; ++q) s += (double)x[(size_t)HVK_BCHECK(order[q], B) * D + k];
    srow[k] = s;
  }
  if (tid == 0) counts[c] += (long long)(e - p);
}

// ---------------------------------------------------------------------------------- finalize
// sums / counts of the n nodes of one tier (at sums, counts) from the tier below (csums, ccounts,
// nc nodes): node i's children are cidx[cptr[i] .. cptr[i + 1]) in ascending id
__global__ __launch_bounds__(kThreads) void ss_tier_sum_kernel(double* sums, long long* counts, int n,
                                                              const double* csums, const long long* ccounts, int nc,
                                                              const int* __restrict__ cptr,
                                                              const int* __restrict__ cidx, int cidx_len, int D) {
  const int i = blockIdx.x, tid = threadIdx.x;
  int lo = cptr[i], hi = cptr[i + 1];
  lo = lo < 0 ? 0 : lo;
  hi = hi > cidx_len ? cidx_len : hi;
  for (int k = tid; k < D; k += kThreads) {
    double s = 0.0;
    for (int q = lo; q < hi; ++q) {
      const int ch = cidx[q];
      if (ch >= 0 && ch < nc) s += csums[(size_t)ch * D + k];
    }
    sums[(size_t)HVK_BCHECK(i, n) * D + k] = s;
  }
  if (tid == 0) {
    long long m = 0;
    for (int q = lo; q < hi; ++q) {
      const int ch = cidx[q];
      if (ch >= 0 && ch < nc) m += ccounts[ch];
    }
    counts[i] = m;
  }
}

__global__ __launch_bounds__(kThreads) void ss_centroid_kernel(const double* __restrict__ sums,
                                                              const long long* __restrict__ counts, int D,
                                                              float* __restrict__ centroids,
                                                              float* __restrict__ cnorm) {
  const int i = blockIdx.x, tid = threadIdx.x;
  const long long n = counts[i];
  const double* s = sums + (size_t)i * D;
  float* c = centroids + (size_t)i * D;
  float ss = 0.f;
  for (int k = tid; k < D; k += kThreads) {
    const float v = n > 0 ? (float)(s[k] / (double)n) : 0.f;  // an empty class: a zero row, never chosen
    c[k] = v;
    ss = __builtin_fmaf(v, v, ss);
  }
  ss = wave_sum_ordered(ss, tid & 63);
  __shared__ float part[kWaves];
  if ((tid & 63) == 0) part[tid >> 6] = ss;
  __syncthreads();
  if (tid == 0) cnorm[i] = n > 0 ? (part[0] + part[1]) + (part[2] + part[3]) : INFINITY;
}

// ---------------------------------------------------------------------------------- flat predict
constexpr int kBM = 64;   // rows per workgroup: 16 per wave
constexpr int kBN = 64;   // classes per tile: 4 accumulators per wave
constexpr int kBK = 32;   // feature columns per LDS chunk
constexpr int kLd = kBK + 4;  // LDS row stride in floats: rows 0..15 start in 16 distinct 4-bank groups
constexpr int kGr = kBK / 4;  // 16-B granules per tile row
constexpr int kU = kBM * kGr / kThreads;  // granules per thread and tile
static_assert(kBM == kBN && kBM * kGr % kThreads == 0 && kBK % 16 == 0 && kLd % 8 == 4, "tile staging");
constexpr int kNoIdx = 0x7fffffff;

// a lower score wins; among equal scores the lower class index (NaN scores never compare below)
__device__ __forceinline__ void take_min(float& m, int& mi, float v, int vi) {
  const bool t = v < m || (v == m && vi < mi);
  m = t ? v : m;
  mi = t ? vi : mi;
}

// 16-B granule g of a [64, kBK] f32 tile: row g / kGr, columns 4 (g % kGr) ..; rows past
// `rows` and columns past D read zero (D % 4 == 0: a granule is all inside or all outside)
__device__ __forceinline__ uint4 ss_tile_ld(const float* base, int r0, int rows, int k0, int D, int g) {
  const int r = r0 + g / kGr, k = k0 + 4 * (g % kGr);
  if (r < rows && k < D) return hvk_ld16(base + (size_t)HVK_BCHECK(r, rows) * D + k);
  return make_uint4(0, 0, 0, 0);
}

__global__ __launch_bounds__(kThreads) void ss_flat_kernel(const float* __restrict__ x, int B, int D,
                                                          const float* __restrict__ cent,
                                                          const float* __restrict__ cnorm, int L,
                                                          int tiles_per_split, float* __restrict__ pmin,
                                                          int* __restrict__ pidx) {
  __shared__ __attribute__((aligned(16))) float xs[kBM * kLd];
  __shared__ __attribute__((aligned(16))) float cs[kBN * kLd];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int m0 = blockIdx.x * kBM, split = blockIdx.y;
  const int tiles = ceil_div(L, kBN);
  const int t_lo = split * tiles_per_split;
  const int t_hi = t_lo + tiles_per_split < tiles ? t_lo + tiles_per_split : tiles;

  float best[4] = {INFINITY, INFINITY, INFINITY, INFINITY};
  int bidx[4] = {kNoIdx, kNoIdx, kNoIdx, kNoIdx};
  const int chunks = ceil_div(D, kBK);

  for (int t = t_lo; t < t_hi; ++t) {
    const int c0 = t * kBN;
    hvk_f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = hvk_f32x4{0.f, 0.f, 0.f, 0.f};
    // chunk 0 into registers; inside the loop the next chunk's loads fly over this chunk's MFMAs
    uint4 xr[kU], cr[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      xr[u] = ss_tile_ld(x, m0, B, 0, D, tid + u * kThreads);
      cr[u] = ss_tile_ld(cent, c0, L, 0, D, tid + u * kThreads);
    }
    for (int ch = 0; ch < chunks; ++ch) {
      __syncthreads();  // the previous chunk's readers are done
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int gi = tid + u * kThreads;
        *reinterpret_cast<uint4*>(&xs[(gi / kGr) * kLd + 4 * (gi % kGr)]) = xr[u];
        *reinterpret_cast<uint4*>(&cs[(gi / kGr) * kLd + 4 * (gi % kGr)]) = cr[u];
      }
      __syncthreads();
      if (ch + 1 < chunks) {
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          xr[u] = ss_tile_ld(x, m0, B, (ch + 1) * kBK, D, tid + u * kThreads);
          cr[u] = ss_tile_ld(cent, c0, L, (ch + 1) * kBK, D, tid + u * kThreads);
        }
      }
      // 16 columns per step: lane group g holds columns 4g .. 4g + 3 of both operands and feeds
      // element s to the s-th MFMA, so A and B agree on k in every lane (the k order inside the
      // 16 is a permutation; a dot product does not care)
#pragma unroll
      for (int kk = 0; kk < kBK; kk += 16) {
        const hvk_f32x4 a = *reinterpret_cast<const hvk_f32x4*>(&xs[(wave * 16 + li) * kLd + kk + 4 * g]);
        hvk_f32x4 bq[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          bq[j] = *reinterpret_cast<const hvk_f32x4*>(&cs[(j * 16 + li) * kLd + kk + 4 * g]);
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], bq[j][s], acc[j], 0, 0, 0);
      }
    }
    hvk_settle(acc[0], acc[1], acc[2], acc[3]);
    // D lane l: row 4 (l >> 4) + r, column l & 15 of each 16-class block j, ascending class order
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = c0 + j * 16 + li;
      const float cn = c < L ? cnorm[HVK_BCHECK(c < L ? c : 0, L)] : INFINITY;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float s = __builtin_fmaf(-2.f, acc[j][r], cn);
        // +inf (an empty class, a column past L) is never below the initial +inf
        if (s < best[r]) {
          best[r] = s;
          bidx[r] = c;
        }
      }
    }
  }
  // across the 16 lanes that share these rows
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int o = 8; o >= 1; o >>= 1) {
      const float v = __shfl_xor(best[r], o);
      const int vi = __shfl_xor(bidx[r], o);
      take_min(best[r], bidx[r], v, vi);
    }
  }
  if (li == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = m0 + wave * 16 + 4 * g + r;
      if (row < B) {
        pmin[(size_t)split * B + HVK_BCHECK(row, B)] = best[r];
        pidx[(size_t)split * B + row] = bidx[r];
      }
    }
  }
}

__global__ __launch_bounds__(kThreads) void ss_flat_reduce_kernel(const float* __restrict__ pmin,
                                                                 const int* __restrict__ pidx, int B, int L,
                                                                 int splits, int* __restrict__ pred) {
  const int b = blockIdx.x * kThreads + threadIdx.x;
  if (b >= B) return;
  float m = INFINITY;
  int mi = kNoIdx;
  for (int s = 0; s < splits; ++s) take_min(m, mi, pmin[(size_t)s * B + b], pidx[(size_t)s * B + b]);
  pred[b] = (mi >= 0 && mi < L) ? mi : 0;  // nothing compared (NaN rows, no fitted class): class 0
}

struct FlatPlan {
  int row_tiles, tiles, tiles_per_split, splits;
};
// the class tiles over about 512 workgroups (two per CU) in all; 64-column chunks and 1024
// workgroups measured no faster (B = 256, L = 10 000: the 64 x 64 tile's 16 flop per byte staged
// through LDS is what binds, not the wait for a chunk)
FlatPlan flat_plan(int B, int L) {
  FlatPlan p;
  p.row_tiles = ceil_div(B, kBM);
  p.tiles = ceil_div(L, kBN);
  int want = 512 / (p.row_tiles > 0 ? p.row_tiles : 1);
  want = want < 1 ? 1 : (want > p.tiles ? p.tiles : want);
  p.tiles_per_split = ceil_div(p.tiles, want);
  p.splits = ceil_div(p.tiles, p.tiles_per_split);
  return p;
}

// ---------------------------------------------------------------------------------- tree predict
struct Tiers {
  int n;
  int base[kMaxTiers + 1];
};

__global__ __launch_bounds__(kThreads) void ss_tree_kernel(const float* __restrict__ x, int B, int D,
                                                          const float* __restrict__ cent,
                                                          const long long* __restrict__ counts, Tiers tiers,
                                                          const int* __restrict__ cptr, const int* __restrict__ cidx,
                                                          int* __restrict__ pred) {
  extern __shared__ __attribute__((aligned(16))) float rows[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x * kWaves + wave;
  float* xr = rows + (size_t)wave * D;
  if (b < B)
    for (int k = lane; k < D; k += 64) xr[k] = x[(size_t)b * D + k];
  __syncthreads();
  if (b >= B) return;
  const int n_idx = tiers.base[tiers.n] - tiers.base[1];  // entries of cidx
  int chosen = 0;
  for (int t = 0; t < tiers.n; ++t) {
    const int n_t = tiers.base[t + 1] - tiers.base[t];
    int lo = 0, hi = n_t;  // tier 0: every node; below: positions in cidx
    if (t > 0) {
      lo = cptr[tiers.base[t - 1] + chosen];
      hi = cptr[tiers.base[t - 1] + chosen + 1];
      lo = lo < 0 ? 0 : lo;
      hi = hi > n_idx ? n_idx : hi;
    }
    float best = 0.f;
    int pick = -1, first = -1;
    for (int q = lo; q < hi; ++q) {  // wave-uniform
      const int node = t > 0 ? cidx[q] : q;
      if (node < 0 || node >= n_t) continue;
      if (first < 0) first = node;
      if (counts[tiers.base[t] + node] <= 0) continue;
      const float* c = cent + (size_t)(tiers.base[t] + node) * D;
      float d = 0.f;
      for (int k = lane; k < D; k += 64) {
        const float e = xr[k] - c[k];
        d = __builtin_fmaf(e, e, d);
      }
      d = wave_sum_ordered(d, lane);
      // ascending id: a strict compare keeps the lowest id among equals; a NaN distance is taken
      // only while nothing else has been
      if (pick < 0 || d < best) {
        best = d;
        pick = node;
      }
    }
    chosen = pick >= 0 ? pick : (first >= 0 ? first : 0);
    if (lane == 0) pred[(size_t)b * tiers.n + t] = chosen;
  }
}

int check_tiers(const char* who, int n_tiers, const int* tier_base, const int* child_ptr, const int* child_idx,
                Tiers* out) {
  if (n_tiers < 1 || n_tiers > kMaxTiers)
    return hvk_set_error(HVK_EINVAL, "%s: n_tiers %d outside [1, %d]", who, n_tiers, kMaxTiers);
  if (!tier_base) return hvk_set_error(HVK_EINVAL, "%s: null pointer (tier_base)", who);
  if (n_tiers > 1 && (!child_ptr || !child_idx))
    return hvk_set_error(HVK_EINVAL, "%s: null pointer (child_ptr / child_idx with %d tiers)", who, n_tiers);
  out->n = n_tiers;
  for (int t = 0; t <= kMaxTiers; ++t) out->base[t] = 0;
  for (int t = 0; t <= n_tiers; ++t) {
    out->base[t] = tier_base[t];
    if ((t == 0 && tier_base[0] != 0) || (t > 0 && tier_base[t] <= tier_base[t - 1]))
      return hvk_set_error(HVK_EINVAL, "%s: tier_base must start at 0 and grow (entry %d is %d)", who, t,
                           tier_base[t]);
  }
  return HVK_OK;
}

}  // namespace

extern "C" {

int hvk_ss_prepare(const void* x, int x_dtype, int B, int D, int ld, int centered, int l2_normalized, float* out,
                   void* stream) {
  if (B < 0 || D < 1 || ld < D)
    return hvk_set_error(HVK_EINVAL, "hvk_ss_prepare: bad shape (B %d, D %d, ld %d: B >= 0, D >= 1, ld >= D)", B, D,
                         ld);
  if (x_dtype != 0 && x_dtype != 1)
    return hvk_set_error(HVK_EINVAL, "hvk_ss_prepare: unknown feature dtype %d (0 f32, 1 bf16)", x_dtype);
  if (!x || !out) return hvk_set_error(HVK_EINVAL, "hvk_ss_prepare: null pointer");
  if (B == 0) return HVK_OK;
  hipLaunchKernelGGL(ss_prepare_kernel, dim3(ceil_div(B, kWaves)), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), x, x_dtype, B, D, ld, centered ? 1 : 0,
                     l2_normalized ? 1 : 0, out);
  HVK_CHECK_LAUNCH("ss_prepare");
  return HVK_OK;
}

int hvk_ss_accumulate(const float* x, int B, int D, const int64_t* labels, int t_stride, int t_off,
                      const int64_t* order, int L, double* sums, long long* counts, double* state, void* stream) {
  if (B < 0 || B == 0x7fffffff || D < 1 || L < 1)  // B + 1 workgroups
    return hvk_set_error(HVK_EINVAL, "hvk_ss_accumulate: bad shape (B %d, D %d, L %d: 0 <= B < 2^31 - 1, D >= 1, L >= 1)",
                         B, D, L);
  if (t_stride < 1 || t_off < 0 || t_off >= t_stride)
    return hvk_set_error(HVK_EINVAL, "hvk_ss_accumulate: label stride %d / offset %d", t_stride, t_off);
  if (!x || !labels || !order || !sums || !counts || !state)
    return hvk_set_error(HVK_EINVAL, "hvk_ss_accumulate: null pointer");
  if (B == 0) return HVK_OK;
  hipLaunchKernelGGL(ss_accumulate_kernel, dim3(B + 1), dim3(kThreads), 0, static_cast<hipStream_t>(stream), x, B, D,
                     labels, t_stride, t_off, order, L, sums, counts, state);
  HVK_CHECK_LAUNCH("ss_accumulate");
  return HVK_OK;
}

int hvk_ss_finalize(double* sums, long long* counts, int D, int n_tiers, const int* tier_base, const int* child_ptr,
                    const int* child_idx, float* centroids, float* cnorm, void* stream) {
  if (D < 1) return hvk_set_error(HVK_EINVAL, "hvk_ss_finalize: bad shape (D %d < 1)", D);
  Tiers tiers;
  if (int rc = check_tiers("hvk_ss_finalize", n_tiers, tier_base, child_ptr, child_idx, &tiers)) return rc;
  if (!sums || !counts || !centroids || !cnorm) return hvk_set_error(HVK_EINVAL, "hvk_ss_finalize: null pointer");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int n_nodes = tiers.base[n_tiers];
  const int n_idx = n_nodes - tiers.base[1];
  for (int t = n_tiers - 2; t >= 0; --t) {
    const int n = tiers.base[t + 1] - tiers.base[t], nc = tiers.base[t + 2] - tiers.base[t + 1];
    hipLaunchKernelGGL(ss_tier_sum_kernel, dim3(n), dim3(kThreads), 0, st, sums + (size_t)tiers.base[t] * D,
                       counts + tiers.base[t], n, sums + (size_t)tiers.base[t + 1] * D, counts + tiers.base[t + 1],
                       nc, child_ptr + tiers.base[t], child_idx, n_idx, D);
    HVK_CHECK_LAUNCH("ss_tier_sum");
  }
  hipLaunchKernelGGL(ss_centroid_kernel, dim3(n_nodes), dim3(kThreads), 0, st, sums, counts, D, centroids, cnorm);
  HVK_CHECK_LAUNCH("ss_centroid");
  return HVK_OK;
}

size_t hvk_ss_predict_flat_workspace(int B, int L) {
  if (B < 1 || L < 1) return 0;
  const FlatPlan p = flat_plan(B, L);
  return (size_t)p.splits * B * (sizeof(float) + sizeof(int));
}

int hvk_ss_predict_flat(const float* x, int B, int D, const float* centroids, const float* cnorm, int L, int* pred,
                        void* workspace, size_t workspace_bytes, void* stream) {
  if (B < 0 || L < 1 || D < 1)
    return hvk_set_error(HVK_EINVAL, "hvk_ss_predict_flat: bad shape (B %d, L %d, D %d: B >= 0, L >= 1, D >= 1)", B,
                         L, D);
  if (D % 4) return hvk_set_error(HVK_EINVAL, "hvk_ss_predict_flat: D %d is not a multiple of 4", D);
  if (L > 0x7fffff00) return hvk_set_error(HVK_EINVAL, "hvk_ss_predict_flat: bad shape (L %d > 2^31 - 256)", L);
  if (!x || !centroids || !cnorm || !pred) return hvk_set_error(HVK_EINVAL, "hvk_ss_predict_flat: null pointer");
  if (((uintptr_t)x | (uintptr_t)centroids) & 15)
    return hvk_set_error(HVK_EINVAL, "hvk_ss_predict_flat: x and centroids must be 16-byte aligned");
  if (B == 0) return HVK_OK;
  const size_t need = hvk_ss_predict_flat_workspace(B, L);
  if (!workspace || workspace_bytes < need)
    return hvk_set_error(HVK_EINVAL, "hvk_ss_predict_flat: workspace of %zu bytes, %zu needed (null pointer or small)",
                         workspace ? workspace_bytes : (size_t)0, need);
  const FlatPlan p = flat_plan(B, L);
  if (p.splits > 65535) return hvk_set_error(HVK_EUNSUPPORTED, "hvk_ss_predict_flat: %d class splits", p.splits);
  float* pmin = static_cast<float*>(workspace);
  int* pidx = reinterpret_cast<int*>(pmin + (size_t)p.splits * B);
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(ss_flat_kernel, dim3(p.row_tiles, p.splits), dim3(kThreads), 0, st, x, B, D, centroids, cnorm, L,
                     p.tiles_per_split, pmin, pidx);
  HVK_CHECK_LAUNCH("ss_flat");
  hipLaunchKernelGGL(ss_flat_reduce_kernel, dim3(ceil_div(B, kThreads)), dim3(kThreads), 0, st,
                     static_cast<const float*>(pmin), static_cast<const int*>(pidx), B, L, p.splits, pred);
  HVK_CHECK_LAUNCH("ss_flat_reduce");
  return HVK_OK;
}

int hvk_ss_predict_tree(const float* x, int B, int D, const float* centroids, const long long* counts, int n_tiers,
                        const int* tier_base, const int* child_ptr, const int* child_idx, int* pred, void* stream) {
  if (B < 0 || D < 1)
    return hvk_set_error(HVK_EINVAL, "hvk_ss_predict_tree: bad shape (B %d, D %d: B >= 0, D >= 1)", B, D);
  if (D > 4096)
    return hvk_set_error(HVK_EUNSUPPORTED, "hvk_ss_predict_tree: D %d > 4096 (four rows per workgroup in LDS)", D);
  Tiers tiers;
  if (int rc = check_tiers("hvk_ss_predict_tree", n_tiers, tier_base, child_ptr, child_idx, &tiers)) return rc;
  if (!x || !centroids || !counts || !pred) return hvk_set_error(HVK_EINVAL, "hvk_ss_predict_tree: null pointer");
  if (B == 0) return HVK_OK;
  hipLaunchKernelGGL(ss_tree_kernel, dim3(ceil_div(B, kWaves)), dim3(kThreads),
                     (size_t)kWaves * D * sizeof(float), static_cast<hipStream_t>(stream), x, B, D, centroids, counts,
                     tiers, child_ptr, child_idx, pred);
  HVK_CHECK_LAUNCH("ss_tree");
  return HVK_OK;
}

}  // extern "C"
