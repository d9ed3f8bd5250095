// CRM decoding on gfx950 (Karthik et al., ICLR 2021): the class of least expected tree distance
// under the model's own softmax, pred_b = argmin_k sum_j tree_dists[k, j] softmax(z_b)_j.
//
// * tree_dist_kernel -- the uint8 [L, L] matrix from the int32 [L, 7] leaf paths, the rule of
//   hvk_eval_metrics' path mode.  A thread owns 16 consecutive bytes of the flat matrix (one 16-B
//   store); the row's path stays in registers and is reloaded where the 16 bytes cross a row end.
// * crm_probs_kernel -- one workgroup per row: max, sum of expf(z - max), then expf(z - max) / sum
//   as f32 [B, Lk] in the workspace, Lk = L rounded up to the K chunk, the padding written as 0.
// * crm_risk_kernel -- P . D^T on the f32-input MFMA (16x16x4), nothing rounded below f32.  A
//   workgroup owns a 32-row x 128-class tile of its own (the byte operand: not f32_tile.h's 64 x
//   64 tile of two f32 operands) and sweeps all of K in 32-column chunks: the P chunk
//   (f32, from the L2-resident workspace) and the D chunk (BYTES, a quarter of the traffic and of
//   the LDS of f32) go registers -> LDS, double-buffered, so the next chunk's global loads fly over
//   this chunk's 32 MFMAs per wave and a chunk costs one barrier.  Lane (li, g) reads 8 bytes of
//   D row li and the 8 floats of P row li at the same k = 8 g ..; v_cvt_f32_ubyte0..3 widens the
//   bytes when the operand is formed, byte s of both feeding the s-th MFMA: A and B agree on k in
//   every lane and every class column sees the same k order, so equal rows of D give equal bits.
//   The [B, L] risks live in accumulators only; the tile is reduced to one (min risk, lowest
//   class) pair per row in the workspace (take_min, eval_common.h).
// * crm_finalize_kernel -- one workgroup: folds the pairs in ascending tile order, writes pred /
//   risk / dist and adds hits and distances to state[13] / state[14] by a fixed butterfly.
// No atomics anywhere: equal inputs give bit-identical outputs and state.
#include <math.h>

#include "eval_common.h"

using namespace hvk_eval;

namespace {

constexpr int kTiers = 7;
constexpr int kMaxL = 1 << 20;  // L * L bytes and every index below stay far inside 64 / 32 bits

// ---------------------------------------------------------------------------------- matrix
__device__ __forceinline__ void load_path(const int* __restrict__ paths, int L, int k, int (&p)[kTiers]) {
#pragma unroll
  for (int q = 0; q < kTiers; ++q) p[q] = paths[(size_t)HVK_BCHECK(k, L) * kTiers + q];
}

__global__ __launch_bounds__(kThreads) void tree_dist_kernel(const int* __restrict__ paths, int L,
                                                            unsigned char* __restrict__ out, int aligned) {
  const size_t total = (size_t)L * L;
  const size_t i0 = ((size_t)blockIdx.x * kThreads + threadIdx.x) * 16;
  if (i0 >= total) return;
  int k = (int)(i0 / (size_t)L), j = (int)(i0 - (size_t)k * L);
  int pk[kTiers];
  load_path(paths, L, k, pk);
  uint32_t w[4] = {0u, 0u, 0u, 0u};
  const int n = total - i0 < 16 ? (int)(total - i0) : 16;
  for (int e = 0; e < n; ++e) {
    int pj[kTiers];
    load_path(paths, L, j, pj);
    uint32_t d = kTiers;
#pragma unroll
    for (int q = 0; q < kTiers; ++q)  // coarse to fine: the finest matching tier sets d last
      if (pk[q] == pj[q]) d = kTiers - 1 - q;
    w[e >> 2] |= d << (8 * (e & 3));
    if (++j == L) {
      j = 0;
      if (++k < L) load_path(paths, L, k, pk);
    }
  }
  if (aligned && n == 16) {
    hvk_st16(out + i0, make_uint4(w[0], w[1], w[2], w[3]));
  } else {
    for (int e = 0; e < n; ++e) out[HVK_BCHECK(i0 + e, total)] = (unsigned char)(w[e >> 2] >> (8 * (e & 3)));
  }
}

// ---------------------------------------------------------------------------------- probs
constexpr int kBM = 32;    // rows per workgroup, every wave holding all of them
constexpr int kBN = 128;   // classes per workgroup: 32 per wave
constexpr int kBK = 32;    // k per chunk: 128 B of a P row, 32 B of a D row
constexpr int kPLd = kBK + 4;   // LDS P row stride in floats: rows 0..15 start in 16 distinct 4-bank groups
constexpr int kDLd = kBK + 16;  // LDS D row stride in bytes: 8-B reads of 16 rows x 2 groups hit 32 distinct bank pairs
constexpr int kPU = kBM * (kBK / 4) / kThreads;  // 16-B granules of P per thread and chunk
static_assert(kPU == 1 && kBN * (kBK / 16) == kThreads && kPLd % 8 == 4 && kDLd % 16 == 0, "tile staging");

__global__ __launch_bounds__(kThreads) void crm_probs_kernel(const void* logits, int bf16, int L, int ld, int Lk,
                                                            float* __restrict__ probs) {
  __shared__ float part[kWaves];
  const int b = blockIdx.x, tid = threadIdx.x;
  const char* row = static_cast<const char*>(logits) + (size_t)b * ld * (bf16 ? 2 : 4);
  float* p = probs + (size_t)b * Lk;
  float m = -INFINITY;
  for (int j = tid; j < L; j += kThreads) m = fmaxf(m, load1(row, bf16, HVK_BCHECK(j, L)));  // fmaxf drops NaNs
  m = block_reduce_ordered(m, part, tid, [](float a, float c) { return fmaxf(a, c); });
  float s = 0.f;
  for (int j = tid; j < L; j += kThreads) {
    const float e = expf(load1(row, bf16, j) - m);  // a NaN logit (or a row of -inf) makes the row NaN
    p[HVK_BCHECK(j, Lk)] = e;
    s += e;
  }
  s = block_reduce_ordered(s, part, tid, [](float a, float c) { return a + c; });
  // a thread divides the entries it wrote itself
  for (int j = tid; j < Lk; j += kThreads) p[j] = j < L ? p[j] / s : 0.f;
}

// ---------------------------------------------------------------------------------- risk
// 16-B granule u of the [32, kBK] chunk of P at column k0: row m0 + u / 8, floats 4 (u % 8) ..;
// rows past B read zero (Lk % kBK == 0: the columns are always inside the padded row)
__device__ __forceinline__ uint4 p_tile_ld(const float* __restrict__ probs, int m0, int B, int Lk, int k0, int u) {
  const int r = m0 + u / (kBK / 4), k = k0 + 4 * (u % (kBK / 4));
  if (r < B) return hvk_ld16(probs + (size_t)HVK_BCHECK(r, B) * Lk + HVK_BCHECK(k, Lk));
  return make_uint4(0, 0, 0, 0);
}

// 16-B granule u of the [128, kBK] byte chunk of D at column k0: class c0 + u / 2, bytes
// 16 (u % 2) ..; classes and columns past L read zero and nothing outside [L, L] is touched.
// ALIGNED (base and L multiples of 16): a granule is all inside or all outside, one 16-B load.
template <bool ALIGNED>
__device__ __forceinline__ uint4 d_tile_ld(const unsigned char* __restrict__ D, int c0, int L, int k0, int u) {
  const int c = c0 + u / 2, k = k0 + 16 * (u % 2);
  uint4 v = make_uint4(0, 0, 0, 0);
  if (c >= L || k >= L) return v;
  const unsigned char* src = D + (size_t)HVK_BCHECK(c, L) * L + k;
  if constexpr (ALIGNED) {
    v = hvk_ld16(src);
  } else {
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    const int n = L - k < 16 ? L - k : 16;
#pragma unroll
    for (int e = 0; e < 16; ++e)
      if (e < n) w[e >> 2] |= (uint32_t)src[e] << (8 * (e & 3));
    v = make_uint4(w[0], w[1], w[2], w[3]);
  }
  return v;
}

// byte e of a dword as f32: with e a constant the backend selects v_cvt_f32_ubyte<e>
__device__ __forceinline__ float ubyte(uint32_t w, int e) { return (float)((w >> (8 * e)) & 0xffu); }

template <bool ALIGNED>
__global__ __launch_bounds__(kThreads) void crm_risk_kernel(const float* __restrict__ probs, int B, int L, int Lk,
                                                           const unsigned char* __restrict__ D,
                                                           float* __restrict__ pmin, int* __restrict__ pidx) {
  __shared__ __attribute__((aligned(16))) float ps[2][kBM * kPLd];
  __shared__ __attribute__((aligned(16))) unsigned char ds[2][kBN * kDLd];
  __shared__ float xmin[kWaves][kBM];
  __shared__ int xidx[kWaves][kBM];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int tile = blockIdx.x, m0 = blockIdx.y * kBM, c0 = tile * kBN;
  const int chunks = Lk / kBK;

  hvk_f32x4 acc[2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n) acc[m][n] = hvk_f32x4{0.f, 0.f, 0.f, 0.f};

  uint4 pr[kPU], dr;
  const auto fetch = [&](int ch) {
#pragma unroll
    for (int u = 0; u < kPU; ++u) pr[u] = p_tile_ld(probs, m0, B, Lk, ch * kBK, tid + u * kThreads);
    dr = d_tile_ld<ALIGNED>(D, c0, L, ch * kBK, tid);
  };
  const auto stage = [&](int buf) {
#pragma unroll
    for (int u = 0; u < kPU; ++u) {
      const int gi = tid + u * kThreads;
      *reinterpret_cast<uint4*>(&ps[buf][(gi / (kBK / 4)) * kPLd + 4 * (gi % (kBK / 4))]) = pr[u];
    }
    *reinterpret_cast<uint4*>(&ds[buf][(tid / 2) * kDLd + 16 * (tid % 2)]) = dr;
  };
  fetch(0);
  stage(0);
  __syncthreads();
  for (int ch = 0; ch < chunks; ++ch) {
    const int buf = ch & 1;
    if (ch + 1 < chunks) fetch(ch + 1);  // in flight over this chunk's MFMAs
    hvk_f32x4 a[2][2];
    uint2 bq[2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int h = 0; h < 2; ++h)
        a[m][h] = *reinterpret_cast<const hvk_f32x4*>(&ps[buf][(m * 16 + li) * kPLd + 8 * g + 4 * h]);
#pragma unroll
    for (int n = 0; n < 2; ++n)
      bq[n] = *reinterpret_cast<const uint2*>(&ds[buf][(wave * 32 + n * 16 + li) * kDLd + 8 * g]);
    // step s: k = 8 g + s in both operands, the four lane groups covering 32 columns in 8 steps
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      float bf[2];
#pragma unroll
      for (int n = 0; n < 2; ++n) bf[n] = ubyte(s < 4 ? bq[n].x : bq[n].y, s & 3);
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
          acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m][s >> 2][s & 3], bf[n], acc[m][n], 0, 0, 0);
    }
    // the other buffer's readers finished before the barrier that ended the previous chunk
    if (ch + 1 < chunks) stage(buf ^ 1);
    __syncthreads();
  }
  hvk_settle(acc[0][0], acc[0][1], acc[1][0], acc[1][1]);

  // D lane l: row 4 (l >> 4) + r, column l & 15 of each 16-class block n, ascending class order:
  // a strict compare keeps the lowest class among equal risks
  float best[2][4];
  int bidx[2][4];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      best[m][r] = INFINITY;
      bidx[m][r] = kNoIdx;
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        const int c = c0 + wave * 32 + n * 16 + li;
        const float v = acc[m][n][r];
        if (c < L && v < best[m][r]) {  // a column past L holds 0, not a risk
          best[m][r] = v;
          bidx[m][r] = c;
        }
      }
      take_min16(best[m][r], bidx[m][r]);
      if (li == 0) {
        const int row = m * 16 + 4 * g + r;
        xmin[wave][row] = best[m][r];
        xidx[wave][row] = bidx[m][r];
      }
    }
  __syncthreads();
  if (tid < kBM && m0 + tid < B) {
    float v = xmin[0][tid];
    int vi = xidx[0][tid];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) take_min(v, vi, xmin[w][tid], xidx[w][tid]);
    pmin[(size_t)tile * B + HVK_BCHECK(m0 + tid, B)] = v;
    pidx[(size_t)tile * B + m0 + tid] = vi;
  }
}

// ---------------------------------------------------------------------------------- finalize
__global__ __launch_bounds__(kThreads) void crm_finalize_kernel(const float* __restrict__ pmin,
                                                               const int* __restrict__ pidx, int B, int L, int tiles,
                                                               const int64_t* __restrict__ targets, int t_stride,
                                                               int t_off, const unsigned char* __restrict__ D,
                                                               int* __restrict__ pred, float* __restrict__ risk,
                                                               int* __restrict__ dist, double* state) {
  const int tid = threadIdx.x;
  double v[2] = {0.0, 0.0};  // hits, sum of distances
  for (int b = tid; b < B; b += kThreads) {
    float m = INFINITY;
    int mi = kNoIdx;
    for (int s = 0; s < tiles; ++s) take_min(m, mi, pmin[(size_t)s * B + b], pidx[(size_t)s * B + b]);
    const int p = (mi >= 0 && mi < L) ? mi : 0;  // nothing compared (a NaN row): class 0
    const int64_t t = targets[(size_t)b * t_stride + t_off];
    int d = -1;
    if (t >= 0 && t < L) {
      d = D[(size_t)HVK_BCHECK(p, L) * L + t];
      v[0] += p == t ? 1.0 : 0.0;
      v[1] += (double)d;
    }
    pred[HVK_BCHECK(b, B)] = p;
    risk[b] = m;
    dist[b] = d;
  }
  __shared__ double part[kWaves][2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const double x = wave_sum_ordered(v[i], tid);
    if ((tid & 63) == 0) part[tid >> 6][i] = x;
  }
  __syncthreads();
  if (tid < 2) {
    double x = part[0][tid];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) x += part[w][tid];
    state[13 + tid] += x;
  }
}

struct CrmPlan {
  int Lk, tiles, row_tiles;
  size_t probs_bytes, bytes;
};
CrmPlan crm_plan(int B, int L) {
  CrmPlan p;
  p.Lk = ceil_div(L, kBK) * kBK;
  p.tiles = ceil_div(L, kBN);
  p.row_tiles = ceil_div(B, kBM);
  p.probs_bytes = (size_t)B * p.Lk * sizeof(float);
  p.bytes = p.probs_bytes + (size_t)p.tiles * B * (sizeof(float) + sizeof(int));
  return p;
}

}  // namespace

extern "C" {

int hvk_tree_dist_matrix(const int* leaf_paths, int L, unsigned char* out, void* stream) {
  if (L < 1 || L > kMaxL) return hvk_set_error(HVK_EINVAL, "hvk_tree_dist_matrix: bad shape (L %d: 1 <= L <= 2^20)", L);
  if (!leaf_paths || !out) return hvk_set_error(HVK_EINVAL, "hvk_tree_dist_matrix: null pointer");
  const size_t groups = ((size_t)L * L + 15) / 16;
  hipLaunchKernelGGL(tree_dist_kernel, dim3((unsigned)((groups + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), leaf_paths, L, out, ((uintptr_t)out & 15) == 0 ? 1 : 0);
  HVK_CHECK_LAUNCH("tree_dist");
  return HVK_OK;
}

size_t hvk_crm_workspace(int B, int L) {
  if (B < 1 || L < 1 || L > kMaxL) return 0;
  return crm_plan(B, L).bytes;
}

int hvk_crm_predict(const void* logits, int logits_dtype, int B, int L, int ld, const int64_t* targets, int t_stride,
                    int t_off, const unsigned char* tree_dists, int* pred, float* risk, int* dist, double* state,
                    void* workspace, size_t workspace_bytes, void* stream) {
  if (B < 0 || L < 1 || ld < L || L > kMaxL)
    return hvk_set_error(HVK_EINVAL, "hvk_crm_predict: bad shape (B %d, L %d, ld %d: B >= 0, 1 <= L <= 2^20, ld >= L)",
                         B, L, ld);
  if (t_stride < 1 || t_off < 0 || t_off >= t_stride)
    return hvk_set_error(HVK_EINVAL, "hvk_crm_predict: target stride %d / offset %d", t_stride, t_off);
  if (logits_dtype != 0 && logits_dtype != 1)
    return hvk_set_error(HVK_EINVAL, "hvk_crm_predict: unknown logits dtype %d (0 f32, 1 bf16)", logits_dtype);
  if (!logits || !targets || !tree_dists || !pred || !risk || !dist || !state)
    return hvk_set_error(HVK_EINVAL, "hvk_crm_predict: null pointer");
  if (B == 0) return HVK_OK;
  const CrmPlan p = crm_plan(B, L);
  if (!workspace || workspace_bytes < p.bytes)
    return hvk_set_error(HVK_EINVAL, "hvk_crm_predict: workspace of %zu bytes, %zu needed (null pointer or small)",
                         workspace ? workspace_bytes : (size_t)0, p.bytes);
  if ((uintptr_t)workspace & 15) return hvk_set_error(HVK_EINVAL, "hvk_crm_predict: workspace must be 16-byte aligned");
  if (p.row_tiles > 65535) return hvk_set_error(HVK_EUNSUPPORTED, "hvk_crm_predict: %d row tiles (B %d)", p.row_tiles, B);
  float* probs = static_cast<float*>(workspace);
  float* pmin = probs + (size_t)B * p.Lk;
  int* pidx = reinterpret_cast<int*>(pmin + (size_t)p.tiles * B);
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(crm_probs_kernel, dim3(B), dim3(kThreads), 0, st, logits, logits_dtype, L, ld, p.Lk, probs);
  HVK_CHECK_LAUNCH("crm_probs");
  const dim3 grid(p.tiles, p.row_tiles);
  if ((((uintptr_t)tree_dists | (uintptr_t)L) & 15) == 0)
    hipLaunchKernelGGL(crm_risk_kernel<true>, grid, dim3(kThreads), 0, st, static_cast<const float*>(probs), B, L,
                       p.Lk, tree_dists, pmin, pidx);
  else
    hipLaunchKernelGGL(crm_risk_kernel<false>, grid, dim3(kThreads), 0, st, static_cast<const float*>(probs), B, L,
                       p.Lk, tree_dists, pmin, pidx);
  HVK_CHECK_LAUNCH("crm_risk");
  hipLaunchKernelGGL(crm_finalize_kernel, dim3(1), dim3(kThreads), 0, st, static_cast<const float*>(pmin),
                     static_cast<const int*>(pidx), B, L, p.tiles, targets, t_stride, t_off, tree_dists, pred, risk,
                     dist, state);
  HVK_CHECK_LAUNCH("crm_finalize");
  return HVK_OK;
}

}  // extern "C"
