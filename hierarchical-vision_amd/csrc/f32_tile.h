// The 64 x 64 x 32 tile on the f32-input MFMA (16x16x4) of the evaluation kernels: ss_flat_kernel
// (simpleshot.hip), lp_fwd_kernel and lp_bwd_kernel (linear_probe.hip).  A 256-thread workgroup
// holds 64 rows of A against 64 rows of B, both row-major over the contraction index and staged
// through LDS in 32-column chunks; wave w owns rows 16 w .. 16 w + 15 of A against all 64 of B.
//
// The result, acc[j] for the 16-row block j of B: lane l holds, in element r, row 4 (l >> 4) + r
// of the wave's 16 rows of A against row l & 15 of block j.
#pragma once
#include "eval_common.h"

namespace hvk_f32_tile {

using hvk_eval::kThreads;

constexpr int kBM = 64;       // rows of A per workgroup: 16 per wave
constexpr int kBN = 64;       // rows of B per tile: 4 accumulators per wave
constexpr int kBK = 32;       // contraction elements per LDS chunk
constexpr int kLd = kBK + 4;  // LDS row stride in floats: rows 0..15 start in 16 distinct 4-bank groups
constexpr int kGr = kBK / 4;  // 16-B granules per tile row
constexpr int kU = kBM * kGr / kThreads;  // granules per thread and tile
static_assert(kBM == kBN && kBM * kGr % kThreads == 0 && kBK % 16 == 0 && kLd % 8 == 4, "tile staging");

// four consecutive floats at (r, k) of a dense [rows, D] matrix; past the rows or the columns: 0.
// vec: D % 4 == 0 and a 16-byte aligned base, so the four are one aligned granule.
__device__ __forceinline__ uint4 ld4(const float* base, int r, int rows, int k, int D, int vec) {
  uint4 v = make_uint4(0, 0, 0, 0);
  if (r >= rows || k >= D) return v;
  const float* p = base + (size_t)HVK_BCHECK(r, rows) * D + k;
  if (vec) return hvk_ld16(p);
  v.x = __float_as_uint(p[0]);
  if (k + 1 < D) v.y = __float_as_uint(p[1]);
  if (k + 2 < D) v.z = __float_as_uint(p[2]);
  if (k + 3 < D) v.w = __float_as_uint(p[3]);
  return v;
}

// 16-B granule g of the [64, kBK] chunk at (r0, k0): row g / kGr, columns 4 (g % kGr) ..
__device__ __forceinline__ uint4 tile_ld(const float* base, int r0, int rows, int k0, int D, int vec, int g) {
  return ld4(base, r0 + g / kGr, rows, k0 + 4 * (g % kGr), D, vec);
}

// acc += one staged chunk: as, bs are [64][kLd] LDS images.  16 columns per step: lane group g
// holds columns 4g .. 4g + 3 of both operands and feeds element s to the s-th MFMA, so A and B
// agree on k in every lane (the k order inside the 16 is a permutation; a dot product does not
// care)
__device__ __forceinline__ void mfma_chunk(const float* as, const float* bs, int tid, hvk_f32x4 (&acc)[4]) {
  const int lane = tid & 63, wave = tid >> 6, li = lane & 15, g = lane >> 4;
#pragma unroll
  for (int kk = 0; kk < kBK; kk += 16) {
    const hvk_f32x4 a = *reinterpret_cast<const hvk_f32x4*>(&as[(wave * 16 + li) * kLd + kk + 4 * g]);
    hvk_f32x4 bq[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) bq[j] = *reinterpret_cast<const hvk_f32x4*>(&bs[(j * 16 + li) * kLd + kk + 4 * g]);
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], bq[j][s], acc[j], 0, 0, 0);
  }
}

// acc = A[a0 .. a0 + 63] . B[b0 .. b0 + 63]^T over all D columns of two dense [rows, D] operands
// (rows past arows / brows count as zero), settled: the caller may read acc at once
__device__ __forceinline__ void sweep(const float* A, int a0, int arows, const float* B, int b0, int brows, int D,
                                      int vec, float* as, float* bs, int tid, hvk_f32x4 (&acc)[4]) {
  const int chunks = hvk_eval::ceil_div(D, kBK);
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = hvk_f32x4{0.f, 0.f, 0.f, 0.f};
  // chunk 0 into registers; inside the loop the next chunk's loads fly over this chunk's MFMAs
  uint4 ar[kU], br[kU];
#pragma unroll
  for (int u = 0; u < kU; ++u) {
    ar[u] = tile_ld(A, a0, arows, 0, D, vec, tid + u * kThreads);
    br[u] = tile_ld(B, b0, brows, 0, D, vec, tid + u * kThreads);
  }
  for (int ch = 0; ch < chunks; ++ch) {
    __syncthreads();  // the previous chunk's readers are done
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int gi = tid + u * kThreads;
      *reinterpret_cast<uint4*>(&as[(gi / kGr) * kLd + 4 * (gi % kGr)]) = ar[u];
      *reinterpret_cast<uint4*>(&bs[(gi / kGr) * kLd + 4 * (gi % kGr)]) = br[u];
    }
    __syncthreads();
    if (ch + 1 < chunks) {
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        ar[u] = tile_ld(A, a0, arows, (ch + 1) * kBK, D, vec, tid + u * kThreads);
        br[u] = tile_ld(B, b0, brows, (ch + 1) * kBK, D, vec, tid + u * kThreads);
      }
    }
    mfma_chunk(as, bs, tid, acc);
  }
  hvk_settle(acc[0], acc[1], acc[2], acc[3]);
}

}  // namespace hvk_f32_tile
