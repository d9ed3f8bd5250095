// Linear-probe evaluation on gfx950 (linear_probe.py:189-234): StandardScaler and the one-vs-rest
// logistic classifier, fitted as the minimiser of sklearn's objective by full-batch accelerated
// gradient with all R binary problems in lock-step.
//
// * lp_moments_kernel / lp_standardize_kernel -- StandardScaler: one thread per column adds the
//   batch's rows to float64 sum / sum of squares in ascending row order (one writer per column, so
//   any split into consecutive batches leaves the same bits); (x - mean) * inv_std in f32.
// * lp_fwd_kernel -- z = xs . W^T + b on the f32-input MFMA (16x16x4), the 64 x 64 tile of
//   ss_flat_kernel (simpleshot.hip): a workgroup holds 64 rows against a range of 64-class tiles.
//   MODE 0 turns the scores into residuals sigma(z) - [label == target] that go to a workspace of
//   one row chunk ([chunk rows, R padded to 64]; masked rows, padded rows and padded classes are
//   zero) and into per-(row tile, class) float64 sums of the loss terms and residuals; MODE 1 stores
//   the scores (decision_function).
// * lp_bwd_kernel -- partial dW = residual^T . xs of one row chunk: a workgroup owns a 64-class x
//   64-column tile and a fixed range of the chunk's rows, both operands staged transposed in LDS so
//   that the MFMA loop is the forward's.  Row splits write their own slab; chunk after chunk adds
//   to it in stream order (one writer per cell).
// * lp_chunk_reduce_kernel / lp_count_kernel / lp_finish_kernel -- the row tiles' float64 partials
//   in ascending order, the rows outside the held-out fold, and dW = (sum of slabs in ascending
//   order) / N_eff + alpha W, db, loss.
// * lp_step_kernel -- one workgroup per binary problem: the accelerated-gradient update with the
//   gradient restart of O'Donoghue & Candes.
// No atomics anywhere: equal inputs give bit-identical outputs.
#include <math.h>

#include "hvk_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

constexpr int ceil_div(int a, int b) { return a / b + (a % b != 0 ? 1 : 0); }

// ---------------------------------------------------------------------------------- scaler
__global__ __launch_bounds__(64) void lp_moments_kernel(const float* __restrict__ x, int B, int D, int ld,
                                                       double* sum, double* sumsq, long long* count) {
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k == 0 && count) *count += B;
  if (k >= D) return;
  double s = sum[k], q = sumsq[k];
  for (int r = 0; r < B; ++r) {
    const double v = (double)x[(size_t)HVK_BCHECK(r, B) * ld + k];
    s += v;
    q += v * v;  // the product of two f32 is exact in float64: fused or not, one rounding
  }
  sum[k] = s;
  sumsq[k] = q;
}

__global__ __launch_bounds__(kThreads) void lp_standardize_kernel(const float* __restrict__ x, int B, int D, int ld,
                                                                 const double* __restrict__ sum,
                                                                 const double* __restrict__ sumsq, double n,
                                                                 float* __restrict__ out, float* __restrict__ mean,
                                                                 float* __restrict__ inv_std) {
  const int k = blockIdx.x * kThreads + threadIdx.x;
  if (k >= D) return;
  const double m = sum[k] / n;
  const double var = sumsq[k] / n - m * m;
  const double sc = var > 0.0 ? sqrt(var) : 1.0;  // a constant column (variance 0) keeps its scale
  const float mf = (float)m, is = (float)(1.0 / sc);
  if (blockIdx.y == 0) {
    mean[k] = mf;
    inv_std[k] = is;
  }
  for (int r = blockIdx.y; r < B; r += gridDim.y) out[(size_t)HVK_BCHECK(r, B) * D + k] = (x[(size_t)r * ld + k] - mf) * is;
}

// ---------------------------------------------------------------------------------- forward tile
constexpr int kBM = 64;       // rows per workgroup: 16 per wave
constexpr int kBN = 64;       // classes per tile: 4 accumulators per wave
constexpr int kBK = 32;       // contraction elements per LDS stage
constexpr int kLd = kBK + 4;  // LDS row stride in floats (simpleshot.hip)
constexpr int kGr = kBK / 4;  // 16-B granules per tile row
constexpr int kU = kBM * kGr / kThreads;
static_assert(kBM == kBN && kBM * kGr % kThreads == 0 && kBK % 16 == 0 && kLd % 8 == 4, "tile staging");

// four consecutive floats at (r, k) of a dense [rows, D] matrix; past the rows or the columns: 0.
// vec: D % 4 == 0 and a 16-byte aligned base, so the four are one aligned granule.
__device__ __forceinline__ uint4 lp_ld(const float* base, int r, int rows, int k, int D, int vec) {
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

__device__ __forceinline__ uint4 lp_tile_ld(const float* base, int r0, int rows, int k0, int D, int vec, int g) {
  return lp_ld(base, r0 + g / kGr, rows, k0 + 4 * (g % kGr), D, vec);
}

struct FwdArgs {
  const float* xs;   // [N, D]
  const float* W;    // [R, D]
  const float* b;    // [R]
  int N, D, R, vec;
  int tiles_per_split;
  // MODE 0
  const int64_t* labels;      // [N]
  const unsigned char* fold;  // [N] or null
  int skip_fold;
  const int* target;  // [R]
  int n0, n_end;      // the chunk's rows [n0, n_end)
  float* res;         // [ceil64(chunk rows), Rp]
  int Rp;
  double* lossp;  // [row tiles, Rp]
  double* dbp;    // [row tiles, Rp]
  // MODE 1
  float* out;  // [N, R]
};

template <int MODE>
__global__ __launch_bounds__(kThreads) void lp_fwd_kernel(FwdArgs a) {
  __shared__ __attribute__((aligned(16))) float xs[kBM * kLd];
  __shared__ __attribute__((aligned(16))) float cs[kBN * kLd];
  __shared__ double part[2][kWaves][kBN];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int m0 = (MODE == 0 ? a.n0 : 0) + blockIdx.x * kBM, split = blockIdx.y;
  const int D = a.D;
  const int tiles = ceil_div(a.R, kBN);
  const int t_lo = split * a.tiles_per_split;
  const int t_hi = t_lo + a.tiles_per_split < tiles ? t_lo + a.tiles_per_split : tiles;
  const int chunks = ceil_div(D, kBK);

  // this lane's four rows: 16 wave + 4 g + r
  int64_t lab[4] = {0, 0, 0, 0};
  bool live[4] = {false, false, false, false};
  if (MODE == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = m0 + wave * 16 + 4 * g + r;
      if (row < a.n_end) {
        lab[r] = a.labels[HVK_BCHECK(row, a.N)];
        live[r] = !(a.fold && (int)a.fold[row] == a.skip_fold);
      }
    }
  }

  for (int t = t_lo; t < t_hi; ++t) {
    const int c0 = t * kBN;
    hvk_f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = hvk_f32x4{0.f, 0.f, 0.f, 0.f};
    uint4 xr[kU], cr[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      xr[u] = lp_tile_ld(a.xs, m0, a.N, 0, D, a.vec, tid + u * kThreads);
      cr[u] = lp_tile_ld(a.W, c0, a.R, 0, D, a.vec, tid + u * kThreads);
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
          xr[u] = lp_tile_ld(a.xs, m0, a.N, (ch + 1) * kBK, D, a.vec, tid + u * kThreads);
          cr[u] = lp_tile_ld(a.W, c0, a.R, (ch + 1) * kBK, D, a.vec, tid + u * kThreads);
        }
      }
      // lane group g holds columns 4g .. 4g + 3 of both operands and feeds element s to the s-th
      // MFMA: A and B agree on k in every lane (simpleshot.hip)
#pragma unroll
      for (int kk = 0; kk < kBK; kk += 16) {
        const hvk_f32x4 av = *reinterpret_cast<const hvk_f32x4*>(&xs[(wave * 16 + li) * kLd + kk + 4 * g]);
        hvk_f32x4 bq[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          bq[j] = *reinterpret_cast<const hvk_f32x4*>(&cs[(j * 16 + li) * kLd + kk + 4 * g]);
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], bq[j][s], acc[j], 0, 0, 0);
      }
    }
    hvk_settle(acc[0], acc[1], acc[2], acc[3]);
    // D lane l: row 4 (l >> 4) + r, column l & 15 of each 16-class block j
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = c0 + j * 16 + li;
      const bool cv = c < a.R;
      const float bias = cv ? a.b[HVK_BCHECK(cv ? c : 0, a.R)] : 0.f;
      if (MODE == 1) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = m0 + wave * 16 + 4 * g + r;
          if (cv && row < a.N) a.out[(size_t)HVK_BCHECK(row, a.N) * a.R + c] = acc[j][r] + bias;
        }
      } else {
        const int tg = cv ? a.target[c] : -1;
        double ls = 0.0, rs = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int lrow = blockIdx.x * kBM + wave * 16 + 4 * g + r;  // row of the chunk
          const float z = acc[j][r] + bias;
          const bool y = cv && lab[r] == (int64_t)tg;
          // e <= 1: neither sigma nor softplus overflows at any z
          const float e = expf(-fabsf(z));
          const float inv = 1.f / (1.f + e);
          const float sig = z >= 0.f ? inv : e * inv;
          const bool on = cv && live[r];
          const float resid = on ? sig - (y ? 1.f : 0.f) : 0.f;
          const float term = on ? fmaxf(y ? -z : z, 0.f) + log1pf(e) : 0.f;  // log(1 + exp(-y z))
          a.res[(size_t)lrow * a.Rp + c] = resid;  // c < Rp, lrow < ceil64(chunk rows)
          ls += (double)term;
          rs += (double)resid;
        }
        // the four lane groups hold rows 4g ..: a + b == b + a, every lane ends with the same bits
        ls += __shfl_xor(ls, 16);
        ls += __shfl_xor(ls, 32);
        rs += __shfl_xor(rs, 16);
        rs += __shfl_xor(rs, 32);
        if (g == 0) {
          part[0][wave][j * 16 + li] = ls;
          part[1][wave][j * 16 + li] = rs;
        }
      }
    }
    if (MODE == 0) {
      __syncthreads();
      if (tid < kBN) {
        const size_t o = (size_t)blockIdx.x * a.Rp + c0 + tid;
        a.lossp[o] = (part[0][0][tid] + part[0][1][tid]) + (part[0][2][tid] + part[0][3][tid]);
        a.dbp[o] = (part[1][0][tid] + part[1][1][tid]) + (part[1][2][tid] + part[1][3][tid]);
      }
      // the next tile writes `part` only after the two barriers of its first stage
    }
  }
}

// lossacc / dbacc [Rp] (+)= the chunk's row tiles in ascending order
__global__ __launch_bounds__(kThreads) void lp_chunk_reduce_kernel(const double* __restrict__ lossp,
                                                                  const double* __restrict__ dbp, int row_tiles,
                                                                  int Rp, double* lossacc, double* dbacc, int first) {
  const int c = blockIdx.x * kThreads + threadIdx.x;
  if (c >= Rp) return;
  double l = 0.0, d = 0.0;
  for (int t = 0; t < row_tiles; ++t) {
    l += lossp[(size_t)t * Rp + c];
    d += dbp[(size_t)t * Rp + c];
  }
  lossacc[c] = first ? l : lossacc[c] + l;
  dbacc[c] = first ? d : dbacc[c] + d;
}

__global__ __launch_bounds__(kThreads) void lp_count_kernel(const unsigned char* __restrict__ fold, int skip_fold,
                                                           int N, long long* n_eff) {
  __shared__ long long part[kWaves];
  const int tid = threadIdx.x;
  long long n = 0;
  for (int i = tid; i < N; i += kThreads) n += (int)fold[i] != skip_fold ? 1 : 0;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) n += __shfl_xor(n, o);
  if ((tid & 63) == 0) part[tid >> 6] = n;
  __syncthreads();
  if (tid == 0) *n_eff = part[0] + part[1] + part[2] + part[3];
}

// ---------------------------------------------------------------------------------- backward tile
// dWp[split][c0 .. c0 + 63][d0 .. d0 + 63] (+)= sum over the split's rows k of res[k][c] xs[n0 + k][d]
__global__ __launch_bounds__(kThreads) void lp_bwd_kernel(const float* __restrict__ res, int Rp,
                                                         const float* __restrict__ xs, int N, int D, int vec, int n0,
                                                         int rows_p, int steps_per_split, float* dWp, int Dp,
                                                         int accumulate) {
  __shared__ __attribute__((aligned(16))) float rt[kBN * kLd];  // [class][row]
  __shared__ __attribute__((aligned(16))) float xt[kBN * kLd];  // [column][row]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int c0 = blockIdx.x * kBN, d0 = blockIdx.y * kBN, split = blockIdx.z;
  const int k_lo = split * steps_per_split * kBK;
  int k_hi = k_lo + steps_per_split * kBK;
  k_hi = k_hi < rows_p ? k_hi : rows_p;  // rows_p % 64 == 0: whole stages

  hvk_f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = hvk_f32x4{0.f, 0.f, 0.f, 0.f};
  // a [kBK rows, 64] stage of each operand: granule gi is row gi / 16, columns 4 (gi % 16) ..
  constexpr int kG = kBN / 4, kV = kBK * kG / kThreads;
  uint4 rr[kV], xr[kV];
  if (k_lo < k_hi) {
#pragma unroll
    for (int u = 0; u < kV; ++u) {
      const int gi = tid + u * kThreads, row = gi / kG, col = 4 * (gi % kG);
      rr[u] = hvk_ld16(res + (size_t)(k_lo + row) * Rp + c0 + col);
      xr[u] = lp_ld(xs, n0 + k_lo + row, N, d0 + col, D, vec);
    }
  }
  for (int k = k_lo; k < k_hi; k += kBK) {
    __syncthreads();
#pragma unroll
    for (int u = 0; u < kV; ++u) {
      const int gi = tid + u * kThreads, row = gi / kG, col = 4 * (gi % kG);
      rt[(col + 0) * kLd + row] = __uint_as_float(rr[u].x);
      rt[(col + 1) * kLd + row] = __uint_as_float(rr[u].y);
      rt[(col + 2) * kLd + row] = __uint_as_float(rr[u].z);
      rt[(col + 3) * kLd + row] = __uint_as_float(rr[u].w);
      xt[(col + 0) * kLd + row] = __uint_as_float(xr[u].x);
      xt[(col + 1) * kLd + row] = __uint_as_float(xr[u].y);
      xt[(col + 2) * kLd + row] = __uint_as_float(xr[u].z);
      xt[(col + 3) * kLd + row] = __uint_as_float(xr[u].w);
    }
    __syncthreads();
    if (k + kBK < k_hi) {
#pragma unroll
      for (int u = 0; u < kV; ++u) {
        const int gi = tid + u * kThreads, row = gi / kG, col = 4 * (gi % kG);
        rr[u] = hvk_ld16(res + (size_t)(k + kBK + row) * Rp + c0 + col);
        xr[u] = lp_ld(xs, n0 + k + kBK + row, N, d0 + col, D, vec);
      }
    }
#pragma unroll
    for (int kk = 0; kk < kBK; kk += 16) {
      const hvk_f32x4 av = *reinterpret_cast<const hvk_f32x4*>(&rt[(wave * 16 + li) * kLd + kk + 4 * g]);
      hvk_f32x4 bq[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) bq[j] = *reinterpret_cast<const hvk_f32x4*>(&xt[(j * 16 + li) * kLd + kk + 4 * g]);
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], bq[j][s], acc[j], 0, 0, 0);
    }
  }
  hvk_settle(acc[0], acc[1], acc[2], acc[3]);
  // D lane l: class 16 wave + 4 (l >> 4) + r of the tile, column 16 j + (l & 15); the slab is
  // padded to [Rp, Dp]: no store leaves it
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const size_t o = ((size_t)split * Rp + c0 + wave * 16 + 4 * g + r) * Dp + d0 + j * 16 + li;
      dWp[o] = accumulate ? dWp[o] + acc[j][r] : acc[j][r];
    }
}

__global__ __launch_bounds__(kThreads) void lp_finish_kernel(const float* __restrict__ dWp, int splits, int Rp,
                                                            int Dp, const double* __restrict__ lossacc,
                                                            const double* __restrict__ dbacc,
                                                            const long long* __restrict__ n_eff, int N,
                                                            const float* __restrict__ W,
                                                            const float* __restrict__ alpha, int R, int D,
                                                            float* __restrict__ dW, float* __restrict__ db,
                                                            double* __restrict__ loss) {
  __shared__ double part[kWaves];
  const int r = blockIdx.x, tid = threadIdx.x;
  const long long n = n_eff ? *n_eff : (long long)N;
  const float nf = (float)n, al = alpha[r];
  double ww = 0.0;
  for (int d = tid; d < D; d += kThreads) {
    float s = 0.f;
    for (int sp = 0; sp < splits; ++sp) s += dWp[((size_t)sp * Rp + r) * Dp + d];
    const float w = W[(size_t)HVK_BCHECK(r, R) * D + d];
    dW[(size_t)r * D + d] = n > 0 ? __builtin_fmaf(al, w, s / nf) : al * w;
    ww += (double)w * (double)w;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) ww += __shfl_xor(ww, o);
  if ((tid & 63) == 0) part[tid >> 6] = ww;
  __syncthreads();
  if (tid == 0) {
    ww = (part[0] + part[1]) + (part[2] + part[3]);
    db[r] = n > 0 ? (float)(dbacc[r] / (double)n) : 0.f;
    loss[r] = (n > 0 ? lossacc[r] / (double)n : 0.0) + 0.5 * (double)al * ww;
  }
}

// the plan of hvk_lp_loss_grad, a function of (N, D, R) alone
constexpr size_t kResBudget = (size_t)128 << 20;  // bytes of residuals per row chunk
constexpr int kMaxChunk = 8192;                   // rows per chunk at most
struct LpPlan {
  int Rp, Dp, ctiles, dtiles, CH, tiles_per_split, csplits, S, steps_per_split;
  size_t off_res, off_dwp, off_lossp, off_dbp, off_lossacc, off_dbacc, off_neff, bytes;
};
void fwd_split(int row_tiles, int ctiles, int* tiles_per_split, int* csplits) {
  int want = 1024 / (row_tiles > 0 ? row_tiles : 1);
  want = want < 1 ? 1 : (want > ctiles ? ctiles : want);
  *tiles_per_split = ceil_div(ctiles, want);
  *csplits = ceil_div(ctiles, *tiles_per_split);
}
LpPlan lp_plan(int N, int D, int R) {
  LpPlan p;
  p.ctiles = ceil_div(R, kBN);
  p.dtiles = ceil_div(D, kBN);
  p.Rp = p.ctiles * kBN;
  p.Dp = p.dtiles * kBN;
  size_t ch = kResBudget / ((size_t)p.Rp * 4) / 64 * 64;
  ch = ch > (size_t)kMaxChunk ? kMaxChunk : (ch < 64 ? 64 : ch);
  const int n64 = ceil_div(N, 64) * 64;  // N <= 2^31 - 64 (checked)
  p.CH = (int)ch < n64 ? (int)ch : n64;
  fwd_split(p.CH / 64, p.ctiles, &p.tiles_per_split, &p.csplits);
  // row splits of the backward: about 1024 workgroups in all
  const long long tiles2 = (long long)p.ctiles * p.dtiles;
  int want = tiles2 >= 1024 ? 1 : (int)(1024 / tiles2);
  const int steps = p.CH / kBK;
  want = want > steps ? steps : want;
  p.steps_per_split = ceil_div(steps, want);
  p.S = ceil_div(steps, p.steps_per_split);
  size_t o = 0;
  auto take = [&o](size_t bytes) {
    const size_t at = o;
    o += (bytes + 255) / 256 * 256;
    return at;
  };
  p.off_res = take((size_t)p.CH * p.Rp * 4);
  p.off_dwp = take((size_t)p.S * p.Rp * p.Dp * 4);
  p.off_lossp = take((size_t)(p.CH / 64) * p.Rp * 8);
  p.off_dbp = take((size_t)(p.CH / 64) * p.Rp * 8);
  p.off_lossacc = take((size_t)p.Rp * 8);
  p.off_dbacc = take((size_t)p.Rp * 8);
  p.off_neff = take(8);
  p.bytes = o;
  return p;
}
constexpr int kMaxR = (int)(kResBudget / (64 * 4));  // 64 rows of residuals fit the budget
constexpr int kMaxN = 0x7fffffff - 64;

// ---------------------------------------------------------------------------------- step
__global__ __launch_bounds__(kThreads) void lp_step_kernel(float* W, float* b, float* Yw, float* Yb,
                                                          const float* __restrict__ dW,
                                                          const float* __restrict__ db, float* t,
                                                          const unsigned char* __restrict__ frozen, int D, float step,
                                                          float tol, float* __restrict__ gmax,
                                                          unsigned char* __restrict__ conv) {
  __shared__ double dpart[kWaves];
  __shared__ float mpart[kWaves];
  const int r = blockIdx.x, tid = threadIdx.x;
  if (frozen && frozen[r]) return;  // the whole workgroup: a problem without a positive row
  float* w = W + (size_t)r * D;
  float* yw = Yw + (size_t)r * D;
  const float* gw = dW + (size_t)r * D;
  double dot = 0.0;
  float gm = 0.f;
  for (int d = tid; d < D; d += kThreads) {
    const float gv = gw[d];
    const float xn = __builtin_fmaf(-step, gv, yw[d]);
    dot += (double)gv * (double)(xn - w[d]);
    gm = fmaxf(gm, fabsf(gv));
  }
  const float gb = db[r];
  if (tid == 0) {
    const float xn = __builtin_fmaf(-step, gb, Yb[r]);
    dot += (double)gb * (double)(xn - b[r]);
    gm = fmaxf(gm, fabsf(gb));
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    dot += __shfl_xor(dot, o);
    gm = fmaxf(gm, __shfl_xor(gm, o));
  }
  if ((tid & 63) == 0) {
    dpart[tid >> 6] = dot;
    mpart[tid >> 6] = gm;
  }
  __syncthreads();
  dot = (dpart[0] + dpart[1]) + (dpart[2] + dpart[3]);
  gm = fmaxf(fmaxf(mpart[0], mpart[1]), fmaxf(mpart[2], mpart[3]));
  // a NaN gradient hides in fmaxf: it shows as a NaN dot product and never counts as converged
  const bool done = gm <= tol && dot == dot;
  if (done) {
    // the iterate becomes the point the gradient was taken at, and stays there
    for (int d = tid; d < D; d += kThreads) w[d] = yw[d];
    if (tid == 0) {
      b[r] = Yb[r];
      gmax[r] = gm;
      conv[r] = 1;
    }
    return;
  }
  const bool restart = dot > 0.0;
  const float t0 = t[r];
  const float t1 = restart ? 1.f : 0.5f * (1.f + sqrtf(__builtin_fmaf(4.f * t0, t0, 1.f)));
  const float beta = restart ? 0.f : (t0 - 1.f) / t1;
  for (int d = tid; d < D; d += kThreads) {
    const float xn = __builtin_fmaf(-step, gw[d], yw[d]);
    yw[d] = __builtin_fmaf(beta, xn - w[d], xn);
    w[d] = xn;
  }
  if (tid == 0) {
    const float xn = __builtin_fmaf(-step, gb, Yb[r]);
    Yb[r] = __builtin_fmaf(beta, xn - b[r], xn);
    b[r] = xn;
    t[r] = t1;
    gmax[r] = dot == dot ? gm : NAN;
    conv[r] = 0;
  }
}

int vec_ok(int D, const void* a, const void* b) { return D % 4 == 0 && ((((uintptr_t)a | (uintptr_t)b) & 15) == 0); }

}  // namespace

extern "C" {

int hvk_lp_moments(const float* x, int B, int D, int ld, double* sum, double* sumsq, long long* count,
                   void* stream) {
  if (B < 0 || D < 1 || ld < D)
    return hvk_set_error(HVK_EINVAL, "hvk_lp_moments: bad shape (B %d, D %d, ld %d: B >= 0, D >= 1, ld >= D)", B, D,
                         ld);
  if (!x || !sum || !sumsq) return hvk_set_error(HVK_EINVAL, "hvk_lp_moments: null pointer");
  if (B == 0) return HVK_OK;
  hipLaunchKernelGGL(lp_moments_kernel, dim3(ceil_div(D, 64)), dim3(64), 0, static_cast<hipStream_t>(stream), x, B, D,
                     ld, sum, sumsq, count);
  HVK_CHECK_LAUNCH("lp_moments");
  return HVK_OK;
}

int hvk_lp_standardize(const float* x, int B, int D, int ld, const double* sum, const double* sumsq, long long n,
                       float* out, float* mean, float* inv_std, void* stream) {
  if (B < 0 || D < 1 || ld < D)
    return hvk_set_error(HVK_EINVAL, "hvk_lp_standardize: bad shape (B %d, D %d, ld %d: B >= 0, D >= 1, ld >= D)", B,
                         D, ld);
  if (n < 1) return hvk_set_error(HVK_EINVAL, "hvk_lp_standardize: bad shape (n %lld < 1 rows in the sums)", n);
  if (!sum || !sumsq || !mean || !inv_std || (B > 0 && (!x || !out)))
    return hvk_set_error(HVK_EINVAL, "hvk_lp_standardize: null pointer");
  const int gy = B < 1 ? 1 : (B < 256 ? B : 256);
  hipLaunchKernelGGL(lp_standardize_kernel, dim3(ceil_div(D, kThreads), gy), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), x, B, D, ld, sum, sumsq, (double)n, out, mean, inv_std);
  HVK_CHECK_LAUNCH("lp_standardize");
  return HVK_OK;
}

size_t hvk_lp_loss_grad_workspace(int N, int D, int R) {
  if (N < 1 || N > kMaxN || D < 1 || R < 1 || R > kMaxR) return 0;
  return lp_plan(N, D, R).bytes;
}

int hvk_lp_loss_grad(const float* xs, int N, int D, const int64_t* labels, const unsigned char* fold, int skip_fold,
                     const float* W, const float* b, const int* target, const float* alpha, int R, float* dW,
                     float* db, double* loss, void* workspace, size_t workspace_bytes, void* stream) {
  if (N < 1 || N > kMaxN || D < 1 || R < 1)
    return hvk_set_error(HVK_EINVAL, "hvk_lp_loss_grad: bad shape (N %d, D %d, R %d: 1 <= N <= 2^31 - 65, D >= 1, R >= 1)",
                         N, D, R);
  if (R > kMaxR) return hvk_set_error(HVK_EUNSUPPORTED, "hvk_lp_loss_grad: R %d > %d binary problems", R, kMaxR);
  if (!xs || !labels || !W || !b || !target || !alpha || !dW || !db || !loss)
    return hvk_set_error(HVK_EINVAL, "hvk_lp_loss_grad: null pointer");
  const LpPlan p = lp_plan(N, D, R);
  if (!workspace || workspace_bytes < p.bytes || ((uintptr_t)workspace & 15))
    return hvk_set_error(HVK_EINVAL,
                         "hvk_lp_loss_grad: workspace of %zu bytes, %zu needed (null pointer, small or not 16-byte aligned)",
                         workspace ? workspace_bytes : (size_t)0, p.bytes);
  if (p.dtiles > 65535 || p.csplits > 65535 || p.S > 65535)
    return hvk_set_error(HVK_EUNSUPPORTED, "hvk_lp_loss_grad: D %d gives %d column tiles", D, p.dtiles);
  char* ws = static_cast<char*>(workspace);
  float* res = reinterpret_cast<float*>(ws + p.off_res);
  float* dWp = reinterpret_cast<float*>(ws + p.off_dwp);
  double* lossp = reinterpret_cast<double*>(ws + p.off_lossp);
  double* dbp = reinterpret_cast<double*>(ws + p.off_dbp);
  double* lossacc = reinterpret_cast<double*>(ws + p.off_lossacc);
  double* dbacc = reinterpret_cast<double*>(ws + p.off_dbacc);
  long long* neff = reinterpret_cast<long long*>(ws + p.off_neff);
  hipStream_t st = static_cast<hipStream_t>(stream);
  FwdArgs a{};
  a.xs = xs; a.W = W; a.b = b; a.N = N; a.D = D; a.R = R;
  a.vec = vec_ok(D, xs, W);
  a.tiles_per_split = p.tiles_per_split;
  a.labels = labels; a.fold = fold; a.skip_fold = skip_fold; a.target = target;
  a.res = res; a.Rp = p.Rp; a.lossp = lossp; a.dbp = dbp; a.out = nullptr;
  for (int n0 = 0; n0 < N; n0 += p.CH) {
    const int rows = N - n0 < p.CH ? N - n0 : p.CH;
    const int row_tiles = ceil_div(rows, kBM);
    a.n0 = n0;
    a.n_end = n0 + rows;
    hipLaunchKernelGGL(lp_fwd_kernel<0>, dim3(row_tiles, p.csplits), dim3(kThreads), 0, st, a);
    HVK_CHECK_LAUNCH("lp_fwd");
    hipLaunchKernelGGL(lp_chunk_reduce_kernel, dim3(ceil_div(p.Rp, kThreads)), dim3(kThreads), 0, st,
                       static_cast<const double*>(lossp), static_cast<const double*>(dbp), row_tiles, p.Rp, lossacc,
                       dbacc, n0 == 0 ? 1 : 0);
    HVK_CHECK_LAUNCH("lp_chunk_reduce");
    hipLaunchKernelGGL(lp_bwd_kernel, dim3(p.ctiles, p.dtiles, p.S), dim3(kThreads), 0, st,
                       static_cast<const float*>(res), p.Rp, xs, N, D, a.vec, n0, row_tiles * kBM, p.steps_per_split,
                       dWp, p.Dp, n0 == 0 ? 0 : 1);
    HVK_CHECK_LAUNCH("lp_bwd");
  }
  if (fold) {
    hipLaunchKernelGGL(lp_count_kernel, dim3(1), dim3(kThreads), 0, st, fold, skip_fold, N, neff);
    HVK_CHECK_LAUNCH("lp_count");
  }
  hipLaunchKernelGGL(lp_finish_kernel, dim3(R), dim3(kThreads), 0, st, static_cast<const float*>(dWp), p.S, p.Rp, p.Dp,
                     static_cast<const double*>(lossacc), static_cast<const double*>(dbacc),
                     fold ? static_cast<const long long*>(neff) : nullptr, N, W, alpha, R, D, dW, db, loss);
  HVK_CHECK_LAUNCH("lp_finish");
  return HVK_OK;
}

int hvk_lp_decision(const float* xs, int B, int D, const float* W, const float* b, int R, float* out,
                    void* stream) {
  if (B < 0 || D < 1 || R < 1)
    return hvk_set_error(HVK_EINVAL, "hvk_lp_decision: bad shape (B %d, D %d, R %d: B >= 0, D >= 1, R >= 1)", B, D, R);
  if (B > kMaxN) return hvk_set_error(HVK_EINVAL, "hvk_lp_decision: bad shape (B %d > 2^31 - 65)", B);
  if (R > 0x7fffff00) return hvk_set_error(HVK_EINVAL, "hvk_lp_decision: bad shape (R %d > 2^31 - 256)", R);
  if (!xs || !W || !b || !out) return hvk_set_error(HVK_EINVAL, "hvk_lp_decision: null pointer");
  if (B == 0) return HVK_OK;
  FwdArgs a{};
  a.xs = xs; a.W = W; a.b = b; a.N = B; a.D = D; a.R = R;
  a.vec = vec_ok(D, xs, W);
  a.out = out;
  const int row_tiles = ceil_div(B, kBM);
  int csplits;
  fwd_split(row_tiles, ceil_div(R, kBN), &a.tiles_per_split, &csplits);
  if (csplits > 65535) return hvk_set_error(HVK_EUNSUPPORTED, "hvk_lp_decision: %d class splits", csplits);
  hipLaunchKernelGGL(lp_fwd_kernel<1>, dim3(row_tiles, csplits), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                     a);
  HVK_CHECK_LAUNCH("lp_decision");
  return HVK_OK;
}

int hvk_lp_step(float* W, float* b, float* Yw, float* Yb, const float* dW, const float* db, float* t,
                const unsigned char* frozen, int R, int D, float step, float tol, float* gmax, unsigned char* converged,
                void* stream) {
  if (R < 1 || D < 1) return hvk_set_error(HVK_EINVAL, "hvk_lp_step: bad shape (R %d, D %d: R >= 1, D >= 1)", R, D);
  if (!(step > 0.f) || !(tol >= 0.f))
    return hvk_set_error(HVK_EINVAL, "hvk_lp_step: step %g must be > 0 and tol %g >= 0", (double)step, (double)tol);
  if (!W || !b || !Yw || !Yb || !dW || !db || !t || !gmax || !converged)
    return hvk_set_error(HVK_EINVAL, "hvk_lp_step: null pointer");
  hipLaunchKernelGGL(lp_step_kernel, dim3(R), dim3(kThreads), 0, static_cast<hipStream_t>(stream), W, b, Yw, Yb, dW,
                     db, t, frozen, D, step, tol, gmax, converged);
  HVK_CHECK_LAUNCH("lp_step");
  return HVK_OK;
}

}  // extern "C"
