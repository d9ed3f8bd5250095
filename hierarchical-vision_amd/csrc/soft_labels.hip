// Soft-labels hierarchical loss (Bertinetto et al., CVPR 2020, section 3.2) on gfx950: the
// cross-entropy against t^(c)_k = w_{d(c,k)} / Z_c, d the tree distance of leaf k from the target
// c.  Definition and tables: include/hvk.h.
//
// In `perm` order every ancestor of the target is one contiguous leaf range and the 8 ranges
// nest, so d(c, k) is the number of the 7 proper ranges that do NOT contain k's position: no
// distance matrix and no [B, L] target is read.
// * Hard targets: one workgroup per sample.  Lanes 0..7 fetch the ranges, thread 0 forms Z_c and
//   the 8 scaled weights w_l / Z_c in LDS; ONE sweep over the row feeds the online (max, sum)
//   pair and sum_k z_k w_d / Z_c (16-B loads where perm is the identity and rows are 16-B
//   aligned).  The backward is one sweep, softmax - w_d / Z_c.
// * Dense targets q [B, L] (LabelSmoothing's column): the loss is the expectation of the hard
//   one, i.e. the CE against t_k = sum_l (w_l - w_{l+1}) R(A_l(k)), R(n) the sum of q_c / Z_c
//   over the leaves of n.  Phase 1 sums R bottom-up over the rank-ordered node slots of the
//   soft-target HXE kernels (a lane per narrow node, a wave per wide one, a barrier between
//   tiers) and takes the row's LSE on the way; phase 2 forms t_k from the ancestors' R.  The
//   backward recomputes t_k, one thread per position.
// No atomics; every reduction has a fixed order.
#include "taxo_row.h"

namespace {

// ----------------------------------------------------------------- hard targets
struct SoftLabelsArgs {
  const float* logits; int B, L; const int* perm; const int64_t* tgt;
  const int* nstart; const int* nend; const int* tbase; const float* weight;
  float* row_loss; float* lse; const float* gout; float* dlogits;
};

// the target's proper ranges and scaled weights, in LDS
struct SoftLabelsRow {
  int lo[kTiers], hi[kTiers];
  float w[kLevels];  // w_l / Z_c; NaN for a target out of range
};

// Lanes 0..7 fetch A_0 .. A_7, thread 0 forms Z_c = sum_l w_l (|A_l| - |A_{l-1}|).  Ends in a
// barrier: every thread may read `r` afterwards.
__device__ __forceinline__ void soft_labels_row(const SoftLabelsArgs& a, int b, SoftLabelsRow& r,
                                                int (&size)[kLevels]) {
  if (threadIdx.x < kLevels) {
    int lo, hi;
    level_range(a, b, threadIdx.x, lo, hi);
    size[threadIdx.x] = hi - lo;  // -1: target out of range
    if (threadIdx.x < kTiers) {
      r.lo[threadIdx.x] = lo;
      r.hi[threadIdx.x] = hi;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float z = 0.f;
    bool bad = false;
    int below = 0;
    for (int l = 0; l < kLevels; ++l) {
      bad |= size[l] < 0;
      z += a.weight[l] * (float)(size[l] - below);
      below = size[l];
    }
    const float inv = bad ? __builtin_nanf("") : 1.f / z;
    for (int l = 0; l < kLevels; ++l) r.w[l] = a.weight[l] * inv;
  }
  __syncthreads();
}

// w_d / Z_c of permuted position pos: d = how many of the 7 proper ranges do not hold pos (they
// nest, so this is the first level that does, also where ranges coincide)
__device__ __forceinline__ float soft_labels_target(const SoftLabelsRow& r, int pos) {
  int d = 0;
#pragma unroll
  for (int l = 0; l < kTiers; ++l) d += (pos < r.lo[l]) | (pos >= r.hi[l]);
  return r.w[d];
}

template <bool VEC>
__global__ __launch_bounds__(256) void soft_labels_fwd_kernel(SoftLabelsArgs a) {
  __shared__ SoftLabelsRow row;
  __shared__ int size[kLevels];
  __shared__ float sm[4], ss[4], st[4];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const float* z = a.logits + (size_t)b * a.L;
  soft_labels_row(a, b, row, size);
  Lse acc{-INFINITY, 0.f};
  float tz = 0.f;  // this thread's share of sum_k z_k w_d / Z_c
  if (VEC) {       // perm == identity, L % 4 == 0, rows 16-B aligned
    for (int pos = 4 * threadIdx.x; pos < a.L; pos += 4 * 256) {
      const float4 x = *reinterpret_cast<const float4*>(z + pos);
      const float xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        acc = lse_push(acc, xs[j]);
        tz += xs[j] * soft_labels_target(row, pos + j);
      }
    }
  } else {
    for (int pos = threadIdx.x; pos < a.L; pos += 256) {
      const float x = z[a.perm ? a.perm[pos] : pos];
      acc = lse_push(acc, x);
      tz += x * soft_labels_target(row, pos);
    }
  }
  acc = wave_lse(acc);
  tz = hvk_wave_sum(tz);
  if (lane == 0) { sm[wv] = acc.m; ss[wv] = acc.s; st[wv] = tz; }
  __syncthreads();
  if (threadIdx.x == 0) {
    Lse tot{sm[0], ss[0]};
    for (int w = 1; w < 4; ++w) {
      tot = lse_merge(tot, Lse{sm[w], ss[w]});
      tz += st[w];
    }
    const float lse = tot.m + __logf(tot.s);
    a.lse[b] = lse;
    a.row_loss[b] = lse - tz;  // sum_k t_k = 1; NaN through row.w for a target out of range
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void soft_labels_bwd_kernel(SoftLabelsArgs a) {
  __shared__ SoftLabelsRow row;
  __shared__ int size[kLevels];
  const int b = blockIdx.x;
  soft_labels_row(a, b, row, size);
  const float g = a.gout[0] / a.B, lse = a.lse[b];
  const float* z = a.logits + (size_t)b * a.L;
  float* dz = a.dlogits + (size_t)b * a.L;
  if (VEC) {
    for (int pos = 4 * threadIdx.x; pos < a.L; pos += 4 * 256) {
      const float4 x = *reinterpret_cast<const float4*>(z + pos);
      float4 d;
      d.x = g * (__expf(x.x - lse) - soft_labels_target(row, pos));
      d.y = g * (__expf(x.y - lse) - soft_labels_target(row, pos + 1));
      d.z = g * (__expf(x.z - lse) - soft_labels_target(row, pos + 2));
      d.w = g * (__expf(x.w - lse) - soft_labels_target(row, pos + 3));
      *reinterpret_cast<float4*>(dz + pos) = d;
    }
  } else {
    for (int pos = threadIdx.x; pos < a.L; pos += 256) {
      const int k = a.perm ? a.perm[pos] : pos;
      dz[k] = g * (__expf(z[k] - lse) - soft_labels_target(row, pos));
    }
  }
}

// ----------------------------------------------------------------- dense targets
struct SoftLabelsDenseArgs {
  const float* logits; const float* q; const float* inv_norm; int B, L, n_nodes; const int* perm;
  const int* rank_off; const int* child_lo; const int* child_hi; const int* anc;
  const float* weight; float* row_loss; float* lse; float* tsum; float* node_r;
  const float* gout; float* dlogits;
};

// a node with at most this many children is summed by one lane, a wider one by its whole wave
constexpr int kSerialWidth = 16;

// children first, first + step, ... < hi of one node summed; leaves also feed the row's LSE
template <bool LEAVES>
__device__ __forceinline__ float dense_children(const SoftLabelsDenseArgs& a, const float* z,
                                                const float* q, const float* nr, int first, int hi,
                                                int step, Lse& acc) {
  float R = 0.f;
  for (int c = first; c < hi; c += step) {
    if (LEAVES) {
      const int k = (int)HVK_BCHECK(a.perm ? a.perm[c] : c, a.L);
      acc = lse_push(acc, z[k]);
      R += q[k] * a.inv_norm[k];
    } else {
      R += nr[HVK_BCHECK(c, a.n_nodes + 1)];
    }
  }
  return R;
}

// t_k of permuted position pos (leaf k) from the saved node sums: sum_l (w_l - w_{l+1}) R(A_l(k)),
// A_0 = the leaf itself, A_1 .. A_6 through anc, A_7 = the root (w_8 = 0)
__device__ __forceinline__ float dense_target(const SoftLabelsDenseArgs& a, const float* dw,
                                              const float* nr, int pos, float rk) {
  float t = dw[0] * rk + dw[kLevels - 1] * nr[a.n_nodes];
#pragma unroll
  for (int q = 0; q < kTiers - 1; ++q)
    t += dw[kTiers - 1 - q] * nr[HVK_BCHECK(a.anc[(size_t)pos * (kTiers - 1) + q], a.n_nodes)];
  return t;
}

__device__ __forceinline__ void dense_weight_steps(const float* w, float (&dw)[kLevels]) {
#pragma unroll
  for (int l = 0; l < kLevels; ++l) dw[l] = w[l] - (l + 1 < kLevels ? w[l + 1] : 0.f);
}

__global__ __launch_bounds__(256) void soft_labels_dense_fwd_kernel(SoftLabelsDenseArgs a) {
  __shared__ float sm[4], ss[4], st[4], sz[4];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const float* z = a.logits + (size_t)b * a.L;
  const float* q = a.q + (size_t)b * a.L;
  // written and read back in this kernel (by other waves, across the tier barrier): no restrict
  float* nr = a.node_r + (size_t)b * (a.n_nodes + 1);
  Lse acc{-INFINITY, 0.f};
  // phase 1: R(n) of tiers 5 .. 0, then the root; every leaf passes through exactly one tier-5 node
  for (int s = 0; s < kTiers; ++s) {
    const int t = s < kTiers - 1 ? kTiers - 2 - s : kTiers - 1;
    const int n0 = a.rank_off[t], n1 = a.rank_off[t + 1];
    for (int base = n0 + wv * 64; base < n1; base += 256) {  // wave-uniform: 64 slots per wave
      const int i = base + lane;
      int lo = 0, hi = 0;
      if (i < n1) {
        lo = a.child_lo[i];
        hi = a.child_hi[i];
      }
      const bool wide = hi - lo > kSerialWidth;
      if (i < n1 && !wide)
        nr[i] = t == kTiers - 2 ? dense_children<true>(a, z, q, nr, lo, hi, 1, acc)
                                : dense_children<false>(a, z, q, nr, lo, hi, 1, acc);
      unsigned long long m = __ballot(wide);
      while (m) {  // the wave's wide nodes, one after the other, 64 lanes strided over the children
        const int j = __ffsll(m) - 1;
        m &= m - 1;
        const int jlo = __shfl(lo, j), jhi = __shfl(hi, j);
        float R = t == kTiers - 2 ? dense_children<true>(a, z, q, nr, jlo + lane, jhi, 64, acc)
                                  : dense_children<false>(a, z, q, nr, jlo + lane, jhi, 64, acc);
        R = hvk_wave_sum(R);
        if (lane == 0) nr[base + j] = R;
      }
    }
    __syncthreads();  // the next tier reads these sums back (workgroup-scope release / acquire)
  }
  // phase 2: t_k, sum_k t_k and sum_k t_k z_k
  float dw[kLevels];
  dense_weight_steps(a.weight, dw);
  float ts = 0.f, tz = 0.f;
  for (int pos = threadIdx.x; pos < a.L; pos += 256) {
    const int k = (int)HVK_BCHECK(a.perm ? a.perm[pos] : pos, a.L);
    const float t = dense_target(a, dw, nr, pos, q[k] * a.inv_norm[k]);
    ts += t;
    tz += t * z[k];
  }
  acc = wave_lse(acc);
  ts = hvk_wave_sum(ts);
  tz = hvk_wave_sum(tz);
  if (lane == 0) { sm[wv] = acc.m; ss[wv] = acc.s; st[wv] = ts; sz[wv] = tz; }
  __syncthreads();
  if (threadIdx.x == 0) {
    Lse tot{sm[0], ss[0]};
    for (int w = 1; w < 4; ++w) {
      tot = lse_merge(tot, Lse{sm[w], ss[w]});
      ts += st[w];
      tz += sz[w];
    }
    const float lse = tot.m + __logf(tot.s);
    a.lse[b] = lse;
    a.tsum[b] = ts;
    a.row_loss[b] = lse * ts - tz;
  }
}

// one thread per permuted position
__global__ __launch_bounds__(256) void soft_labels_dense_bwd_kernel(SoftLabelsDenseArgs a, int chunks) {
  const int b = blockIdx.x / chunks;
  const int pos = (blockIdx.x - b * chunks) * 256 + threadIdx.x;
  if (pos >= a.L) return;
  const float* __restrict__ nr = a.node_r + (size_t)b * (a.n_nodes + 1);
  float dw[kLevels];
  dense_weight_steps(a.weight, dw);
  const int k = (int)HVK_BCHECK(a.perm ? a.perm[pos] : pos, a.L);
  const size_t i = (size_t)b * a.L + k;
  const float t = dense_target(a, dw, nr, pos, a.q[i] * a.inv_norm[k]);
  a.dlogits[i] = a.gout[0] / a.B * (__expf(a.logits[i] - a.lse[b]) * a.tsum[b] - t);
}

bool rows_16b(const float* p, const float* q, int L) {
  return L % 4 == 0 && (reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(q)) % 16 == 0;
}

}  // namespace

extern "C" {

int hvk_soft_labels_fwd(const float* logits, int B, int L, const int* perm, const int64_t* targets,
                        const int* node_start, const int* node_end, const int* tier_base,
                        const float* level_weight, float* row_loss, float* lse, void* stream) {
  if (!logits || !targets || !node_start || !node_end || !tier_base || !level_weight ||
      !row_loss || !lse)
    return hvk_set_error(HVK_EINVAL, "hvk_soft_labels_fwd: null pointer");
  if (B < 0 || L <= 0) return hvk_set_error(HVK_EINVAL, "hvk_soft_labels_fwd: bad shape");
  if (B == 0) return HVK_OK;
  SoftLabelsArgs a{logits, B, L, perm, targets, node_start, node_end, tier_base, level_weight,
                   row_loss, lse, nullptr, nullptr};
  if (!perm && rows_16b(logits, logits, L))
    hipLaunchKernelGGL(soft_labels_fwd_kernel<true>, dim3(B), dim3(256), 0,
                       static_cast<hipStream_t>(stream), a);
  else
    hipLaunchKernelGGL(soft_labels_fwd_kernel<false>, dim3(B), dim3(256), 0,
                       static_cast<hipStream_t>(stream), a);
  HVK_CHECK_LAUNCH("soft_labels_fwd");
  return HVK_OK;
}

int hvk_soft_labels_bwd(const float* logits, int B, int L, const int* perm, const int64_t* targets,
                        const int* node_start, const int* node_end, const int* tier_base,
                        const float* level_weight, const float* lse, const float* grad_out,
                        float* dlogits, void* stream) {
  if (!logits || !targets || !node_start || !node_end || !tier_base || !level_weight || !lse ||
      !grad_out || !dlogits)
    return hvk_set_error(HVK_EINVAL, "hvk_soft_labels_bwd: null pointer");
  if (B < 0 || L <= 0) return hvk_set_error(HVK_EINVAL, "hvk_soft_labels_bwd: bad shape");
  if (B == 0) return HVK_OK;
  SoftLabelsArgs a{logits, B, L, perm, targets, node_start, node_end, tier_base, level_weight,
                   nullptr, const_cast<float*>(lse), grad_out, dlogits};
  if (!perm && rows_16b(logits, dlogits, L))
    hipLaunchKernelGGL(soft_labels_bwd_kernel<true>, dim3(B), dim3(256), 0,
                       static_cast<hipStream_t>(stream), a);
  else
    hipLaunchKernelGGL(soft_labels_bwd_kernel<false>, dim3(B), dim3(256), 0,
                       static_cast<hipStream_t>(stream), a);
  HVK_CHECK_LAUNCH("soft_labels_bwd");
  return HVK_OK;
}

int hvk_soft_labels_dense_fwd(const float* logits, const float* q, const float* inv_norm, int B,
                              int L, const int* perm, int n_nodes, const int* rank_off,
                              const int* child_lo, const int* child_hi, const int* anc,
                              const float* level_weight, float* row_loss, float* lse, float* tsum,
                              float* node_r, void* stream) {
  if (!logits || !q || !inv_norm || !rank_off || !child_lo || !child_hi || !anc || !level_weight ||
      !row_loss || !lse || !tsum || !node_r)
    return hvk_set_error(HVK_EINVAL, "hvk_soft_labels_dense_fwd: null pointer");
  if (B < 0 || L <= 0 || n_nodes <= 0)
    return hvk_set_error(HVK_EINVAL, "hvk_soft_labels_dense_fwd: bad shape");
  if (B == 0) return HVK_OK;
  SoftLabelsDenseArgs a{logits, q, inv_norm, B, L, n_nodes, perm, rank_off, child_lo, child_hi,
                        anc, level_weight, row_loss, lse, tsum, node_r, nullptr, nullptr};
  hipLaunchKernelGGL(soft_labels_dense_fwd_kernel, dim3(B), dim3(256), 0,
                     static_cast<hipStream_t>(stream), a);
  HVK_CHECK_LAUNCH("soft_labels_dense_fwd");
  return HVK_OK;
}

int hvk_soft_labels_dense_bwd(const float* logits, const float* q, const float* inv_norm, int B,
                              int L, const int* perm, int n_nodes, const int* anc,
                              const float* level_weight, const float* lse, const float* tsum,
                              const float* node_r, const float* grad_out, float* dlogits,
                              void* stream) {
  if (!logits || !q || !inv_norm || !anc || !level_weight || !lse || !tsum || !node_r ||
      !grad_out || !dlogits)
    return hvk_set_error(HVK_EINVAL, "hvk_soft_labels_dense_bwd: null pointer");
  if (B < 0 || L <= 0 || n_nodes <= 0)
    return hvk_set_error(HVK_EINVAL, "hvk_soft_labels_dense_bwd: bad shape");
  if (B == 0) return HVK_OK;
  const int chunks = (L + 255) / 256;
  if ((long long)B * chunks > 0x7fffffffLL)
    return hvk_set_error(HVK_EINVAL, "hvk_soft_labels_dense_bwd: B * ceil(L / 256) exceeds the grid");
  SoftLabelsDenseArgs a{logits, q, inv_norm, B, L, n_nodes, perm, nullptr, nullptr, nullptr, anc,
                        level_weight, nullptr, const_cast<float*>(lse), const_cast<float*>(tsum),
                        const_cast<float*>(node_r), grad_out, dlogits};
  hipLaunchKernelGGL(soft_labels_dense_bwd_kernel, dim3(B * chunks), dim3(256), 0,
                     static_cast<hipStream_t>(stream), a, chunks);
  HVK_CHECK_LAUNCH("soft_labels_dense_bwd");
  return HVK_OK;
}

}  // extern "C"
