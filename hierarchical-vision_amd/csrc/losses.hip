// Taxonomy losses on gfx950.
//
// * Multitask CE (hierarchy.py:65-94) -- all tiers' heads in ONE launch over a
//   concatenated logit matrix; one wave per (tier, sample) row; hard int targets or
//   dense soft targets (LabelSmoothing, algorithmic.py:91-116).  Also the flat CE of
//   models.py:112 (n_heads = 1).
// * HXE (hierarchical cross-entropy; not implemented by the reference,
//   hierarchy.py:183-185): per sample, a segmented log-sum-exp over the nested
//   leaf ranges of the target's ancestors, each range contiguous in `perm` order.
//   One workgroup per sample; every range is a strided wavefront scan with an
//   online (max, sum) pair and a cross-wave merge.
// * HXE with soft targets (LabelSmoothing on the HXE variant): the expectation of the hard
//   loss under a leaf weight vector; every node's LSE and weight sum, bottom-up over
//   rank-ordered node slots, one workgroup per sample; the backward is one pass over the leaves.
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

// ----------------------------------------------------------------- multitask CE
__global__ __launch_bounds__(256) void mt_ce_fwd_kernel(const float* __restrict__ logits, int ld,
                                                        int B, int n_heads,
                                                        const int* __restrict__ off,
                                                        const int64_t* __restrict__ tgt,
                                                        const float* __restrict__ soft,
                                                        float* row_loss, float* lse_out) {
  const int wid = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (wid >= B * n_heads) return;
  const int h = wid / B, b = wid % B;
  const int c0 = off[h], c1 = off[h + 1];
  const float* z = logits + (size_t)b * ld;
  Lse acc{-INFINITY, 0.f};
  float tz = 0.f, tsum = 0.f;
  for (int c = c0 + lane; c < c1; c += 64) {
    const float x = z[c];
    acc = lse_push(acc, x);
    if (soft) {
      const float t = soft[(size_t)b * ld + c];
      tz += t * x;
      tsum += t;
    }
  }
  acc = wave_lse(acc);
  const float lse = acc.m + __logf(acc.s);
  float loss;
  if (soft) {
    tz = hvk_wave_sum(tz);
    tsum = hvk_wave_sum(tsum);
    loss = lse * tsum - tz;
  } else {
    const int64_t t = tgt[(size_t)b * n_heads + h];
    // a target outside [0, classes) (torch's CE raises "Target out of bounds"): NaN loss, no
    // out-of-range read
    loss = (t >= 0 && t < c1 - c0) ? lse - z[c0 + (int)t] : __builtin_nanf("");
  }
  if (lane == 0) {
    row_loss[wid] = loss;
    lse_out[wid] = lse;
  }
}

__global__ __launch_bounds__(256) void mt_ce_bwd_kernel(const float* __restrict__ logits, int ld,
                                                        int B, int n_heads,
                                                        const int* __restrict__ off,
                                                        const int64_t* __restrict__ tgt,
                                                        const float* __restrict__ soft,
                                                        const float* __restrict__ lse,
                                                        const float* __restrict__ coeff,
                                                        const float* __restrict__ gout,
                                                        float* dlogits) {
  const int wid = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (wid >= B * n_heads) return;
  const int h = wid / B, b = wid % B;
  const int c0 = off[h], c1 = off[h + 1];
  const float g = gout[0] * coeff[h] / B;
  const float l = lse[wid];
  const float* z = logits + (size_t)b * ld;
  float* dz = dlogits + (size_t)b * ld;
  float tsum = 1.f;
  if (soft) {
    float s = 0.f;
    for (int c = c0 + lane; c < c1; c += 64) s += soft[(size_t)b * ld + c];
    tsum = hvk_wave_sum(s);
  }
  const int t = soft ? -1 : (int)tgt[(size_t)b * n_heads + h];
  for (int c = c0 + lane; c < c1; c += 64) {
    const float p = __expf(z[c] - l);
    const float tv = soft ? soft[(size_t)b * ld + c] : (c - c0 == t ? 1.f : 0.f);
    dz[c] = g * (p * tsum - tv);
  }
}

// ----------------------------------------------------------------- HXE
struct HxeArgs {
  const float* logits; int B, L; const int* perm; const int64_t* tgt;
  const int* nstart; const int* nend; const int* tbase; const float* coeff;
  float* row_loss; float* lse; const float* gout; float* dlogits;
};

// segment [lo, hi) in permuted positions of the target's node at level l (l = 7: all)
__device__ __forceinline__ void level_range(const HxeArgs& a, int b, int l, int& lo, int& hi) {
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

__global__ __launch_bounds__(256) void hxe_fwd_kernel(HxeArgs a) {
  __shared__ float sm[4], ss[4];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const float* z = a.logits + (size_t)b * a.L;
  float loss = 0.f;
  for (int l = 0; l < kLevels; ++l) {
    int lo, hi;
    level_range(a, b, l, lo, hi);
    Lse acc{-INFINITY, 0.f};
    for (int pos = lo + threadIdx.x; pos < hi; pos += blockDim.x)
      acc = lse_push(acc, z[a.perm ? a.perm[pos] : pos]);
    acc = wave_lse(acc);
    if (lane == 0) { sm[wv] = acc.m; ss[wv] = acc.s; }
    __syncthreads();
    Lse tot{sm[0], ss[0]};
    for (int w = 1; w < 4; ++w) tot = lse_merge(tot, Lse{sm[w], ss[w]});
    __syncthreads();
    const float v = hi < lo ? __builtin_nanf("") : tot.m + __logf(tot.s);  // NaN: target out of range
    loss += a.coeff[l] * v;
    if (threadIdx.x == 0) a.lse[(size_t)b * kLevels + l] = v;
  }
  if (threadIdx.x == 0) a.row_loss[b] = loss;
}

__global__ __launch_bounds__(256) void hxe_bwd_kernel(HxeArgs a) {
  const int b = blockIdx.x;
  __shared__ int lo[kLevels], hi[kLevels];
  __shared__ float lv[kLevels];
  if (threadIdx.x < kLevels) {
    level_range(a, b, threadIdx.x, lo[threadIdx.x], hi[threadIdx.x]);
    lv[threadIdx.x] = a.lse[(size_t)b * kLevels + threadIdx.x];
  }
  __syncthreads();
  const float g = a.gout[0] / a.B;
  const float* z = a.logits + (size_t)b * a.L;
  float* dz = a.dlogits + (size_t)b * a.L;
  for (int pos = threadIdx.x; pos < a.L; pos += blockDim.x) {
    const int k = a.perm ? a.perm[pos] : pos;
    const float x = z[k];
    float d = 0.f;
#pragma unroll
    for (int l = 0; l < kLevels; ++l)
      if (pos >= lo[l] && pos < hi[l]) d += a.coeff[l] * __expf(x - lv[l]);
    dz[k] = g * d;
  }
}

// ----------------------------------------------------------------- HXE, soft targets
// The expectation of the hard loss under a non-negative leaf weight vector t (include/hvk.h):
// every internal node n needs LSE(n) and T(n) = sum of t over its leaves.  Nodes are indexed by
// slot = rank_off[tier] + rank of the node within its tier by node_start (slot n_nodes = the
// root), so the children of a slot are one contiguous range [child_lo, child_hi): permuted leaf
// positions for tier 5, slots of the next finer tier above it.  The forward works bottom-up, one
// workgroup per sample: tier 5 reduces its leaves, each coarser tier merges its children's
// (LSE, T) from the saved [B, n_nodes + 1] buffers, a barrier between tiers.  Every node keeps
// its own running max; there are no atomics and every reduction has a fixed order.
struct HxeSoftArgs {
  const float* logits; const float* soft; int B, L, n_nodes; const int* perm;
  const int* rank_off; const int* child_lo; const int* child_hi; const int* anc;
  const float* coeff; float* row_loss; float* node_lse; float* node_t;
  const float* gout; float* dlogits;
};

// a node with at most this many children is reduced by one lane, a wider one by its whole wave
constexpr int kSerialWidth = 16;

// children first, first + step, ... < hi of one node folded into (acc, T); tz += t_k z_k (leaves)
template <bool LEAVES>
__device__ __forceinline__ void soft_children(const HxeSoftArgs& a, const float* z, const float* t,
                                              const float* nl, const float* nt, int first, int hi,
                                              int step, Lse& acc, float& T, float& tz) {
  for (int c = first; c < hi; c += step) {
    if (LEAVES) {
      const int k = a.perm ? a.perm[c] : c;
      const float x = z[k], w = t[k];
      acc = lse_push(acc, x);
      T += w;
      tz += w * x;
    } else {
      acc = lse_merge(acc, Lse{nl[c], 1.f});
      T += nt[c];
    }
  }
}

__global__ __launch_bounds__(256) void hxe_soft_fwd_kernel(HxeSoftArgs a) {
  __shared__ float sred[2][4];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const float* z = a.logits + (size_t)b * a.L;
  const float* t = a.soft + (size_t)b * a.L;
  // written and read back in this kernel (by other waves, across the tier barrier): no restrict
  float* nl = a.node_lse + (size_t)b * (a.n_nodes + 1);
  float* nt = a.node_t + (size_t)b * (a.n_nodes + 1);
  float part = 0.f;  // this thread's share of sum_n c_l T(n) LSE(n)
  float tz = 0.f;    // ... and of sum_k t_k z_k
  for (int s = 0; s < kTiers; ++s) {
    const int q = s < kTiers - 1 ? kTiers - 2 - s : kTiers - 1;  // tiers 5 .. 0, then 6 = the root
    const int n0 = a.rank_off[q], n1 = a.rank_off[q + 1];
    const float cl = a.coeff[q < kTiers - 1 ? kTiers - 1 - q : kLevels - 1];
    for (int base = n0 + wv * 64; base < n1; base += 256) {  // wave-uniform: 64 slots per wave
      const int i = base + lane;
      int lo = 0, hi = 0;
      if (i < n1) {
        lo = a.child_lo[i];
        hi = a.child_hi[i];
      }
      const bool wide = hi - lo > kSerialWidth;
      if (i < n1 && !wide) {
        Lse acc{-INFINITY, 0.f};
        float T = 0.f;
        if (q == kTiers - 2) soft_children<true>(a, z, t, nl, nt, lo, hi, 1, acc, T, tz);
        else soft_children<false>(a, z, t, nl, nt, lo, hi, 1, acc, T, tz);
        const float v = acc.m + __logf(acc.s);
        nl[i] = v;
        nt[i] = T;
        if (T != 0.f) part += cl * T * v;
      }
      unsigned long long m = __ballot(wide);
      while (m) {  // the wave's wide nodes, one after the other, 64 lanes strided over the children
        const int j = __ffsll(m) - 1;
        m &= m - 1;
        const int jlo = __shfl(lo, j), jhi = __shfl(hi, j);
        Lse acc{-INFINITY, 0.f};
        float T = 0.f;
        if (q == kTiers - 2) soft_children<true>(a, z, t, nl, nt, jlo + lane, jhi, 64, acc, T, tz);
        else soft_children<false>(a, z, t, nl, nt, jlo + lane, jhi, 64, acc, T, tz);
        acc = wave_lse(acc);
        T = hvk_wave_sum(T);
        if (lane == 0) {
          const float v = acc.m + __logf(acc.s);
          nl[base + j] = v;
          nt[base + j] = T;
          if (T != 0.f) part += cl * T * v;
        }
      }
    }
    __syncthreads();  // the next tier reads these (LSE, T) back (workgroup-scope release / acquire)
  }
  part = hvk_wave_sum(part);
  tz = hvk_wave_sum(tz);
  if (lane == 0) {
    sred[0][wv] = part;
    sred[1][wv] = tz;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) {
      part += sred[0][w];
      tz += sred[1][w];
    }
    a.row_loss[b] = a.coeff[0] * tz + part;
  }
}

// one thread per permuted position: the six ancestors' (LSE, T) through anc [L, 6], plus the root
__global__ __launch_bounds__(256) void hxe_soft_bwd_kernel(HxeSoftArgs a, int chunks) {
  const int b = blockIdx.x / chunks;
  const int pos = (blockIdx.x - b * chunks) * 256 + threadIdx.x;
  if (pos >= a.L) return;
  const float* __restrict__ nl = a.node_lse + (size_t)b * (a.n_nodes + 1);
  const float* __restrict__ nt = a.node_t + (size_t)b * (a.n_nodes + 1);
  const int k = a.perm ? a.perm[pos] : pos;
  const float x = a.logits[(size_t)b * a.L + k];
  float d = a.coeff[0] * a.soft[(size_t)b * a.L + k];
#pragma unroll
  for (int q = 0; q < kTiers; ++q) {
    const int i = q < kTiers - 1 ? a.anc[(size_t)pos * (kTiers - 1) + q] : a.n_nodes;
    const float T = nt[i];
    if (T != 0.f) d += a.coeff[q < kTiers - 1 ? kTiers - 1 - q : kLevels - 1] * T * __expf(x - nl[i]);
  }
  a.dlogits[(size_t)b * a.L + k] = a.gout[0] / a.B * d;
}

}  // namespace

extern "C" {

int hvk_multitask_ce_fwd(const float* logits, int ld, int B, int n_heads, const int* head_off,
                         const int64_t* targets, const float* soft, float* row_loss, float* lse,
                         void* stream) {
  if (!logits || !head_off || !row_loss || !lse || (!targets && !soft))
    return hvk_set_error(HVK_EINVAL, "hvk_multitask_ce_fwd: null pointer");
  if (B <= 0 || n_heads <= 0 || ld <= 0)
    return hvk_set_error(HVK_EINVAL, "hvk_multitask_ce_fwd: bad shape");
  const int rows = B * n_heads;
  hipLaunchKernelGGL(mt_ce_fwd_kernel, dim3((rows + 3) / 4), dim3(256), 0,
                     static_cast<hipStream_t>(stream), logits, ld, B, n_heads, head_off, targets,
                     soft, row_loss, lse);
  HVK_CHECK_LAUNCH("multitask_ce_fwd");
  return HVK_OK;
}

int hvk_multitask_ce_bwd(const float* logits, int ld, int B, int n_heads, const int* head_off,
                         const int64_t* targets, const float* soft, const float* lse,
                         const float* coeff, const float* grad_out, float* dlogits,
                         void* stream) {
  if (!logits || !head_off || !lse || !coeff || !grad_out || !dlogits || (!targets && !soft))
    return hvk_set_error(HVK_EINVAL, "hvk_multitask_ce_bwd: null pointer");
  const int rows = B * n_heads;
  hipLaunchKernelGGL(mt_ce_bwd_kernel, dim3((rows + 3) / 4), dim3(256), 0,
                     static_cast<hipStream_t>(stream), logits, ld, B, n_heads, head_off, targets,
                     soft, lse, coeff, grad_out, dlogits);
  HVK_CHECK_LAUNCH("multitask_ce_bwd");
  return HVK_OK;
}

int hvk_hxe_fwd(const float* logits, int B, int L, const int* perm, const int64_t* targets,
                const int* node_start, const int* node_end, const int* tier_base,
                const float* level_coeff, float* row_loss, float* lse, void* stream) {
  if (!logits || !targets || !node_start || !node_end || !tier_base || !level_coeff ||
      !row_loss || !lse)
    return hvk_set_error(HVK_EINVAL, "hvk_hxe_fwd: null pointer");
  if (B <= 0 || L <= 0) return hvk_set_error(HVK_EINVAL, "hvk_hxe_fwd: bad shape");
  HxeArgs a{logits, B, L, perm, targets, node_start, node_end, tier_base, level_coeff,
            row_loss, lse, nullptr, nullptr};
  hipLaunchKernelGGL(hxe_fwd_kernel, dim3(B), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  HVK_CHECK_LAUNCH("hxe_fwd");
  return HVK_OK;
}

int hvk_hxe_bwd(const float* logits, int B, int L, const int* perm, const int64_t* targets,
                const int* node_start, const int* node_end, const int* tier_base,
                const float* level_coeff, const float* lse, const float* grad_out,
                float* dlogits, void* stream) {
  if (!logits || !targets || !node_start || !node_end || !tier_base || !level_coeff || !lse ||
      !grad_out || !dlogits)
    return hvk_set_error(HVK_EINVAL, "hvk_hxe_bwd: null pointer");
  HxeArgs a{logits, B, L, perm, targets, node_start, node_end, tier_base, level_coeff,
            nullptr, const_cast<float*>(lse), grad_out, dlogits};
  hipLaunchKernelGGL(hxe_bwd_kernel, dim3(B), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  HVK_CHECK_LAUNCH("hxe_bwd");
  return HVK_OK;
}

int hvk_hxe_soft_fwd(const float* logits, const float* soft, int B, int L, const int* perm,
                     int n_nodes, const int* rank_off, const int* child_lo, const int* child_hi,
                     const float* level_coeff, float* row_loss, float* node_lse, float* node_t,
                     void* stream) {
  if (!logits || !soft || !rank_off || !child_lo || !child_hi || !level_coeff || !row_loss ||
      !node_lse || !node_t)
    return hvk_set_error(HVK_EINVAL, "hvk_hxe_soft_fwd: null pointer");
  if (B <= 0 || L <= 0 || n_nodes <= 0)
    return hvk_set_error(HVK_EINVAL, "hvk_hxe_soft_fwd: bad shape");
  HxeSoftArgs a{logits, soft, B, L, n_nodes, perm, rank_off, child_lo, child_hi, nullptr,
                level_coeff, row_loss, node_lse, node_t, nullptr, nullptr};
  hipLaunchKernelGGL(hxe_soft_fwd_kernel, dim3(B), dim3(256), 0, static_cast<hipStream_t>(stream),
                     a);
  HVK_CHECK_LAUNCH("hxe_soft_fwd");
  return HVK_OK;
}

int hvk_hxe_soft_bwd(const float* logits, const float* soft, int B, int L, const int* perm,
                     int n_nodes, const int* anc, const float* level_coeff, const float* node_lse,
                     const float* node_t, const float* grad_out, float* dlogits, void* stream) {
  if (!logits || !soft || !anc || !level_coeff || !node_lse || !node_t || !grad_out || !dlogits)
    return hvk_set_error(HVK_EINVAL, "hvk_hxe_soft_bwd: null pointer");
  if (B <= 0 || L <= 0 || n_nodes <= 0)
    return hvk_set_error(HVK_EINVAL, "hvk_hxe_soft_bwd: bad shape");
  const int chunks = (L + 255) / 256;
  if ((long long)B * chunks > 0x7fffffffLL)
    return hvk_set_error(HVK_EINVAL, "hvk_hxe_soft_bwd: B * ceil(L / 256) exceeds the grid");
  HxeSoftArgs a{logits, soft, B, L, n_nodes, perm, nullptr, nullptr, nullptr, anc, level_coeff,
                nullptr, const_cast<float*>(node_lse), const_cast<float*>(node_t), grad_out,
                dlogits};
  hipLaunchKernelGGL(hxe_soft_bwd_kernel, dim3(B * chunks), dim3(256), 0,
                     static_cast<hipStream_t>(stream), a, chunks);
  HVK_CHECK_LAUNCH("hxe_soft_bwd");
  return HVK_OK;
}

}  // extern "C"
