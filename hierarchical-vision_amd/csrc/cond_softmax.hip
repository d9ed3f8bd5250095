// The conditional-softmax taxonomy head on gfx950 (hierarchy.py: ConditionalSoftmaxCrossEntropy,
// cond_softmax_scores, EvalMetrics decoding="cond"): every node has a logit, the softmax runs over
// a node's siblings only, and a leaf's probability is the product of the conditionals on its path,
//   log p(n | parent) = z_t[n] - LSE_{m in g(n)} z_t[m],   log p(leaf k) = sum_t log p(anc_t(k) | anc_{t-1}(k)).
// The sibling groups are a CSR over the concatenated column space (Taxonomy.sibling_tables): group
// 0 the children of the root, group 1 + off[t - 1] + p the children of node p of tier t - 1, so
// tier t's columns are CSR positions [off[t], off[t + 1]); sib_col null = the identity.
//
// * cond_fwd_kernel -- one WAVE per row, four rows a workgroup: a row touches only the 7 groups of
//   its target's path.  Lanes stride over a group, an online (max, shifted sum) and a plain sum per
//   lane, one lane-ordered butterfly: LSE, the group mean (label smoothing), the tier's NLL.
// * cond_bwd_kernel -- the whole [B, ldg] gradient in ONE sweep of 16-B stores: a vector outside the
//   row's 7 active column ranges stores zeros without a load; inside, softmax from the saved LSEs.
//   Identity: the ranges are 7 column intervals in registers; with sib_col membership is
//   "parent(c) == y_{t-1}" through the parents table.  No zero-fill-then-scatter, no atomics.
// * cond_decode_kernel -- one workgroup per row: tiers 0-5 to LDS as f32 (joint.hip's staging),
//   then top-down, one barrier a tier.  The work item is a PARENT: a wave takes 64 parents at a
//   time; a lane whose group has at most kSplit children reduces it alone (narrow), the wider
//   groups of the 64 are then taken one by one by the whole wave (wide: lanes stride, butterfly).
//   Either way the children are rewritten in place, c_t[child] = (z - LSE) + c_{t-1}[parent], and
//   no group LSE is stored.  The leaf tier is the same pass over the genus nodes with its children
//   in global memory: s_k = (z_6[k] - LSE_g) + c_5[g] is stored when asked for and folded into the
//   RowAcc of eval_row.h (argmax, rank, lse).  A group's path depends on its size alone, so the
//   bits do not change from run to run.
#include <math.h>
#include <stdio.h>

#include "eval_row.h"
#include "../../include/hvk.h"

using namespace hvk_eval;

namespace {

constexpr int kTiers = 7;
constexpr int kCoarse = kTiers - 1;
constexpr int kMaxCoarse = 15360;  // f32 coarse logits in one workgroup's LDS: 60 KB (joint.hip)
constexpr int kMaxLeaves = 1 << 24;
// widest group one lane reduces alone.  A narrow group of s children costs its wave about 2 s
// element visits (64 groups side by side, the wave waits for the widest); a wide one costs
// 2 ceil(s / 64) visits plus a 6-level butterfly of 4 shuffles and 2 expf a level, some 30 visits'
// worth: past 32 children the whole wave is the cheaper way.
constexpr int kSplit = 32;
constexpr int kBwdVecs = 4;  // 16-B vectors a thread of cond_bwd_kernel stores

struct Lse {
  float m, s;
};
__device__ __forceinline__ Lse lse_push(Lse a, float x) {
  if (x > a.m) {
    a.s = a.s * shifted_exp(a.m, x) + 1.f;
    a.m = x;
  } else {
    a.s += shifted_exp(x, a.m);
  }
  return a;
}
// the operands keep their order: both lanes of a butterfly pair reach the same bits
__device__ __forceinline__ Lse lse_merge(Lse a, Lse b) {
  const float m = fmaxf(a.m, b.m);
  return Lse{m, a.s * shifted_exp(a.m, m) + b.s * shifted_exp(b.m, m)};
}
__device__ __forceinline__ Lse wave_lse(Lse v, int lane) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const Lse w{__shfl_xor(v.m, o), __shfl_xor(v.s, o)};
    const bool up = (lane & o) != 0;
    const float lm = up ? w.m : v.m, ls = up ? w.s : v.s, hm = up ? v.m : w.m, hs = up ? v.s : w.s;
    v = lse_merge(Lse{lm, ls}, Lse{hm, hs});
  }
  return v;
}
__device__ __forceinline__ float lse_value(Lse a) { return a.m + logf(a.s); }

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The taxonomy as the three kernels read it.  Every table entry is clamped into the range it
// indexes before it is followed: a malformed table gives wrong numbers, never a stray access.
struct Tree {
  int off[kTiers + 1];  // tier t = columns [off[t], off[t + 1])
  const int* parents;   // [off[7] - off[1]]
  const int* sib_ptr;   // [1 + off[6] + 1]
  const int* sib_col;   // [off[7]] or null: the identity
};
// CSR positions [lo, hi) of group g, whose children are nodes of tier t
__device__ __forceinline__ void group_range(const Tree& T, int t, int g, int& lo, int& hi) {
  lo = clampi(T.sib_ptr[g], T.off[t], T.off[t + 1]);
  hi = clampi(T.sib_ptr[g + 1], lo, T.off[t + 1]);
}
__device__ __forceinline__ int group_col(const Tree& T, int t, int j) {
  return T.sib_col ? clampi(T.sib_col[j], T.off[t], T.off[t + 1] - 1) : j;
}
__device__ __forceinline__ int parent_of(const Tree& T, int t, int n) {  // t >= 1, n in tier t
  return T.parents[HVK_BCHECK(T.off[t] - T.off[1] + n, T.off[kTiers] - T.off[1])];
}

// the target path of row b: y[t], valid when every id is in its tier and parent(y_t) == y_{t-1}
__device__ __forceinline__ bool load_path(const Tree& T, const int64_t* tgt, int b, int (&y)[kTiers]) {
  bool ok = true;
#pragma unroll
  for (int t = 0; t < kTiers; ++t) {
    const int64_t v = tgt[(size_t)b * kTiers + t];
    const bool in = v >= 0 && v < T.off[t + 1] - T.off[t];
    y[t] = in ? (int)v : 0;
    ok = ok && in;
  }
#pragma unroll
  for (int t = 1; t < kTiers; ++t) ok = ok && parent_of(T, t, y[t]) == y[t - 1];
  return ok;
}

// ================================================================================ forward
struct FwdArgs {
  const void* logits;
  int bf16, B, ld;
  Tree T;
  const int64_t* tgt;  // [B, 7]
  float lam[kTiers];
  float eps;
  float* row_loss;  // [B]
  float* lse;       // [B, 7]
  float* tier_nll;  // [B, 7]
};

__global__ __launch_bounds__(kThreads) void cond_fwd_kernel(FwdArgs a) {
  const int lane = threadIdx.x & 63, b = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (b >= a.B) return;  // no barrier below
  const Tree& T = a.T;
  const char* row = static_cast<const char*>(a.logits) + (size_t)b * a.ld * (a.bf16 ? 2 : 4);
  int y[kTiers];
  const bool ok = load_path(T, a.tgt, b, y);
  const float nanf_ = __builtin_nanf("");
  float loss = 0.f;
#pragma unroll
  for (int t = 0; t < kTiers; ++t) {
    int lo, hi;
    group_range(T, t, t ? 1 + T.off[t - 1] + y[t - 1] : 0, lo, hi);
    Lse acc{-INFINITY, 0.f};
    float sum = 0.f;
    for (int j = lo + lane; j < hi; j += 64) {
      const float x = load1(row, a.bf16, HVK_BCHECK(group_col(T, t, j), a.ld));
      acc = lse_push(acc, x);
      sum += x;
    }
    acc = wave_lse(acc, lane);
    sum = wave_sum_ordered(sum, lane);
    const float l = lse_value(acc);
    const float zy = load1(row, a.bf16, HVK_BCHECK(T.off[t] + y[t], a.ld));
    // (LSE - z_y) + eps (z_y - mean): LSE - (1 - eps) z_y - eps mean, exactly 0 for an only child
    const float nll = ok ? __builtin_fmaf(a.eps, zy - sum / (float)(hi - lo), l - zy) : nanf_;
    loss = __builtin_fmaf(a.lam[t], nll, loss);
    if (lane == 0) {
      a.lse[(size_t)b * kTiers + t] = ok ? l : nanf_;
      a.tier_nll[(size_t)b * kTiers + t] = nll;
    }
  }
  if (lane == 0) a.row_loss[b] = loss;
}

// ================================================================================ backward
struct BwdArgs {
  const void* logits;
  int bf16, B, ld;
  Tree T;
  const int64_t* tgt;
  float lam[kTiers];
  float eps;
  const float* lse;   // [B, 7]
  const float* gout;  // [1]
  void* dlogits;      // [B, ldg], the logits' dtype, 16-B aligned rows
  int ldg;
};

template <bool BF16, bool IDENT>
__global__ __launch_bounds__(kThreads) void cond_bwd_kernel(BwdArgs a) {
  constexpr int esz = BF16 ? 2 : 4, N = 16 / esz;
  const int b = blockIdx.y;
  const Tree& T = a.T;
  const int ncol = T.off[kTiers], nvec = a.ldg / N;
  const char* row = static_cast<const char*>(a.logits) + (size_t)b * a.ld * esz;
  char* grow = static_cast<char*>(a.dlogits) + (size_t)b * a.ldg * esz;
  int y[kTiers];
  const bool ok = load_path(T, a.tgt, b, y);
  // per tier (row-uniform, so scalar registers): the active column interval (identity), the saved
  // LSE, lam_t gout / B, eps / |g_t|
  int lo[kTiers], hi[kTiers];
  float lse[kTiers], coef[kTiers], epsn[kTiers];
  const float scale = a.gout[0] / (float)a.B;
#pragma unroll
  for (int t = 0; t < kTiers; ++t) {
    group_range(T, t, t ? 1 + T.off[t - 1] + y[t - 1] : 0, lo[t], hi[t]);
    lse[t] = a.lse[(size_t)b * kTiers + t];
    coef[t] = a.lam[t] * scale;
    epsn[t] = a.eps / (float)(hi[t] - lo[t]);
  }
  const float nanf_ = __builtin_nanf("");
#pragma unroll
  for (int u = 0; u < kBwdVecs; ++u) {
    const int v = (blockIdx.x * kBwdVecs + u) * kThreads + threadIdx.x;
    if (v >= nvec) continue;
    const int c0 = v * N;
    float g[N];
#pragma unroll
    for (int e = 0; e < N; ++e) g[e] = 0.f;
    bool any = !ok && c0 < ncol;
    if constexpr (IDENT) {
#pragma unroll
      for (int t = 0; t < kTiers; ++t) any = any || (c0 < hi[t] && c0 + N > lo[t]);
    } else {
      any = c0 < ncol;  // membership is per column, through its parent
    }
    if (any) {
#pragma unroll
      for (int e = 0; e < N; ++e) {
        const int c = c0 + e;
        if (c >= ncol) continue;  // pad columns: zeros
        if (!ok) {  // not a path of the taxonomy: a NaN gradient row, as the loss is NaN
          g[e] = nanf_;
          continue;
        }
        int t = -1;
        if constexpr (IDENT) {
#pragma unroll
          for (int q = 0; q < kTiers; ++q) t = (c >= lo[q] && c < hi[q]) ? q : t;
        } else {
#pragma unroll
          for (int q = 0; q < kTiers; ++q)
            if (c >= T.off[q] && c < T.off[q + 1] && (q == 0 || parent_of(T, q, c - T.off[q]) == y[q ? q - 1 : 0])) t = q;
        }
        if (t < 0) continue;
        // softmax_g(c) - (1 - eps) [c = y_t] - eps / |g| as (p - [c = y]) + eps ([c = y] - 1 / |g|):
        // exactly 0 for an only child (p = 1)
        float l = lse[0], cf = coef[0], en = epsn[0];
        int yc = T.off[0] + y[0];
#pragma unroll
        for (int q = 1; q < kTiers; ++q)
          if (t == q) l = lse[q], cf = coef[q], en = epsn[q], yc = T.off[q] + y[q];
        const float p = expf(load1(row, BF16, HVK_BCHECK(c, a.ld)) - l);
        const float hot = c == yc ? 1.f : 0.f;
        g[e] = cf * ((p - hot) + (a.eps * hot - en));
      }
    }
    uint4 w;
    if constexpr (BF16) {
      w = hvk_pack8(g);
    } else {
      w = make_uint4(__float_as_uint(g[0]), __float_as_uint(g[1]), __float_as_uint(g[2]), __float_as_uint(g[3]));
    }
    hvk_st16(grow + (size_t)HVK_BCHECK(v, nvec) * 16, w);
  }
}

// ================================================================================ decode
struct DecArgs {
  const void* logits;
  int bf16, B, ld;
  Tree T;
  const int64_t* targets;
  int t_stride, t_off;
  const int* leaf_paths;  // [L, 7]
  int* pred;
  int* rank;
  float* nll;
  float* lse;
  int* dist;
  unsigned char* tier_hit;
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

// log p of a child given its group's LSE, on top of its parent's path score
__device__ __forceinline__ float child_score(float z, float lse, float base) { return (z - lse) + base; }

// The LSE of CSR positions [lo, hi) by the path its width selects; `get(j)` is the logit at position
// j.  Narrow: every calling lane walks the group alone, in order.  Wide: the 64 lanes stride over
// it and fold their partial sums in a lane-ordered butterfly (all lanes must call, lo / hi uniform).
template <class Get>
__device__ __forceinline__ float narrow_lse(int lo, int hi, Get get) {
  Lse acc{-INFINITY, 0.f};
  for (int j = lo; j < hi; ++j) acc = lse_push(acc, get(j));
  return lse_value(acc);
}
template <class Get>
__device__ __forceinline__ float wide_lse(int lo, int hi, int lane, Get get) {
  Lse acc{-INFINITY, 0.f};
  for (int j = lo + lane; j < hi; j += 64) acc = lse_push(acc, get(j));
  return lse_value(wave_lse(acc, lane));
}

// One tier's pass over its parents: parent p of [0, n_par) owns group g0 + p; get(j) reads the
// logit of CSR position j, put(j, lse, p) rewrites / consumes the child.  A wave takes the parents
// 64 at a time (chunks wave, wave + 4, ...).
template <class Get, class Put>
__device__ __forceinline__ void tier_pass(const Tree& T, int t, int g0, int n_par, int tid, Get get, Put put) {
  const int lane = tid & 63;
  for (int p0 = (tid >> 6) * 64; p0 < n_par; p0 += kThreads) {
    const int p = p0 + lane;
    int lo = 0, hi = 0;
    if (p < n_par) group_range(T, t, g0 + p, lo, hi);
    const bool wide = hi - lo > kSplit;
    if (!wide && hi > lo) {
      const float l = narrow_lse(lo, hi, get);
      for (int j = lo; j < hi; ++j) put(j, l, p);
    }
    unsigned long long todo = __ballot(wide);
    while (todo) {  // wave-uniform
      const int src = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const int wlo = __shfl(lo, src), whi = __shfl(hi, src), wp = p0 + src;
      const float l = wide_lse(wlo, whi, lane, get);
      for (int j = wlo + lane; j < whi; j += 64) put(j, l, wp);
    }
  }
}

template <bool BF16, bool SCORES>
__global__ __launch_bounds__(kThreads) void cond_decode_kernel(DecArgs a) {
  constexpr int esz = BF16 ? 2 : 4, N = 16 / esz;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  __shared__ RowAcc leaf_part[kWaves];
  const int b = blockIdx.x, tid = threadIdx.x;
  const Tree& T = a.T;
  const char* row = static_cast<const char*>(a.logits) + (size_t)b * a.ld * esz;
  const int nc = T.off[kCoarse], L = T.off[kTiers] - nc;
  const float nanf_ = __builtin_nanf("");

  // ---- tiers 0-5 -> LDS (f32), one HBM read per logit (joint.hip's staging) ---------------------
  float* c;
  {
    const uintptr_t ad = (uintptr_t)row;
    int head = (ad & (esz - 1)) ? nc : (int)(((16 - (ad & 15)) & 15) / esz);
    head = head < nc ? head : nc;
    const int nv = (nc - head) / N, done = head + nv * N;
    c = lds + ((4 - (head & 3)) & 3);  // c[head + v N] is 16-B aligned in LDS
    for (int j = tid; j < head; j += kThreads) c[j] = load1(row, BF16, HVK_BCHECK(j, nc));
    for (int j = done + tid; j < nc; j += kThreads) c[j] = load1(row, BF16, HVK_BCHECK(j, nc));
    const char* body = row + (size_t)head * esz;
    constexpr int UN = 4;
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

  // ---- top-down over the coarse tiers, in place: c_t[child] = (z - LSE_g) + c_{t-1}[parent] ------
#pragma unroll
  for (int t = 0; t < kCoarse; ++t) {
    const int n_par = t ? T.off[t] - T.off[t - 1] : 1, g0 = t ? 1 + T.off[t - 1] : 0;
    const float* above = t ? c + T.off[t - 1] : nullptr;
    tier_pass(T, t, g0, n_par, tid, [&](int j) { return c[group_col(T, t, j)]; },
              [&](int j, float l, int p) {
                const int col = group_col(T, t, j);
                c[col] = child_score(c[col], l, above ? above[p] : 0.f);
              });
    __syncthreads();
  }

  // ---- the leaf tier: the same pass over the genus nodes, children in global memory --------------
  const int n5 = nc - T.off[kCoarse - 1], g5 = 1 + T.off[kCoarse - 1];
  const float* c5 = c + T.off[kCoarse - 1];
  const auto zleaf = [&](int j) { return load1(row, BF16, HVK_BCHECK(group_col(T, kCoarse, j), a.ld)); };
  const int64_t t64 = a.targets[(size_t)b * a.t_stride + a.t_off];
  const bool valid = t64 >= 0 && t64 < L;
  const int tl = valid ? (int)t64 : -1;
  // the target's score by the sweep's own path and expression: bitwise the s_k met at k == t
  float st = nanf_;
  if (valid) {
    const int p = clampi(parent_of(T, kCoarse, tl), 0, n5 - 1);
    int lo, hi;
    group_range(T, kCoarse, g5 + p, lo, hi);
    const float l = hi - lo > kSplit ? wide_lse(lo, hi, tid & 63, zleaf) : narrow_lse(lo, hi, zleaf);
    st = child_score(load1(row, BF16, HVK_BCHECK(nc + tl, a.ld)), l, c5[p]);
  }
  float* srow = SCORES ? a.scores + (size_t)b * L : nullptr;
  RowAcc acc{-INFINITY, kNoIdx, 0.f, 0};
  tier_pass(T, kCoarse, g5, n5, tid, zleaf, [&](int j, float l, int p) {
    const int k = group_col(T, kCoarse, j) - nc;
    const float s[1] = {child_score(load1(row, BF16, HVK_BCHECK(nc + k, a.ld)), l, c5[p])};
    if constexpr (SCORES) srow[HVK_BCHECK(k, L)] = s[0];
    acc = push_group<1>(acc, s, k, st, tl);
  });
  acc = wave_merge(acc, tid);
  if ((tid & 63) == 0) leaf_part[tid >> 6] = acc;
  __syncthreads();
  if (tid != 0) return;
  acc = leaf_part[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) acc = merge(acc, leaf_part[w]);

  const int pred = (acc.mi >= 0 && acc.mi < L) ? acc.mi : 0;
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
      if (a.leaf_paths[(size_t)HVK_BCHECK(pred, L) * kTiers + q] == a.leaf_paths[(size_t)HVK_BCHECK(tl, L) * kTiers + q]) {
        hit |= 1u << q;
        dist = kTiers - 1 - q;
      }
    }
  }
  a.dist[b] = dist;
  a.tier_hit[b] = (unsigned char)hit;
}

// ================================================================================ host
// null: fine; else what is wrong with the tier offsets (decode: also the LDS limit)
const char* check_offsets(const int* off, bool decode, char* buf, size_t cap) {
  if (!off) return "null tier_off";
  if (off[0] != 0) return "tier_off[0] must be 0";
  for (int t = 0; t < kTiers; ++t)
    if (off[t + 1] <= off[t]) return "tier_off must grow strictly (every tier holds a node)";
  if (off[kTiers] - off[kCoarse] > kMaxLeaves) return "more than 2^24 leaves";
  if (decode && off[kCoarse] > kMaxCoarse) {
    snprintf(buf, cap, "tiers 0-5 hold %d nodes, above the %d f32 values (60 KB) one workgroup keeps in LDS",
             off[kCoarse], kMaxCoarse);
    return buf;
  }
  return nullptr;
}

Tree make_tree(const int* off, const int* parents, const int* sib_ptr, const int* sib_col) {
  Tree T{};
  for (int t = 0; t <= kTiers; ++t) T.off[t] = off[t];
  T.parents = parents, T.sib_ptr = sib_ptr, T.sib_col = sib_col;
  return T;
}

// the arguments the loss's two directions share
int check_loss(const char* who, const void* logits, int dtype, int B, int ld, const int* off, const int64_t* targets,
               const int* parents, const int* sib_ptr, const float* coeffs, float smoothing) {
  char buf[160];
  if (const char* why = check_offsets(off, false, buf, sizeof(buf))) return hvk_set_error(HVK_EINVAL, "%s: %s", who, why);
  if (B < 0 || ld < off[kTiers])
    return hvk_set_error(HVK_EINVAL, "%s: bad shape (B %d, ld %d < %d columns)", who, B, ld, off[kTiers]);
  if (dtype != 0 && dtype != 1) return hvk_set_error(HVK_EINVAL, "%s: unknown logits dtype %d (0 f32, 1 bf16)", who, dtype);
  if (!logits || !targets || !parents || !sib_ptr || !coeffs) return hvk_set_error(HVK_EINVAL, "%s: null pointer", who);
  for (int t = 0; t < kTiers; ++t)
    if (!(coeffs[t] >= 0.f) || isinf(coeffs[t]))
      return hvk_set_error(HVK_EINVAL, "%s: coefficient %d = %g (finite, >= 0)", who, t, (double)coeffs[t]);
  if (!(smoothing >= 0.f && smoothing < 1.f))
    return hvk_set_error(HVK_EINVAL, "%s: smoothing %g outside [0, 1)", who, (double)smoothing);
  return HVK_OK;
}

}  // namespace

extern "C" {

int hvk_cond_softmax_supported(const int* tier_off) {
  char buf[160];
  return check_offsets(tier_off, true, buf, sizeof(buf)) == nullptr;
}

int hvk_cond_softmax_fwd(const void* logits, int logits_dtype, int B, int ld, const int* tier_off,
                         const int64_t* targets, const int* parents, const int* sib_ptr, const int* sib_col,
                         const float* coeffs, float smoothing, float* row_loss, float* lse, float* tier_nll,
                         void* stream) {
  if (int rc = check_loss("hvk_cond_softmax_fwd", logits, logits_dtype, B, ld, tier_off, targets, parents, sib_ptr,
                          coeffs, smoothing))
    return rc;
  if (!row_loss || !lse || !tier_nll) return hvk_set_error(HVK_EINVAL, "hvk_cond_softmax_fwd: null pointer");
  if (B == 0) return HVK_OK;
  FwdArgs a{};
  a.logits = logits, a.bf16 = logits_dtype, a.B = B, a.ld = ld;
  a.T = make_tree(tier_off, parents, sib_ptr, sib_col);
  a.tgt = targets, a.eps = smoothing, a.row_loss = row_loss, a.lse = lse, a.tier_nll = tier_nll;
  for (int t = 0; t < kTiers; ++t) a.lam[t] = coeffs[t];
  hipLaunchKernelGGL(cond_fwd_kernel, dim3(ceil_div(B, kWaves)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
  HVK_CHECK_LAUNCH("cond_softmax_fwd");
  return HVK_OK;
}

int hvk_cond_softmax_bwd(const void* logits, int logits_dtype, int B, int ld, const int* tier_off,
                         const int64_t* targets, const int* parents, const int* sib_ptr, const int* sib_col,
                         const float* coeffs, float smoothing, const float* lse, const float* gout, void* dlogits,
                         int ldg, void* stream) {
  if (int rc = check_loss("hvk_cond_softmax_bwd", logits, logits_dtype, B, ld, tier_off, targets, parents, sib_ptr,
                          coeffs, smoothing))
    return rc;
  if (!lse || !gout || !dlogits) return hvk_set_error(HVK_EINVAL, "hvk_cond_softmax_bwd: null pointer");
  const int N = logits_dtype ? 8 : 4;
  if (ldg < tier_off[kTiers] || ldg % N != 0 || ((uintptr_t)dlogits & 15))
    return hvk_set_error(HVK_EINVAL,
                         "hvk_cond_softmax_bwd: gradient rows of %d elements at %p (>= %d columns, whole 16-B "
                         "vectors, 16-B aligned)", ldg, dlogits, tier_off[kTiers]);
  if (B == 0) return HVK_OK;
  if (B > 65535) return hvk_set_error(HVK_EUNSUPPORTED, "hvk_cond_softmax_bwd: B %d above 65535 rows a launch", B);
  BwdArgs a{};
  a.logits = logits, a.bf16 = logits_dtype, a.B = B, a.ld = ld;
  a.T = make_tree(tier_off, parents, sib_ptr, sib_col);
  a.tgt = targets, a.eps = smoothing, a.lse = lse, a.gout = gout, a.dlogits = dlogits, a.ldg = ldg;
  for (int t = 0; t < kTiers; ++t) a.lam[t] = coeffs[t];
  const dim3 grid(ceil_div(ldg / N, kThreads * kBwdVecs), B);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (logits_dtype) {
    if (sib_col) hipLaunchKernelGGL((cond_bwd_kernel<true, false>), grid, dim3(kThreads), 0, st, a);
    else hipLaunchKernelGGL((cond_bwd_kernel<true, true>), grid, dim3(kThreads), 0, st, a);
  } else {
    if (sib_col) hipLaunchKernelGGL((cond_bwd_kernel<false, false>), grid, dim3(kThreads), 0, st, a);
    else hipLaunchKernelGGL((cond_bwd_kernel<false, true>), grid, dim3(kThreads), 0, st, a);
  }
  HVK_CHECK_LAUNCH("cond_softmax_bwd");
  return HVK_OK;
}

int hvk_cond_softmax_decode(const void* logits, int logits_dtype, int B, int ld, const int* tier_off,
                            const int64_t* targets, int t_stride, int t_off, const int* parents,
                            const int* sib_ptr, const int* sib_col, const int* leaf_paths, int topk, int* pred,
                            int* rank, float* nll, float* lse, int* dist, unsigned char* tier_hit, float* scores,
                            double* state, void* stream) {
  char buf[160];
  if (const char* why = check_offsets(tier_off, true, buf, sizeof(buf)))
    return hvk_set_error(tier_off && tier_off[0] == 0 && tier_off[kCoarse] > kMaxCoarse ? HVK_EUNSUPPORTED : HVK_EINVAL,
                         "hvk_cond_softmax_decode: %s", why);
  if (B < 0 || ld < tier_off[kTiers])
    return hvk_set_error(HVK_EINVAL, "hvk_cond_softmax_decode: bad shape (B %d, ld %d < %d columns)", B, ld,
                         tier_off[kTiers]);
  if (topk < 1) return hvk_set_error(HVK_EINVAL, "hvk_cond_softmax_decode: topk %d < 1", topk);
  if (t_stride < 1 || t_off < 0 || t_off >= t_stride)
    return hvk_set_error(HVK_EINVAL, "hvk_cond_softmax_decode: target stride %d / offset %d", t_stride, t_off);
  if (logits_dtype != 0 && logits_dtype != 1)
    return hvk_set_error(HVK_EINVAL, "hvk_cond_softmax_decode: unknown logits dtype %d (0 f32, 1 bf16)", logits_dtype);
  if (!logits || !targets || !parents || !sib_ptr || !leaf_paths || !pred || !rank || !nll || !lse || !dist ||
      !tier_hit || !state)
    return hvk_set_error(HVK_EINVAL, "hvk_cond_softmax_decode: null pointer");
  if (B == 0) return HVK_OK;
  DecArgs a{};
  a.logits = logits, a.bf16 = logits_dtype, a.B = B, a.ld = ld;
  a.T = make_tree(tier_off, parents, sib_ptr, sib_col);
  a.targets = targets, a.t_stride = t_stride, a.t_off = t_off, a.leaf_paths = leaf_paths;
  a.pred = pred, a.rank = rank, a.nll = nll, a.lse = lse, a.dist = dist, a.tier_hit = tier_hit, a.scores = scores;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t lds = (size_t)(tier_off[kCoarse] + 4) * sizeof(float);
  const int L = tier_off[kTiers] - tier_off[kCoarse];
  if (logits_dtype) {
    if (scores) hipLaunchKernelGGL((cond_decode_kernel<true, true>), dim3(B), dim3(kThreads), lds, st, a);
    else hipLaunchKernelGGL((cond_decode_kernel<true, false>), dim3(B), dim3(kThreads), lds, st, a);
  } else {
    if (scores) hipLaunchKernelGGL((cond_decode_kernel<false, true>), dim3(B), dim3(kThreads), lds, st, a);
    else hipLaunchKernelGGL((cond_decode_kernel<false, false>), dim3(B), dim3(kThreads), lds, st, a);
  }
  HVK_CHECK_LAUNCH("cond_softmax_decode");
  hvk_eval_accumulate_launch(B, topk < L ? topk : L, rank, nll, dist, tier_hit, state, st);
  HVK_CHECK_LAUNCH("eval_accumulate");
  return HVK_OK;
}

}  // extern "C"
