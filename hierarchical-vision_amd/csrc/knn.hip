// Weighted k-nearest-neighbour evaluation on gfx950 (Wu et al., CVPR 2018): the k largest
// similarities q . b of every query row over a bank of L2-normalised bf16 rows, and the weighted
// vote of those neighbours, flat and top-down through the taxonomy.
//
// * knn_topk_kernel -- a workgroup holds 64 query rows (a wave 16 of them) against a range of
//   64-row bank tiles.  Query and bank chunks of KC columns pass through a double-buffered LDS
//   stage, the next chunk's global loads in flight under the current chunk's bf16 MFMAs
//   (16x16x32, f32 accumulation).  A score is the chain of D / 32 MFMAs of its own (row, column)
//   cell from zero, in ascending k: it does not depend on the tile or the split the bank row
//   falls in.  Scores leave the accumulators only through the selection: every row keeps its
//   running k best in LDS (order-preserving u32 keys and bank indices) and its k-th best as a
//   float in a register of the 16 lanes that share the row; an accumulator element is compared
//   with it, the wave ballots, and the rare survivors are inserted one at a time by the whole
//   wave: replace the worst entry, rescan the k entries (k / 64 per lane) for the new worst with
//   two DPP / permlane reductions.  Only the owning wave touches a row's list.
// * knn_merge_kernel -- one wave per query row: the splits' lists pass through the same
//   insertion into one list, which a rank sort writes out by (similarity descending, bank index
//   ascending); the order of equal similarities is decided by the comparison, never by arrival.
// * knn_vote_kernel -- one wave per query row: weights exp((s_i - s_0) / temperature) and the
//   neighbours' tier ids in LDS; a neighbour's vote is the sum over the neighbours of the same
//   label in ascending rank (pairwise comparisons, no per-class array), for up to 8 prefixes k_j;
//   flat on the leaf column, and top-down with the neighbours outside the node just chosen masked.
// No atomics anywhere: equal inputs give bit-identical outputs, for any number of splits.
#include <math.h>

#include "eval_common.h"

using namespace hvk_eval;

namespace {

constexpr int kBM = 64;         // query rows per workgroup, bank rows per tile
constexpr int kMaxK = 256;      // neighbours
constexpr int kMaxD = 1024;     // feature width
constexpr int kMaxKs = 8;       // prefixes per vote launch
constexpr int kLdsLimit = 160 * 1024;
constexpr uint32_t kPadKey = 0x007fffffu;  // okey(-inf)

// f32 -> u32 whose unsigned order is the float order (no NaN gets here), and back
__device__ __forceinline__ uint32_t okey(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float okey_inv(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// min / max over the wave, VALU only (DPP inside a row of 16, permlane swaps across rows); every
// lane returns the result.  Every lane of the wave must execute them.
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_u32(uint32_t x) {
  return (uint32_t)__builtin_amdgcn_mov_dpp((int)x, CTRL, 0xF, 0xF, false);
}
template <bool MAX>
__device__ __forceinline__ uint32_t pick_u32(uint32_t a, uint32_t b) {
  return MAX ? (a > b ? a : b) : (a < b ? a : b);
}
template <bool MAX>
__device__ __forceinline__ uint32_t wave_minmax_u32(uint32_t v) {
  v = pick_u32<MAX>(v, dpp_u32<0xB1>(v));   // quad_perm [1,0,3,2]
  v = pick_u32<MAX>(v, dpp_u32<0x4E>(v));   // quad_perm [2,3,0,1]
  v = pick_u32<MAX>(v, dpp_u32<0x141>(v));  // row_half_mirror
  v = pick_u32<MAX>(v, dpp_u32<0x140>(v));  // row_mirror
  const auto a = __builtin_amdgcn_permlane16_swap(v, v, false, false);
  v = pick_u32<MAX>(a[0], a[1]);
  const auto b = __builtin_amdgcn_permlane32_swap(v, v, false, false);
  return pick_u32<MAX>(b[0], b[1]);
}

// One row's running k best in LDS, unordered: keys ks[k], bank indices is[k], and the worst entry
// (lowest key, among equals the highest index as u32: a pad's -1 is the worst of all) as
// w[0] key, w[1] index, w[2] position.  Used by one wave at a time; volatile keeps the program
// order of the LDS accesses, which the in-order LDS queue of a wave turns into visibility.
struct RowList {
  volatile uint32_t* ks;
  volatile int* is;
  volatile uint32_t* w;
};

__device__ __forceinline__ uint32_t list_rescan(const RowList& l, int k, int lane) {
  uint32_t ms = 0xffffffffu, mi = 0u;
  int mp = 0;
  for (int e = lane; e < k; e += 64) {
    const uint32_t s = l.ks[e], i = (uint32_t)l.is[e];
    if (s < ms || (s == ms && i >= mi)) ms = s, mi = i, mp = e;
  }
  const uint32_t gs = wave_minmax_u32<false>(ms);
  const uint32_t gi = wave_minmax_u32<true>(ms == gs ? mi : 0u);
  const unsigned long long b = __ballot(ms == gs && mi == gi);  // several lanes: equal pads
  const int src = b ? __ffsll((long long)b) - 1 : 0;
  const int p = __builtin_amdgcn_readlane(mp, __builtin_amdgcn_readfirstlane(src));
  if (lane == 0) l.w[0] = gs, l.w[1] = gi, l.w[2] = (uint32_t)p;
  return gs;
}

// the candidate (key, idx) against the row's worst; returns the worst key afterwards
__device__ __forceinline__ uint32_t list_insert(const RowList& l, int k, uint32_t key, int idx, int lane) {
  const uint32_t ws = __builtin_amdgcn_readfirstlane(l.w[0]);
  const uint32_t wi = __builtin_amdgcn_readfirstlane(l.w[1]);
  if (!(key > ws || (key == ws && (uint32_t)idx < wi))) return ws;
  const int p = (int)__builtin_amdgcn_readfirstlane(l.w[2]);
  if (lane == 0 && p >= 0 && p < k) l.ks[p] = key, l.is[p] = idx;
  return list_rescan(l, k, lane);
}

__device__ __forceinline__ void list_clear(const RowList& l, int k, int lane) {
  for (int e = lane; e < k; e += 64) l.ks[e] = kPadKey, l.is[e] = -1;
  if (lane == 0) l.w[0] = kPadKey, l.w[1] = 0xffffffffu, l.w[2] = 0u;
}

// ---------------------------------------------------------------------------------- top-k
template <int KC>
struct Chunk {
  static constexpr int kLd = KC + 8;         // halves per LDS row: 16-B reads of 16 rows hit 64 banks
  static constexpr int kGran = KC / 8;       // 16-B granules per row
  static constexpr int kPer = kBM * kGran / kThreads;  // granules per thread
  static constexpr int kHalves = kBM * kLd;  // one operand of one stage
};

template <int KC>
__device__ __forceinline__ void chunk_load(const hvk_bf16* __restrict__ base, int rows, int row0, int D, int k0,
                                           int tid, uint4 (&r)[Chunk<KC>::kPer]) {
#pragma unroll
  for (int i = 0; i < Chunk<KC>::kPer; ++i) {
    const int gi = tid + kThreads * i;
    const int row = row0 + gi / Chunk<KC>::kGran, kk = k0 + (gi % Chunk<KC>::kGran) * 8;
    r[i] = make_uint4(0u, 0u, 0u, 0u);
    // D % 8 == 0 and a 16-byte aligned base (hvk_knn_topk): whole granules
    if (row < rows && kk < D) r[i] = *reinterpret_cast<const uint4*>(base + (size_t)HVK_BCHECK(row, rows) * D + kk);
  }
}
template <int KC>
__device__ __forceinline__ void chunk_store(hvk_bf16* lds, int tid, const uint4 (&r)[Chunk<KC>::kPer]) {
#pragma unroll
  for (int i = 0; i < Chunk<KC>::kPer; ++i) {
    const int gi = tid + kThreads * i;
    *reinterpret_cast<uint4*>(lds + (gi / Chunk<KC>::kGran) * Chunk<KC>::kLd + (gi % Chunk<KC>::kGran) * 8) = r[i];
  }
}

size_t topk_lds_bytes(int KC, int k) {
  return (size_t)4 * kBM * (KC + 8) * sizeof(hvk_bf16) + (size_t)kBM * k * 8 + (size_t)kBM * 3 * 4;
}

template <int KC>
__global__ __launch_bounds__(kThreads) void knn_topk_kernel(const hvk_bf16* __restrict__ q, int B,
                                                           const hvk_bf16* __restrict__ bank, int N, int D, int k,
                                                           int tiles_per_split, uint32_t* __restrict__ pkey,
                                                           int* __restrict__ pidx) {
  using C = Chunk<KC>;
  extern __shared__ __attribute__((aligned(16))) unsigned char knn_lds[];
  hvk_bf16* stage = reinterpret_cast<hvk_bf16*>(knn_lds);  // [2][q | bank][kBM][kLd]
  uint32_t* lkey = reinterpret_cast<uint32_t*>(stage + 4 * C::kHalves);
  int* lidx = reinterpret_cast<int*>(lkey + kBM * k);
  uint32_t* lworst = reinterpret_cast<uint32_t*>(lidx + kBM * k);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int m0 = blockIdx.x * kBM, split = blockIdx.y;
  const int tiles = ceil_div(N, kBM);
  const int t_lo = split * tiles_per_split;
  const int t_hi = t_lo + tiles_per_split < tiles ? t_lo + tiles_per_split : tiles;
  const int ksteps = ceil_div(D, KC);

  auto row_list = [&](int r) {
    return RowList{lkey + r * k, lidx + r * k, lworst + r * 3};
  };
  for (int r = 0; r < 16; ++r) list_clear(row_list(wave * 16 + r), k, lane);

  float thr[4];
  bool row_ok[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    thr[r] = -INFINITY;
    row_ok[r] = m0 + wave * 16 + 4 * g + r < B;
  }

  uint4 rq[C::kPer], rb[C::kPer];
  int cur = 0;
  if (t_lo < t_hi) {
    chunk_load<KC>(q, B, m0, D, 0, tid, rq);
    chunk_load<KC>(bank, N, t_lo * kBM, D, 0, tid, rb);
    chunk_store<KC>(stage, tid, rq);
    chunk_store<KC>(stage + C::kHalves, tid, rb);
  }
  __syncthreads();

  for (int t = t_lo; t < t_hi; ++t) {
    hvk_f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = hvk_f32x4{0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < ksteps; ++s) {
      const bool last = s + 1 == ksteps;
      const bool more = !last || t + 1 < t_hi;
      if (more) {  // the next chunk's loads fly under this chunk's MFMAs
        chunk_load<KC>(q, B, m0, D, last ? 0 : (s + 1) * KC, tid, rq);
        chunk_load<KC>(bank, N, (last ? t + 1 : t) * kBM, D, last ? 0 : (s + 1) * KC, tid, rb);
      }
      const hvk_bf16* qs = stage + cur * 2 * C::kHalves;
      const hvk_bf16* bs = qs + C::kHalves;
#pragma unroll
      for (int u = 0; u < KC / 32; ++u) {
        const uint4 a = *reinterpret_cast<const uint4*>(qs + (wave * 16 + li) * C::kLd + u * 32 + 8 * g);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint4 b = *reinterpret_cast<const uint4*>(bs + (16 * j + li) * C::kLd + u * 32 + 8 * g);
          acc[j] = hvk_mfma16(a, b, acc[j]);
        }
      }
      if (more) {
        hvk_bf16* nq = stage + (cur ^ 1) * 2 * C::kHalves;
        chunk_store<KC>(nq, tid, rq);
        chunk_store<KC>(nq + C::kHalves, tid, rb);
      }
      __syncthreads();  // the stage just read may be overwritten, the one just written read
      cur ^= 1;
    }
    hvk_settle(acc[0], acc[1], acc[2], acc[3]);
    // acc[j][r]: query row 4 g + r of the wave's 16 against bank row c0 + 16 j + li
    const int c0 = t * kBM;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool col_ok = c0 + 16 * j + li < N;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float sc = acc[j][r];
        unsigned long long m = __ballot(col_ok && row_ok[r] && sc >= thr[r]);  // a NaN never passes
        while (m) {  // wave-uniform; rare once the lists are warm
          const int src = __ffsll((long long)m) - 1;
          m &= m - 1;
          const float cs = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(sc), src));  // src: uniform
          const int gs = src >> 4;
          const uint32_t worst = list_insert(row_list(wave * 16 + 4 * gs + r), k, okey(cs), c0 + 16 * j + (src & 15), lane);
          if (g == gs) thr[r] = okey_inv(worst);
        }
      }
    }
  }
  // this split's lists, unordered
  for (int r = 0; r < 16; ++r) {
    const int row = m0 + wave * 16 + r;
    if (row >= B) break;
    const RowList l = row_list(wave * 16 + r);
    const size_t o = ((size_t)split * B + HVK_BCHECK(row, B)) * k;
    for (int e = lane; e < k; e += 64) pkey[o + e] = l.ks[e], pidx[o + e] = l.is[e];
  }
}

__global__ __launch_bounds__(64) void knn_merge_kernel(const uint32_t* __restrict__ pkey, const int* __restrict__ pidx,
                                                      int B, int k, int splits, float* __restrict__ sims,
                                                      int* __restrict__ idx) {
  __shared__ uint32_t lkey[kMaxK];
  __shared__ int lidx[kMaxK];
  __shared__ uint32_t lworst[3];
  const int lane = threadIdx.x, row = blockIdx.x;
  const RowList l{lkey, lidx, lworst};
  for (int e = lane; e < k; e += 64) {
    const size_t o = (size_t)HVK_BCHECK(row, B) * k + e;
    l.ks[e] = pkey[o], l.is[e] = pidx[o];
  }
  uint32_t worst = list_rescan(l, k, lane);
  for (int s = 1; s < splits; ++s) {
    const size_t o = ((size_t)s * B + row) * k;
    for (int e0 = 0; e0 < k; e0 += 64) {
      const int e = e0 + lane;
      const uint32_t key = e < k ? pkey[o + e] : 0u;
      const int ci = e < k ? pidx[o + e] : -1;
      unsigned long long m = __ballot(e < k && key >= worst);
      while (m) {
        const int src = __ffsll((long long)m) - 1;
        m &= m - 1;
        worst = list_insert(l, k, __builtin_amdgcn_readlane(key, src), __builtin_amdgcn_readlane(ci, src), lane);
      }
    }
  }
  // rank sort: (key descending, index ascending as u32, position among equal pads)
  for (int e = lane; e < k; e += 64) {
    const uint32_t s = l.ks[e], i = (uint32_t)l.is[e];
    int rank = 0;
    for (int f = 0; f < k; ++f) {
      const uint32_t sf = l.ks[f], jf = (uint32_t)l.is[f];
      rank += (sf > s || (sf == s && (jf < i || (jf == i && f < e)))) ? 1 : 0;
    }
    const size_t o = (size_t)row * k + HVK_BCHECK(rank, k);
    sims[o] = okey_inv(s);
    idx[o] = (int)i;
  }
}

struct TopkPlan {
  int KC, row_tiles, tiles, tiles_per_split, splits;
  size_t lds;
};
// the bank tiles over about two workgroups per CU in all, or one where the lists of a large k
// leave room for a single workgroup's LDS per CU (256 CUs); KC = 64 unless the lists leave room
// for 32-column stages only (k > 246)
TopkPlan topk_plan(int B, int N, int k, int splits) {
  TopkPlan p;
  p.KC = topk_lds_bytes(64, k) <= (size_t)kLdsLimit ? 64 : 32;
  p.lds = topk_lds_bytes(p.KC, k);
  p.row_tiles = ceil_div(B, kBM);
  p.tiles = ceil_div(N, kBM);
  int want = splits;
  if (want <= 0) want = (2 * p.lds <= (size_t)kLdsLimit ? 512 : 256) / (p.row_tiles > 0 ? p.row_tiles : 1);
  want = want < 1 ? 1 : (want > p.tiles ? p.tiles : want);
  p.tiles_per_split = ceil_div(p.tiles, want);
  p.splits = ceil_div(p.tiles, p.tiles_per_split);
  return p;
}

// ---------------------------------------------------------------------------------- vote
struct VoteArgs {
  const float* sims;
  const int* idx;
  const int* labels;
  int* leaf;
  int* path;
  int B, k, N, T, n_k;
  int ks[kMaxKs];
  float inv_temp;
};

// (vote, id) of lane a against b: the larger vote, among equal votes the lower id; id < 0: none
__device__ __forceinline__ void take_vote(float& v, int& id, float ov, int oid) {
  const bool t = oid >= 0 && (id < 0 || ov > v || (ov == v && oid < id));
  v = t ? ov : v;
  id = t ? oid : id;
}

// the node of tier t with the largest vote among the first kj neighbours whose tier-tm id is
// `parent` (tm < 0: all); a neighbour's vote is summed in ascending rank
__device__ __forceinline__ int vote_pick(const float* w, const int* lab, int T, int kj, int t, int tm, int parent,
                                         int lane) {
  float best = 0.f;
  int pick = -1;
  for (int i = lane; i < kj; i += 64) {
    const int id = lab[i * T + t];
    if (id < 0 || (tm >= 0 && lab[i * T + tm] != parent)) continue;
    float v = 0.f;
    for (int m = 0; m < kj; ++m)
      if (lab[m * T + t] == id && (tm < 0 || lab[m * T + tm] == parent)) v += w[m];
    take_vote(best, pick, v, id);
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const float ov = __shfl_xor(best, o);
    const int oid = __shfl_xor(pick, o);
    take_vote(best, pick, ov, oid);
  }
  return pick < 0 ? 0 : pick;  // no valid neighbour at all
}

__global__ __launch_bounds__(64) void knn_vote_kernel(VoteArgs a) {
  __shared__ float w[kMaxK];
  __shared__ int lab[kMaxK * 7];
  const int lane = threadIdx.x, row = blockIdx.x;
  const size_t o = (size_t)HVK_BCHECK(row, a.B) * a.k;
  const float s0 = a.sims[o];
  for (int i = lane; i < a.k; i += 64) {
    const int id = a.idx[o + i];
    const bool ok = id >= 0 && id < a.N;  // a pad (-1), or an index that names no bank row
    bool pos = ok;
    for (int t = 0; t < a.T; ++t) {
      const int v = ok ? a.labels[(size_t)id * a.T + t] : -1;
      pos = pos && v >= 0;
      lab[i * a.T + t] = v;
    }
    if (!pos)  // a negative tier id: the neighbour takes no part
      for (int t = 0; t < a.T; ++t) lab[i * a.T + t] = -1;
    w[i] = pos ? expf((a.sims[o + i] - s0) * a.inv_temp) : 0.f;
  }
  __syncthreads();
  for (int j = 0; j < a.n_k; ++j) {
    const int kj = a.ks[j];
    const int leaf = vote_pick(w, lab, a.T, kj, a.T - 1, -1, 0, lane);
    if (lane == 0) a.leaf[(size_t)j * a.B + row] = leaf;
    int chosen = 0;
    for (int t = 0; t < a.T; ++t) {
      chosen = vote_pick(w, lab, a.T, kj, t, t - 1, chosen, lane);
      if (lane == 0) a.path[((size_t)j * a.B + row) * a.T + t] = chosen;
    }
  }
}

// null: supported; else why not
const char* unsupported(int D, int k, char* buf, size_t cap) {
  if (D % 8 || D > kMaxD) {
    snprintf(buf, cap, "D %d (a multiple of 8, at most %d)", D, kMaxD);
    return buf;
  }
  if (k > kMaxK) {
    snprintf(buf, cap, "k %d above %d", k, kMaxK);
    return buf;
  }
  return nullptr;
}

template <int KC>
int launch_topk(const TopkPlan& p, const hvk_bf16* q, int B, const hvk_bf16* bank, int N, int D, int k,
                uint32_t* pkey, int* pidx, hipStream_t st) {
  const auto kernel = knn_topk_kernel<KC>;
  if (p.lds > 64 * 1024) {  // above the 64 KB a launch may take unasked: ask for it (no stream work)
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds);
    if (e != hipSuccess)
      return hvk_set_error(HVK_EHIP, "hvk_knn_topk: %zu bytes of LDS: %s", p.lds, hipGetErrorString(e));
  }
  hipLaunchKernelGGL(kernel, dim3(p.row_tiles, p.splits), dim3(kThreads), p.lds, st, q, B, bank, N, D, k,
                     p.tiles_per_split, pkey, pidx);
  HVK_CHECK_LAUNCH("knn_topk");
  return HVK_OK;
}

}  // namespace

extern "C" {

int hvk_knn_supported(int D, int k) {
  char buf[96];
  return D >= 8 && k >= 1 && unsupported(D, k, buf, sizeof(buf)) == nullptr;
}

size_t hvk_knn_workspace(int B, int N, int k, int splits) {
  if (B < 1 || N < 1 || N > 0x7fffff00 || k < 1 || k > kMaxK || splits < 0) return 0;
  const TopkPlan p = topk_plan(B, N, k, splits);
  return (size_t)p.splits * B * k * (sizeof(uint32_t) + sizeof(int));
}

int hvk_knn_topk(const void* q, int B, const void* bank, int N, int D, int k, int splits, float* sims, int* idx,
                 void* workspace, size_t workspace_bytes, void* stream) {
  if (B < 0 || N < 1 || N > 0x7fffff00 || D < 1 || k < 1 || splits < 0)
    return hvk_set_error(HVK_EINVAL,
                         "hvk_knn_topk: bad shape (B %d, N %d, D %d, k %d, splits %d: B >= 0, 1 <= N <= 2^31 - 256, "
                         "D >= 1, k >= 1, splits >= 0)",
                         B, N, D, k, splits);
  char buf[96];
  if (const char* why = unsupported(D, k, buf, sizeof(buf)))
    return hvk_set_error(HVK_EUNSUPPORTED, "hvk_knn_topk: unsupported %s", why);
  if (!q || !bank || !sims || !idx) return hvk_set_error(HVK_EINVAL, "hvk_knn_topk: null pointer");
  if (((uintptr_t)q | (uintptr_t)bank) & 15)
    return hvk_set_error(HVK_EINVAL, "hvk_knn_topk: q and bank must be 16-byte aligned");
  if (B == 0) return HVK_OK;
  const size_t need = hvk_knn_workspace(B, N, k, splits);
  if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 3))
    return hvk_set_error(HVK_EINVAL, "hvk_knn_topk: workspace of %zu bytes, %zu needed (null pointer, small or unaligned)",
                         workspace ? workspace_bytes : (size_t)0, need);
  const TopkPlan p = topk_plan(B, N, k, splits);
  if (p.splits > 65535) return hvk_set_error(HVK_EUNSUPPORTED, "hvk_knn_topk: unsupported %d bank splits", p.splits);
  uint32_t* pkey = static_cast<uint32_t*>(workspace);
  int* pidx = reinterpret_cast<int*>(pkey + (size_t)p.splits * B * k);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const hvk_bf16* qb = static_cast<const hvk_bf16*>(q);
  const hvk_bf16* bb = static_cast<const hvk_bf16*>(bank);
  if (int rc = p.KC == 64 ? launch_topk<64>(p, qb, B, bb, N, D, k, pkey, pidx, st)
                          : launch_topk<32>(p, qb, B, bb, N, D, k, pkey, pidx, st))
    return rc;
  hipLaunchKernelGGL(knn_merge_kernel, dim3(B), dim3(64), 0, st, static_cast<const uint32_t*>(pkey),
                     static_cast<const int*>(pidx), B, k, p.splits, sims, idx);
  HVK_CHECK_LAUNCH("knn_merge");
  return HVK_OK;
}

int hvk_knn_vote(const float* sims, const int* idx, int B, int k, const int* labels, int N, int T, const int* ks,
                 int n_k, float temperature, int* leaf, int* path, void* stream) {
  if (B < 0 || N < 1 || k < 1)
    return hvk_set_error(HVK_EINVAL, "hvk_knn_vote: bad shape (B %d, N %d, k %d: B >= 0, N >= 1, k >= 1)", B, N, k);
  if (k > kMaxK) return hvk_set_error(HVK_EUNSUPPORTED, "hvk_knn_vote: unsupported k %d above %d", k, kMaxK);
  if (T != 1 && T != 7) return hvk_set_error(HVK_EINVAL, "hvk_knn_vote: bad shape (T %d: 1 or 7 tiers)", T);
  if (!(temperature > 0.f)) return hvk_set_error(HVK_EINVAL, "hvk_knn_vote: temperature %g must be positive", temperature);
  if (!sims || !idx || !labels || !ks || !leaf || !path) return hvk_set_error(HVK_EINVAL, "hvk_knn_vote: null pointer");
  if (n_k < 1 || n_k > kMaxKs)
    return hvk_set_error(HVK_EINVAL, "hvk_knn_vote: bad shape (n_k %d outside [1, %d])", n_k, kMaxKs);
  VoteArgs a{};
  for (int j = 0; j < n_k; ++j) {
    if (ks[j] < 1 || ks[j] > k)
      return hvk_set_error(HVK_EINVAL, "hvk_knn_vote: bad shape (ks[%d] = %d outside [1, k = %d])", j, ks[j], k);
    a.ks[j] = ks[j];
  }
  if (B == 0) return HVK_OK;
  a.sims = sims, a.idx = idx, a.labels = labels, a.leaf = leaf, a.path = path;
  a.B = B, a.k = k, a.N = N, a.T = T, a.n_k = n_k, a.inv_temp = 1.f / temperature;
  hipLaunchKernelGGL(knn_vote_kernel, dim3(B), dim3(64), 0, static_cast<hipStream_t>(stream), a);
  HVK_CHECK_LAUNCH("knn_vote");
  return HVK_OK;
}

}  // extern "C"
