// What the evaluation kernels share (metrics.hip, joint.hip, simpleshot.hip, linear_probe.hip,
// crm.hip): the 256-thread workgroup, the element load, the (min, lowest index) rule and the
// reductions whose operand order is fixed, so that equal inputs give bit-identical outputs.
#pragma once
#include "hvk_common.h"

namespace hvk_eval {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kNoIdx = 0x7fffffff;  // the index while nothing has compared

// ceil(a / b) for a >= 0 without the a + b - 1 that overflows next to 2^31
constexpr int ceil_div(int a, int b) { return a / b + (a % b != 0 ? 1 : 0); }

// element j of an f32 or bf16 row, as f32
__device__ __forceinline__ float load1(const void* row, int bf16, int j) {
  if (bf16) return __uint_as_float((uint32_t) static_cast<const hvk_bf16*>(row)[j] << 16);
  return static_cast<const float*>(row)[j];
}

// a lower value wins; among equal values the lower index (a NaN never compares below)
__device__ __forceinline__ void take_min(float& m, int& mi, float v, int vi) {
  const bool t = v < m || (v == m && vi < mi);
  m = t ? v : m;
  mi = t ? vi : mi;
}

// take_min across the 16 lanes that share a row of an MFMA result (lanes l, l ^ 8, ..., l ^ 1)
__device__ __forceinline__ void take_min16(float& m, int& mi) {
#pragma unroll
  for (int o = 8; o >= 1; o >>= 1) {
    const float v = __shfl_xor(m, o);
    const int vi = __shfl_xor(mi, o);
    take_min(m, mi, v, vi);
  }
}

// wave butterfly with the same operand order in both lanes of a pair (the lower lane's value on
// the left): every lane ends with the same bits.  `lane`: the lane or the thread index.
template <typename T, typename Op>
__device__ __forceinline__ T wave_reduce_ordered(T v, int lane, Op op) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const T w = __shfl_xor(v, o);
    v = (lane & o) ? op(w, v) : op(v, w);
  }
  return v;
}
template <typename T>
__device__ __forceinline__ T wave_sum_ordered(T v, int lane) {
  return wave_reduce_ordered(v, lane, [](T a, T c) { return a + c; });
}

// the four waves' values combined as op(op(w0, w1), op(w2, w3)); every thread returns the same bits
template <typename T, typename Op>
__device__ __forceinline__ T block_reduce_ordered(T v, T* part, int tid, Op op) {
  v = wave_reduce_ordered(v, tid, op);
  __syncthreads();  // part's readers of the previous reduction are done
  if ((tid & 63) == 0) part[tid >> 6] = v;
  __syncthreads();
  return op(op(part[0], part[1]), op(part[2], part[3]));
}

}  // namespace hvk_eval
