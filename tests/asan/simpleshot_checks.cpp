// Host-side argument validation and workspace arithmetic of the SimpleShot entry points
// (hvk_ss_prepare / accumulate / finalize / predict_flat / predict_tree) under AddressSanitizer,
// beside eval_metrics_checks.cpp and built the same way (`make -C hierarchical-vision_amd/csrc
// asan`): every call below must return before any HIP call, so no GPU is needed.  tier_base is the
// one array these entry points read on the host: it is passed at its exact length, so a read past
// n_tiers + 1 entries is an ASan report.  Exit status 0 and no ASan report = pass.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/hvk.h"

static int g_fail = 0;
#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) {                                                     \
      fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_fail;                                                        \
    }                                                                  \
  } while (0)

static void refused(int rc, const char* who, const char* word, int line) {
  if (rc != HVK_EINVAL || !strstr(hvk_last_error_string(), who) || !strstr(hvk_last_error_string(), word)) {
    fprintf(stderr, "FAILED %s:%d: status %d, text \"%s\" (expected HVK_EINVAL from %s naming \"%s\")\n", __FILE__,
            line, rc, hvk_last_error_string(), who, word);
    ++g_fail;
  }
}
#define REFUSED(call, who, word) refused(call, who, word, __LINE__)

// non-null device addresses that are never dereferenced on these paths
static float* const X = reinterpret_cast<float*>(0x1000);
static int64_t* const T = reinterpret_cast<int64_t*>(0x2000);
static int* const I = reinterpret_cast<int*>(0x3000);
static float* const F = reinterpret_cast<float*>(0x4000);
static double* const S = reinterpret_cast<double*>(0x6000);
static long long* const N = reinterpret_cast<long long*>(0x7000);
static void* const W = reinterpret_cast<void*>(0x8000);

// tier_base on the heap at its exact length
static std::vector<int> tiers(std::initializer_list<int> v) { return std::vector<int>(v); }

int main() {
  EXPECT(hvk_abi_version() == HVK_ABI_VERSION && HVK_ABI_VERSION >= 18);

  // ---- prepare
  const char* who = "hvk_ss_prepare";
  REFUSED(hvk_ss_prepare(X, 0, -1, 8, 8, 1, 1, F, nullptr), who, "shape");
  REFUSED(hvk_ss_prepare(X, 0, 4, 0, 8, 1, 1, F, nullptr), who, "shape");
  REFUSED(hvk_ss_prepare(X, 0, 4, 8, 7, 1, 1, F, nullptr), who, "shape");
  REFUSED(hvk_ss_prepare(X, 2, 4, 8, 8, 1, 1, F, nullptr), who, "dtype");
  REFUSED(hvk_ss_prepare(X, -1, 4, 8, 8, 1, 1, F, nullptr), who, "dtype");
  REFUSED(hvk_ss_prepare(nullptr, 0, 4, 8, 8, 1, 1, F, nullptr), who, "null");
  REFUSED(hvk_ss_prepare(X, 1, 4, 8, 8, 1, 1, nullptr, nullptr), who, "null");
  EXPECT(hvk_ss_prepare(X, 1, 0, 8, 16, 0, 0, F, nullptr) == HVK_OK);
  REFUSED(hvk_ss_prepare(X, 1, 0, 8, 4, 0, 0, F, nullptr), who, "shape");  // an empty batch is still checked

  // ---- accumulate
  who = "hvk_ss_accumulate";
  REFUSED(hvk_ss_accumulate(X, -1, 8, T, 7, 6, T, 10, S, N, S, nullptr), who, "shape");
  REFUSED(hvk_ss_accumulate(X, 4, 0, T, 7, 6, T, 10, S, N, S, nullptr), who, "shape");
  REFUSED(hvk_ss_accumulate(X, 4, 8, T, 7, 6, T, 0, S, N, S, nullptr), who, "shape");
  REFUSED(hvk_ss_accumulate(X, 0x7fffffff, 8, T, 7, 6, T, 10, S, N, S, nullptr), who, "shape");
  REFUSED(hvk_ss_accumulate(X, 4, 8, T, 7, 7, T, 10, S, N, S, nullptr), who, "stride");
  REFUSED(hvk_ss_accumulate(X, 4, 8, T, 0, 0, T, 10, S, N, S, nullptr), who, "stride");
  REFUSED(hvk_ss_accumulate(X, 4, 8, T, 1, -1, T, 10, S, N, S, nullptr), who, "stride");
  REFUSED(hvk_ss_accumulate(nullptr, 4, 8, T, 7, 6, T, 10, S, N, S, nullptr), who, "null");
  REFUSED(hvk_ss_accumulate(X, 4, 8, nullptr, 7, 6, T, 10, S, N, S, nullptr), who, "null");
  REFUSED(hvk_ss_accumulate(X, 4, 8, T, 7, 6, nullptr, 10, S, N, S, nullptr), who, "null");
  REFUSED(hvk_ss_accumulate(X, 4, 8, T, 7, 6, T, 10, nullptr, N, S, nullptr), who, "null");
  REFUSED(hvk_ss_accumulate(X, 4, 8, T, 7, 6, T, 10, S, nullptr, S, nullptr), who, "null");
  REFUSED(hvk_ss_accumulate(X, 4, 8, T, 7, 6, T, 10, S, N, nullptr, nullptr), who, "null");
  EXPECT(hvk_ss_accumulate(X, 0, 8, T, 1, 0, T, 10, S, N, S, nullptr) == HVK_OK);

  // ---- finalize (its tier_base is read on the host)
  who = "hvk_ss_finalize";
  const std::vector<int> t3 = tiers({0, 2, 5, 15}), t1 = tiers({0, 10}), t8 = tiers({0, 1, 2, 3, 4, 5, 6, 7, 8});
  const std::vector<int> flat_tb = tiers({0, 2, 2, 15}), late = tiers({1, 2, 5, 15}), back = tiers({0, 5, 3});
  REFUSED(hvk_ss_finalize(S, N, 0, 3, t3.data(), I, I, F, F, nullptr), who, "shape");
  REFUSED(hvk_ss_finalize(S, N, 8, 0, t3.data(), I, I, F, F, nullptr), who, "n_tiers");
  REFUSED(hvk_ss_finalize(S, N, 8, 9, t8.data(), I, I, F, F, nullptr), who, "n_tiers");
  REFUSED(hvk_ss_finalize(S, N, 8, -1, t3.data(), I, I, F, F, nullptr), who, "n_tiers");
  REFUSED(hvk_ss_finalize(S, N, 8, 3, nullptr, I, I, F, F, nullptr), who, "null");
  REFUSED(hvk_ss_finalize(S, N, 8, 3, t3.data(), nullptr, I, F, F, nullptr), who, "null");
  REFUSED(hvk_ss_finalize(S, N, 8, 3, t3.data(), I, nullptr, F, F, nullptr), who, "null");
  REFUSED(hvk_ss_finalize(S, N, 8, 3, flat_tb.data(), I, I, F, F, nullptr), who, "tier_base");
  REFUSED(hvk_ss_finalize(S, N, 8, 3, late.data(), I, I, F, F, nullptr), who, "tier_base");
  REFUSED(hvk_ss_finalize(S, N, 8, 2, back.data(), I, I, F, F, nullptr), who, "tier_base");
  REFUSED(hvk_ss_finalize(nullptr, N, 8, 3, t3.data(), I, I, F, F, nullptr), who, "null");
  REFUSED(hvk_ss_finalize(S, nullptr, 8, 3, t3.data(), I, I, F, F, nullptr), who, "null");
  REFUSED(hvk_ss_finalize(S, N, 8, 3, t3.data(), I, I, nullptr, F, nullptr), who, "null");
  REFUSED(hvk_ss_finalize(S, N, 8, 3, t3.data(), I, I, F, nullptr, nullptr), who, "null");
  REFUSED(hvk_ss_finalize(nullptr, N, 8, 1, t1.data(), nullptr, nullptr, F, F, nullptr), who, "null");
  REFUSED(hvk_ss_finalize(nullptr, N, 8, 8, t8.data(), I, I, F, F, nullptr), who, "null");  // 8 tiers: 9 entries read

  // ---- flat predict and its workspace
  who = "hvk_ss_predict_flat";
  EXPECT(hvk_ss_predict_flat_workspace(0, 10) == 0 && hvk_ss_predict_flat_workspace(4, 0) == 0);
  EXPECT(hvk_ss_predict_flat_workspace(-3, 10) == 0 && hvk_ss_predict_flat_workspace(4, -1) == 0);
  EXPECT(hvk_ss_predict_flat_workspace(1, 1) == 8);
  EXPECT(hvk_ss_predict_flat_workspace(67, 37) == 67 * 8);
  EXPECT(hvk_ss_predict_flat_workspace(300, 400) == 300 * 8 * 7);
  EXPECT(hvk_ss_predict_flat_workspace(256, 10000) == 256 * 8 * 79);
  // the largest shapes: the byte count stays a multiple of one (min, index) pair per row and fits
  const size_t big = hvk_ss_predict_flat_workspace(0x7fffffff, 0x7fffff00);
  EXPECT(big % (8ull * 0x7fffffff) == 0 && big / (8ull * 0x7fffffff) >= 1);
  for (int B : {1, 63, 64, 65, 4096, 1 << 20})
    for (int L : {1, 64, 65, 10000, 1 << 24}) {
      const size_t n = hvk_ss_predict_flat_workspace(B, L);
      EXPECT(n % (8ull * B) == 0 && n / (8ull * B) >= 1 && n / (8ull * B) <= (size_t)(L + 63) / 64);
    }
  REFUSED(hvk_ss_predict_flat(X, -1, 8, F, F, 10, I, W, 1 << 20, nullptr), who, "shape");
  REFUSED(hvk_ss_predict_flat(X, 4, 8, F, F, 0, I, W, 1 << 20, nullptr), who, "shape");
  REFUSED(hvk_ss_predict_flat(X, 4, 0, F, F, 10, I, W, 1 << 20, nullptr), who, "shape");
  REFUSED(hvk_ss_predict_flat(X, 4, 8, F, F, 0x7fffff01, I, W, 1 << 20, nullptr), who, "shape");
  REFUSED(hvk_ss_predict_flat(X, 4, 6, F, F, 10, I, W, 1 << 20, nullptr), who, "multiple of 4");
  REFUSED(hvk_ss_predict_flat(X, 4, 1, F, F, 10, I, W, 1 << 20, nullptr), who, "multiple of 4");
  REFUSED(hvk_ss_predict_flat(nullptr, 4, 8, F, F, 10, I, W, 1 << 20, nullptr), who, "null");
  REFUSED(hvk_ss_predict_flat(X, 4, 8, nullptr, F, 10, I, W, 1 << 20, nullptr), who, "null");
  REFUSED(hvk_ss_predict_flat(X, 4, 8, F, nullptr, 10, I, W, 1 << 20, nullptr), who, "null");
  REFUSED(hvk_ss_predict_flat(X, 4, 8, F, F, 10, nullptr, W, 1 << 20, nullptr), who, "null");
  REFUSED(hvk_ss_predict_flat(X + 1, 4, 8, F, F, 10, I, W, 1 << 20, nullptr), who, "aligned");
  REFUSED(hvk_ss_predict_flat(X, 4, 8, F + 2, F, 10, I, W, 1 << 20, nullptr), who, "aligned");
  REFUSED(hvk_ss_predict_flat(X, 4, 8, F, F, 10, I, nullptr, 1 << 20, nullptr), who, "workspace");
  REFUSED(hvk_ss_predict_flat(X, 4, 8, F, F, 10, I, W, 31, nullptr), who, "workspace");  // 32 needed
  EXPECT(hvk_ss_predict_flat(X, 0, 8, F, F, 10, I, nullptr, 0, nullptr) == HVK_OK);
  REFUSED(hvk_ss_predict_flat(X, 0, 6, F, F, 10, I, nullptr, 0, nullptr), who, "multiple of 4");

  // ---- tree predict
  who = "hvk_ss_predict_tree";
  REFUSED(hvk_ss_predict_tree(X, -1, 8, F, N, 3, t3.data(), I, I, I, nullptr), who, "shape");
  REFUSED(hvk_ss_predict_tree(X, 4, 0, F, N, 3, t3.data(), I, I, I, nullptr), who, "shape");
  EXPECT(hvk_ss_predict_tree(X, 4, 4100, F, N, 3, t3.data(), I, I, I, nullptr) == HVK_EUNSUPPORTED);
  REFUSED(hvk_ss_predict_tree(X, 4, 8, F, N, 0, t3.data(), I, I, I, nullptr), who, "n_tiers");
  REFUSED(hvk_ss_predict_tree(X, 4, 8, F, N, 9, t8.data(), I, I, I, nullptr), who, "n_tiers");
  REFUSED(hvk_ss_predict_tree(X, 4, 8, F, N, 3, nullptr, I, I, I, nullptr), who, "null");
  REFUSED(hvk_ss_predict_tree(X, 4, 8, F, N, 3, t3.data(), nullptr, I, I, nullptr), who, "null");
  REFUSED(hvk_ss_predict_tree(X, 4, 8, F, N, 3, t3.data(), I, nullptr, I, nullptr), who, "null");
  REFUSED(hvk_ss_predict_tree(X, 4, 8, F, N, 3, late.data(), I, I, I, nullptr), who, "tier_base");
  REFUSED(hvk_ss_predict_tree(X, 4, 8, F, N, 3, flat_tb.data(), I, I, I, nullptr), who, "tier_base");
  REFUSED(hvk_ss_predict_tree(nullptr, 4, 8, F, N, 3, t3.data(), I, I, I, nullptr), who, "null");
  REFUSED(hvk_ss_predict_tree(X, 4, 8, nullptr, N, 3, t3.data(), I, I, I, nullptr), who, "null");
  REFUSED(hvk_ss_predict_tree(X, 4, 8, F, nullptr, 3, t3.data(), I, I, I, nullptr), who, "null");
  REFUSED(hvk_ss_predict_tree(X, 4, 8, F, N, 3, t3.data(), I, I, nullptr, nullptr), who, "null");
  EXPECT(hvk_ss_predict_tree(X, 0, 8, F, N, 3, t3.data(), I, I, I, nullptr) == HVK_OK);
  EXPECT(hvk_ss_predict_tree(X, 0, 8, F, N, 1, t1.data(), nullptr, nullptr, I, nullptr) == HVK_OK);
  EXPECT(hvk_ss_predict_tree(X, 0, 8, F, N, 8, t8.data(), I, I, I, nullptr) == HVK_OK);

  if (g_fail) {
    fprintf(stderr, "%d simpleshot host check(s) failed\n", g_fail);
    return 1;
  }
  printf("simpleshot host checks ok\n");
  return 0;
}
