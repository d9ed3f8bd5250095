// Host-side argument validation of hvk_eval_metrics under AddressSanitizer, beside
// host_checks.cpp and built the same way (`make -C hierarchical-vision_amd/csrc asan`): every
// call below must return before any HIP call, so no GPU is needed.  Exit status 0 and no ASan
// report = pass.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/hvk.h"

static int g_fail = 0;
#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) {                                                     \
      fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_fail;                                                        \
    }                                                                  \
  } while (0)

// non-null addresses that are never dereferenced on these paths
static void* const P = reinterpret_cast<void*>(0x1000);
static int64_t* const T = reinterpret_cast<int64_t*>(0x2000);
static int* const I = reinterpret_cast<int*>(0x3000);
static float* const F = reinterpret_cast<float*>(0x4000);
static unsigned char* const U = reinterpret_cast<unsigned char*>(0x5000);
static double* const S = reinterpret_cast<double*>(0x6000);

// one call with everything valid except what the caller overrides
struct Call {
  const void* logits = P;
  int dtype = 0, B = 4, L = 10, ld = 10;
  const int64_t* targets = T;
  int t_stride = 1, t_off = 0;
  const void* tree_dists = nullptr;
  int dist_dtype = 0;
  const int* leaf_paths = nullptr;
  const int64_t* target_paths = nullptr;
  int topk = 5;
  int* pred = I;
  int* rank = I;
  float* nll = F;
  int* dist = I;
  unsigned char* tier_hit = nullptr;
  double* state = S;
  int run() const {
    return hvk_eval_metrics(logits, dtype, B, L, ld, targets, t_stride, t_off, tree_dists, dist_dtype, leaf_paths,
                            target_paths, topk, pred, rank, nll, dist, tier_hit, state, nullptr);
  }
};

static void refused(const Call& c, const char* word, int line) {
  const int rc = c.run();
  if (rc != HVK_EINVAL || !strstr(hvk_last_error_string(), "hvk_eval_metrics") ||
      !strstr(hvk_last_error_string(), word)) {
    fprintf(stderr, "FAILED %s:%d: status %d, text \"%s\" (expected HVK_EINVAL naming \"%s\")\n", __FILE__, line, rc,
            hvk_last_error_string(), word);
    ++g_fail;
  }
}
#define REFUSED(c, word) refused(c, word, __LINE__)

int main() {
  EXPECT(hvk_abi_version() == HVK_ABI_VERSION && HVK_ABI_VERSION >= 17);
  Call c;
  // shapes
  c = Call(); c.B = -1; REFUSED(c, "shape");
  c = Call(); c.L = 0; REFUSED(c, "shape");
  c = Call(); c.ld = 9; REFUSED(c, "shape");
  c = Call(); c.topk = 0; REFUSED(c, "topk");
  c = Call(); c.t_stride = 0; REFUSED(c, "stride");
  c = Call(); c.t_stride = 7; c.t_off = 7; REFUSED(c, "stride");
  // dtypes
  c = Call(); c.dtype = 2; REFUSED(c, "dtype");
  c = Call(); c.dtype = -1; REFUSED(c, "dtype");
  c = Call(); c.tree_dists = P; c.dist_dtype = 2; REFUSED(c, "dtype");
  // required pointers
  c = Call(); c.logits = nullptr; REFUSED(c, "null");
  c = Call(); c.targets = nullptr; REFUSED(c, "null");
  c = Call(); c.pred = nullptr; REFUSED(c, "null");
  c = Call(); c.rank = nullptr; REFUSED(c, "null");
  c = Call(); c.nll = nullptr; REFUSED(c, "null");
  c = Call(); c.dist = nullptr; REFUSED(c, "null");
  c = Call(); c.state = nullptr; REFUSED(c, "null");
  // distance sources
  c = Call(); c.leaf_paths = I; REFUSED(c, "target_paths");
  c = Call(); c.tree_dists = P; c.leaf_paths = I; c.target_paths = T; REFUSED(c, "both");
  c = Call(); c.tier_hit = U; REFUSED(c, "tier_hit");
  c = Call(); c.tree_dists = P; c.tier_hit = U; REFUSED(c, "tier_hit");
  // an empty batch is fine and launches nothing, in every mode; its arguments are still checked
  c = Call(); c.B = 0; EXPECT(c.run() == HVK_OK);
  c = Call(); c.B = 0; c.dtype = 1; c.ld = 16; c.tree_dists = P; c.dist_dtype = 1; EXPECT(c.run() == HVK_OK);
  c = Call(); c.B = 0; c.leaf_paths = I; c.target_paths = T; c.tier_hit = U; c.t_stride = 7; c.t_off = 6;
  EXPECT(c.run() == HVK_OK);
  c = Call(); c.B = 0; c.topk = 0; REFUSED(c, "topk");
  c = Call(); c.B = 0; c.state = nullptr; REFUSED(c, "null");

  if (g_fail) {
    fprintf(stderr, "%d eval-metrics host check(s) failed\n", g_fail);
    return 1;
  }
  printf("eval metrics host checks ok\n");
  return 0;
}
