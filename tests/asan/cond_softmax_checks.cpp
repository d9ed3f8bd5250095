// Host-side argument validation and the LDS limit of the conditional-softmax entry points
// (hvk_cond_softmax_supported / fwd / bwd / decode) under AddressSanitizer, beside
// simpleshot_checks.cpp and built the same way (`make -C hierarchical-vision_amd/csrc asan`): every
// call below must return before any HIP call, so no GPU is needed.  tier_off and coeffs are the
// arrays these entry points read on the host: they are passed at their exact length, so a read past
// 8 / 7 entries is an ASan report.  Exit status 0 and no ASan report = pass.
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

static void refused(int rc, int want, const char* who, const char* word, int line) {
  if (rc != want || !strstr(hvk_last_error_string(), who) || !strstr(hvk_last_error_string(), word)) {
    fprintf(stderr, "FAILED %s:%d: status %d, text \"%s\" (expected %d from %s naming \"%s\")\n", __FILE__, line, rc,
            hvk_last_error_string(), want, who, word);
    ++g_fail;
  }
}
#define REFUSED(call, who, word) refused(call, HVK_EINVAL, who, word, __LINE__)

// non-null device addresses that are never dereferenced on these paths
static float* const X = reinterpret_cast<float*>(0x1000);
static int64_t* const T = reinterpret_cast<int64_t*>(0x2000);
static int* const I = reinterpret_cast<int*>(0x3000);
static float* const F = reinterpret_cast<float*>(0x4000);
static unsigned char* const H = reinterpret_cast<unsigned char*>(0x5000);
static double* const S = reinterpret_cast<double*>(0x6000);

int main() {
  EXPECT(hvk_abi_version() == HVK_ABI_VERSION && HVK_ABI_VERSION >= 25);
  typedef std::vector<int> V;
  const V ok{0, 1, 3, 6, 11, 20, 37, 168}, inat{0, 3, 16, 67, 340, 1443, 6327, 16327};
  const V edge{0, 1, 2, 3, 4, 5, 15360, 15367}, over{0, 1, 2, 3, 4, 5, 15361, 15368};
  const V late{1, 2, 3, 4, 5, 6, 7, 8}, flat{0, 1, 3, 3, 11, 20, 37, 168}, leaves{0, 1, 2, 3, 4, 5, 6, 7 + (1 << 24)};
  const std::vector<float> one(7, 1.f), neg{1, 1, 1, -1, 1, 1, 1}, inf{1, 1, 1, 1, 1, 1, 1.f / 0.f};

  // ---- the decoder's limit: tiers 0-5 in 60 KB of LDS
  EXPECT(hvk_cond_softmax_supported(ok.data()) == 1 && hvk_cond_softmax_supported(inat.data()) == 1);
  EXPECT(hvk_cond_softmax_supported(edge.data()) == 1 && hvk_cond_softmax_supported(over.data()) == 0);
  EXPECT(hvk_cond_softmax_supported(nullptr) == 0 && hvk_cond_softmax_supported(late.data()) == 0);
  EXPECT(hvk_cond_softmax_supported(flat.data()) == 0 && hvk_cond_softmax_supported(leaves.data()) == 0);

  // ---- forward
  const char* who = "hvk_cond_softmax_fwd";
  REFUSED(hvk_cond_softmax_fwd(X, 0, 4, 168, nullptr, T, I, I, I, one.data(), 0.f, F, F, F, nullptr), who, "tier_off");
  REFUSED(hvk_cond_softmax_fwd(X, 0, 4, 168, flat.data(), T, I, I, I, one.data(), 0.f, F, F, F, nullptr), who, "tier_off");
  REFUSED(hvk_cond_softmax_fwd(X, 0, -1, 168, ok.data(), T, I, I, I, one.data(), 0.f, F, F, F, nullptr), who, "shape");
  REFUSED(hvk_cond_softmax_fwd(X, 0, 4, 167, ok.data(), T, I, I, I, one.data(), 0.f, F, F, F, nullptr), who, "shape");
  REFUSED(hvk_cond_softmax_fwd(X, 2, 4, 168, ok.data(), T, I, I, I, one.data(), 0.f, F, F, F, nullptr), who, "dtype");
  REFUSED(hvk_cond_softmax_fwd(nullptr, 0, 4, 168, ok.data(), T, I, I, I, one.data(), 0.f, F, F, F, nullptr), who, "null");
  REFUSED(hvk_cond_softmax_fwd(X, 0, 4, 168, ok.data(), T, I, nullptr, I, one.data(), 0.f, F, F, F, nullptr), who, "null");
  REFUSED(hvk_cond_softmax_fwd(X, 0, 4, 168, ok.data(), T, I, I, I, nullptr, 0.f, F, F, F, nullptr), who, "null");
  REFUSED(hvk_cond_softmax_fwd(X, 0, 4, 168, ok.data(), T, I, I, I, one.data(), 0.f, F, F, nullptr, nullptr), who, "null");
  REFUSED(hvk_cond_softmax_fwd(X, 0, 4, 168, ok.data(), T, I, I, I, neg.data(), 0.f, F, F, F, nullptr), who, "coefficient 3");
  REFUSED(hvk_cond_softmax_fwd(X, 0, 4, 168, ok.data(), T, I, I, I, inf.data(), 0.f, F, F, F, nullptr), who, "coefficient 6");
  REFUSED(hvk_cond_softmax_fwd(X, 0, 4, 168, ok.data(), T, I, I, I, one.data(), 1.f, F, F, F, nullptr), who, "smoothing");
  REFUSED(hvk_cond_softmax_fwd(X, 0, 4, 168, ok.data(), T, I, I, I, one.data(), 0.f / 0.f, F, F, F, nullptr), who, "smoothing");
  // an empty batch, the identity (no sib_col), and no LDS limit on the loss
  EXPECT(hvk_cond_softmax_fwd(X, 1, 0, 168, ok.data(), T, I, I, nullptr, one.data(), 0.1f, F, F, F, nullptr) == HVK_OK);
  EXPECT(hvk_cond_softmax_fwd(X, 1, 0, 15368, over.data(), T, I, I, nullptr, one.data(), 0.f, F, F, F, nullptr) == HVK_OK);

  // ---- backward: the gradient buffer is whole, aligned 16-B vectors
  who = "hvk_cond_softmax_bwd";
  REFUSED(hvk_cond_softmax_bwd(X, 0, 4, 160, ok.data(), T, I, I, I, one.data(), 0.f, F, F, X, 168, nullptr), who, "shape");
  REFUSED(hvk_cond_softmax_bwd(X, 0, 4, 168, ok.data(), T, I, I, I, one.data(), 0.f, nullptr, F, X, 168, nullptr), who, "null");
  REFUSED(hvk_cond_softmax_bwd(X, 0, 4, 168, ok.data(), T, I, I, I, one.data(), 0.f, F, F, nullptr, 168, nullptr), who, "null");
  REFUSED(hvk_cond_softmax_bwd(X, 0, 4, 168, ok.data(), T, I, I, I, one.data(), 0.f, F, F, X, 164, nullptr), who, "gradient rows");
  REFUSED(hvk_cond_softmax_bwd(X, 0, 4, 168, ok.data(), T, I, I, I, one.data(), 0.f, F, F, X, 170, nullptr), who, "gradient rows");
  REFUSED(hvk_cond_softmax_bwd(X, 1, 4, 168, ok.data(), T, I, I, I, one.data(), 0.f, F, F, X, 172, nullptr), who, "gradient rows");
  REFUSED(hvk_cond_softmax_bwd(X, 0, 4, 168, ok.data(), T, I, I, I, one.data(), 0.f, F, F, X + 1, 168, nullptr), who, "gradient rows");
  EXPECT(hvk_cond_softmax_bwd(X, 0, 0, 168, ok.data(), T, I, I, nullptr, one.data(), 0.f, F, F, X, 172, nullptr) == HVK_OK);
  EXPECT(hvk_cond_softmax_bwd(X, 1, 0, 168, ok.data(), T, I, I, I, one.data(), 0.f, F, F, X, 176, nullptr) == HVK_OK);
  refused(hvk_cond_softmax_bwd(X, 0, 65536, 168, ok.data(), T, I, I, I, one.data(), 0.f, F, F, X, 168, nullptr),
          HVK_EUNSUPPORTED, who, "65535", __LINE__);

  // ---- decode
  who = "hvk_cond_softmax_decode";
  REFUSED(hvk_cond_softmax_decode(X, 0, 4, 168, nullptr, T, 1, 0, I, I, I, I, 5, I, I, F, F, I, H, F, S, nullptr), who, "tier_off");
  REFUSED(hvk_cond_softmax_decode(X, 0, 4, 8, leaves.data(), T, 1, 0, I, I, I, I, 5, I, I, F, F, I, H, F, S, nullptr), who, "2^24");
  refused(hvk_cond_softmax_decode(X, 0, 4, 15368, over.data(), T, 1, 0, I, I, I, I, 5, I, I, F, F, I, H, F, S, nullptr),
          HVK_EUNSUPPORTED, who, "15360", __LINE__);
  REFUSED(hvk_cond_softmax_decode(X, 0, 4, 100, ok.data(), T, 1, 0, I, I, I, I, 5, I, I, F, F, I, H, F, S, nullptr), who, "shape");
  REFUSED(hvk_cond_softmax_decode(X, 0, 4, 168, ok.data(), T, 1, 0, I, I, I, I, 0, I, I, F, F, I, H, F, S, nullptr), who, "topk");
  REFUSED(hvk_cond_softmax_decode(X, 0, 4, 168, ok.data(), T, 7, 7, I, I, I, I, 5, I, I, F, F, I, H, F, S, nullptr), who, "stride");
  REFUSED(hvk_cond_softmax_decode(X, 3, 4, 168, ok.data(), T, 7, 6, I, I, I, I, 5, I, I, F, F, I, H, F, S, nullptr), who, "dtype");
  REFUSED(hvk_cond_softmax_decode(nullptr, 0, 4, 168, ok.data(), T, 7, 6, I, I, I, I, 5, I, I, F, F, I, H, F, S, nullptr), who, "null");
  REFUSED(hvk_cond_softmax_decode(X, 0, 4, 168, ok.data(), T, 7, 6, I, nullptr, I, I, 5, I, I, F, F, I, H, F, S, nullptr), who, "null");
  REFUSED(hvk_cond_softmax_decode(X, 0, 4, 168, ok.data(), T, 7, 6, I, I, I, I, 5, I, I, F, F, I, nullptr, F, S, nullptr), who, "null");
  REFUSED(hvk_cond_softmax_decode(X, 0, 4, 168, ok.data(), T, 7, 6, I, I, I, I, 5, I, I, F, F, I, H, F, nullptr, nullptr), who, "null");
  // an empty batch; neither sib_col nor the scores are required
  EXPECT(hvk_cond_softmax_decode(X, 1, 0, 168, ok.data(), T, 7, 6, I, I, nullptr, I, 5, I, I, F, F, I, H, nullptr, S, nullptr) == HVK_OK);
  EXPECT(hvk_cond_softmax_decode(X, 0, 0, 15367, edge.data(), T, 1, 0, I, I, I, I, 1, I, I, F, F, I, H, F, S, nullptr) == HVK_OK);

  if (g_fail) {
    fprintf(stderr, "%d conditional-softmax host check(s) failed\n", g_fail);
    return 1;
  }
  printf("conditional-softmax host checks ok\n");
  return 0;
}
