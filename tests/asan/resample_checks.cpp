// Host-side argument validation of hvk_resized_crop_u8 under AddressSanitizer, beside
// simpleshot_checks.cpp and built the same way (`make -C hierarchical-vision_amd/csrc asan`):
// every call below must return before any HIP call, so no GPU is needed.  The entry point's
// tables (meta, box) are device memory it never reads on the host: they are passed as addresses
// that fault if touched.  Exit status 0 and no ASan report = pass.
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

static void refused(int rc, const char* who, const char* word, int line) {
  if (rc != HVK_EINVAL || !strstr(hvk_last_error_string(), who) || !strstr(hvk_last_error_string(), word)) {
    fprintf(stderr, "FAILED %s:%d: status %d, text \"%s\" (expected HVK_EINVAL from %s naming \"%s\")\n", __FILE__,
            line, rc, hvk_last_error_string(), who, word);
    ++g_fail;
  }
}
#define REFUSED(call, who, word) refused(call, who, word, __LINE__)

// non-null device addresses that are never dereferenced on these paths
static uint8_t* const SRC = reinterpret_cast<uint8_t*>(0x1000);
static int64_t* const META = reinterpret_cast<int64_t*>(0x2000);
static int32_t* const BOX = reinterpret_cast<int32_t*>(0x3000);
static uint8_t* const OUT = reinterpret_cast<uint8_t*>(0x4000);

int main() {
  EXPECT(hvk_abi_version() == HVK_ABI_VERSION && HVK_ABI_VERSION >= 20);

  const char* who = "hvk_resized_crop_u8";
  // the batch and the output side (1 .. 1024)
  REFUSED(hvk_resized_crop_u8(SRC, META, BOX, -1, 224, 224, OUT, nullptr), who, "shape");
  REFUSED(hvk_resized_crop_u8(SRC, META, BOX, 4, 0, 224, OUT, nullptr), who, "shape");
  REFUSED(hvk_resized_crop_u8(SRC, META, BOX, 4, 224, 0, OUT, nullptr), who, "shape");
  REFUSED(hvk_resized_crop_u8(SRC, META, BOX, 4, -224, 224, OUT, nullptr), who, "shape");
  REFUSED(hvk_resized_crop_u8(SRC, META, BOX, 4, 1025, 224, OUT, nullptr), who, "shape");
  REFUSED(hvk_resized_crop_u8(SRC, META, BOX, 4, 224, 1025, OUT, nullptr), who, "shape");
  REFUSED(hvk_resized_crop_u8(SRC, META, BOX, 4, 0x7fffffff, 0x7fffffff, OUT, nullptr), who, "shape");
  // more tiles than one launch's grid: 2^21 images x 32 x 64 tiles of 1024 x 1024
  REFUSED(hvk_resized_crop_u8(SRC, META, BOX, 1 << 21, 1024, 1024, OUT, nullptr), who, "tiles");
  REFUSED(hvk_resized_crop_u8(SRC, META, BOX, 0x7fffffff, 1024, 1024, OUT, nullptr), who, "tiles");
  // pointers
  REFUSED(hvk_resized_crop_u8(nullptr, META, BOX, 4, 224, 224, OUT, nullptr), who, "null");
  REFUSED(hvk_resized_crop_u8(SRC, nullptr, BOX, 4, 224, 224, OUT, nullptr), who, "null");
  REFUSED(hvk_resized_crop_u8(SRC, META, nullptr, 4, 224, 224, OUT, nullptr), who, "null");
  REFUSED(hvk_resized_crop_u8(SRC, META, BOX, 4, 224, 224, nullptr, nullptr), who, "null");
  // an empty batch: nothing to launch, but its shape is still checked
  EXPECT(hvk_resized_crop_u8(SRC, META, BOX, 0, 224, 224, OUT, nullptr) == HVK_OK);
  EXPECT(hvk_resized_crop_u8(nullptr, nullptr, nullptr, 0, 1, 1024, nullptr, nullptr) == HVK_OK);
  REFUSED(hvk_resized_crop_u8(SRC, META, BOX, 0, 224, 1025, OUT, nullptr), who, "shape");

  if (g_fail) {
    fprintf(stderr, "%d resample host check(s) failed\n", g_fail);
    return 1;
  }
  printf("resample host checks ok\n");
  return 0;
}
