// Device-side RandomResizedCrop + flip and Resize + CenterCrop (the reference's CPU input
// pipeline, data.py:114-126, torchvision on PIL): crop a box out of a decoded uint8 HWC image,
// resample the crop bilinearly to a virtual vh x vw image, emit a window of it as uint8 CHW,
// optionally mirrored.  The resampling is PIL's 8-bit path restated (Resample.c: precompute_coeffs,
// normalize_coeffs_8bpc, ImagingResampleHorizontal_8bpc / Vertical_8bpc, PRECISION_BITS = 22):
// horizontal pass, rounded to uint8, then vertical pass, both in 32-bit integers with coefficients
// (int)(0.5 + w / ww * 2^22).  The coefficients are the only floating-point values; they are
// computed in IEEE double with contraction OFF (one fma in `center - support` moves a tap), so the
// output equals Image.crop(...).resize(..., BILINEAR) byte for byte.
//
// One workgroup per (image, RS_TH output rows, RS_TW output columns), 3 waves:
//  1. the tile's two coefficient tables into LDS (one thread per output index, ww summed serially
//     in tap order);
//  2. the source rows the tile's vertical taps need, resampled horizontally into an LDS uint8 tile
//     in output-column order (the flip is folded into the horizontal table);
//  3. the vertical pass from LDS, written as runs of RS_TW consecutive bytes per channel plane.
// A scale of 64 needs 129 source rows for ONE output row, so steps 2-3 loop over sub-bands of output
// rows whose source rows fit the tile (RS_CAP): any scale in the supported range runs, larger ones with fewer
// output rows per pass.
#include "hvk_common.h"
#include "../../include/hvk.h"

namespace {

constexpr int RS_TW = 32;          // output columns per workgroup
constexpr int RS_TH = 16;          // output rows per workgroup
constexpr int RS_L = 3 * RS_TW;    // bytes per tile row (column-major pixels, channel fastest)
constexpr int RS_THREADS = 2 * RS_L;
constexpr int RS_KMAX = 129;       // taps at scale 64: 2 * 64 + 1 (odd: conflict-free table rows)
constexpr int RS_CAP = 192;        // source rows held per sub-band (>= RS_KMAX)
constexpr int RS_MAX_SRC = 8192;
constexpr int RS_MAX_OUT = 1024;
constexpr int RS_MAX_SCALE = 64;
constexpr int RS_PREC = 22;

// bilinear_filter((x - center + 0.5) * ss) of tap position x
__device__ __forceinline__ double rs_weight(int x, double center, double ss) {
#pragma clang fp contract(off)
  double d = ((double)x - center + 0.5) * ss;
  if (d < 0.0) d = -d;
  return d < 1.0 ? 1.0 - d : 0.0;
}

// Coefficients of output index v of an axis resampled n_in -> n_out (PIL precompute_coeffs +
// normalize_coeffs_8bpc, bilinear): first tap and tap count returned, k[0 .. count) written.
// Equal sizes skip the pass (Resample.c need_horizontal / need_vertical): one unit tap.
__device__ void rs_axis_coefs(int n_in, int n_out, int v, int kmax, int* __restrict__ k, int& first, int& count) {
#pragma clang fp contract(off)
  if (n_in == n_out) {
    k[0] = 1 << RS_PREC;
    first = v;
    count = 1;
    return;
  }
  const double scale = (double)n_in / (double)n_out;
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = fs;  // bilinear support 1.0 * filterscale
  const double ss = 1.0 / fs;
  const double center = ((double)v + 0.5) * scale;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + support + 0.5);
  if (xmax > n_in) xmax = n_in;
  int n = xmax - xmin;
  n = n < 0 ? 0 : (n > kmax ? kmax : n);  // <= 2 support + 1 <= kmax in the supported range
  double ww = 0.0;
  for (int t = 0; t < n; ++t) ww += rs_weight(t + xmin, center, ss);
  for (int t = 0; t < n; ++t) {
    double w = rs_weight(t + xmin, center, ss);
    if (ww != 0.0) w = w / ww;
    k[t] = (int)(0.5 + w * (double)(1 << RS_PREC));
  }
  first = xmin;
  count = n;
}

__device__ __forceinline__ uint8_t rs_clip8(int acc) {
  acc >>= RS_PREC;
  return (uint8_t)(acc < 0 ? 0 : (acc > 255 ? 255 : acc));
}

// the supported range of one image's table rows (include/hvk.h); a row outside it is never
// dereferenced: its output is zero-filled
__device__ __forceinline__ bool rs_box_ok(long long off, int H, int W, const int* bx, int out_h, int out_w) {
  const int i = bx[0], j = bx[1], h = bx[2], w = bx[3], vh = bx[4], vw = bx[5], oy = bx[6], ox = bx[7];
  if (off < 0 || H < 1 || W < 1 || H > RS_MAX_SRC || W > RS_MAX_SRC) return false;
  if (i < 0 || j < 0 || h < 1 || w < 1 || h > H - i || w > W - j) return false;
  if (vh < 1 || vw < 1 || oy < 0 || ox < 0 || out_h > vh - oy || out_w > vw - ox) return false;
  if ((long long)h > (long long)RS_MAX_SCALE * vh || (long long)w > (long long)RS_MAX_SCALE * vw) return false;
  return true;
}

__global__ __launch_bounds__(RS_THREADS) void resized_crop_u8_kernel(const uint8_t* __restrict__ src,
                                                                     const long long* __restrict__ meta,
                                                                     const int* __restrict__ box, int B,
                                                                     int out_h, int out_w, int xtiles,
                                                                     int ytiles, uint8_t* __restrict__ out) {
  __shared__ int hk[RS_TW * RS_KMAX];
  __shared__ int vk[RS_TH * RS_KMAX];
  __shared__ int hfirst[RS_TW], hcount[RS_TW], vfirst[RS_TH], vcount[RS_TH];
  __shared__ uint8_t tile[RS_CAP * RS_L];

  const int tid = threadIdx.x;
  const int xt = blockIdx.x % xtiles;
  const int yt = (blockIdx.x / xtiles) % ytiles;
  const int b = blockIdx.x / (xtiles * ytiles);
  if (b >= B) return;
  const int x0 = xt * RS_TW, y0 = yt * RS_TH;
  const int ncols = min(RS_TW, out_w - x0), nrows = min(RS_TH, out_h - y0);
  const long long plane = (long long)out_h * out_w;
  [[maybe_unused]] const long long out_total = (long long)B * 3 * plane;

  const long long off = meta[3 * b];
  const int H = (int)meta[3 * b + 1], W = (int)meta[3 * b + 2];
  const int* bx = box + 9 * b;
  const int l = tid % RS_L, half = tid / RS_L;  // this thread's tile byte and row parity

  if (!rs_box_ok(off, H, W, bx, out_h, out_w)) {
    const int c = l / RS_TW, xi = l % RS_TW;
    for (int y = half; y < nrows; y += 2)
      if (xi < ncols) out[HVK_BCHECK(((long long)b * 3 + c) * plane + (long long)(y0 + y) * out_w + x0 + xi, out_total)] = 0;
    return;
  }
  const int bi = bx[0], bj = bx[1], bh = bx[2], bw = bx[3], vh = bx[4], vw = bx[5], oy = bx[6], ox = bx[7];
  const bool flip = bx[8] != 0;

  // 1. coefficient tables: wave 0 the columns, wave 1 the rows
  if (tid < RS_TW) {
    int first = 0, count = 0;
    if (tid < ncols) {
      const int xo = x0 + tid;
      rs_axis_coefs(bw, vw, ox + (flip ? out_w - 1 - xo : xo), RS_KMAX, hk + tid * RS_KMAX, first, count);
    }
    hfirst[tid] = first;
    hcount[tid] = count;
  } else if (tid >= 64 && tid < 64 + RS_TH) {
    const int y = tid - 64;
    int first = 0, count = 0;
    if (y < nrows) rs_axis_coefs(bh, vh, oy + y0 + y, RS_KMAX, vk + y * RS_KMAX, first, count);
    vfirst[y] = first;
    vcount[y] = count;
  }
  __syncthreads();

  const uint8_t* img = src + off;
  [[maybe_unused]] const long long img_bytes = (long long)H * W * 3;
  for (int ya = 0; ya < nrows;) {
    // the sub-band [ya, yb): as many output rows as keep their source rows within RS_CAP
    // (first and last tap rise with y; one row alone needs <= RS_KMAX <= RS_CAP)
    const int r0 = vfirst[ya];
    int yb = ya + 1;
    while (yb < nrows && vfirst[yb] + vcount[yb] - r0 <= RS_CAP) ++yb;
    const int nsrc = min(vfirst[yb - 1] + vcount[yb - 1] - r0, RS_CAP);

    // 2. horizontal pass: crop rows [r0, r0 + nsrc) -> tile, byte l = (column l / 3, channel l % 3)
    {
      const int xi = l / 3, c = l % 3;
      const int n = hcount[xi];
      const int* k = hk + xi * RS_KMAX;
      const long long col = (long long)(bj + hfirst[xi]) * 3 + c;
      for (int r = half; r < nsrc; r += 2) {
        const long long row = (long long)(bi + r0 + r) * W * 3 + col;
        int acc = 1 << (RS_PREC - 1);
        for (int t = 0; t < n; ++t) acc += (int)img[HVK_BCHECK(row + 3 * t, img_bytes)] * k[t];
        tile[r * RS_L + l] = rs_clip8(acc);
      }
    }
    __syncthreads();

    // 3. vertical pass: thread l = (channel l / RS_TW, column l % RS_TW): consecutive lanes write
    // consecutive bytes of one output row of one channel plane
    {
      const int c = l / RS_TW, xi = l % RS_TW;
      if (xi < ncols)
        for (int y = ya + half; y < yb; y += 2) {
          const int n = vcount[y];
          const int* k = vk + y * RS_KMAX;
          const uint8_t* p = tile + (vfirst[y] - r0) * RS_L + xi * 3 + c;
          int acc = 1 << (RS_PREC - 1);
          for (int t = 0; t < n; ++t) acc += (int)p[t * RS_L] * k[t];
          out[HVK_BCHECK(((long long)b * 3 + c) * plane + (long long)(y0 + y) * out_w + x0 + xi, out_total)] =
              rs_clip8(acc);
        }
    }
    __syncthreads();
    ya = yb;
  }
}

}  // namespace

extern "C" {

int hvk_resized_crop_u8(const uint8_t* src, const int64_t* meta, const int32_t* box, int B, int out_h, int out_w,
                        uint8_t* out, void* stream) {
  if (B < 0 || out_h < 1 || out_w < 1 || out_h > RS_MAX_OUT || out_w > RS_MAX_OUT)
    return hvk_set_error(HVK_EINVAL, "hvk_resized_crop_u8: bad shape B=%d out=%dx%d (output side 1..%d)", B, out_h,
                         out_w, RS_MAX_OUT);
  if (B == 0) return HVK_OK;
  if (!src || !meta || !box || !out) return hvk_set_error(HVK_EINVAL, "hvk_resized_crop_u8: null pointer");
  const int xtiles = (out_w + RS_TW - 1) / RS_TW, ytiles = (out_h + RS_TH - 1) / RS_TH;
  const long long grid = (long long)B * xtiles * ytiles;
  if (grid > 0x7fffffffLL)
    return hvk_set_error(HVK_EINVAL, "hvk_resized_crop_u8: bad shape B=%d out=%dx%d (too many tiles)", B, out_h,
                         out_w);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const long long* m = reinterpret_cast<const long long*>(meta);
  hipLaunchKernelGGL(resized_crop_u8_kernel, dim3((unsigned)grid), dim3(RS_THREADS), 0, st, src, m, box, B, out_h,
                     out_w, xtiles, ytiles, out);
  HVK_CHECK_LAUNCH("resized_crop_u8");
  return HVK_OK;
}

}  // extern "C"
