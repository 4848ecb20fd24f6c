// OpenEarthMap tile preparation on the GPU: everything dataset/base_dataset.py does to a decoded tile between
// rasterio's read and the training loop, fused into one pass per batch --
//   crop (:140-174) -> pad to the crop size, image 0 / label ignore (:88-104) -> horizontal flip (:106-110) -> rot90 x k (:134-138)
//   -> channel reversal + /255 + (x - mean) / std (:29-34) -> CHW float image, int64 label (:36-43),
// plus the label re-indexing of dataset/oem.py:113-133 / oem_ft.py:197 as a 256-entry lookup table.  The random draws (crop offsets, flip,
// k) stay on the host, in the reference's order; decoding the GeoTIFF stays on the host too (rasterio).  One thread per output pixel.
#include "common.h"

namespace {

struct AugTile {            // 32 bytes, device table entry
  const uint8_t* img;       // [H][W][3] uint8 (rasterio (3,H,W) -> np.rollaxis(image, 0, 3))
  const uint8_t* lbl;       // [H][W] uint8, or null (unlabeled test tiles)
  int H, W;
  int h_off, w_off;         // crop origin
};
struct AugFlags { int flip, rot_k; };

__global__ __launch_bounds__(256) void augment_kernel(const AugTile* __restrict__ tiles, const int* __restrict__ flags, int B, int ch, int cw,
                                                      double m0, double m1, double m2, double s0, double s1, double s2, int ignore_label,
                                                      const uint8_t* __restrict__ lut, float* __restrict__ out_img, long long* __restrict__ out_lbl) {
  const long long total = (long long)B * ch * cw;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int x = (int)(i % cw), y = (int)((i / cw) % ch), b = (int)(i / ((long long)cw * ch));
    const AugTile t = tiles[b];
    const int flip = flags[2 * b], k = flags[2 * b + 1] & 3;
    // np.rot90(m, k, (0, 1)) on the square crop: out[y][x] = m[r][c]
    int r, c;
    if (k == 0) { r = y; c = x; }
    else if (k == 1) { r = x; c = cw - 1 - y; }
    else if (k == 2) { r = ch - 1 - y; c = cw - 1 - x; }
    else { r = ch - 1 - x; c = y; }
    if (flip) c = cw - 1 - c;                       // np.flip(axis=1) happened before the rotation
    const int sy = t.h_off + r, sx = t.w_off + c;   // crop; beyond the tile: the padding
    const bool inside = r < t.H - t.h_off && c < t.W - t.w_off && sy < t.H && sx < t.W;
    float v0 = 0.f, v1 = 0.f, v2 = 0.f;
    long long lab = ignore_label;
    if (inside) {
      const uint8_t* p = t.img + ((size_t)sy * t.W + sx) * 3;
      v0 = (float)p[2]; v1 = (float)p[1]; v2 = (float)p[0];      // image[:, :, ::-1]
      if (t.lbl) { const int l = t.lbl[(size_t)sy * t.W + sx]; lab = lut ? lut[l] : l; }
    }
    const size_t plane = (size_t)ch * cw, o = (size_t)b * 3 * plane + (size_t)y * cw + x;
    // numpy: float32 / 255.0 stays float32; `image -= mean` / `image /= std` with python-list operands compute in float64 and store float32
    out_img[o] = (float)((double)(float)((double)(v0 / 255.0f) - m0) / s0);
    out_img[o + plane] = (float)((double)(float)((double)(v1 / 255.0f) - m1) / s1);
    out_img[o + 2 * plane] = (float)((double)(float)((double)(v2 / 255.0f) - m2) / s2);
    if (out_lbl) out_lbl[(size_t)b * plane + (size_t)y * cw + x] = lab;
  }
}

// ---- random rescale + colour jitter in the same pass (sl_augment_batch_ex; the contract is in include/segland_hip.h) ----------------------------------------------
struct AugTileEx {          // 80 bytes, device table entry
  const uint8_t* img;       // [rows][W][3] uint8: source rows [row0, row0 + rows) of the tile
  const uint8_t* lbl;       // [rows][W] uint8, or null
  int H, W;                 // the FULL tile
  int row0, rows;
  int Hs, Ws;               // the virtual rescaled tile
  int h_off, w_off;         // crop origin in the rescaled grid
  int flip, rot_k;
  int jitter;               // 0: the photometric stage is skipped
  float alpha, bias, sigma;
  int reserved[2];
};

// align_corners=False source coordinate of rescaled index P (size S -> Ss) in integers: p0 = floor(n / d), frac = (n - p0 d) / d with n = max((2P + 1) S - Ss, 0), d = 2 Ss;
// the label's nearest index floor((2P + 1) S / d) is p0 or p0 + 1 (d = 2 Ss: it is p0 + 1 exactly when the remainder reaches Ss).  (2P + 1) S < 2^31: P < 16384, S <= 32768.
__device__ __forceinline__ void aug_tap(int P, int S, int Ss, int& p0, int& p1, float& frac, int& pl) {
  const int n = max((2 * P + 1) * S - Ss, 0);
  const unsigned d = 2u * (unsigned)Ss;
  const unsigned q = (unsigned)n / d, rem = (unsigned)n - q * d;
  p0 = (int)q;
  p1 = min(p0 + 1, S - 1);
  frac = (float)((double)rem / (double)d);
  pl = min(p0 + (rem >= (unsigned)Ss ? 1 : 0), S - 1);
}

__device__ __forceinline__ float aug_clip255(float v) { return fminf(fmaxf(v, 0.f), 255.f); }

// grid (blocks per tile, B): a block stays inside one tile, so the record, the rotation and the jitter switch are uniform (scalar loads, no divergence)
__global__ __launch_bounds__(256) void augment_ex_kernel(const AugTileEx* __restrict__ tiles, int ch, int cw, double m0, double m1, double m2, double s0, double s1,
                                                         double s2, int ignore_label, const uint8_t* __restrict__ lut, float* __restrict__ out_img,
                                                         long long* __restrict__ out_lbl) {
  const int b = blockIdx.y;
  const AugTileEx t = tiles[b];
  const int k = t.rot_k & 3, npix = ch * cw;
  const size_t plane = (size_t)npix;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += gridDim.x * blockDim.x) {
    const int x = i % cw, y = i / cw;
    int r, c;                                       // as augment_kernel: undo rot90 x k, then the flip
    if (k == 0) { r = y; c = x; }
    else if (k == 1) { r = x; c = cw - 1 - y; }
    else if (k == 2) { r = ch - 1 - y; c = cw - 1 - x; }
    else { r = ch - 1 - x; c = y; }
    if (t.flip) c = cw - 1 - c;
    const int Y = t.h_off + r, X = t.w_off + c;     // in the rescaled grid; beyond it: the padding
    float v0 = 0.f, v1 = 0.f, v2 = 0.f;             // R, G, B (source channel order)
    long long lab = ignore_label;
    if (Y < t.Hs && X < t.Ws) {
      int y0, y1, ly, x0, x1, lx;
      float fy, fx;
      aug_tap(Y, t.H, t.Hs, y0, y1, fy, ly);
      aug_tap(X, t.W, t.Ws, x0, x1, fx, lx);
      const uint8_t* ra = t.img + (size_t)(y0 - t.row0) * t.W * 3;
      const uint8_t* rb = t.img + (size_t)(y1 - t.row0) * t.W * 3;
      const uint8_t *p00 = ra + x0 * 3, *p01 = ra + x1 * 3, *p10 = rb + x0 * 3, *p11 = rb + x1 * 3;
      const float gx = 1.f - fx, gy = 1.f - fy;
      v0 = ((float)p00[0] * gx + (float)p01[0] * fx) * gy + ((float)p10[0] * gx + (float)p11[0] * fx) * fy;
      v1 = ((float)p00[1] * gx + (float)p01[1] * fx) * gy + ((float)p10[1] * gx + (float)p11[1] * fx) * fy;
      v2 = ((float)p00[2] * gx + (float)p01[2] * fx) * gy + ((float)p10[2] * gx + (float)p11[2] * fx) * fy;
      if (t.jitter) {                               // brightness + contrast, then saturation about the grey value
        v0 = aug_clip255(v0 * t.alpha + t.bias); v1 = aug_clip255(v1 * t.alpha + t.bias); v2 = aug_clip255(v2 * t.alpha + t.bias);
        const float g = 0.299f * v0 + 0.587f * v1 + 0.114f * v2;
        v0 = aug_clip255(g + (v0 - g) * t.sigma); v1 = aug_clip255(g + (v1 - g) * t.sigma); v2 = aug_clip255(g + (v2 - g) * t.sigma);
      }
      if (t.lbl) { const int l = t.lbl[(size_t)(ly - t.row0) * t.W + lx]; lab = lut ? lut[l] : l; }
    }
    const size_t o = (size_t)b * 3 * plane + (size_t)i;
    // the tail of augment_kernel: image[:, :, ::-1], float32 / 255.0, then the float64 subtract and divide stored as float32
    out_img[o] = (float)((double)(float)((double)(v2 / 255.0f) - m0) / s0);
    out_img[o + plane] = (float)((double)(float)((double)(v1 / 255.0f) - m1) / s1);
    out_img[o + 2 * plane] = (float)((double)(float)((double)(v0 / 255.0f) - m2) / s2);
    if (out_lbl) out_lbl[(size_t)b * plane + (size_t)i] = lab;
  }
}

}  // namespace

extern "C" int sl_augment_batch_ex(const void* tiles_dev, int B, int crop_h, int crop_w, const double* mean3_host, const double* std3_host, int ignore_label,
                                   const uint8_t* label_lut_dev, float* out_img, long long* out_lbl, sl_stream_t stream) {
  SL_REQUIRE(tiles_dev && out_img && mean3_host && std3_host && B > 0 && B <= 65535 && crop_h > 0 && crop_w > 0, "augment_batch_ex: bad args");
  SL_REQUIRE((long long)crop_h * crop_w <= 0x7fffffffLL - 256 * 4096, "augment_batch_ex: crop too large");
  static_assert(sizeof(AugTileEx) == 80 && sizeof(AugTileEx) % 16 == 0, "table layout is part of the ABI");
  static_assert(offsetof(AugTileEx, H) == 16 && offsetof(AugTileEx, row0) == 24 && offsetof(AugTileEx, Hs) == 32 && offsetof(AugTileEx, h_off) == 40 &&
                offsetof(AugTileEx, flip) == 48 && offsetof(AugTileEx, jitter) == 56 && offsetof(AugTileEx, alpha) == 60, "table layout is part of the ABI");
  const int npix = crop_h * crop_w, bx = (npix + 255) / 256;
  return sl_launch("augment_ex_kernel", augment_ex_kernel, dim3(bx > 4096 ? 4096 : bx, B), dim3(256), 0, (hipStream_t)stream, (const AugTileEx*)tiles_dev, crop_h, crop_w,
                   mean3_host[0], mean3_host[1], mean3_host[2], std3_host[0], std3_host[1], std3_host[2], ignore_label, label_lut_dev, out_img, out_lbl);
}

extern "C" int sl_augment_batch(const void* tiles_dev, const int* flip_rot_dev, int B, int crop_h, int crop_w, const double* mean3_host,
                                const double* std3_host, int ignore_label, const uint8_t* label_lut_dev, float* out_img, long long* out_lbl,
                                sl_stream_t stream) {
  SL_REQUIRE(tiles_dev && flip_rot_dev && out_img && mean3_host && std3_host && B > 0 && crop_h > 0 && crop_w > 0, "augment_batch: bad args");
  static_assert(sizeof(AugTile) == 32, "table layout is part of the ABI");
  const long long n = (long long)B * crop_h * crop_w;
  const int grid = (int)((n + 255) / 256 > 16384 ? 16384 : (n + 255) / 256);
  return sl_launch("augment_kernel", augment_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const AugTile*)tiles_dev, flip_rot_dev, B, crop_h, crop_w,
                   mean3_host[0], mean3_host[1], mean3_host[2], std3_host[0], std3_host[1], std3_host[2], ignore_label, label_lut_dev, out_img, out_lbl);
}
