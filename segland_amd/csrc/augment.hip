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

// ---- arbitrary-angle rotation + Gaussian blur in the same pass (sl_augment_batch_geo; the contract is in include/segland_hip.h) ---------------------------------------
struct AugTileGeo {         // 128 bytes, device table entry: the first 72 bytes are AugTileEx's
  const uint8_t* img;
  const uint8_t* lbl;
  int H, W;
  int row0, rows;
  int Hs, Ws;
  int h_off, w_off;
  int flip, rot_k;
  int jitter;
  float alpha, bias, sigma;
  int rotate;               // 0: the integer crop-frame coordinates of augment_ex_kernel
  int blur_k;               // 0: no blur, else the odd kernel size 3..11
  double cos_t, sin_t;
  float blur_w[6];          // half kernel, centre first
  int reserved[2];
};

constexpr int GEO_P = 32;                        // a block owns a GEO_P x GEO_P patch of one tile's output: 256 threads, 4 pixels each
constexpr int GEO_RMAX = 5;                      // blur_k <= 11
constexpr int GEO_T = GEO_P + 2 * GEO_RMAX;      // patch + halo
// LDS row strides in dwords, both ODD: after an odd rot90 count the lanes of a wave walk down a COLUMN of the (r, c) patch, and a stride that is a multiple of the 32 banks
// would put all of them on one bank; an odd stride spreads a column over all banks, and lanes along a row are conflict-free at any stride
constexpr int GEO_RS = GEO_T + 1;                // 43: resampled pixels
constexpr int GEO_HS = GEO_P + 1;                // 33: after the horizontal pass

// the real-valued counterpart of aug_tap: s = ((P + 0.5) S) / Ss - 0.5 in double; taps from s clamped to [0, S - 1], nearest label index floor(s + 0.5) clamped likewise
__device__ __forceinline__ void aug_tap_real(double P, int S, int Ss, int& p0, int& p1, float& frac, int& pl) {
  const double s = ((P + 0.5) * (double)S) / (double)Ss - 0.5;
  const double sc = fmin(fmax(s, 0.0), (double)(S - 1));
  p0 = (int)sc;
  p1 = min(p0 + 1, S - 1);
  frac = (float)(sc - (double)p0);
  pl = (int)fmin(fmax(floor(s + 0.5), 0.0), (double)(S - 1));
}

// steps 2-4 of the contract for crop position (r, c): R, G, B before blur and jitter; lab = -1: padding, -2: inside without a label, else the label after the table
__device__ __forceinline__ void aug_geo_sample(const AugTileGeo& t, int r, int c, int ch, int cw, const uint8_t* __restrict__ lut, bool want_label, float& v0, float& v1,
                                               float& v2, int& lab) {
  v0 = v1 = v2 = 0.f;
  lab = -1;
  int y0, y1, ly, x0, x1, lx;
  float fy, fx;
  if (!t.rotate) {
    const int Y = t.h_off + r, X = t.w_off + c;
    if (!(Y < t.Hs && X < t.Ws)) return;
    aug_tap(Y, t.H, t.Hs, y0, y1, fy, ly);
    aug_tap(X, t.W, t.Ws, x0, x1, fx, lx);
  } else {
    const double hx = 0.5 * (double)cw, hy = 0.5 * (double)ch, dx = (double)c - hx, dy = (double)r - hy;
    const double U = (double)t.w_off + (hx + (t.cos_t * dx - t.sin_t * dy));
    const double V = (double)t.h_off + (hy + (t.sin_t * dx + t.cos_t * dy));
    const double iu = floor(U + 0.5), iv = floor(V + 0.5);
    if (!(iu >= 0.0 && iu < (double)t.Ws && iv >= 0.0 && iv < (double)t.Hs)) return;      // a NaN lands here too
    aug_tap_real(V, t.H, t.Hs, y0, y1, fy, ly);
    aug_tap_real(U, t.W, t.Ws, x0, x1, fx, lx);
  }
  // a wrong record gives wrong pixels, never a read outside the buffer: rows into [row0, row0 + rows), columns into [0, W)
  const int rl = t.row0, rh = t.row0 + t.rows - 1;
  y0 = min(max(y0, rl), rh); y1 = min(max(y1, rl), rh); ly = min(max(ly, rl), rh);
  x0 = min(max(x0, 0), t.W - 1); x1 = min(max(x1, 0), t.W - 1); lx = min(max(lx, 0), t.W - 1);
  const uint8_t* ra = t.img + (size_t)(y0 - t.row0) * t.W * 3;
  const uint8_t* rb = t.img + (size_t)(y1 - t.row0) * t.W * 3;
  const uint8_t *p00 = ra + x0 * 3, *p01 = ra + x1 * 3, *p10 = rb + x0 * 3, *p11 = rb + x1 * 3;
  const float gx = 1.f - fx, gy = 1.f - fy;
  v0 = ((float)p00[0] * gx + (float)p01[0] * fx) * gy + ((float)p10[0] * gx + (float)p11[0] * fx) * fy;
  v1 = ((float)p00[1] * gx + (float)p01[1] * fx) * gy + ((float)p10[1] * gx + (float)p11[1] * fx) * fy;
  v2 = ((float)p00[2] * gx + (float)p01[2] * fx) * gy + ((float)p10[2] * gx + (float)p11[2] * fx) * fy;
  lab = -2;
  if (want_label && t.lbl) { const int l = t.lbl[(size_t)(ly - t.row0) * t.W + lx]; lab = lut ? lut[l] : l; }
}

// cv2.BORDER_REFLECT_101 on [0, n): -i -> i, n - 1 + i -> n - 1 - i (one reflection: the halo is narrower than the crop); the clamp only guards positions nobody reads
__device__ __forceinline__ int aug_reflect101(int i, int n) {
  i = i < 0 ? -i : i;
  i = i >= n ? 2 * (n - 1) - i : i;
  return min(max(i, 0), n - 1);
}

// grid (patches per tile, B): the record, and with it the rotation, the blur radius and the jitter switch, is uniform in a block
__global__ __launch_bounds__(256) void augment_geo_kernel(const AugTileGeo* __restrict__ tiles, int ch, int cw, double m0, double m1, double m2, double s0, double s1,
                                                          double s2, int ignore_label, const uint8_t* __restrict__ lut, float* __restrict__ out_img,
                                                          long long* __restrict__ out_lbl) {
  __shared__ float s_raw[3][GEO_T * GEO_RS];      // R, G, B of the patch + halo in crop-frame (r, c) order
  __shared__ int s_lab[GEO_T * GEO_RS];           // the lab of aug_geo_sample
  __shared__ float s_hor[3][GEO_T * GEO_HS];      // after the horizontal pass: halo rows, patch columns
  const int b = blockIdx.y;
  const AugTileGeo& t = tiles[b];                 // read in place: the 32-dword record next to the six doubles would not fit the scalar registers as a copy
  const int k = t.rot_k & 3, R =min(max(t.blur_k, 0) >> 1, GEO_RMAX);
  const size_t plane = (size_t)ch * cw;
  const int npx = (cw + GEO_P - 1) / GEO_P;
  const int ya = (blockIdx.x / npx) * GEO_P, xa = (blockIdx.x % npx) * GEO_P, yb = min(ya + GEO_P, ch), xb = min(xa + GEO_P, cw);
  const int tx = threadIdx.x & (GEO_P - 1), ty = threadIdx.x / GEO_P;
  // the (r, c) rectangle of the output patch [ya, yb) x [xa, xb): undo rot90 x k, then the flip
  int rlo, rhi, clo, chi;
  if (k == 0) { rlo = ya; rhi = yb; clo = xa; chi = xb; }
  else if (k == 1) { rlo = xa; rhi = xb; clo = cw - yb; chi = cw - ya; }
  else if (k == 2) { rlo = ch - yb; rhi = ch - ya; clo = cw - xb; chi = cw - xa; }
  else { rlo = ch - xb; rhi = ch - xa; clo = ya; chi = yb; }
  if (t.flip) { const int lo = cw - chi; chi = cw - clo; clo = lo; }
  const int th = rhi - rlo + 2 * R, tw = chi - clo + 2 * R, pw = chi - clo;
  if (R) {                                        // block-uniform: without a blur no LDS pass runs
    for (int i = threadIdx.x; i < th * tw; i += 256) {
      const int li = i / tw, lj = i - li * tw;
      const bool own = li >= R && li < th - R && lj >= R && lj < tw - R;
      float v0, v1, v2;
      int lab;
      aug_geo_sample(t, aug_reflect101(rlo - R + li, ch), aug_reflect101(clo - R + lj, cw), ch, cw, lut, own, v0, v1, v2, lab);
      const int o = li * GEO_RS + lj;
      s_raw[0][o] = v0; s_raw[1][o] = v1; s_raw[2][o] = v2;
      s_lab[o] = lab;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < th * pw; i += 256) {      // horizontal pass: lanes along a row
      const int li = i / pw, lj = i - li * pw, o = li * GEO_RS + lj + R;
      float a0 = t.blur_w[0] * s_raw[0][o], a1 = t.blur_w[0] * s_raw[1][o], a2 = t.blur_w[0] * s_raw[2][o];
#pragma unroll
      for (int d = 1; d <= GEO_RMAX; ++d)
        if (d <= R) {
          a0 += t.blur_w[d] * (s_raw[0][o - d] + s_raw[0][o + d]);
          a1 += t.blur_w[d] * (s_raw[1][o - d] + s_raw[1][o + d]);
          a2 += t.blur_w[d] * (s_raw[2][o - d] + s_raw[2][o + d]);
        }
      const int h = li * GEO_HS + lj;
      s_hor[0][h] = a0; s_hor[1][h] = a1; s_hor[2][h] = a2;
    }
    __syncthreads();
  }
#pragma unroll 1
  for (int q = 0; q < GEO_P / 8; ++q) {
    const int y = ya + ty + 8 * q, x = xa + tx;
    if (y >= yb || x >= xb) continue;
    int r, c;                                       // as augment_kernel: undo rot90 x k, then the flip
    if (k == 0) { r = y; c = x; }
    else if (k == 1) { r = x; c = cw - 1 - y; }
    else if (k == 2) { r = ch - 1 - y; c = cw - 1 - x; }
    else { r = ch - 1 - x; c = y; }
    if (t.flip) c = cw - 1 - c;
    float v0 = 0.f, v1 = 0.f, v2 = 0.f;
    int lab;
    if (R) {                                        // vertical pass from the LDS; padding pixels stay 0
      const int li = r - rlo + R, lj = c - clo, h = li * GEO_HS + lj;
      lab = s_lab[li * GEO_RS + lj + R];
      if (lab != -1) {
        v0 = t.blur_w[0] * s_hor[0][h]; v1 = t.blur_w[0] * s_hor[1][h]; v2 = t.blur_w[0] * s_hor[2][h];
#pragma unroll
        for (int d = 1; d <= GEO_RMAX; ++d)
          if (d <= R) {
            v0 += t.blur_w[d] * (s_hor[0][h - d * GEO_HS] + s_hor[0][h + d * GEO_HS]);
            v1 += t.blur_w[d] * (s_hor[1][h - d * GEO_HS] + s_hor[1][h + d * GEO_HS]);
            v2 += t.blur_w[d] * (s_hor[2][h - d * GEO_HS] + s_hor[2][h + d * GEO_HS]);
          }
      }
    } else {
      aug_geo_sample(t, r, c, ch, cw, lut, true, v0, v1, v2, lab);
    }
    if (lab != -1 && t.jitter) {                    // as augment_ex_kernel
      v0 = aug_clip255(v0 * t.alpha + t.bias); v1 = aug_clip255(v1 * t.alpha + t.bias); v2 = aug_clip255(v2 * t.alpha + t.bias);
      const float g = 0.299f * v0 + 0.587f * v1 + 0.114f * v2;
      v0 = aug_clip255(g + (v0 - g) * t.sigma); v1 = aug_clip255(g + (v1 - g) * t.sigma); v2 = aug_clip255(g + (v2 - g) * t.sigma);
    }
    const size_t i = (size_t)y * cw + x, o = (size_t)b * 3 * plane + i;
    out_img[o] = (float)((double)(float)((double)(v2 / 255.0f) - m0) / s0);
    out_img[o + plane] = (float)((double)(float)((double)(v1 / 255.0f) - m1) / s1);
    out_img[o + 2 * plane] = (float)((double)(float)((double)(v0 / 255.0f) - m2) / s2);
    if (out_lbl) out_lbl[(size_t)b * plane + i] = lab >= 0 ? lab : ignore_label;
  }
}

}  // namespace

extern "C" int sl_augment_batch_geo(const void* tiles_dev, int B, int crop_h, int crop_w, const double* mean3_host, const double* std3_host, int ignore_label,
                                    const uint8_t* label_lut_dev, float* out_img, long long* out_lbl, sl_stream_t stream) {
  SL_REQUIRE(tiles_dev && out_img && mean3_host && std3_host && B > 0 && B <= 65535 && crop_h > 0 && crop_w > 0, "augment_batch_geo: bad args");
  SL_REQUIRE((long long)crop_h * crop_w <= 0x7fffffffLL - 256 * 4096, "augment_batch_geo: crop too large");
  static_assert(sizeof(AugTileGeo) == 128 && sizeof(AugTileGeo) % 16 == 0, "table layout is part of the ABI");
  static_assert(offsetof(AugTileGeo, H) == 16 && offsetof(AugTileGeo, row0) == 24 && offsetof(AugTileGeo, Hs) == 32 && offsetof(AugTileGeo, h_off) == 40 &&
                offsetof(AugTileGeo, flip) == 48 && offsetof(AugTileGeo, jitter) == 56 && offsetof(AugTileGeo, alpha) == 60 && offsetof(AugTileGeo, rotate) == 72 &&
                offsetof(AugTileGeo, blur_k) == 76 && offsetof(AugTileGeo, cos_t) == 80 && offsetof(AugTileGeo, sin_t) == 88 && offsetof(AugTileGeo, blur_w) == 96 &&
                offsetof(AugTileGeo, reserved) == 120, "table layout is part of the ABI");
  const long long patches = (long long)((crop_h + GEO_P - 1) / GEO_P) * ((crop_w + GEO_P - 1) / GEO_P);
  return sl_launch("augment_geo_kernel", augment_geo_kernel, dim3((unsigned)patches, B), dim3(256), 0, (hipStream_t)stream, (const AugTileGeo*)tiles_dev, crop_h, crop_w,
                   mean3_host[0], mean3_host[1], mean3_host[2], std3_host[0], std3_host[1], std3_host[2], ignore_label, label_lut_dev, out_img, out_lbl);
}

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
