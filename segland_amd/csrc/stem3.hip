// Deep ResNet stem for gfx950, first layer: conv 3x3 s2 p1 (3 -> 64) straight from the NCHW float image and its weight gradient
// (networks/backbones/resnet.py:144,187).  conv2 / conv3 of the deep stem are ordinary 64-channel layers and run on the conv kernels; the
// BN + ReLU + maxpool behind conv3 is the channel-count form of the pool kernels in stem.hip.
// Cin = 3 makes this layer pure traffic (12 B in, 128 B out per output pixel in bf16), so everything that touches the output tile rides in the one launch:
// the BatchNorm statistic partials in training, or the folded BatchNorm + ReLU on frozen statistics.
#include "common.h"

namespace {

constexpr int TS = 16;                 // output tile edge
constexpr int PS = (TS - 1) * 2 + 3;   // input patch edge = 33
constexpr int NTAP = 27;               // 3*3*3
constexpr int MP = 48;                 // bf16 patch row pitch: tile rows are 2*MP elements = 48 banks apart, so the 32 pixels of an MFMA operand (two tile rows) hit 32 different banks
constexpr int KSTEPS = 2;              // 32 = 27 taps zero padded

inline int tiles(int B, int H, int W) { return B * cdiv((H + 1) / 2, TS) * cdiv((W + 1) / 2, TS); }
inline int wgrad_blocks(int ntiles) { return ntiles < 512 ? ntiles : 512; }

// patch[c][PS][PS] of image rows 2*oy0-1 .., zero outside
__device__ __forceinline__ void load_patch_f32(float* patch, const float* img, int b, int H, int W, int oy0, int ox0, int tid) {
  for (int e = tid; e < 3 * PS * PS; e += 256) {
    const int c = e / (PS * PS), r = (e / PS) % PS, q = e % PS;
    const int iy = 2 * oy0 - 1 + r, ix = 2 * ox0 - 1 + q;
    float v = 0.f;
    if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W) v = img[((size_t)(b * 3 + c) * H + iy) * W + ix];
    patch[e] = v;
  }
}

// the same as bf16 [3][PS][MP]: 99 patch rows, two threads per row (17 + 16 elements), no division in the loop.
// lo != nullptr: the image as a bf16 pair, hi = bf16(v) and lo = bf16(v - hi) (16 mantissa bits between them)
__device__ __forceinline__ void load_patch_bf16(bf16_t* patch, const float* img, int b, int H, int W, int oy0, int ox0, int tid, bf16_t* lo = nullptr) {
  const int rr = tid >> 1, half = tid & 1;
  if (rr < 3 * PS) {
    const int c = rr / PS, r = rr - c * PS;
    const int iy = 2 * oy0 - 1 + r, ix0 = 2 * ox0 - 1;
    const bool rowok = (unsigned)iy < (unsigned)H;
    const float* src = img + ((size_t)(b * 3 + c) * H + (rowok ? iy : 0)) * W;
    bf16_t* dst = patch + rr * MP;
    const int q0 = half * 17, q1 = half ? PS : 17;
    for (int q = q0; q < q1; ++q) {
      const int ix = ix0 + q;
      const float v = rowok && (unsigned)ix < (unsigned)W ? src[ix] : 0.f;
      const bf16_t h = from_f<bf16_t>(v);
      dst[q] = h;
      if (lo) lo[rr * MP + q] = from_f<bf16_t>(v - to_f<bf16_t>(h));
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// fp32 (parity mode): direct LDS-tiled convolution, one exact fma chain per output in tap order (c, ky, kx).  wave = channel group of 16, lane = 4 pixels of a tile row.
// scale != nullptr: y = relu(conv * scale + shift) (frozen BatchNorm); part != nullptr: (sum, sum of squares) of the block's accumulators -> part[block][2][64].
__global__ __launch_bounds__(256) void stem3_conv_fwd_kernel(const float* __restrict__ img, const float* __restrict__ w, float* __restrict__ y, float* __restrict__ part,
                                                             const float* __restrict__ scale, const float* __restrict__ shift, int B, int H, int W) {
  __shared__ __attribute__((aligned(16))) float wl[NTAP * 64];      // [27][64]
  __shared__ float patch[3 * PS * PS];
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  const int tx = cdiv(Wo, TS), ty = cdiv(Ho, TS);
  const int tid = threadIdx.x;
  int blk = blockIdx.x;
  const int bx = blk % tx; blk /= tx;
  const int by = blk % ty; const int b = blk / ty;
  for (int e = tid; e < 64 * NTAP; e += 256) { const int n = e / NTAP, t = e % NTAP; wl[t * 64 + n] = w[e]; }
  load_patch_f32(patch, img, b, H, W, by * TS, bx * TS, tid);
  __syncthreads();

  const int pg = tid & 63, cg = tid >> 6;
  const int py = pg >> 2, px0 = (pg & 3) * 4;
  float acc[4][16];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int k = 0; k < 16; ++k) acc[j][k] = 0.f;
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const float* prow = patch + (c * PS + 2 * py + ky) * PS + 2 * px0;
      const float* wrow = wl + ((c * 3 + ky) * 3) * 64 + cg * 16;
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        float wv[16];
#pragma unroll
        for (int k = 0; k < 16; k += 4) { const float4 t = *(const float4*)(wrow + kx * 64 + k); wv[k] = t.x; wv[k + 1] = t.y; wv[k + 2] = t.z; wv[k + 3] = t.w; }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float a = prow[2 * j + kx];
#pragma unroll
          for (int k = 0; k < 16; ++k) acc[j][k] = fmaf(a, wv[k], acc[j][k]);
        }
      }
    }
  const int oy = by * TS + py;
  float s1[16], s2[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) { s1[k] = 0.f; s2[k] = 0.f; }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ox = bx * TS + px0 + j;
    if (oy < Ho && ox < Wo) {
#pragma unroll
      for (int k = 0; k < 16; ++k) { s1[k] += acc[j][k]; s2[k] += acc[j][k] * acc[j][k]; }
      if (scale) {
#pragma unroll
        for (int k = 0; k < 16; ++k) { const float t = acc[j][k] * scale[cg * 16 + k] + shift[cg * 16 + k]; acc[j][k] = t > 0.f ? t : 0.f; }
      }
      float* o = y + ((size_t)(b * Ho + oy) * Wo + ox) * 64 + cg * 16;
#pragma unroll
      for (int k = 0; k < 16; k += 4) *(uint4*)(o + k) = pack16<float>(&acc[j][k]);
    }
  }
  if (part) {
#pragma unroll
    for (int k = 0; k < 16; ++k) { s1[k] = wave_sum(s1[k]); s2[k] = wave_sum(s2[k]); }
    if (pg == 0) {
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        part[((size_t)blockIdx.x * 2 + 0) * 64 + cg * 16 + k] = s1[k];
        part[((size_t)blockIdx.x * 2 + 1) * 64 + cg * 16 + k] = s2[k];
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// bf16 forward on the matrix cores: the 16x16-pixel output tile of a block is a [256 pixels] x [32 = 27 taps, zero padded] x [64 channels] GEMM whose pixel
// operand is gathered from the bf16 image patch in the LDS (no im2col in memory).  Operand roles as in the 7x7 kernel (stem.hip): first MFMA operand = weight
// rows (-> accumulator registers), second = pixel rows (-> lanes); a wave owns 64 pixels x 64 channels: 2 pixel blocks x 2 channel blocks x 2 k-steps = 8 MFMAs.
// The weight fragments come ready-made from an 8 KiB table (stem3_weight_frag_kernel, one tiny launch per call).
// The image is the one operand of the network that arrives in fp32, and this layer has only 27 taps to average a rounding over: rounding image and weights to
// bf16 here was the largest single source of ReLU / maxpool flips further down the stem (measured on the stem's gradients: DESIGN.md 3.10).  So both operands are
// bf16 PAIRS (hi + lo) and a k-step is three MFMAs per accumulator, w_hi x_hi + w_hi x_lo + w_lo x_hi (the lo x lo term is below 2^-16): 24 MFMAs per wave instead
// of 8, in a kernel whose time is its 184 MB of traffic.

// wfrag[(part*4 + nb*2 + ks)*64 + lane] = W[nb*32 + (lane & 31)][ks*16 + (lane >> 5)*8 .. +8] as bf16 (taps >= 27 zero); part 0: hi = bf16(w), part 1: lo = bf16(w - hi)
__global__ void stem3_weight_frag_kernel(const float* __restrict__ w, uint4* __restrict__ wfrag) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 2 * KSTEPS * 64) return;
  const int lane = t & 63, ks = (t >> 6) % KSTEPS, nb = (t >> 6) / KSTEPS;
  const int n = nb * 32 + (lane & 31), k0 = ks * 16 + (lane >> 5) * 8;
  unsigned short v[8], u[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float x = k0 + e < NTAP ? w[n * NTAP + k0 + e] : 0.f;
    v[e] = from_f<bf16_t>(x);
    u[e] = from_f<bf16_t>(x - to_f<bf16_t>(v[e]));
  }
  wfrag[t] = make_uint4(v[0] | ((unsigned)v[1] << 16), v[2] | ((unsigned)v[3] << 16), v[4] | ((unsigned)v[5] << 16), v[6] | ((unsigned)v[7] << 16));
  wfrag[2 * KSTEPS * 64 + t] = make_uint4(u[0] | ((unsigned)u[1] << 16), u[2] | ((unsigned)u[3] << 16), u[4] | ((unsigned)u[5] << 16), u[6] | ((unsigned)u[7] << 16));
}

__host__ __device__ constexpr int tap_off(int k) { return k < NTAP ? ((k / 9) * PS + (k % 9) / 3) * MP + (k % 3) : 0; }

template <int KS>
__device__ __forceinline__ void stem3_kstep(const bf16_t* __restrict__ patch, const bf16_t* __restrict__ patch_lo, const int (&pbase)[2], int fh, const uint4* __restrict__ wfrag, int lane,
                                            f32x16_t (&acc)[2][2]) {
  constexpr int LO = 2 * KSTEPS * 64;
  const uint4 w0 = wfrag[(0 * KSTEPS + KS) * 64 + lane], w1 = wfrag[(1 * KSTEPS + KS) * 64 + lane];
  const uint4 l0 = wfrag[LO + (0 * KSTEPS + KS) * 64 + lane], l1 = wfrag[LO + (1 * KSTEPS + KS) * 64 + lane];
  int off[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) off[e] = fh ? tap_off(KS * 16 + 8 + e) : tap_off(KS * 16 + e);      // two immediates and a select
#pragma unroll
  for (int rb = 0; rb < 2; ++rb) {
    unsigned v[8], u[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { v[e] = patch[pbase[rb] + off[e]]; u[e] = patch_lo[pbase[rb] + off[e]]; }
    // taps >= 27 read patch[pbase + 0] against a ZERO weight
    const bf16x8_t a = __builtin_bit_cast(bf16x8_t, make_uint4(v[0] | (v[1] << 16), v[2] | (v[3] << 16), v[4] | (v[5] << 16), v[6] | (v[7] << 16)));
    const bf16x8_t al = __builtin_bit_cast(bf16x8_t, make_uint4(u[0] | (u[1] << 16), u[2] | (u[3] << 16), u[4] | (u[5] << 16), u[6] | (u[7] << 16)));
    // the two small terms first, then the leading one
    acc[rb][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, l0), a, acc[rb][0], 0, 0, 0);
    acc[rb][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, l1), a, acc[rb][1], 0, 0, 0);
    acc[rb][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, w0), al, acc[rb][0], 0, 0, 0);
    acc[rb][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, w1), al, acc[rb][1], 0, 0, 0);
    acc[rb][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, w0), a, acc[rb][0], 0, 0, 0);
    acc[rb][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, w1), a, acc[rb][1], 0, 0, 0);
  }
}

// Sum of v[i] over the 32 lanes of a wave half for all 32 i at once: at each step a lane keeps the half of its values whose index bit equals its lane bit and
// adds its partner's; after five steps lane l holds the total of value (l & 31).  31 shuffles instead of 160; the order of the additions is fixed.
__device__ __forceinline__ float half_wave_transpose_sum(float (&v)[32], int lane) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) {
    const bool up = lane & o;
#pragma unroll
    for (int i = 0; i < o; ++i) {
      const float lo = v[i], hi = v[i + o];
      v[i] = (up ? hi : lo) + __shfl_xor(up ? lo : hi, o, 64);
    }
  }
  return v[0];
}

__global__ __launch_bounds__(256) void stem3_conv_fwd_mfma_kernel(const float* __restrict__ img, const uint4* __restrict__ wfrag, bf16_t* __restrict__ y, float* __restrict__ part,
                                                                  const float* __restrict__ scale, const float* __restrict__ shift, int B, int H, int W) {
  __shared__ __attribute__((aligned(16))) bf16_t smem[256 * 72];      // the patch as a bf16 pair, 2 x [3][PS][MP] (19 008 B), then the staging tile [256][64 + 8]
  __shared__ float red[4 * 2 * 64];
  bf16_t* patch = smem;
  bf16_t* patch_lo = smem + 3 * PS * MP;
  bf16_t* outt = smem;
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  const int tx = cdiv(Wo, TS), ty = cdiv(Ho, TS);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int blk = blockIdx.x;
  const int bx = blk % tx; blk /= tx;
  const int by = blk % ty; const int b = blk / ty;
  load_patch_bf16(patch, img, b, H, W, by * TS, bx * TS, tid, patch_lo);
  __syncthreads();

  const int l31 = lane & 31, fh = lane >> 5;
  f32x16_t acc[2][2];
#pragma unroll
  for (int rb = 0; rb < 2; ++rb)
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[rb][nb][r] = 0.f;
  int pbase[2];                                            // pixel of this lane in row block rb: p = wave*64 + rb*32 + l31 -> (py, px) of the tile
  bool valid[2];
#pragma unroll
  for (int rb = 0; rb < 2; ++rb) {
    const int pidx = wave * 64 + rb * 32 + l31;
    pbase[rb] = (2 * (pidx >> 4)) * MP + 2 * (pidx & 15);
    valid[rb] = by * TS + (pidx >> 4) < Ho && bx * TS + (pidx & 15) < Wo;
  }
  stem3_kstep<0>(patch, patch_lo, pbase, fh, wfrag, lane, acc);
  stem3_kstep<1>(patch, patch_lo, pbase, fh, wfrag, lane, acc);
  __syncthreads();                                         // the patch is dead: the staging tile takes its place
  // D layout: lane = pixel (l31), register r = channel (r&3) + 8*(r>>2) + 4*fh of the 32-channel block
  if (part) {                                              // statistics of the fp32 accumulators, pixels outside the map excluded
    float s[32], q[32];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float a0 = valid[0] ? acc[0][nb][r] : 0.f, a1 = valid[1] ? acc[1][nb][r] : 0.f;
        s[nb * 16 + r] = a0 + a1; q[nb * 16 + r] = a0 * a0 + a1 * a1;
      }
    const float ts = half_wave_transpose_sum(s, lane), tq = half_wave_transpose_sum(q, lane);
    const int r = l31 & 15, ch = (l31 >> 4) * 32 + (r & 3) + 8 * (r >> 2) + 4 * fh;       // lane l31 holds value index l31 = nb*16 + r
    red[(wave * 2 + 0) * 64 + ch] = ts; red[(wave * 2 + 1) * 64 + ch] = tq;
  }
  float sc[2][16], sh[2][16];
  if (scale) {
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
      for (int r = 0; r < 16; ++r) { const int ch = nb * 32 + (r & 3) + 8 * (r >> 2) + 4 * fh; sc[nb][r] = scale[ch]; sh[nb][r] = shift[ch]; }
  }
#pragma unroll
  for (int rb = 0; rb < 2; ++rb) {
    const int pidx = wave * 64 + rb * 32 + l31;
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
      for (int qd = 0; qd < 4; ++qd) {
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          o[e] = acc[rb][nb][4 * qd + e];
          if (scale) { const float t = o[e] * sc[nb][4 * qd + e] + sh[nb][4 * qd + e]; o[e] = t > 0.f ? t : 0.f; }
        }
        uint2 pk;
        pk.x = (unsigned)from_f<bf16_t>(o[0]) | ((unsigned)from_f<bf16_t>(o[1]) << 16);
        pk.y = (unsigned)from_f<bf16_t>(o[2]) | ((unsigned)from_f<bf16_t>(o[3]) << 16);
        *(uint2*)(outt + pidx * 72 + nb * 32 + 8 * qd + 4 * fh) = pk;
      }
  }
  __syncthreads();
  for (int e = tid; e < 256 * 8; e += 256) {               // 8 x 16-byte chunks per pixel row
    const int pidx = e >> 3, ch8 = e & 7;
    const int oy = by * TS + (pidx >> 4), ox = bx * TS + (pidx & 15);
    if (oy < Ho && ox < Wo) *(uint4*)(y + ((size_t)(b * Ho + oy) * Wo + ox) * 64 + ch8 * 8) = *(const uint4*)(outt + pidx * 72 + ch8 * 8);
  }
  if (part && tid < 128) {
    const int which = tid >> 6, ch = tid & 63;
    part[((size_t)blockIdx.x * 2 + which) * 64 + ch] = red[(0 * 2 + which) * 64 + ch] + red[(1 * 2 + which) * 64 + ch] + red[(2 * 2 + which) * 64 + ch] + red[(3 * 2 + which) * 64 + ch];
  }
}

// ---------------------------------------------------------------------------------------------------------------
// fp32 weight gradient, direct: thread = (output channel n, wave g); wave g owns the (c, ky) rows g, g+4, g+8 of the 9, three kx each.  A block walks
// tiles_per_blk tiles and writes one partial ws[blk][64][27] (OIHW order inside).
__global__ __launch_bounds__(256) void stem3_wgrad_kernel(const float* __restrict__ img, const float* __restrict__ dc, float* __restrict__ ws,
                                                          int B, int H, int W, int tiles_per_blk, int ntiles) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* dyl = sm;                    // [256 px][64]
  float* patch = sm + 256 * 64;       // [3][33][33]
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  const int tx = cdiv(Wo, TS), ty = cdiv(Ho, TS);
  const int tid = threadIdx.x, n = tid & 63;
  const int g = __builtin_amdgcn_readfirstlane(tid >> 6);
  float acc[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int k = 0; k < 3; ++k) acc[i][k] = 0.f;
  for (int t = 0; t < tiles_per_blk; ++t) {
    int tile = blockIdx.x * tiles_per_blk + t;
    if (tile >= ntiles) break;
    const int bx = tile % tx; tile /= tx;
    const int by = tile % ty; const int b = tile / ty;
    __syncthreads();
    load_patch_f32(patch, img, b, H, W, by * TS, bx * TS, tid);
    for (int e = tid; e < 256 * 64; e += 256) {
      const int p = e >> 6, c = e & 63;
      const int oy = by * TS + (p >> 4), ox = bx * TS + (p & 15);
      float v = 0.f;
      if (oy < Ho && ox < Wo) v = dc[((size_t)(b * Ho + oy) * Wo + ox) * 64 + c];
      dyl[e] = v;
    }
    __syncthreads();
    for (int p = 0; p < 256; ++p) {
      const float a = dyl[p * 64 + n];
      const int py = p >> 4, px = p & 15;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const int id = g + 4 * i;
        if (id < 9) {
          const int c = id / 3, ky = id - 3 * c;
          const float* prow = patch + (c * PS + 2 * py + ky) * PS + 2 * px;
#pragma unroll
          for (int k = 0; k < 3; ++k) acc[i][k] = fmaf(a, prow[k], acc[i][k]);
        }
      }
    }
  }
  float* o = ws + (size_t)blockIdx.x * 64 * NTAP + n * NTAP;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int id = g + 4 * i;
    if (id < 9) {
#pragma unroll
      for (int k = 0; k < 3; ++k) o[id * 3 + k] = acc[i][k];
    }
  }
}

// bf16 weight gradient on the matrix cores: dw[n][k] = sum over pixels of dc[p][n] * patch(p, k).  The reduction index is the pixel, so both MFMA operands are
// gathered K-major from the LDS: first operand = dc^T (rows = output channels -> registers), second = the im2col view of the bf16 image patch (rows = the 32
// padded taps -> lanes), 8 consecutive pixels of one tile row per lane.  A wave reduces its 64 pixels of every tile the persistent block walks into two 32x32
// accumulators (64 channels x 32 taps); the four waves are summed through the LDS at the end and the block writes one [64][27] partial.
__global__ __launch_bounds__(256) void stem3_wgrad_mfma_kernel(const float* __restrict__ img, const bf16_t* __restrict__ dc, float* __restrict__ ws,
                                                               int B, int H, int W, int ntiles) {
  __shared__ __attribute__((aligned(16))) bf16_t patch[3 * PS * MP];      //  9 504 B
  __shared__ __attribute__((aligned(16))) bf16_t dct[256 * 72];           // 36 864 B
  float* red = (float*)dct;                                               // [4][16][64] floats, after the tile loop
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  const int tx = cdiv(Wo, TS), ty = cdiv(Ho, TS);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, fh = lane >> 5;
  f32x16_t acc[2];
#pragma unroll
  for (int nb = 0; nb < 2; ++nb)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[nb][r] = 0.f;
  const int toff = l31 < NTAP ? ((l31 / 9) * PS + (l31 % 9) / 3) * MP + (l31 % 3) : 0;      // taps >= 27: any valid address, the column is dropped
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    int blk = tile;
    const int bx = blk % tx; blk /= tx;
    const int by = blk % ty; const int b = blk / ty;
    load_patch_bf16(patch, img, b, H, W, by * TS, bx * TS, tid);
    for (int e = tid; e < 256 * 8; e += 256) {             // the dc tile, zero outside the map
      const int pidx = e >> 3, ch8 = e & 7;
      const int oy = by * TS + (pidx >> 4), ox = bx * TS + (pidx & 15);
      uint4 v = make_uint4(0, 0, 0, 0);
      if (oy < Ho && ox < Wo) v = *(const uint4*)(dc + ((size_t)(b * Ho + oy) * Wo + ox) * 64 + ch8 * 8);
      *(uint4*)(dct + pidx * 72 + ch8 * 8) = v;
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      // pixels p = wave*64 + ks*16 + fh*8 + e: tile row py = wave*4 + ks, columns px = fh*8 + e
      const int prow = wave * 64 + ks * 16 + fh * 8;
      const int pb = (2 * (wave * 4 + ks)) * MP + 2 * (fh * 8);
      unsigned v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = patch[pb + toff + 2 * e];
      const uint4 fb = make_uint4(v[0] | (v[1] << 16), v[2] | (v[3] << 16), v[4] | (v[5] << 16), v[6] | (v[7] << 16));
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) {
        unsigned u[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) u[e] = dct[(prow + e) * 72 + nb * 32 + l31];
        const uint4 fa = make_uint4(u[0] | (u[1] << 16), u[2] | (u[3] << 16), u[4] | (u[5] << 16), u[6] | (u[7] << 16));
        acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, fa), __builtin_bit_cast(bf16x8_t, fb), acc[nb], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  // D layout: lane l31 = tap, register r = channel (r&3) + 8*(r>>2) + 4*fh of the block.  Sum the four waves, one accumulator at a time.
  float* out = ws + (size_t)blockIdx.x * 64 * NTAP;
#pragma unroll
  for (int nb = 0; nb < 2; ++nb) {
#pragma unroll
    for (int r = 0; r < 16; ++r) red[(wave * 16 + r) * 64 + lane] = acc[nb][r];
    __syncthreads();
    for (int e = tid; e < 16 * 64; e += 256) {
      const int r = e >> 6, ln = e & 63;
      const float t = red[(0 * 16 + r) * 64 + ln] + red[(1 * 16 + r) * 64 + ln] + red[(2 * 16 + r) * 64 + ln] + red[(3 * 16 + r) * 64 + ln];
      const int n = nb * 32 + (r & 3) + 8 * (r >> 2) + 4 * (ln >> 5), k = ln & 31;
      if (k < NTAP) out[n * NTAP + k] = t;
    }
    __syncthreads();
  }
}

}  // namespace

extern "C" int sl_stem3_conv_stat_rows(int B, int H, int W) { return (B > 0 && H > 0 && W > 0) ? tiles(B, H, W) : 0; }

extern "C" size_t sl_stem3_conv_fwd_workspace(int dtype) { return dtype == SL_BF16 ? 2 * 2 * KSTEPS * 64 * sizeof(uint4) : 0; }      // hi and lo fragment tables

extern "C" int sl_stem3_conv_fwd(int dtype, const float* img_nchw, const float* w_oihw, const float* scale, const float* shift, void* y, float* stat_partial,
                                 int B, int H, int W, void* workspace, sl_stream_t stream) {
  SL_REQUIRE(img_nchw && w_oihw && y && B > 0 && H > 0 && W > 0, "stem3_conv_fwd: bad args");
  SL_REQUIRE((scale == nullptr) == (shift == nullptr), "stem3_conv_fwd: scale and shift come in pairs");
  SL_REQUIRE(!(scale && stat_partial), "stem3_conv_fwd: the folded-BatchNorm form writes no statistics");
  SL_REQUIRE(dtype == SL_BF16 || dtype == SL_F32, "stem3_conv_fwd: bad dtype");
  SL_REQUIRE((long long)B * 3 * H * W < (1ll << 31) && (long long)B * ((H + 1) / 2) * ((W + 1) / 2) * 64 < (1ll << 31), "stem3_conv_fwd: more than 2^31 elements");
  dim3 grid(tiles(B, H, W));
  if (dtype == SL_BF16) {
    SL_REQUIRE(workspace && ((size_t)workspace & 15) == 0, "stem3_conv_fwd: bf16 needs the 16-byte aligned workspace of sl_stem3_conv_fwd_workspace()");
    uint4* wfrag = (uint4*)workspace;                                           // the weights in MFMA fragment order, rebuilt on every call (8 KiB)
    SL_TRY(sl_launch("stem3_weight_frag_kernel", stem3_weight_frag_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, w_oihw, wfrag));
    return sl_launch("stem3_conv_fwd_mfma_kernel", stem3_conv_fwd_mfma_kernel, grid, dim3(256), 0, (hipStream_t)stream, img_nchw, (const uint4*)wfrag, (bf16_t*)y, stat_partial, scale, shift, B, H, W);
  }
  return sl_launch("stem3_conv_fwd_kernel", stem3_conv_fwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, img_nchw, w_oihw, (float*)y, stat_partial, scale, shift, B, H, W);
}

extern "C" size_t sl_stem3_conv_bwd_weight_workspace(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)wgrad_blocks(tiles(B, H, W)) * 64 * NTAP * sizeof(float);
}

extern "C" int sl_stem3_conv_bwd_weight(int dtype, const float* img_nchw, const void* dc1, float* dw_oihw, void* workspace, size_t workspace_bytes,
                                        int B, int H, int W, sl_stream_t stream) {
  SL_REQUIRE(img_nchw && dc1 && dw_oihw && workspace && B > 0 && H > 0 && W > 0, "stem3_conv_bwd_weight: bad args");
  SL_REQUIRE(dtype == SL_BF16 || dtype == SL_F32, "stem3_conv_bwd_weight: bad dtype");
  SL_REQUIRE((long long)B * 3 * H * W < (1ll << 31) && (long long)B * ((H + 1) / 2) * ((W + 1) / 2) * 64 < (1ll << 31), "stem3_conv_bwd_weight: more than 2^31 elements");
  const int ntiles = tiles(B, H, W), nblk = wgrad_blocks(ntiles), tpb = cdiv(ntiles, nblk);
  if (workspace_bytes < (size_t)nblk * 64 * NTAP * sizeof(float)) { sl_set_error("stem3_conv_bwd_weight: workspace too small"); return SL_EWORKSPACE; }
  hipStream_t st = (hipStream_t)stream;
  if (dtype == SL_BF16) {
    SL_TRY(sl_launch("stem3_wgrad_mfma_kernel", stem3_wgrad_mfma_kernel, dim3(nblk), dim3(256), 0, st, img_nchw, (const bf16_t*)dc1, (float*)workspace, B, H, W, ntiles));
  } else {
    const size_t lds = (256 * 64 + 3 * PS * PS) * sizeof(float);
    SL_TRY(sl_launch("stem3_wgrad_kernel", stem3_wgrad_kernel, dim3(nblk), dim3(256), lds, st, img_nchw, (const float*)dc1, (float*)workspace, B, H, W, tpb, ntiles));
  }
  return sl_colsum_finalize((const float*)workspace, nblk, 64 * NTAP, dw_oihw, stream);       // fixed-order sum of the block partials
}
