// BatchNorm2d (train + eval) forward/backward around the conv kernels; all HBM-bound, 16-byte vectorised NHWC.
// Reference call sites: networks/backbones/resnet.py:45,48,50,88,111 and networks/pspnet_pop.py:20,28.
#include "common.h"

namespace {

// ------------------------------------------------------------------------------------------------ finalize
// Column sums of the [rows][2][C] partial buffers: a block owns 64 channels, 16 row-lanes stride over the rows (8 loads in
// flight each), then a fixed-order 16-way LDS tree -- bit-stable, and ~100x less latency than one serial thread per channel.
template <int FIN_CH, int FIN_RL>
__device__ __forceinline__ void colsum2(const float* __restrict__ part, int rows, int C, int c, int rl, double& s, double& q,
                                        double (*red)[FIN_RL][FIN_CH]) {
  double a0 = 0.0, a1 = 0.0;
  if (c < C) {
    int r = rl;
    for (; r + 7 * FIN_RL < rows; r += 8 * FIN_RL) {
      float v0[8], v1[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        v0[u] = part[((size_t)(r + u * FIN_RL) * 2 + 0) * C + c];
        v1[u] = part[((size_t)(r + u * FIN_RL) * 2 + 1) * C + c];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) { a0 += (double)v0[u]; a1 += (double)v1[u]; }
    }
    for (; r < rows; r += FIN_RL) { a0 += (double)part[((size_t)r * 2 + 0) * C + c]; a1 += (double)part[((size_t)r * 2 + 1) * C + c]; }
  }
  const int cl = threadIdx.x % FIN_CH;
  red[0][rl][cl] = a0; red[1][rl][cl] = a1;
  __syncthreads();
  s = 0.0; q = 0.0;
  if (rl == 0) {
#pragma unroll
    for (int j = 0; j < FIN_RL; ++j) { s += red[0][j][cl]; q += red[1][j][cl]; }
  }
}

template <int FIN_CH, int FIN_RL>
__global__ __launch_bounds__(FIN_CH * FIN_RL) void bn_finalize_train_kernel(const float* __restrict__ part, int rows, int C, double count,
                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                         float* rmean, float* rvar, float momentum, float eps,
                                         float* mean, float* invstd, float* scale, float* shift, const float* __restrict__ cbias, int nbias) {
  __shared__ double red[2][FIN_RL][FIN_CH];
  const int c = blockIdx.x * FIN_CH + threadIdx.x % FIN_CH, rl = threadIdx.x / FIN_CH;
  double s, q;
  colsum2<FIN_CH, FIN_RL>(part, rows, C, c, rl, s, q, red);
  if (rl != 0 || c >= C) return;
  const double mu = s / count;
  double var = q / count - mu * mu;
  if (var < 0.0) var = 0.0;
  const double is = 1.0 / sqrt(var + (double)eps);
  mean[c] = (float)mu;
  invstd[c] = (float)is;
  const double g = gamma ? (double)gamma[c] : 1.0, b = beta ? (double)beta[c] : 0.0;
  scale[c] = (float)(g * is);
  shift[c] = (float)(b - mu * g * is);
  if (rmean) {
    const double unbiased = count > 1.0 ? var * count / (count - 1.0) : var;
    // cbias: the statistics are those of the RAW conv output; the conv's bias shifts the mean only (it cancels in the normalised output) and enters the running mean here
    const double mb = (cbias && c < nbias) ? mu + (double)cbias[c] : mu;
    rmean[c] = (float)((1.0 - momentum) * (double)rmean[c] + momentum * mb);
    rvar[c] = (float)((1.0 - momentum) * (double)rvar[c] + momentum * unbiased);
  }
}

__global__ void bn_finalize_eval_kernel(int C, const float* gamma, const float* beta, const float* rmean, const float* rvar,
                                        float eps, float* mean, float* invstd, float* scale, float* shift) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const double is = 1.0 / sqrt((double)rvar[c] + (double)eps);
  const double g = gamma ? (double)gamma[c] : 1.0, b = beta ? (double)beta[c] : 0.0;
  if (mean) mean[c] = rmean[c];
  if (invstd) invstd[c] = (float)is;
  scale[c] = (float)(g * is);
  shift[c] = (float)(b - (double)rmean[c] * g * is);
}

// ------------------------------------------------------------------------------------------------ forward apply
// FIXEDC: 256 % (C/V) == 0, so a thread's channel vector never changes along its grid-stride walk and the per-channel
// coefficients live in registers; the loop is then a pure 16-byte stream (4 independent loads in flight per operand).
template <typename T, bool FIXEDC>
__global__ __launch_bounds__(256) void bn_act_fwd_kernel(const T* __restrict__ x, const float* __restrict__ scale, const float* __restrict__ shift,
                                  const T* __restrict__ res, int relu, T* __restrict__ y, uint8_t* __restrict__ mask_out, unsigned nvec, unsigned nvc) {
  constexpr int V = Vec16<T>::N;
  float sc[V], sh[V];
  if (FIXEDC) {
    const unsigned c = (threadIdx.x % nvc) * V;
#pragma unroll
    for (int k = 0; k < V; ++k) { sc[k] = scale[c + k]; sh[k] = shift[c + k]; }
  }
  // a block-iteration owns 1024 consecutive vectors (16 KiB per operand).  Walking the tensor from its end (the bytes the producing conv
  // wrote last) was measured for all three BN passes: no difference, the Infinity Cache does not retain these streams
  const unsigned nchunk = (nvec + 1023u) >> 10;
  for (unsigned ch = blockIdx.x; ch < nchunk; ch += gridDim.x) {
    const unsigned i0 = (ch << 10) + threadIdx.x;
    uint4 xv[4], rv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const unsigned i = i0 + u * 256u;
      if (i < nvec) { xv[u] = ((const uint4*)x)[i]; if (res) rv[u] = ((const uint4*)res)[i]; }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const unsigned i = i0 + u * 256u;
      if (i >= nvec) break;
      if (!FIXEDC) {
        const unsigned c = (i % nvc) * V;
#pragma unroll
        for (int k = 0; k < V; ++k) { sc[k] = scale[c + k]; sh[k] = shift[c + k]; }
      }
      float a[V], r[V], o[V];
      unpack16<T>(xv[u], a);
      if (res) unpack16<T>(rv[u], r);
      unsigned bits = 0;
#pragma unroll
      for (int k = 0; k < V; ++k) {
        float v = a[k] * sc[k] + sh[k];
        if (res) v += r[k];
        if (relu) v = v > 0.f ? v : 0.f;
        bits |= (v > 0.f ? 1u : 0u) << k;
        o[k] = v;
      }
      ((uint4*)y)[i] = pack16<T>(o);
      if (mask_out) mask_out[i] = (uint8_t)bits;       // 1 byte per 16-byte vector: bit k = (y_k > 0)
    }
  }
}

// Stage entry of a bottleneck (resnet.py:71-76): y = act(bn3(c3) + bnd(c_ds)) in ONE pass -- the normalised shortcut is never written.  The same stream as
// bn_act_fwd_kernel with two coefficient pairs; bit-identical to bn_act_fwd(x2, relu = 0) followed by bn_act_fwd(x, residual = that): the shortcut value is
// rounded to T (pack16 / unpack16: what the round trip through memory did) before it is added.
template <typename T, bool FIXEDC>
__global__ __launch_bounds__(256) void bn_act2_fwd_kernel(const T* __restrict__ x, const float* __restrict__ scale, const float* __restrict__ shift,
                                   const T* __restrict__ x2, const float* __restrict__ scale2, const float* __restrict__ shift2,
                                   int relu, T* __restrict__ y, uint8_t* __restrict__ mask_out, unsigned nvec, unsigned nvc) {
  constexpr int V = Vec16<T>::N;
  float sc[V], sh[V], sc2[V], sh2[V];
  if (FIXEDC) {
    const unsigned c = (threadIdx.x % nvc) * V;
#pragma unroll
    for (int k = 0; k < V; ++k) { sc[k] = scale[c + k]; sh[k] = shift[c + k]; sc2[k] = scale2[c + k]; sh2[k] = shift2[c + k]; }
  }
  const unsigned nchunk = (nvec + 1023u) >> 10;
  for (unsigned ch = blockIdx.x; ch < nchunk; ch += gridDim.x) {
    const unsigned i0 = (ch << 10) + threadIdx.x;
    uint4 xv[4], dv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const unsigned i = i0 + u * 256u;
      if (i < nvec) { xv[u] = ((const uint4*)x)[i]; dv[u] = ((const uint4*)x2)[i]; }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const unsigned i = i0 + u * 256u;
      if (i >= nvec) break;
      if (!FIXEDC) {
        const unsigned c = (i % nvc) * V;
#pragma unroll
        for (int k = 0; k < V; ++k) { sc[k] = scale[c + k]; sh[k] = shift[c + k]; sc2[k] = scale2[c + k]; sh2[k] = shift2[c + k]; }
      }
      float a[V], d[V], r[V], o[V];
      unpack16<T>(xv[u], a);
      unpack16<T>(dv[u], d);
#pragma unroll
      for (int k = 0; k < V; ++k) d[k] = d[k] * sc2[k] + sh2[k];
      unpack16<T>(pack16<T>(d), r);                     // the shortcut as the tensor type holds it
      unsigned bits = 0;
#pragma unroll
      for (int k = 0; k < V; ++k) {
        float v = a[k] * sc[k] + sh[k];
        v += r[k];
        if (relu) v = v > 0.f ? v : 0.f;
        bits |= (v > 0.f ? 1u : 0u) << k;
        o[k] = v;
      }
      ((uint4*)y)[i] = pack16<T>(o);
      if (mask_out) mask_out[i] = (uint8_t)bits;
    }
  }
}

// ------------------------------------------------------------------------------------------------ backward reduce
// partial[blk][0][c] = sum g, partial[blk][1][c] = sum g * (x - mean) * invstd over the block's rows
// DUAL: a second BatchNorm whose output was added to the first one's before the same ReLU (bn3 + downsample BN of a bottleneck, resnet.py:71-76): both backward
// passes gate the SAME gradient, so one sweep over dy and the bits serves both (x2, mean2, invstd2 -> part2)
template <typename T, bool DUAL = false>
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const T* __restrict__ dy, const T* __restrict__ y, const uint8_t* __restrict__ mask, const T* __restrict__ x,
                                                            const float* __restrict__ mean, const float* __restrict__ invstd,
                                                            float* __restrict__ part, long long rows, int C,
                                                            const T* __restrict__ x2 = nullptr, const float* __restrict__ mean2 = nullptr, const float* __restrict__ invstd2 = nullptr,
                                                            float* __restrict__ part2 = nullptr) {
  constexpr int V = Vec16<T>::N;
  __shared__ float red[(DUAL ? 3 : 2) * 256 * V];
  const unsigned lb = blockIdx.x;
  const int nvec = C / V;
  const int tpr = nvec < 256 ? nvec : 256;      // threads per row
  const int rpb = 256 / tpr;                    // rows handled in parallel
  const int tr = threadIdx.x / tpr, tc = threadIdx.x % tpr;
  // block b owns the row groups b, b + nblk, b + 2 nblk, ...: the chip reads ONE moving window of the tensor, like the streaming passes
  // (measured 4.2 vs 4.0 TB/s for a contiguous row range per block; 2 or 4 rows in flight per thread were SLOWER: 3.9 / 3.2 TB/s)
  const long long r_begin = (long long)lb * rpb, r_end = rows, rstep = (long long)gridDim.x * rpb;
  constexpr int NS = DUAL ? 3 : 2;
  for (int vc = tc; vc < nvec; vc += tpr) {
    float s1[V], s2[V], s3[V], mu[V], is[V], mu2[V], is2[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
      s1[k] = 0.f; s2[k] = 0.f; s3[k] = 0.f; mu[k] = mean[vc * V + k]; is[k] = invstd[vc * V + k];
      if (DUAL) { mu2[k] = mean2[vc * V + k]; is2[k] = invstd2[vc * V + k]; }
    }
    if (tr < rpb) {
      auto acc = [&](const uint4& gq, const uint4& xq, const uint4& yq, unsigned mb, const uint4& x2q) {
        float g[V], xv[V], yv[V];
        unpack16<T>(gq, g);
        unpack16<T>(xq, xv);
        if (mask) {
#pragma unroll
          for (int k = 0; k < V; ++k) g[k] = (mb >> k) & 1u ? g[k] : 0.f;
        } else if (y) {
          unpack16<T>(yq, yv);
#pragma unroll
          for (int k = 0; k < V; ++k) g[k] = yv[k] > 0.f ? g[k] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < V; ++k) { s1[k] += g[k]; s2[k] += g[k] * ((xv[k] - mu[k]) * is[k]); }
        if (DUAL) {
          float x2v[V];
          unpack16<T>(x2q, x2v);
#pragma unroll
          for (int k = 0; k < V; ++k) s3[k] += g[k] * ((x2v[k] - mu2[k]) * is2[k]);
        }
      };
      long long r = r_begin + tr;
      for (; r < r_end; r += rstep) {
        const size_t o = (size_t)r * nvec + vc;
        uint4 yq = make_uint4(0, 0, 0, 0), x2q = make_uint4(0, 0, 0, 0);
        if (!mask && y) yq = ((const uint4*)y)[o];
        if (DUAL) x2q = ((const uint4*)x2)[o];
        acc(((const uint4*)dy)[o], ((const uint4*)x)[o], yq, mask ? mask[o] : 0u, x2q);
      }
    }
    // reduce over the rpb row-lanes that share this channel vector
    __syncthreads();
#pragma unroll
    for (int k = 0; k < V; ++k) {
      red[(threadIdx.x * V + k) * NS + 0] = s1[k]; red[(threadIdx.x * V + k) * NS + 1] = s2[k];
      if (DUAL) red[(threadIdx.x * V + k) * NS + 2] = s3[k];
    }
    __syncthreads();
    if (tr == 0) {
#pragma unroll
      for (int k = 0; k < V; ++k) {
        float a = 0.f, b = 0.f, c3 = 0.f;
        for (int j = 0; j < rpb; ++j) {
          a += red[((j * tpr + tc) * V + k) * NS + 0]; b += red[((j * tpr + tc) * V + k) * NS + 1];
          if (DUAL) c3 += red[((j * tpr + tc) * V + k) * NS + 2];
        }
        part[((size_t)lb * 2 + 0) * C + vc * V + k] = a;
        part[((size_t)lb * 2 + 1) * C + vc * V + k] = b;
        if (DUAL) { part2[((size_t)lb * 2 + 0) * C + vc * V + k] = a; part2[((size_t)lb * 2 + 1) * C + vc * V + k] = c3; }
      }
    }
  }
}

template <int FIN_CH, int FIN_RL>
__global__ __launch_bounds__(FIN_CH * FIN_RL) void bn_bwd_finalize_kernel(const float* __restrict__ part, int nblk, int C, double count, const float* gamma,
                                       const float* mean, const float* invstd, int train, float* dgamma, float* dbeta,
                                       float* cA, float* cB, float* cC) {
  __shared__ double red[2][FIN_RL][FIN_CH];
  const int c = blockIdx.x * FIN_CH + threadIdx.x % FIN_CH, rl = threadIdx.x / FIN_CH;
  double s1, s2;
  colsum2<FIN_CH, FIN_RL>(part, nblk, C, c, rl, s1, s2, red);
  if (rl != 0 || c >= C) return;
  if (dgamma) dgamma[c] = (float)s2;
  if (dbeta) dbeta[c] = (float)s1;
  const double g = gamma ? (double)gamma[c] : 1.0, is = (double)invstd[c];
  cA[c] = (float)(g * is);
  if (train) {     // dx = g*is*(dy - S1/M - xhat*S2/M) = cA*dy + cB*(x-mean) + cC
    cB[c] = (float)(-g * is * is * s2 / count);
    cC[c] = (float)(-g * is * s1 / count);
  } else {
    cB[c] = 0.f; cC[c] = 0.f;
  }
}

template <typename T, bool FIXEDC, bool DUAL = false>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const T* __restrict__ dy, const T* __restrict__ y, const uint8_t* __restrict__ mask, const T* __restrict__ x,
                                    const float* __restrict__ cA, const float* __restrict__ cB, const float* __restrict__ cC,
                                    const float* __restrict__ mean, T* __restrict__ dx, T* __restrict__ dres, unsigned nvec, unsigned nvc,
                                    const T* __restrict__ x2 = nullptr, const float* __restrict__ cA2 = nullptr, const float* __restrict__ cB2 = nullptr,
                                    const float* __restrict__ cC2 = nullptr, const float* __restrict__ mean2 = nullptr, T* __restrict__ dx2 = nullptr) {
  constexpr int V = Vec16<T>::N;
  float a_[V], b_[V], c_[V], cc[V];      // dx = a*g + b*(x - c) + cc
  float a2[V], b2[V], c2[V], cc2[V];     // DUAL: the second BatchNorm fed by the same gated gradient
  auto coeffs = [&](unsigned c) {
#pragma unroll
    for (int k = 0; k < V; ++k) {
      a_[k] = cA[c + k]; b_[k] = cB[c + k]; c_[k] = mean[c + k]; cc[k] = cC[c + k];
      if (DUAL) { a2[k] = cA2[c + k]; b2[k] = cB2[c + k]; c2[k] = mean2[c + k]; cc2[k] = cC2[c + k]; }
    }
  };
  if (FIXEDC) coeffs((threadIdx.x % nvc) * V);
  const unsigned nchunk = (nvec + 511u) >> 9;          // 512 consecutive vectors per block-iteration
  for (unsigned ch = blockIdx.x; ch < nchunk; ch += gridDim.x) {
    const unsigned i0 = (ch << 9) + threadIdx.x;
    uint4 gv[2], xv[2], yv[2], x2v[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const unsigned i = i0 + u * 256u;
      if (i < nvec) {
        gv[u] = ((const uint4*)dy)[i]; xv[u] = ((const uint4*)x)[i];
        if (y && !mask) yv[u] = ((const uint4*)y)[i];
        if (DUAL) x2v[u] = ((const uint4*)x2)[i];
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const unsigned i = i0 + u * 256u;
      if (i >= nvec) break;
      if (!FIXEDC) coeffs((i % nvc) * V);
      float g[V], xx[V], yy[V], o[V];
      unpack16<T>(gv[u], g);
      unpack16<T>(xv[u], xx);
      if (mask) {
        const unsigned b = mask[i];
#pragma unroll
        for (int k = 0; k < V; ++k) g[k] = (b >> k) & 1u ? g[k] : 0.f;
      } else if (y) {
        unpack16<T>(yv[u], yy);
#pragma unroll
        for (int k = 0; k < V; ++k) g[k] = yy[k] > 0.f ? g[k] : 0.f;
      }
#pragma unroll
      for (int k = 0; k < V; ++k) o[k] = a_[k] * g[k] + b_[k] * (xx[k] - c_[k]) + cc[k];
      ((uint4*)dx)[i] = pack16<T>(o);
      if (dres) ((uint4*)dres)[i] = pack16<T>(g);
      if (DUAL) {
        float x2x[V];
        unpack16<T>(x2v[u], x2x);
#pragma unroll
        for (int k = 0; k < V; ++k) o[k] = a2[k] * g[k] + b2[k] * (x2x[k] - c2[k]) + cc2[k];
        ((uint4*)dx2)[i] = pack16<T>(o);
      }
    }
  }
}

// Block shape of the two finalize kernels: 32 channels x 32 row lanes (measured against 64 x 16 and 16 x 64 in round 2: -0.26 ms per ResNet-50 step).  Round 4 tried 1024 threads
// per 32 channels with 16-byte loads, every load of a thread in flight at once and a shuffle + 16-wave LDS reduction: 7.7 / 7.2 us per launch against 5.9 / 6.0 for this form
// (gpurun r4c: rocprofv3 --stats of bench.py) -- removed.

inline int ew_blocks(long long nvec) { long long b = (nvec + 255) / 256; return (int)(b < 1 ? 1 : (b > 16384 ? 16384 : b)); }
inline int reduce_blocks(long long rows) { long long b = (rows + 63) / 64; return (int)(b < 1 ? 1 : (b > 1024 ? 1024 : b)); }

}  // namespace

extern "C" int sl_bn_finalize_train(const float* stat_partial, int stat_rows, int C, long long count, const float* gamma,
                                    const float* beta, float* running_mean, float* running_var, float momentum, float eps,
                                    float* mean, float* invstd, float* scale, float* shift, sl_stream_t stream) {
  SL_REQUIRE(stat_partial && mean && invstd && scale && shift && C > 0 && stat_rows > 0 && count > 0, "bn_finalize_train: bad args");
  SL_REQUIRE((running_mean == nullptr) == (running_var == nullptr), "bn_finalize_train: running stats must come in pairs");
  return sl_launch("bn_finalize_train_kernel", bn_finalize_train_kernel<32, 32>, dim3(cdiv(C, 32)), dim3(1024), 0, (hipStream_t)stream, stat_partial, stat_rows, C, (double)count, gamma, beta,
                   running_mean, running_var, momentum, eps, mean, invstd, scale, shift, (const float*)nullptr, 0);
}

extern "C" int sl_bn_finalize_train_bias(const float* stat_partial, int stat_rows, int C, long long count, const float* gamma,
                                         const float* beta, float* running_mean, float* running_var, float momentum, float eps,
                                         float* mean, float* invstd, float* scale, float* shift, const float* conv_bias, int bias_n, sl_stream_t stream) {
  SL_REQUIRE(stat_partial && mean && invstd && scale && shift && C > 0 && stat_rows > 0 && count > 0, "bn_finalize_train_bias: bad args");
  SL_REQUIRE(running_mean && running_var && conv_bias && bias_n > 0 && bias_n <= C, "bn_finalize_train_bias: running stats and bias_n in 1..C conv bias entries are required");
  return sl_launch("bn_finalize_train_kernel", bn_finalize_train_kernel<32, 32>, dim3(cdiv(C, 32)), dim3(1024), 0, (hipStream_t)stream, stat_partial, stat_rows, C, (double)count, gamma, beta,
                   running_mean, running_var, momentum, eps, mean, invstd, scale, shift, conv_bias, bias_n);
}

extern "C" int sl_bn_finalize_eval(int C, const float* gamma, const float* beta, const float* running_mean,
                                   const float* running_var, float eps, float* mean, float* invstd, float* scale,
                                   float* shift, sl_stream_t stream) {
  SL_REQUIRE(running_mean && running_var && scale && shift && C > 0, "bn_finalize_eval: bad args");
  return sl_launch("bn_finalize_eval_kernel", bn_finalize_eval_kernel, dim3(cdiv(C, 64)), dim3(64), 0, (hipStream_t)stream, C, gamma, beta, running_mean,
                   running_var, eps, mean, invstd, scale, shift);
}

// the element-wise passes: C / V channel vectors per row; a block's threads keep their channels when 256 is a multiple of that (FIXEDC)
static bool fixed_channels(unsigned nvc) { return nvc <= 256 && 256 % nvc == 0; }

extern "C" int sl_bn_act_fwd(int dtype, const void* x, const float* scale, const float* shift, const void* residual,
                             int relu, void* y, uint8_t* relu_mask, long long rows, int C, sl_stream_t stream) {
  SL_REQUIRE(x && scale && shift && y && rows > 0 && C > 0 && C % 8 == 0, "bn_act_fwd: bad args");
  return sl_by_dtype(dtype, "bn_act_fwd", [&](auto t) -> int {
    using T = decltype(t);
    const long long nvec = rows * C / Vec16<T>::N;
    SL_REQUIRE(nvec < (1ll << 31), "bn_act_fwd: tensor too large");
    const unsigned nvc = C / Vec16<T>::N;
    return sl_launch("bn_act_fwd_kernel", fixed_channels(nvc) ? bn_act_fwd_kernel<T, true> : bn_act_fwd_kernel<T, false>, dim3(ew_blocks((nvec + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                     (const T*)x, scale, shift, (const T*)residual, relu, (T*)y, relu_mask, (unsigned)nvec, nvc);
  });
}

extern "C" int sl_bn_act2_fwd(int dtype, const void* x, const float* scale, const float* shift, const void* x2, const float* scale2, const float* shift2,
                              int relu, void* y, uint8_t* relu_mask, long long rows, int C, sl_stream_t stream) {
  SL_REQUIRE(x && scale && shift && x2 && scale2 && shift2 && y && rows > 0 && C > 0 && C % 8 == 0, "bn_act2_fwd: bad args");
  return sl_by_dtype(dtype, "bn_act2_fwd", [&](auto t) -> int {
    using T = decltype(t);
    const long long nvec = rows * C / Vec16<T>::N;
    SL_REQUIRE(nvec < (1ll << 31), "bn_act2_fwd: tensor too large");
    const unsigned nvc = C / Vec16<T>::N;
    return sl_launch("bn_act2_fwd_kernel", fixed_channels(nvc) ? bn_act2_fwd_kernel<T, true> : bn_act2_fwd_kernel<T, false>, dim3(ew_blocks((nvec + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                     (const T*)x, scale, shift, (const T*)x2, scale2, shift2, relu, (T*)y, relu_mask, (unsigned)nvec, nvc);
  });
}

extern "C" int sl_bn_bwd_reduce_rows(long long rows, int C) { (void)C; return reduce_blocks(rows); }

extern "C" int sl_bn_bwd_reduce(int dtype, const void* dy, const void* y, const uint8_t* relu_mask, const void* x, const float* mean,
                                const float* invstd, float* partial, long long rows, int C, sl_stream_t stream) {
  SL_REQUIRE(dy && x && mean && invstd && partial && rows > 0 && C > 0 && C % 8 == 0, "bn_bwd_reduce: bad args");
  return sl_by_dtype(dtype, "bn_bwd_reduce", [&](auto t) -> int {
    using T = decltype(t);
    return sl_launch("bn_bwd_reduce_kernel", bn_bwd_reduce_kernel<T>, dim3(reduce_blocks(rows)), dim3(256), 0, (hipStream_t)stream, (const T*)dy, (const T*)y, relu_mask, (const T*)x, mean, invstd,
                     partial, rows, C, nullptr, nullptr, nullptr, nullptr);
  });
}

extern "C" int sl_bn_bwd_finalize(const float* partial, int nblk, int C, long long count, const float* gamma,
                                  const float* mean, const float* invstd, int train, float* dgamma, float* dbeta,
                                  float* cA, float* cB, float* cC, sl_stream_t stream) {
  SL_REQUIRE(partial && invstd && cA && cB && cC && nblk > 0 && C > 0 && count > 0, "bn_bwd_finalize: bad args");
  return sl_launch("bn_bwd_finalize_kernel", bn_bwd_finalize_kernel<32, 32>, dim3(cdiv(C, 32)), dim3(1024), 0, (hipStream_t)stream, partial, nblk, C, (double)count, gamma, mean, invstd, train,
                   dgamma, dbeta, cA, cB, cC);
}

extern "C" int sl_bn_bwd_apply(int dtype, const void* dy, const void* y, const uint8_t* relu_mask, const void* x, const float* cA, const float* cB,
                               const float* cC, const float* mean, void* dx, void* dres, long long rows, int C,
                               sl_stream_t stream) {
  SL_REQUIRE(dy && x && cA && cB && cC && mean && dx && rows > 0 && C > 0 && C % 8 == 0, "bn_bwd_apply: bad args");
  return sl_by_dtype(dtype, "bn_bwd_apply", [&](auto t) -> int {
    using T = decltype(t);
    const long long nvec = rows * C / Vec16<T>::N;
    SL_REQUIRE(nvec < (1ll << 31), "bn_bwd_apply: tensor too large");
    const unsigned nvc = C / Vec16<T>::N;
    return sl_launch("bn_bwd_apply_kernel", fixed_channels(nvc) ? bn_bwd_apply_kernel<T, true> : bn_bwd_apply_kernel<T, false>, dim3(ew_blocks((nvec + 1) / 2)), dim3(256), 0, (hipStream_t)stream,
                     (const T*)dy, (const T*)y, relu_mask, (const T*)x, cA, cB, cC, mean, (T*)dx, (T*)dres, (unsigned)nvec, nvc, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  });
}

// Two BatchNorms behind one ReLU (bn3 + the downsample BN of the first bottleneck of a stage): ONE sweep over dy and the ReLU bits for both reduces / both applies.
extern "C" int sl_bn_bwd_reduce2(int dtype, const void* dy, const uint8_t* relu_mask, const void* x1, const float* mean1, const float* invstd1, float* partial1,
                                 const void* x2, const float* mean2, const float* invstd2, float* partial2, long long rows, int C, sl_stream_t stream) {
  SL_REQUIRE(dy && x1 && x2 && mean1 && invstd1 && mean2 && invstd2 && partial1 && partial2 && rows > 0 && C > 0 && C % 8 == 0, "bn_bwd_reduce2: bad args");
  return sl_by_dtype(dtype, "bn_bwd_reduce2", [&](auto t) -> int {
    using T = decltype(t);
    return sl_launch("bn_bwd_reduce_kernel", bn_bwd_reduce_kernel<T, true>, dim3(reduce_blocks(rows)), dim3(256), 0, (hipStream_t)stream, (const T*)dy, nullptr, relu_mask, (const T*)x1, mean1, invstd1,
                     partial1, rows, C, (const T*)x2, mean2, invstd2, partial2);
  });
}

extern "C" int sl_bn_bwd_apply2(int dtype, const void* dy, const uint8_t* relu_mask, const void* x1, const float* cA1, const float* cB1, const float* cC1,
                                const float* mean1, void* dx1, const void* x2, const float* cA2, const float* cB2, const float* cC2, const float* mean2, void* dx2,
                                long long rows, int C, sl_stream_t stream) {
  SL_REQUIRE(dy && x1 && x2 && cA1 && cB1 && cC1 && mean1 && dx1 && cA2 && cB2 && cC2 && mean2 && dx2 && rows > 0 && C > 0 && C % 8 == 0, "bn_bwd_apply2: bad args");
  return sl_by_dtype(dtype, "bn_bwd_apply2", [&](auto t) -> int {
    using T = decltype(t);
    const long long nvec = rows * C / Vec16<T>::N;
    SL_REQUIRE(nvec < (1ll << 31), "bn_bwd_apply2: tensor too large");
    const unsigned nvc = C / Vec16<T>::N;
    return sl_launch("bn_bwd_apply_kernel", fixed_channels(nvc) ? bn_bwd_apply_kernel<T, true, true> : bn_bwd_apply_kernel<T, false, true>, dim3(ew_blocks((nvec + 1) / 2)), dim3(256), 0, (hipStream_t)stream,
                     (const T*)dy, nullptr, relu_mask, (const T*)x1, cA1, cB1, cC1, mean1, (T*)dx1, nullptr, (unsigned)nvec, nvc, (const T*)x2, cA2, cB2, cC2, mean2, (T*)dx2);
  });
}
