// Fused bilinear upsample (align_corners=True) + cross-entropy (loss/criterion.py:51-52), the ft pseudo-label step
// (networks/pspnet_pop.py:221-231), upsample+argmax (eval_base.py:168-169), IoU histogram (utils/pyt_utils.py:293-305)
// and masked average pooling (networks/pspnet.py:7-15).  The H x W logits are never materialised.
#include "common.h"

namespace {

constexpr int KMAXC = 33;  // max logit channels (background + 32 prototypes) of sl_upsample_ce_* / sl_pseudo_label / sl_upsample_argmax / sl_upsample_logits / sl_tta_fuse / sl_slide_fuse: the ONE limit of this file
constexpr int KNC = 16;    // up to KNC channels run on the <KNC> instantiations and the one-pass tiled backward (device code as before the wide head); more on <KMAXC> and the
                           // channel-sliced tiled backward.  KW below is the per-thread array width of an instantiation.

struct UpGeom { int B, K, h, w, H, W; float sy, sx; };

// Class weights and label smoothing of the weighted forms (nn.CrossEntropyLoss(weight, label_smoothing); loss/criterion.py:33,51-52).  For a valid pixel of label t
//   c_k = (1 - eps) w_t [k == t] + (eps / K) w_k,   numerator = -sum_k c_k logp_k,   denominator = w_t,
//   d numerator / d v_k = softmax_k C_t - c_k   with   C_t = (1 - eps) w_t + (eps / K) sum_j w_j   (sum_j in index order, inside the kernel).
// The plain kernels are the <WT = false> instantiations: CeW<false> is empty and every statement of the weighted form sits under `if constexpr (WT)`.
template <bool WT> struct CeW {};
template <> struct CeW<true> { const float* w; float keep, epsk; };   // w[K] on the device, keep = 1 - eps, epsk = eps / K

// The hybrid form (cross-entropy + multiclass soft Dice with softmax, the MulticlassHybridLoss swap of loss/criterion.py:34) of the backward kernels: <DC = true>.
// Over the valid pixels of sample b:  I_c = sum p_c [t == c],  P_c = sum p_c,  T_c = sum [t == c],  dice = mean_b sum_c w_c (1 - N_c / D_c),  N = 2 I + smooth,
// D = P + T + smooth.  With the table coef[b][c] = (a, g) = (-2 w_c / (B D), w_c N / (B D^2)) of the finalize kernel and q_c = g_c + a_c [c == t]
//   d dice / d v_k = p_k (q_k - sum_c p_c q_c),
// added to the pixel's cross-entropy gradient BEFORE the bilinear scatter: per-pixel gradient = f0 * (cross-entropy form) + f1 * (Dice form), f0 = gscale[0] / denominator,
// f1 = gscale[1].  CeD<false> is empty and every statement of the hybrid form sits under `if constexpr (DC)`: the <DC = false> instantiations are the kernels as they were.
// In the hybrid kernels, and in the focal ones (FC below), the class-weight pointer may be null (weights of one): cew_at, whose first argument says so.
template <bool DC> struct CeD {};
template <> struct CeD<true> { const float* coef; };                  // [B][K][2] on the device
template <bool NULLOK, bool WT>
__device__ __forceinline__ float cew_at(const CeW<WT>& cw, int k) {
  if constexpr (!WT) return 1.f;
  else if constexpr (NULLOK) return cw.w ? cw.w[k] : 1.f;
  else return cw.w[k];
}
__device__ __forceinline__ float dice_q(int k, int t, float qa, float qg) { return qg + (k == t ? qa : 0.f); }   // q_k = g_k + a_k [k == t]

// Focal modulation (Lin et al.) of the cross-entropy term, <FC = true>; the contract is in include/segland_hip.h.  With e_k = exp(v_k - m), s = sum_k e_k (index order),
//   u = (sum_{k != t} e_k) / s   (index order, skipping t: 1 - p_t without the cancellation of 1 - e_t / s; exactly 0 when every other exponential underflows),
//   mod = u^gamma,   pixel numerator = mod * num0   (num0, den: the cross-entropy numerator and denominator of ce_pixel; den is unchanged),
//   d numerator / d v_k = mod * (cross-entropy form)_k + beta * (p_k - [k == t]),   beta = gamma * num0 * (mod / u) * p_t,   mod = beta = 0 where u == 0.
// The kernels evaluate mod / u = u^(gamma - 1) = exp2f((gamma - 1) * log2f(u)) once (gamma >= 1: at most 1, and exactly 1 for gamma == 1) and mod = u * (mod / u):
// one logarithm and one exponential of the hardware's base, no division by u.  The gfx950 exp2f / log2f are good to ~1 ulp; the power's relative error is that of the
// exponent, |(gamma - 1) log2 u| * 2^-24 * ln 2, and a pixel whose exponent is large (u tiny) enters the sums with a weight that small.  powf costs a polynomial
// with extended-precision bookkeeping per pixel for digits the 2e-5 / 1e-3 bounds of these kernels never see.
// CeF<false> is empty and every statement of the focal form sits under `if constexpr (FC)`: the <FC = false> instantiations are the kernels as they were (the same
// instructions; their symbols carry one template argument more).
template <bool FC> struct CeF {};
template <> struct CeF<true> { float gamma; };
__device__ __forceinline__ float focal_modu(float u, float gamma) { return u > 0.f ? exp2f((gamma - 1.f) * log2f(u)) : 0.f; }

// Lovasz-softmax term (Berman et al.) of the backward kernels, <LV = true>; the contract is in include/segland_hip.h.  The forward (upsample_lovasz_hist_kernel,
// lovasz_scan_kernel below) quantises every class's errors e_c = |[t == c] - p_c| to LOV_NB bins and leaves the table tab[c][bin] = dJ_c[bin] / (count of the bin *
// present classes); for a valid pixel q_c = ([t == c] ? -1 : +1) * tab[c][bin(e_c)], a constant for the gradient, and
//   d lovasz / d v_k = p_k (q_k - sum_c p_c q_c),
// the Dice term's form, added to the pixel's gradient BEFORE the bilinear scatter with the scale f2 = gscale[2].  The label's own error is u = (sum_{k != t} e_k) / s, the
// focal form's cancellation-free 1 - p_t.  The table is read from global memory (K * LOV_NB floats, L2-resident): no LDS buffer.
// CeL<false> is empty and every statement of the term sits under `if constexpr (LV)`: the <LV = false> instantiations are the kernels as they were.
constexpr int LOV_NB = 1024;
template <bool LV> struct CeL {};
template <> struct CeL<true> { const float* tab; };                   // [K][LOV_NB] on the device
__device__ __forceinline__ int lov_bin(float e) { const int j = (int)(e * (float)LOV_NB); return j < 0 ? 0 : (j < LOV_NB - 1 ? j : LOV_NB - 1); }
__device__ __forceinline__ float lov_q(const float* __restrict__ tab, int k, int t, float p, float u) {
  return k == t ? -tab[k * LOV_NB + lov_bin(u)] : tab[k * LOV_NB + lov_bin(p)];
}

// The gradient of one valid pixel of label t with respect to its interpolated logits, in the three forms above: built once per pixel, at(k) once per channel.  wt = w_t,
// wsum = sum_j w_j, p = softmax_k, w = w_k, (qa, qg) = coef[b][k], sq = sum_c p_c q_c.  <false, false> is p - [k == t] and nothing else; without DC the caller applies
// the scale gscale[0] / denominator after the bilinear scatter, with DC f0 and f1 are inside.  A new loss term goes here and into ce_pixel, nowhere else.
// FC: (mod, beta) of the pixel from ce_pixel; the cross-entropy form becomes mod * form + beta * (p - [k == t]), before f0 as before the scatter.
// LV: f2 = gscale[2], sl = sum_c p_c q_c of the Lovasz q, lq = q_k; the scales are inside as with DC (f0 too, with or without DC).
template <bool LV> struct PixLov {};
template <> struct PixLov<true> { float f2, sl; };
template <bool WT, bool DC, bool FC = false, bool LV = false>
struct PixGrad : PixLov<LV> {
  int t; float hit, ct, epsk, f0, f1, sq, mod, beta;
  __device__ __forceinline__ PixGrad(int t_, float wt, const CeW<WT>& cw, float wsum, float f0_, float f1_, float sq_, float mod_ = 1.f, float beta_ = 0.f)
      : t(t_), hit(1.f), ct(1.f), epsk(0.f), f0(f0_), f1(f1_), sq(sq_), mod(mod_), beta(beta_) {
    if constexpr (WT) { hit = cw.keep * wt; ct = hit + cw.epsk * wsum; epsk = cw.epsk; }
  }
  __device__ __forceinline__ PixGrad(int t_, float wt, const CeW<WT>& cw, float wsum, float f0_, float f1_, float sq_, float mod_, float beta_, float f2_, float sl_)
      : PixGrad(t_, wt, cw, wsum, f0_, f1_, sq_, mod_, beta_) {
    if constexpr (LV) { this->f2 = f2_; this->sl = sl_; }
  }
  __device__ __forceinline__ float at(int k, float p, float w, float qa, float qg, float lq = 0.f) const {
    float ce;
    if constexpr (WT) ce = p * ct - ((k == t ? hit : 0.f) + epsk * w);
    else ce = p - (k == t ? 1.f : 0.f);
    if constexpr (FC) ce = mod * ce + beta * (p - (k == t ? 1.f : 0.f));
    if constexpr (LV) {
      float r = f0 * ce + this->f2 * (p * (lq - this->sl));
      if constexpr (DC) r += f1 * (p * (dice_q(k, t, qa, qg) - sq));
      return r;
    } else if constexpr (DC) return f0 * ce + f1 * (p * (dice_q(k, t, qa, qg) - sq));
    else return ce;
  }
};

__host__ inline float ac1_scale(int in, int out) { return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f; }

// ATen upsample_bilinear2d source index, align_corners = True
__device__ __forceinline__ void src_index_ac1(int dst, int in, float scale, int& i0, int& i1, float& l1) {
  const float src = scale * (float)dst;
  i0 = (int)src;
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = src - (float)i0;
  l1 = l1 < 0.f ? 0.f : (l1 > 1.f ? 1.f : l1);
}
// the backward direction: the first / last destination index in [lo, hi] whose two sources can include cell i
__device__ __forceinline__ int foot_lo(int i, float scale, int lo) { return scale > 0.f ? max(lo, (int)floorf((float)(i - 1) / scale)) : lo; }
__device__ __forceinline__ int foot_hi(int i, float scale, int hi) { return scale > 0.f ? min(hi, (int)ceilf((float)(i + 1) / scale)) : hi; }

// interpolated logits of pixel (Y,X) of image b into v[0..K)
template <int KW>
__device__ __forceinline__ void pixel_logits(const UpGeom& g, const float* __restrict__ lg, int b, int Y, int X, float* v) {
  int y0, y1, x0, x1; float ly, lx;
  src_index_ac1(Y, g.h, g.sy, y0, y1, ly);
  src_index_ac1(X, g.w, g.sx, x0, x1, lx);
  const float wy0 = 1.f - ly, wx0 = 1.f - lx;
  const float* p = lg + (size_t)b * g.K * g.h * g.w;
#pragma unroll
  for (int k = 0; k < KW; ++k) {
    if (k < g.K) {
      const float* q = p + (size_t)k * g.h * g.w;
      v[k] = wy0 * (wx0 * q[y0 * g.w + x0] + lx * q[y0 * g.w + x1]) + ly * (wx0 * q[y1 * g.w + x0] + lx * q[y1 * g.w + x1]);
    } else v[k] = -INFINITY;
  }
}

// The fuse core of tta_fuse_kernel and slide_fuse_kernel: what one term (a view, a window) contributes to a pixel and how the pixel is finished.  Each kernel keeps its
// own loop over the terms and its own weights; the float operations and their order are these, once.
// softmax over v[0..K) in place: max subtracted, expf, one division per channel
template <int KW>
__device__ __forceinline__ void fuse_softmax(int K, float* v) {
  float m = v[0];
#pragma unroll
  for (int k = 1; k < KW; ++k) if (k < K) m = fmaxf(m, v[k]);
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < KW; ++k) if (k < K) { v[k] = expf(v[k] - m); s += v[k]; }
#pragma unroll
  for (int k = 0; k < KW; ++k) if (k < K) v[k] = v[k] / s;
}
// acc_k = wt * v_k for the first term (acc is not zeroed), acc_k + wt * v_k after; a branch, not a select per channel: `first` is the same in every lane in both kernels
template <int KW>
__device__ __forceinline__ void fuse_accumulate(bool first, float wt, const float* v, float* acc) {
  if (first) {
#pragma unroll
    for (int k = 0; k < KW; ++k) acc[k] = wt * v[k];
  } else {
#pragma unroll
    for (int k = 0; k < KW; ++k) acc[k] = acc[k] + wt * v[k];
  }
}
// fused_k = acc_k / den, stored at pixel `pix` of plane bk + k of the fused map unless that is null; returns the label, the first maximum (torch.argmax)
template <int KW>
__device__ __forceinline__ uint8_t fuse_finish(int K, const float* acc, float den, float* __restrict__ fused, size_t bk, size_t plane, size_t pix) {
  int best = 0; float bv = 0.f;
#pragma unroll
  for (int k = 0; k < KW; ++k) if (k < K) {
    const float fk = acc[k] / den;
    if (k == 0 || fk > bv) { bv = fk; best = k; }
    if (fused) fused[(bk + k) * plane + pix] = fk;
  }
  return (uint8_t)best;
}

// Cross-entropy term of one valid pixel of label t from its logits v, for both forward kernels: ce_max gives m = max_k v_k and vt = v_t, the kernel sums
// s = sum_k exp(v_k - m) (the hybrid one keeps the exponentials: with that loop in here too its K = 33 instantiation lost a wave per SIMD), ce_pixel gives the
// numerator and denominator (plain: -logp_t and 1; WT: the weighted form above).
template <int KW>
__device__ __forceinline__ float ce_max(const float* v, int t, float& vt) {
  float m = v[0];
  vt = 0.f;
#pragma unroll
  for (int k = 0; k < KW; ++k) { m = fmaxf(m, v[k]); if (k == t) vt = v[k]; }
  return m;
}
// FC: the caller also hands so = sum_{k != t} e_k and et = e_t from the exponentials of its sum s; num becomes mod * num0, and (mod, beta) are the PixGrad's.
struct CePix { float num, den, mod, beta; };
template <int KW, bool WT, bool DC, bool FC = false>
__device__ __forceinline__ CePix ce_pixel(int K, const float* v, float m, float s, float vt, int t, const CeW<WT>& cw, const CeF<FC>& cf = CeF<FC>(), float so = 0.f, float et = 0.f) {
  CePix o;
  if constexpr (WT) {
    const float lse = logf(s) + m, wt = cew_at<DC || FC>(cw, t);
    float sm = 0.f;                                     // sum_k w_k (-logp_k), in index order
#pragma unroll
    for (int k = 0; k < KW; ++k) if (k < K) sm += cew_at<DC || FC>(cw, k) * (lse - v[k]);
    o.num = cw.keep * wt * (lse - vt) + cw.epsk * sm;
    o.den = wt;
  } else {
    o.num = logf(s) + m - vt;
    o.den = 1.f;
  }
  if constexpr (FC) {
    const float u = so / s, modu = focal_modu(u, cf.gamma);
    o.mod = modu * u;
    o.beta = cf.gamma * o.num * modu * (et / s);
    o.num = o.mod * o.num;
  }
  return o;
}

// part[blk] = (sum of pixel losses, number of valid pixels); WT: (sum of the pixel numerators, sum of w_t)
// cf sits in the four bytes of padding behind `ignore`: at the end, the empty CeF<false> moves the grid size this kernel reads behind its arguments by eight bytes
// (one immediate of the weighted instantiations would differ from the kernel as it was).
template <int KW, bool WT, bool FC>
__global__ __launch_bounds__(256) void upsample_ce_fwd_kernel(UpGeom g, const float* __restrict__ lg, const int64_t* __restrict__ tgt,
                                                              int ignore, CeF<FC> cf, float* __restrict__ part, CeW<WT> cw) {
  __shared__ float red[2][4];
  const long long total = (long long)g.B * g.H * g.W;
  float loss = 0.f, cnt = 0.f;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += gridDim.x * 256LL) {
    const long long t = tgt[i];
    if (t == ignore || t < 0 || t >= g.K) continue;
    const int X = (int)(i % g.W); const long long r = i / g.W;
    const int Y = (int)(r % g.H), b = (int)(r / g.H);
    float v[KW];
    pixel_logits<KW>(g, lg, b, Y, X, v);
    float vt;
    const float m = ce_max<KW>(v, (int)t, vt);
    float s = 0.f, so = 0.f, et = 0.f;
    if constexpr (FC) {
#pragma unroll
      for (int k = 0; k < KW; ++k) if (k < g.K) { const float e = expf(v[k] - m); s += e; if (k == (int)t) et = e; else so += e; }
    } else {
#pragma unroll
      for (int k = 0; k < KW; ++k) if (k < g.K) s += expf(v[k] - m);
    }
    const CePix px = ce_pixel<KW, WT, false, FC>(g.K, v, m, s, vt, (int)t, cw, cf, so, et);
    loss += px.num; cnt += px.den;
  }
  loss = wave_sum(loss); cnt = wave_sum(cnt);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { red[0][wave] = loss; red[1][wave] = cnt; }
  __syncthreads();
  if (threadIdx.x == 0) {
    part[blockIdx.x * 2 + 0] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    part[blockIdx.x * 2 + 1] = red[1][0] + red[1][1] + red[1][2] + red[1][3];
  }
}

__global__ void upsample_ce_finalize_kernel(const float* __restrict__ part, int nblk, float* __restrict__ out) {
  __shared__ double rs[256], rc[256];
  double s = 0.0, c = 0.0;
  for (int i = threadIdx.x; i < nblk; i += 256) { s += (double)part[2 * i]; c += (double)part[2 * i + 1]; }
  rs[threadIdx.x] = s; rc[threadIdx.x] = c;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) { rs[threadIdx.x] += rs[threadIdx.x + o]; rc[threadIdx.x] += rc[threadIdx.x + o]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { out[0] = (float)(rs[0] / rc[0]); out[1] = (float)rc[0]; }
}

// Forward of the hybrid form.  Block blockIdx.x = b * nbs + j strides over the H * W pixels of sample b alone (a row of partials never mixes samples), evaluates each
// pixel's softmax once and reduces the cross-entropy partials (the arithmetic of upsample_ce_fwd_kernel) and the per-class Dice sums:
//   part[blk][2 + 3K] = (cross-entropy numerator, denominator, I[0..K), P[0..K), T[0..K))
template <int KW, bool WT, bool FC>
__global__ __launch_bounds__(256) void upsample_ce_dice_fwd_kernel(UpGeom g, int nbs, const float* __restrict__ lg, const int64_t* __restrict__ tgt,
                                                                   int ignore, float* __restrict__ part, CeW<WT> cw, CeF<FC> cf) {
  __shared__ float red[4][2 + 3 * KW];
  const int b = blockIdx.x / nbs, jb = blockIdx.x - b * nbs;
  const int hw = g.H * g.W;
  const int64_t* tb = tgt + (size_t)b * hw;
  float loss = 0.f, cnt = 0.f;
  float si[KW], sp[KW], st[KW];
#pragma unroll
  for (int k = 0; k < KW; ++k) { si[k] = 0.f; sp[k] = 0.f; st[k] = 0.f; }
  const int stride = nbs * 256;
  int i = jb * 256 + (int)threadIdx.x;
  long long tn = i < hw ? tb[i] : -1;                  // the next label is in flight while this pixel is evaluated
  for (; i < hw; i += stride) {
    const long long t = tn;
    tn = i + stride < hw ? tb[i + stride] : -1;
    if (t == ignore || t < 0 || t >= g.K) continue;
    const int Y = i / g.W, X = i - Y * g.W;
    float v[KW], e[KW], vt;
    pixel_logits<KW>(g, lg, b, Y, X, v);
    const float m = ce_max<KW>(v, (int)t, vt);
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < KW; ++k) { e[k] = k < g.K ? expf(v[k] - m) : 0.f; if (k < g.K) s += e[k]; }
    float so = 0.f, et = 0.f;
    if constexpr (FC) {
#pragma unroll
      for (int k = 0; k < KW; ++k) if (k < g.K) { if (k == (int)t) et = e[k]; else so += e[k]; }
    }
    const CePix px = ce_pixel<KW, WT, true, FC>(g.K, v, m, s, vt, (int)t, cw, cf, so, et);
    loss += px.num; cnt += px.den;
    const float inv = 1.f / s;
#pragma unroll
    for (int k = 0; k < KW; ++k) {
      const float p = e[k] * inv;
      sp[k] += p;
      si[k] += k == (int)t ? p : 0.f;
      st[k] += k == (int)t ? 1.f : 0.f;
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  loss = wave_sum(loss); cnt = wave_sum(cnt);
  if (lane == 0) { red[wave][0] = loss; red[wave][1] = cnt; }
#pragma unroll
  for (int k = 0; k < KW; ++k) {
    if (k < g.K) {                                      // uniform: every lane of the wave takes the shuffles
      const float a = wave_sum(si[k]), p = wave_sum(sp[k]), c = wave_sum(st[k]);
      if (lane == 0) { red[wave][2 + k] = a; red[wave][2 + g.K + k] = p; red[wave][2 + 2 * g.K + k] = c; }
    }
  }
  __syncthreads();
  const int ncol = 2 + 3 * g.K;
  if ((int)threadIdx.x < ncol) part[(size_t)blockIdx.x * ncol + threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// One block of 1024 threads sums the partial rows in double, in a fixed order (no atomics), CB samples at a time: thread (sample, q, c) adds the rows q, q + RS, ... of
// column c, threads (sample, c) add the RS strands, threads (sample, k) turn (I, P, T) into the sample's Dice terms and the backward's coefficients, thread 0 keeps the
// running sums over the samples in index order.  out = (cross-entropy, its denominator, dice);  coef[b][k] = (a, g) = (-2 w_k / (B D), w_k N / (B D^2)).
__global__ __launch_bounds__(1024) void upsample_ce_dice_finalize_kernel(const float* __restrict__ part, int B, int K, int nbs, const float* __restrict__ w, double smooth,
                                                                         float* __restrict__ out, float* __restrict__ coef) {
  __shared__ double sh[1024], col[256], term[85];
  const int tid = threadIdx.x, ncol = 2 + 3 * K;
  const int RS = ncol <= 64 ? 4 : 1024 / ncol;         // four strands and 4 .. 51 samples per round (CB * ncol <= 256, CB * K <= 84); above 20 channels all threads on one sample (ncol <= 101)
  const int per = RS * ncol, CB = 1024 / per;
  double ce_n = 0.0, ce_d = 0.0, dice = 0.0;
  for (int b0 = 0; b0 < B; b0 += CB) {
    const int nb = min(CB, B - b0);
    {
      const int sb = tid / per, rem = tid - sb * per, q = rem / ncol, c = rem - q * ncol;
      double s = 0.0;
      if (sb < nb) for (int r = q; r < nbs; r += RS) s += (double)part[((size_t)(b0 + sb) * nbs + r) * ncol + c];
      sh[tid] = s;
    }
    __syncthreads();
    if (tid < nb * ncol) {
      const int sb = tid / ncol, c = tid - sb * ncol;
      double a = 0.0;
      for (int q = 0; q < RS; ++q) a += sh[sb * per + q * ncol + c];
      col[tid] = a;
    }
    __syncthreads();
    if (tid < nb * K) {
      const int sb = tid / K, k = tid - sb * K, b = b0 + sb;
      const double* cs = col + sb * ncol;
      const double wk = w ? (double)w[k] : 1.0;
      const double N = 2.0 * cs[2 + k] + smooth, D = cs[2 + K + k] + cs[2 + 2 * K + k] + smooth;
      term[tid] = wk * (1.0 - N / D);
      coef[((size_t)b * K + k) * 2 + 0] = (float)(-2.0 * wk / ((double)B * D));
      coef[((size_t)b * K + k) * 2 + 1] = (float)(wk * N / ((double)B * D * D));
    }
    __syncthreads();
    if (tid == 0) {
      for (int sb = 0; sb < nb; ++sb) {
        ce_n += col[sb * ncol]; ce_d += col[sb * ncol + 1];
        double d = 0.0;
        for (int k = 0; k < K; ++k) d += term[sb * K + k];
        dice += d;
      }
    }
    // the next round writes sh first (last read before the second barrier), col after its first barrier and term after its second: thread 0 is past its reads by then
  }
  if (tid == 0) { out[0] = (float)(ce_n / ce_d); out[1] = (float)ce_d; out[2] = (float)(dice / (double)B); }
}

// four lanes per low-resolution cell (each takes every 4th footprint row), gather over the pixels whose bilinear
// footprint touches the cell, then a 4-lane shuffle reduction: deterministic, no atomics.
template <int KW, bool WT, bool DC, bool FC, bool LV>
__global__ __launch_bounds__(256) void upsample_ce_bwd_kernel(UpGeom g, const float* __restrict__ lg, const int64_t* __restrict__ tgt,
                                                              const float* __restrict__ loss_cnt, const float* __restrict__ gscale,
                                                              int ignore, float* __restrict__ dlg, CeW<WT> cw, CeD<DC> cd, CeF<FC> cf, CeL<LV> cl) {
  constexpr bool NOK = DC || FC || LV;                  // the class-weight pointer may be null
  const long long cells = (long long)g.B * g.h * g.w;
  const long long ci = (blockIdx.x * 256LL + threadIdx.x) >> 2;
  const int sub = threadIdx.x & 3;
  const bool live = ci < cells;
  const long long cc = live ? ci : 0;
  const int j = (int)(cc % g.w); const long long r = cc / g.w;
  const int i = (int)(r % g.h), b = (int)(r / g.h);
  float acc[KW];
#pragma unroll
  for (int k = 0; k < KW; ++k) acc[k] = 0.f;
  const int Ylo = foot_lo(i, g.sy, 0), Yhi = foot_hi(i, g.sy, g.H - 1);
  const int Xlo = foot_lo(j, g.sx, 0), Xhi = foot_hi(j, g.sx, g.W - 1);
  float wsum = 0.f;
  if constexpr (WT) {
#pragma unroll
    for (int k = 0; k < KW; ++k) if (k < g.K) wsum += cew_at<NOK>(cw, k);
  }
  float qa[DC ? KW : 1], qg[DC ? KW : 1], f0 = 0.f, f1 = 0.f;      // DC: the (a, g) of this cell's sample and the two scales
  float f2 = 0.f;                                       // LV: the third scale
  if constexpr (LV) { f0 = gscale[0] / loss_cnt[1]; f2 = gscale[2]; }
  if constexpr (DC) {
    f0 = gscale[0] / loss_cnt[1]; f1 = gscale[1];
#pragma unroll
    for (int k = 0; k < KW; ++k) {
      qa[k] = k < g.K ? cd.coef[((size_t)b * g.K + k) * 2] : 0.f;
      qg[k] = k < g.K ? cd.coef[((size_t)b * g.K + k) * 2 + 1] : 0.f;
    }
  }
  if (live) {
    for (int Y = Ylo + sub; Y <= Yhi; Y += 4) {
      int y0, y1; float ly;
      src_index_ac1(Y, g.h, g.sy, y0, y1, ly);
      const float wy = (y0 == i ? 1.f - ly : 0.f) + (y1 == i ? ly : 0.f);
      if (wy == 0.f) continue;
      for (int X = Xlo; X <= Xhi; ++X) {
        int x0, x1; float lx;
        src_index_ac1(X, g.w, g.sx, x0, x1, lx);
        const float wx = (x0 == j ? 1.f - lx : 0.f) + (x1 == j ? lx : 0.f);
        if (wx == 0.f) continue;
        const long long t = tgt[((size_t)b * g.H + Y) * g.W + X];
        if (t == ignore || t < 0 || t >= g.K) continue;
        float v[KW];
        pixel_logits<KW>(g, lg, b, Y, X, v);
        float m = v[0];
#pragma unroll
        for (int k = 0; k < KW; ++k) m = fmaxf(m, v[k]);
        float s = 0.f, lso = 0.f;                         // LV: lso = sum_{k != t} e_k, in index order
        CePix px = {};                                    // FC: the pixel's (mod, beta), from the logits before the exponentials take their place
        if constexpr (FC) {
          float e[KW], vt = 0.f, so = 0.f, et = 0.f;
#pragma unroll
          for (int k = 0; k < KW; ++k) {
            e[k] = k < g.K ? expf(v[k] - m) : 0.f; s += e[k];
            if (k == (int)t) { vt = v[k]; et = e[k]; } else so += e[k];
          }
          px = ce_pixel<KW, WT, DC, true>(g.K, v, m, s, vt, (int)t, cw, cf, so, et);
#pragma unroll
          for (int k = 0; k < KW; ++k) v[k] = e[k];
          if constexpr (LV) lso = so;
        } else {
#pragma unroll
          for (int k = 0; k < KW; ++k) {
            v[k] = k < g.K ? expf(v[k] - m) : 0.f; s += v[k];
            if constexpr (LV) if (k != (int)t) lso += v[k];
          }
        }
        const float wgt = wy * wx, inv = 1.f / s;
        float sq = 0.f;                                   // DC: sum_c p_c q_c, in index order
#pragma unroll
        for (int k = 0; k < KW; ++k) {
          v[k] *= inv;
          if constexpr (DC) sq += v[k] * dice_q(k, (int)t, qa[k], qg[k]);
        }
        float lq[LV ? KW : 1], sl = 0.f;                  // LV: the Lovasz q of every channel and sum_c p_c q_c, in index order
        if constexpr (LV) {
          const float u = lso * inv;
#pragma unroll
          for (int k = 0; k < KW; ++k) { lq[k] = k < g.K ? lov_q(cl.tab, k, (int)t, v[k], u) : 0.f; sl += v[k] * lq[k]; }
        }
        const PixGrad<WT, DC, FC, LV> pg((int)t, cew_at<NOK>(cw, (int)t), cw, wsum, f0, f1, sq, FC ? px.mod : 1.f, FC ? px.beta : 0.f, f2, sl);
        constexpr bool PLAIN = !WT && !DC && !LV;         // reads no table: runs over all KW unguarded (acc beyond K is never stored)
#pragma unroll
        for (int k = 0; k < KW; ++k)
          if (PLAIN || k < g.K) acc[k] += wgt * pg.at(k, v[k], cew_at<NOK>(cw, k), DC ? qa[k] : 0.f, DC ? qg[k] : 0.f, LV ? lq[k] : 0.f);
      }
    }
  }
  float f = 1.f;                                        // DC, LV: the scales are inside the pixel gradients
  if constexpr (!DC && !LV) f = gscale[0] / loss_cnt[1];
#pragma unroll
  for (int k = 0; k < KW; ++k) {
    float a = acc[k];
    a += __shfl_xor(a, 1, 64);
    a += __shfl_xor(a, 2, 64);
    if (live && sub == 0 && k < g.K) dlg[(((size_t)b * g.K + k) * g.h + i) * g.w + j] = a * f;
  }
}

// Tiled form of the same gradient: a block owns CT x CT low-resolution cells and evaluates the softmax of every pixel of their joint
// footprint ONCE (the per-cell gather above evaluates each pixel for each of the ~4 cells it touches, from global memory), then applies the
// separable bilinear weights in two LDS passes:  H1[Y][j][k] = sum_X wx(X, j) G[Y][X][k],  dlg[i][j][k] = sum_Y wy(Y, i) H1[Y][j][k].
// Sums run in a fixed order (deterministic); they are associated differently from the gather kernel (last-bit differences).
//
// For K > KNC, G[NY][NX][K] does not fit the LDS any more (x8 upsampling, CT = 4: 44 x 44 pixels x 33 channels x 4 B = 256 KB of 160 KiB), so the channel-sliced
// ("wide") kernel takes the channels through G and H1 in slices of KS <= KNC (the host picks the fewest slices that fit; KS == K in the one-pass kernel).
constexpr int CT = 4;
struct UpTile { int NYmax, NXmax, KS; };

// The LDS of both tiled kernels: ONE list of buffers, in this order, in floats.  The host sums it (tile_lds_bytes), the device carves the block's LDS by it (tile_frame).
enum TileBuf {
  T_LGT,   // [(CT+2)^2][K] logits of the cells around the tile (clamped at the map border)
  T_WY0,   // [NY][3] per footprint row: cell y0 and cell y1 as int, weight ly on y1
  T_WX0,   // [NX][3]
  T_WXJ,   // [NX][CT] weight of footprint column X on cell j0 + jr
  T_WYI,   // [NY][CT]
  T_ST,    // wide: [NY][NX][SW] max, 1 / sum, label as int (-1: the pixel does not count); DC: the fourth word is sum_c p_c q_c over ALL K channels;
           // LV: two words behind those, the Lovasz sum_c p_c q_c over ALL K channels and u;  FC: the last two words are the pixel's (mod, beta)
  T_H1,    // [NY][CT][KS]
  T_G,     // [NY][NX][KS]
  T_WL,    // WT: [K] class weights
  T_CF,    // DC: [K][2] Dice coefficients (a, g) of this block's sample
  T_NBUF
};
// I: size_t on the host, which sizes a launch it may still refuse; int on the device, where the sum has passed the host's 150 KiB limit
template <typename I>
__host__ __device__ inline void tile_extents(int K, const UpTile& ut, bool wt, bool dc, bool fc, bool lv, bool wide, I* n) {
  const I NY = ut.NYmax, NX = ut.NXmax;
  n[T_LGT] = (I)(CT + 2) * (CT + 2) * K;
  n[T_WY0] = 3 * NY; n[T_WX0] = 3 * NX; n[T_WXJ] = CT * NX; n[T_WYI] = CT * NY;
  n[T_ST] = wide ? ((dc ? 4 : 3) + (lv ? 2 : 0) + (fc ? 2 : 0)) * NY * NX : 0;
  n[T_H1] = NY * CT * ut.KS; n[T_G] = NY * NX * ut.KS;
  n[T_WL] = wt ? K : 0; n[T_CF] = dc ? 2 * K : 0;
}
inline size_t tile_lds_bytes(int K, const UpTile& ut, bool wt, bool dc, bool fc, bool lv, bool wide) {
  size_t n[T_NBUF], s = 0;
  tile_extents(K, ut, wt, dc, fc, lv, wide, n);
  for (int i = 0; i < T_NBUF; ++i) s += n[i];
  return s * sizeof(float);
}

// The block's tile: sample b, cells [i0, i1] x [j0, j1], their joint footprint [Ylo, Yhi] x [Xlo, Xhi] of NY x NX pixels, and its LDS buffers.
struct TileFrame {
  int b, i0, j0, i1, j1, Ylo, Yhi, Xlo, Xhi, NY, NX;
  float* buf[T_NBUF];
};
// Carves the LDS and fills lgt, the weight and coefficient tables and wy0 / wx0 / wyi / wxj; ends with the barrier.
template <int NT, bool WT, bool DC, bool WIDE, bool FC = false, bool LV = false>
__device__ __forceinline__ TileFrame tile_frame(const UpGeom& g, const UpTile& ut, float* sm, const float* __restrict__ lg, const CeW<WT>& cw, const CeD<DC>& cd) {
  TileFrame f;
  const int K = g.K, tid = threadIdx.x;
  int n[T_NBUF];
  tile_extents(K, ut, WT, DC, FC, LV, WIDE, n);
#pragma unroll
  for (int i = 0; i < T_NBUF; ++i) { f.buf[i] = sm; sm += n[i]; }
  float *lgt = f.buf[T_LGT], *wy0 = f.buf[T_WY0], *wx0 = f.buf[T_WX0], *wxj = f.buf[T_WXJ], *wyi = f.buf[T_WYI];
  const int tw = cdiv(g.w, CT), th = cdiv(g.h, CT);
  int blk = blockIdx.x;
  const int tj = blk % tw; blk /= tw;
  const int ti = blk % th; const int b = blk / th;
  const int i0 = ti * CT, j0 = tj * CT;
  const int i1 = min(i0 + CT, g.h) - 1, j1 = min(j0 + CT, g.w) - 1;          // last cell of the tile
  const int Ylo = foot_lo(i0, g.sy, 0), Yhi = foot_hi(i1, g.sy, g.H - 1);
  const int Xlo = foot_lo(j0, g.sx, 0), Xhi = foot_hi(j1, g.sx, g.W - 1);
  const int NY = Yhi - Ylo + 1, NX = Xhi - Xlo + 1;
  const float* lb = lg + (size_t)b * K * g.h * g.w;
  for (int e = tid; e < (CT + 2) * (CT + 2) * K; e += NT) {
    const int k = e % K, c = e / K, cy = c / (CT + 2), cx = c - cy * (CT + 2);
    const int yy = min(max(i0 - 1 + cy, 0), g.h - 1), xx = min(max(j0 - 1 + cx, 0), g.w - 1);
    lgt[e] = lb[((size_t)k * g.h + yy) * g.w + xx];
  }
  if constexpr (WT) for (int e = tid; e < K; e += NT) f.buf[T_WL][e] = cew_at<DC || FC || LV>(cw, e);
  if constexpr (DC) for (int e = tid; e < 2 * K; e += NT) f.buf[T_CF][e] = cd.coef[(size_t)b * K * 2 + e];
  for (int e = tid; e < NY; e += NT) {
    int y0, y1; float ly; src_index_ac1(Ylo + e, g.h, g.sy, y0, y1, ly);
    wy0[3 * e] = __int_as_float(y0); wy0[3 * e + 1] = __int_as_float(y1); wy0[3 * e + 2] = ly;
#pragma unroll
    for (int r = 0; r < CT; ++r) wyi[e * CT + r] = (y0 == i0 + r ? 1.f - ly : 0.f) + (y1 == i0 + r ? ly : 0.f);
  }
  for (int e = tid; e < NX; e += NT) {
    int x0, x1; float lx; src_index_ac1(Xlo + e, g.w, g.sx, x0, x1, lx);
    wx0[3 * e] = __int_as_float(x0); wx0[3 * e + 1] = __int_as_float(x1); wx0[3 * e + 2] = lx;
#pragma unroll
    for (int r = 0; r < CT; ++r) wxj[e * CT + r] = (x0 == j0 + r ? 1.f - lx : 0.f) + (x1 == j0 + r ? lx : 0.f);
  }
  __syncthreads();
  f.b = b; f.i0 = i0; f.j0 = j0; f.i1 = i1; f.j1 = j1; f.Ylo = Ylo; f.Yhi = Yhi; f.Xlo = Xlo; f.Xhi = Xhi; f.NY = NY; f.NX = NX;
  return f;
}

// the four neighbourhood cells a footprint pixel (yr, xr) interpolates from, and its weights
struct UpTap {
  const float *q00, *q01, *q10, *q11;
  float wya, wxa, ly, lx;
  __device__ __forceinline__ float at(int k) const { return wya * (wxa * q00[k] + lx * q01[k]) + ly * (wxa * q10[k] + lx * q11[k]); }
};
__device__ __forceinline__ UpTap up_tap(const float* lgt, const float* wy0, const float* wx0, int yr, int xr, int i0, int j0, int K) {
  UpTap t;
  const int y0 = __float_as_int(wy0[3 * yr]), y1 = __float_as_int(wy0[3 * yr + 1]); t.ly = wy0[3 * yr + 2];
  const int x0 = __float_as_int(wx0[3 * xr]), x1 = __float_as_int(wx0[3 * xr + 1]); t.lx = wx0[3 * xr + 2];
  t.wya = 1.f - t.ly; t.wxa = 1.f - t.lx;
  // a footprint pixel at the rim may interpolate from a cell outside the (CT+2)^2 neighbourhood; it then has zero weight on every cell of
  // this tile, so any finite value will do: clamp the index
  const int ry0 = min(max(y0 - i0 + 1, 0), CT + 1), ry1 = min(max(y1 - i0 + 1, 0), CT + 1);
  const int rx0 = min(max(x0 - j0 + 1, 0), CT + 1), rx1 = min(max(x1 - j0 + 1, 0), CT + 1);
  t.q00 = lgt + (ry0 * (CT + 2) + rx0) * K; t.q01 = lgt + (ry0 * (CT + 2) + rx1) * K;
  t.q10 = lgt + (ry1 * (CT + 2) + rx0) * K; t.q11 = lgt + (ry1 * (CT + 2) + rx1) * K;
  return t;
}

// The separable bilinear scatter of channels [k0, k0 + kn) held in G with channel stride KS.  Pass 2a, along X: H1[Y][j][k] = sum_X wx(X, j) G[Y][X][k].
template <int NT>
__device__ __forceinline__ void scatter_x(const UpGeom& g, const TileFrame& f, int kn, int KS) {
  const float *G = f.buf[T_G], *wxj = f.buf[T_WXJ];
  float* H1 = f.buf[T_H1];
  for (int e = threadIdx.x; e < f.NY * CT * kn; e += NT) {
    const int kk = e % kn, r = e / kn, jr = r % CT, yr = r / CT;
    const int j = f.j0 + jr;
    float acc = 0.f;
    if (j <= f.j1) {
      const int xa = foot_lo(j, g.sx, f.Xlo) - f.Xlo, xb = foot_hi(j, g.sx, f.Xhi) - f.Xlo;
      const float* grow = G + (size_t)yr * f.NX * KS + kk;
      for (int xr = xa; xr <= xb; ++xr) acc += wxj[xr * CT + jr] * grow[xr * KS];
    }
    H1[(yr * CT + jr) * KS + kk] = acc;
  }
}
// Pass 2b, along Y, times the final scale, store: dlg[i][j][k0 + k] = scale * sum_Y wy(Y, i) H1[Y][j][k].
template <int NT>
__device__ __forceinline__ void scatter_y_store(const UpGeom& g, const TileFrame& f, int k0, int kn, int KS, float scale, float* __restrict__ dlg) {
  const float *H1 = f.buf[T_H1], *wyi = f.buf[T_WYI];
  for (int e = threadIdx.x; e < CT * CT * kn; e += NT) {
    const int kk = e % kn, c = e / kn, ir = c / CT, jr = c - ir * CT;
    const int i = f.i0 + ir, j = f.j0 + jr;
    if (i > f.i1 || j > f.j1) continue;
    const int ya = foot_lo(i, g.sy, f.Ylo), yb = foot_hi(i, g.sy, f.Yhi);
    float acc = 0.f;
    for (int yr = ya - f.Ylo; yr <= yb - f.Ylo; ++yr) acc += wyi[yr * CT + ir] * H1[(yr * CT + jr) * KS + kk];
    dlg[(((size_t)f.b * g.K + k0 + kk) * g.h + i) * g.w + j] = acc * scale;
  }
}

template <int NT, bool WT, bool DC, bool FC, bool LV>
__global__ __launch_bounds__(NT) void upsample_ce_bwd_tiled_kernel(UpGeom g, UpTile ut, const float* __restrict__ lg, const int64_t* __restrict__ tgt,
                                                                   const float* __restrict__ loss_cnt, const float* __restrict__ gscale,
                                                                   int ignore, float* __restrict__ dlg, CeW<WT> cw, CeD<DC> cd, CeF<FC> fo, CeL<LV> cl) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  constexpr int KW = KNC;                            // this kernel serves K <= KNC (G holds all K channels of every footprint pixel)
  const int K = g.K;
  // This kernel keeps its own prologue and scatter passes, in the order of TileBuf (no statistics): through tile_frame / scatter_x / scatter_y_store its plain and
  // weighted forms, the default training step's kernels, measured 0.5 .. 2 % slower on equal arithmetic.
  float* lgt = sm;
  float* wy0 = lgt + (CT + 2) * (CT + 2) * K;
  float* wx0 = wy0 + 3 * ut.NYmax;
  float* wxj = wx0 + 3 * ut.NXmax;
  float* wyi = wxj + CT * ut.NXmax;
  float* H1 = wyi + CT * ut.NYmax;
  float* G = H1 + ut.NYmax * CT * K;
  float* wl = nullptr;
  if constexpr (WT) wl = G + (size_t)ut.NYmax * ut.NXmax * K;
  float* cf = nullptr;
  if constexpr (DC) cf = G + (size_t)ut.NYmax * ut.NXmax * K + (WT ? K : 0);
  const int tid = threadIdx.x;
  const int tw = cdiv(g.w, CT), th = cdiv(g.h, CT);
  int blk = blockIdx.x;
  const int tj = blk % tw; blk /= tw;
  const int ti = blk % th; const int b = blk / th;
  const int i0 = ti * CT, j0 = tj * CT;
  const int i1 = min(i0 + CT, g.h) - 1, j1 = min(j0 + CT, g.w) - 1;          // last cell of the tile
  const int Ylo = foot_lo(i0, g.sy, 0), Yhi = foot_hi(i1, g.sy, g.H - 1);
  const int Xlo = foot_lo(j0, g.sx, 0), Xhi = foot_hi(j1, g.sx, g.W - 1);
  const int NY = Yhi - Ylo + 1, NX = Xhi - Xlo + 1;
  const float* lb = lg + (size_t)b * K * g.h * g.w;
  for (int e = tid; e < (CT + 2) * (CT + 2) * K; e += NT) {
    const int k = e % K, c = e / K, cy = c / (CT + 2), cx = c - cy * (CT + 2);
    const int yy = min(max(i0 - 1 + cy, 0), g.h - 1), xx = min(max(j0 - 1 + cx, 0), g.w - 1);
    lgt[e] = lb[((size_t)k * g.h + yy) * g.w + xx];
  }
  if constexpr (WT) for (int e = tid; e < K; e += NT) wl[e] = cew_at<DC || FC || LV>(cw, e);
  if constexpr (DC) for (int e = tid; e < 2 * K; e += NT) cf[e] = cd.coef[(size_t)b * K * 2 + e];
  for (int e = tid; e < NY; e += NT) {
    int y0, y1; float ly; src_index_ac1(Ylo + e, g.h, g.sy, y0, y1, ly);
    wy0[3 * e] = __int_as_float(y0); wy0[3 * e + 1] = __int_as_float(y1); wy0[3 * e + 2] = ly;
#pragma unroll
    for (int r = 0; r < CT; ++r) wyi[e * CT + r] = (y0 == i0 + r ? 1.f - ly : 0.f) + (y1 == i0 + r ? ly : 0.f);
  }
  for (int e = tid; e < NX; e += NT) {
    int x0, x1; float lx; src_index_ac1(Xlo + e, g.w, g.sx, x0, x1, lx);
    wx0[3 * e] = __int_as_float(x0); wx0[3 * e + 1] = __int_as_float(x1); wx0[3 * e + 2] = lx;
#pragma unroll
    for (int r = 0; r < CT; ++r) wxj[e * CT + r] = (x0 == j0 + r ? 1.f - lx : 0.f) + (x1 == j0 + r ? lx : 0.f);
  }
  __syncthreads();
  // ---- pass 1: softmax - onehot of every footprint pixel, once
  // the thread's labels first, all loads in flight (a load at the top of every iteration was a chain of ~8 memory round trips per block)
  constexpr int TPF = 2048 / NT;
  long long tpre[TPF];
#pragma unroll
  for (int u = 0; u < TPF; ++u) {
    const int pix = tid + NT * u;
    const int yr = pix / NX, xr = pix - yr * NX;
    tpre[u] = pix < NY * NX ? tgt[((size_t)b * g.H + Ylo + yr) * g.W + Xlo + xr] : (long long)ignore;
  }
  float wsum = 0.f;
  if constexpr (WT) for (int k = 0; k < K; ++k) wsum += wl[k];
  float f0 = 0.f, f1 = 0.f, f2 = 0.f;
  if constexpr (DC) { f0 = gscale[0] / loss_cnt[1]; f1 = gscale[1]; }
  if constexpr (LV) { f0 = gscale[0] / loss_cnt[1]; f2 = gscale[2]; }
#pragma unroll 1
  for (int u = 0; tid + NT * u < NY * NX; ++u) {
    const int pix = tid + NT * u;
    const int yr = pix / NX, xr = pix - yr * NX;
    float* out = G + (size_t)pix * K;
    long long t;
    if (u < TPF) {
      t = tpre[0];
#pragma unroll
      for (int q = 1; q < TPF; ++q) t = u == q ? tpre[q] : t;
    } else t = tgt[((size_t)b * g.H + Ylo + yr) * g.W + Xlo + xr];
    if (t == ignore || t < 0 || t >= K) {
      for (int k = 0; k < K; ++k) out[k] = 0.f;
      continue;
    }
    const UpTap tap = up_tap(lgt, wy0, wx0, yr, xr, i0, j0, K);
    float v[KW];
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < KW; ++k) {
      if (k < K) { v[k] = tap.at(k); m = fmaxf(m, v[k]); }
      else v[k] = -INFINITY;
    }
    float ssum = 0.f;
    [[maybe_unused]] float lso = 0.f;                  // LV: sum_{k != t} e_k, in index order
    CePix px = {};                                     // FC: the pixel's (mod, beta), from the logits before the exponentials take their place
    if constexpr (FC) {
      float e[KW], vt = 0.f, so = 0.f, et = 0.f;
#pragma unroll
      for (int k = 0; k < KW; ++k) {
        e[k] = k < K ? __expf(v[k] - m) : 0.f; ssum += e[k];
        if (k == (int)t) { vt = v[k]; et = e[k]; } else so += e[k];
      }
      px = ce_pixel<KW, WT, DC, true>(K, v, m, ssum, vt, (int)t, cw, fo, so, et);
#pragma unroll
      for (int k = 0; k < KW; ++k) v[k] = e[k];
      if constexpr (LV) lso = so;
    } else {
#pragma unroll
      for (int k = 0; k < KW; ++k) {
        v[k] = k < K ? __expf(v[k] - m) : 0.f; ssum += v[k];      // hardware exp2-based: 2 ulp, the gradient's tolerance is 1e-3
        if constexpr (LV) if (k != (int)t) lso += v[k];
      }
    }
    const float inv = 1.f / ssum;
    // DC normalises v first (sq = sum_c p_c q_c, in index order, needs every p); the other forms multiply by inv at the one use below, under the same k < K guard as
    // the store: a normalising loop of its own costs them 16 selects per pixel (measured: +3 % on this kernel)
    float sq = 0.f;
    if constexpr (DC) {
#pragma unroll
      for (int k = 0; k < KW; ++k) if (k < K) { v[k] *= inv; sq += v[k] * dice_q(k, (int)t, cf[2 * k], cf[2 * k + 1]); }
    }
    if constexpr (LV) {                                // normalised v (by the loop above with DC), the Lovasz q of every channel and sum_c p_c q_c, in index order
      float lq[KW], sl = 0.f;
      const float u = lso * inv;
#pragma unroll
      for (int k = 0; k < KW; ++k) {
        if constexpr (!DC) v[k] *= inv;
        lq[k] = k < K ? lov_q(cl.tab, k, (int)t, v[k], u) : 0.f;
        sl += v[k] * lq[k];
      }
      const PixGrad<WT, DC, FC, LV> pg((int)t, WT ? wl[t] : 1.f, cw, wsum, f0, f1, sq, FC ? px.mod : 1.f, FC ? px.beta : 0.f, f2, sl);
#pragma unroll
      for (int k = 0; k < KW; ++k) if (k < K) out[k] = pg.at(k, v[k], WT ? wl[k] : 0.f, DC ? cf[2 * k] : 0.f, DC ? cf[2 * k + 1] : 0.f, lq[k]);
    } else {
      const PixGrad<WT, DC, FC> pg((int)t, WT ? wl[t] : 1.f, cw, wsum, f0, f1, sq, FC ? px.mod : 1.f, FC ? px.beta : 0.f);
#pragma unroll
      for (int k = 0; k < KW; ++k) if (k < K) out[k] = pg.at(k, DC ? v[k] : v[k] * inv, WT ? wl[k] : 0.f, DC ? cf[2 * k] : 0.f, DC ? cf[2 * k + 1] : 0.f);
    }
  }
  __syncthreads();
  // ---- pass 2a: along X
  for (int e = tid; e < NY * CT * K; e += NT) {
    const int k = e % K, r = e / K, jr = r % CT, yr = r / CT;
    const int j = j0 + jr;
    float acc = 0.f;
    if (j <= j1) {
      const int xa = foot_lo(j, g.sx, Xlo) - Xlo, xb = foot_hi(j, g.sx, Xhi) - Xlo;
      const float* grow = G + (size_t)yr * NX * K + k;
      for (int xr = xa; xr <= xb; ++xr) acc += wxj[xr * CT + jr] * grow[xr * K];
    }
    H1[e] = acc;
  }
  __syncthreads();
  // ---- pass 2b: along Y, scale, store
  float f = 1.f;                                     // DC, LV: the scales are inside G
  if constexpr (!DC && !LV) f = gscale[0] / loss_cnt[1];
  for (int e = tid; e < CT * CT * K; e += NT) {
    const int k = e % K, c = e / K, ir = c / CT, jr = c - ir * CT;
    const int i = i0 + ir, j = j0 + jr;
    if (i > i1 || j > j1) continue;
    const int ya = foot_lo(i, g.sy, Ylo), yb = foot_hi(i, g.sy, Yhi);
    float acc = 0.f;
    for (int yr = ya - Ylo; yr <= yb - Ylo; ++yr) acc += wyi[yr * CT + ir] * H1[(yr * CT + jr) * K + k];
    dlg[(((size_t)b * K + k) * g.h + i) * g.w + j] = acc * f;
  }
}

// The tiled gradient for K > KNC, channels in slices of ut.KS.  One pass over the footprint first computes every pixel's max and 1 / sum over ALL K channels from lgt
// and keeps them with the label (three words per pixel); pass 1 and the scatter then run once per slice on those statistics.
// Each pixel's softmax is still evaluated once (2 K exponentials instead of K); sums in a fixed order, no atomics.
// FC: the focal (mod, beta) of a pixel need all K channels (the cross-entropy numerator, the sum without t), so pass 0, the only one that sees them all, evaluates
// ce_pixel on the pixel's K logits in registers and keeps the two values as two more statistics words; the slices read them back into their PixGrad.
// LV: pass 0 also keeps the Lovasz sum_c p_c q_c over all K channels and u, from the p = __expf(v - m) * inv the slices evaluate again (the same bins both times).
template <int NT, bool WT, bool DC, bool FC, bool LV>
__global__ __launch_bounds__(NT) void upsample_ce_bwd_tiled_wide_kernel(UpGeom g, UpTile ut, const float* __restrict__ lg, const int64_t* __restrict__ tgt,
                                                                        const float* __restrict__ loss_cnt, const float* __restrict__ gscale,
                                                                        int ignore, float* __restrict__ dlg, CeW<WT> cw, CeD<DC> cd, CeF<FC> fo, CeL<LV> cl) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  constexpr int LO = DC ? 4 : 3;                     // LV: its two statistics words
  constexpr int SW = LO + (LV ? 2 : 0) + (FC ? 2 : 0);   // statistics words per footprint pixel
  const int K = g.K, KS = ut.KS, tid = threadIdx.x;
  const TileFrame f = tile_frame<NT, WT, DC, true, FC, LV>(g, ut, sm, lg, cw, cd);
  const int b = f.b, i0 = f.i0, j0 = f.j0, Ylo = f.Ylo, Xlo = f.Xlo, NY = f.NY, NX = f.NX;
  float *st = f.buf[T_ST], *G = f.buf[T_G];
  const float *lgt = f.buf[T_LGT], *wy0 = f.buf[T_WY0], *wx0 = f.buf[T_WX0], *wl = f.buf[T_WL], *cf = f.buf[T_CF];
  // ---- pass 0: max and 1 / sum over all K channels of every footprint pixel, once
  for (int pix = tid; pix < NY * NX; pix += NT) {
    const int yr = pix / NX, xr = pix - yr * NX;
    const long long t = tgt[((size_t)b * g.H + Ylo + yr) * g.W + Xlo + xr];
    float* s = st + SW * pix;
    if (t == ignore || t < 0 || t >= K) { s[2] = __int_as_float(-1); continue; }
    const UpTap tap = up_tap(lgt, wy0, wx0, yr, xr, i0, j0, K);
    float m = -INFINITY;
    for (int k = 0; k < K; ++k) m = fmaxf(m, tap.at(k));
    float ssum = 0.f;
    if constexpr (FC) {
      float v[KMAXC], vt = 0.f, so = 0.f, et = 0.f, sq = 0.f;
#pragma unroll
      for (int k = 0; k < KMAXC; ++k) {
        v[k] = k < K ? tap.at(k) : -INFINITY;
        const float e = k < K ? __expf(v[k] - m) : 0.f;
        ssum += e;
        if (k == (int)t) { vt = v[k]; et = e; } else so += e;
        if constexpr (DC) if (k < K) sq += e * dice_q(k, (int)t, cf[2 * k], cf[2 * k + 1]);
      }
      if constexpr (DC) s[3] = sq * (1.f / ssum);
      const CePix px = ce_pixel<KMAXC, WT, DC, true>(K, v, m, ssum, vt, (int)t, cw, fo, so, et);
      s[SW - 2] = px.mod; s[SW - 1] = px.beta;
    } else if constexpr (DC) {
      float sq = 0.f;                                  // sum_c e_c q_c from the same exponentials, in index order
      for (int k = 0; k < K; ++k) { const float e = __expf(tap.at(k) - m); ssum += e; sq += e * dice_q(k, (int)t, cf[2 * k], cf[2 * k + 1]); }
      s[3] = sq * (1.f / ssum);
    } else {
      for (int k = 0; k < K; ++k) ssum += __expf(tap.at(k) - m);
    }
    s[0] = m; s[1] = 1.f / ssum; s[2] = __int_as_float((int)t);
    if constexpr (LV) {
      const float inv = 1.f / ssum;
      float so = 0.f, sl = 0.f;
      for (int k = 0; k < K; ++k) if (k != (int)t) so += __expf(tap.at(k) - m);
      const float u = so * inv;
      for (int k = 0; k < K; ++k) { const float p = __expf(tap.at(k) - m) * inv; sl += p * lov_q(cl.tab, k, (int)t, p, u); }
      s[LO] = sl; s[LO + 1] = u;
    }
  }
  __syncthreads();
  const float f0 = gscale[0] / loss_cnt[1];          // DC: applied per pixel with f1 before the scatter
  float f1 = 0.f, f2 = 0.f;
  if constexpr (DC) f1 = gscale[1];
  if constexpr (LV) f2 = gscale[2];
  float wsum = 0.f;
  if constexpr (WT) for (int k = 0; k < K; ++k) wsum += wl[k];
  for (int k0 = 0; k0 < K; k0 += KS) {
    const int kn = min(KS, K - k0);
    // ---- pass 1: softmax - onehot of the slice's channels
    for (int pix = tid; pix < NY * NX; pix += NT) {
      const int yr = pix / NX, xr = pix - yr * NX;
      const float* s = st + SW * pix;
      float* out = G + (size_t)pix * KS;
      const int t = __float_as_int(s[2]);
      if (t < 0) {
        for (int kk = 0; kk < kn; ++kk) out[kk] = 0.f;
        continue;
      }
      const UpTap tap = up_tap(lgt, wy0, wx0, yr, xr, i0, j0, K);
      const float m = s[0], inv = s[1];
      const PixGrad<WT, DC, FC, LV> pg(t, WT ? wl[t] : 1.f, cw, wsum, f0, f1, DC ? s[3] : 0.f, FC ? s[SW - 2] : 1.f, FC ? s[SW - 1] : 0.f, f2, LV ? s[LO] : 0.f);
      for (int kk = 0; kk < kn; ++kk) {
        const int k = k0 + kk;
        const float p = __expf(tap.at(k) - m) * inv;
        float lq = 0.f;
        if constexpr (LV) lq = lov_q(cl.tab, k, t, p, s[LO + 1]);
        out[kk] = pg.at(k, p, WT ? wl[k] : 0.f, DC ? cf[2 * k] : 0.f, DC ? cf[2 * k + 1] : 0.f, lq);
      }
    }
    __syncthreads();
    scatter_x<NT>(g, f, kn, KS);
    __syncthreads();
    // the next slice's pass 1 writes G only, and H1 is written again after the barrier that follows it
    scatter_y_store<NT>(g, f, k0, kn, KS, (DC || LV) ? 1.f : f0, dlg);
  }
}

template <bool PSEUDO, int KW>
__global__ void upsample_argmax_kernel(UpGeom g, const float* __restrict__ lg, uint8_t* __restrict__ labels, int64_t* __restrict__ mask,
                                       int n_base) {
  const long long total = (long long)g.B * g.H * g.W;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    if (PSEUDO && mask[i] != 0) continue;
    const int X = (int)(i % g.W); const long long r = i / g.W;
    const int Y = (int)(r % g.H), b = (int)(r / g.H);
    float v[KW];
    pixel_logits<KW>(g, lg, b, Y, X, v);
    int best = 0; float bv = v[0];
#pragma unroll
    for (int k = 1; k < KW; ++k) if (k < g.K && v[k] > bv) { bv = v[k]; best = k; }   // first maximum wins (torch.argmax)
    if (PSEUDO) mask[i] = best > 0 ? best + n_base : 0;
    else labels[i] = (uint8_t)best;
  }
}

// probability-map dump of eval_base.py:168,189-190: the full-resolution logits F.interpolate(align_corners=True) produced, NCHW float
template <int KW>
__global__ void upsample_logits_kernel(UpGeom g, const float* __restrict__ lg, float* __restrict__ out) {
  const long long total = (long long)g.B * g.H * g.W;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int X = (int)(i % g.W); const long long r = i / g.W;
    const int Y = (int)(r % g.H), b = (int)(r / g.H);
    float v[KW];
    pixel_logits<KW>(g, lg, b, Y, X, v);
    const size_t plane = (size_t)g.H * g.W;
#pragma unroll
    for (int k = 0; k < KW; ++k) if (k < g.K) out[((size_t)b * g.K + k) * plane + (size_t)Y * g.W + X] = v[k];
  }
}

// Test-time augmentation (sl_tta_fuse): the views of ONE model -- scales, each plain and flipped -- fused on the label grid.  TtaViews is SlTtaViews as the kernel takes it
// by value (no device table, no copy): the pointers and sizes of the views plus what the host works out once, the align_corners scales and the weight sum (list order).
struct TtaViews { int n; float wsum; const float* lg[SL_TTA_MAX_VIEWS]; int h[SL_TTA_MAX_VIEWS], w[SL_TTA_MAX_VIEWS], flip[SL_TTA_MAX_VIEWS]; float sy[SL_TTA_MAX_VIEWS], sx[SL_TTA_MAX_VIEWS], wt[SL_TTA_MAX_VIEWS]; };

// One thread per output pixel, the views in a runtime loop (the view index is wave-uniform: the view's parameters are scalar loads from the kernel arguments).  A flipped view is read
// at the mirrored pixel -- torch.flip(F.interpolate(l, (H, W), align_corners=True)) is an index remap of pixel_logits, not a second interpolation.  mode 0: t = fuse_softmax
// of the sample, mode 1: t = the sample.  fused_k = (sum_i wt_i t_ik) / wsum (fuse_accumulate, fuse_finish).  fused may be null: then one byte per pixel is all that is written.
template <int KW>
__global__ __launch_bounds__(256) void tta_fuse_kernel(TtaViews a, int B, int K, int H, int W, int mode, uint8_t* __restrict__ labels, float* __restrict__ fused) {
  const long long total = (long long)B * H * W;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += gridDim.x * 256LL) {
    const int X = (int)(i % W); const long long r = i / W;
    const int Y = (int)(r % H), b = (int)(r / H);
    float acc[KW];
    for (int n = 0; n < a.n; ++n) {
      UpGeom g; g.B = B; g.K = K; g.h = a.h[n]; g.w = a.w[n]; g.H = H; g.W = W; g.sy = a.sy[n]; g.sx = a.sx[n];
      const int f = a.flip[n];
      const float wt = a.wt[n];
      float v[KW];
      pixel_logits<KW>(g, a.lg[n], b, (f & 2) ? H - 1 - Y : Y, (f & 1) ? W - 1 - X : X, v);
      if (mode == 0) fuse_softmax<KW>(K, v);
      fuse_accumulate<KW>(n == 0, wt, v, acc);
    }
    const size_t plane = (size_t)H * W;
    labels[i] = fuse_finish<KW>(K, acc, a.wsum, fused, (size_t)b * K, plane, (size_t)Y * W + X);
  }
}

// Sliding-window inference (sl_slide_fuse): the overlapping windows of ONE scene batch fused on the scene grid.  The grid of one side of length L with crop c and stride s
// (1 <= s <= c): window side c' = min(c, L), n = max(L - c' + s - 1, 0) / s + 1 windows, window i at min(i * s, L - c') -- the last one is shifted back to end at the border.
__host__ inline long long slide_count(long long L, long long c, long long s) {
  const long long cs = c < L ? c : L, span = L - cs + s - 1;
  return (span > 0 ? span : 0) / s + 1;
}
// SlideGeom is SlSlide as the kernel takes it by value: c = the window side (the crop clamped to the scene), s = the stride, n = the window count per side, and the
// align_corners scales from h x w to the window, worked out once on the host.
struct SlideGeom { int B, K, H, W, h, w, ch, cw, sh, sw, ny, nx, mode, blend; float sy, sx; };

// The windows of one side that cover coordinate P, lo..hi: the offsets are monotone, so the covering set is a contiguous index range and no window is searched for.  Every
// window but the last sits at i * s, and (n - 2) * s < L - c <= (n - 1) * s.  hi, the last offset <= P: the shifted last window from P = L - c on, else P / s (<= n - 2).
// lo, the first offset > P - c: with t = P - c + 1 > 0 the first i with i * s >= t, which is at most n - 1 because t <= L - c.
__device__ __forceinline__ void slide_cover(int P, int L, int c, int s, int n, int& lo, int& hi) {
  hi = P >= L - c ? n - 1 : P / s;
  const int t = P - c + 1;
  lo = t > 0 ? min((t + s - 1) / s, n - 1) : 0;
}

// One thread per output pixel; its covering windows in ascending (iy, ix) order, ix innermost, each sampled with pixel_logits at the local pixel (the window's logits are
// "image" (b * ny + iy) * nx + ix of an h x w -> ch x cw upsampling).  mode 0: t = fuse_softmax of the sample, mode 1: t = the interpolated logits.  blend 0: wt = 1,
// blend 1: wt = min(y + 1, ch - y) * min(x + 1, cw - x) on the local pixel (an exact integer in float).  den is the sum of wt taken as fuse_accumulate takes acc;
// fused_k = acc_k / den (fuse_finish).  v and acc stay in registers: no LDS, no atomics.  fused may be null: then one byte per pixel is all that is written.
template <int KW>
__global__ __launch_bounds__(256) void slide_fuse_kernel(SlideGeom a, const float* __restrict__ lg, uint8_t* __restrict__ labels, float* __restrict__ fused) {
  UpGeom g; g.B = a.B * a.ny * a.nx; g.K = a.K; g.h = a.h; g.w = a.w; g.H = a.ch; g.W = a.cw; g.sy = a.sy; g.sx = a.sx;
  const int K = a.K;
  const long long total = (long long)a.B * a.H * a.W;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += gridDim.x * 256LL) {
    const int X = (int)(i % a.W); const long long r = i / a.W;
    const int Y = (int)(r % a.H), b = (int)(r / a.H);
    int iy0, iy1, ix0, ix1;
    slide_cover(Y, a.H, a.ch, a.sh, a.ny, iy0, iy1);
    slide_cover(X, a.W, a.cw, a.sw, a.nx, ix0, ix1);
    float acc[KW];
    float den = 0.f;
    bool first = true;
    for (int iy = iy0; iy <= iy1; ++iy) {
      const int y = Y - min(iy * a.sh, a.H - a.ch);
      for (int ix = ix0; ix <= ix1; ++ix) {
        const int x = X - min(ix * a.sw, a.W - a.cw);
        float v[KW];
        pixel_logits<KW>(g, lg, (b * a.ny + iy) * a.nx + ix, y, x, v);
        if (a.mode == SL_SLIDE_PROB) fuse_softmax<KW>(K, v);
        const float wt = a.blend == SL_SLIDE_TENT ? (float)min(y + 1, a.ch - y) * (float)min(x + 1, a.cw - x) : 1.f;
        fuse_accumulate<KW>(first, wt, v, acc);
        den = first ? wt : den + wt;
        first = false;
      }
    }
    const size_t plane = (size_t)a.H * a.W;
    labels[i] = fuse_finish<KW>(K, acc, den, fused, (size_t)b * K, plane, (size_t)Y * a.W + X);
  }
}

// fusemat.py:35-52: mats[idx] += prob in list order, argmax(mat / n, axis=0): float sum in the same order, first maximum wins (np.argmax)
__global__ void fuse_argmax_kernel(const float* const* __restrict__ mats, int n, int K, long long hw, uint8_t* __restrict__ out) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < hw; i += (long long)gridDim.x * blockDim.x) {
    int best = 0; float bv = 0.f;
    for (int k = 0; k < K; ++k) {
      float s = mats[0][(size_t)k * hw + i];
      for (int m = 1; m < n; ++m) s += mats[m][(size_t)k * hw + i];
      s = s / (float)n;
      if (k == 0 || s > bv) { bv = s; best = k; }
    }
    out[i] = (uint8_t)best;
  }
}

__global__ __launch_bounds__(256) void iou_hist_kernel(const uint8_t* __restrict__ pred, const int64_t* __restrict__ tgt, long long n, int K,
                                                       int ignore, unsigned long long* __restrict__ hist) {
  __shared__ unsigned int h[3 * 256];
  for (int i = threadIdx.x; i < 3 * K; i += 256) h[i] = 0;
  __syncthreads();
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n; i += gridDim.x * 256LL) {
    const long long t = tgt[i];
    if (t == ignore) continue;                       // output[target == ignore] = ignore: contributes to no bin
    const int p = pred[i];
    if (p < K) atomicAdd(&h[K + p], 1u);
    if (t >= 0 && t < K) { atomicAdd(&h[2 * K + (int)t], 1u); if (p == (int)t) atomicAdd(&h[p], 1u); }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 3 * K; i += 256) if (h[i]) atomicAdd(&hist[i], (unsigned long long)h[i]);
}

// cm[t][p] += 1 for every pixel whose label t != ignore (utils/pyt_utils.py:182-200 get_confusion_matrix over the kept pixels);
// labels outside [0, K) are skipped (the reference would fold them into a neighbouring bin through t*K + p -- they cannot occur:
// the eval drivers filter ignore first and K covers every class).
__global__ __launch_bounds__(256) void confusion_kernel(const uint8_t* __restrict__ pred, const int64_t* __restrict__ tgt, long long n, int K,
                                                        int ignore, unsigned long long* __restrict__ cm) {
  extern __shared__ unsigned int hc[];
  for (int i = threadIdx.x; i < K * K; i += 256) hc[i] = 0;
  __syncthreads();
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n; i += gridDim.x * 256LL) {
    const long long t = tgt[i];
    if (t == ignore || t < 0 || t >= K) continue;
    const int p = pred[i];
    if (p < K) atomicAdd(&hc[(int)t * K + p], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < K * K; i += 256) if (hc[i]) atomicAdd(&cm[i], (unsigned long long)hc[i]);
}

// Boundary IoU (Cheng et al.) and trimap counts of sl_boundary_counts; the contract is in include/segland_hip.h.  One block per BD_TILE x BD_TILE output tile of one
// image.  The band test "some label in the (2d+1)^2 square differs from the centre" is separable, and with one bit per pair of neighbours it needs no loop over d:
//   row pass     lane = column.  e(c) = [L(r,c) != L(r,c+1)] over the RW = BD_TILE + 2d columns of region row r is two ballots (128 bits); the 2d bits from x on are zero
//                iff the row window [x, x+2d] of the region, centred on tile column x, holds one label.  v(r,x) = centre label | BD_MIX if it does not.
//   column pass  lane = row.  g(r) = [v(r,x) != v(r+1,x) or either carries BD_MIX] down column x is two ballots again; the 2d bits from y on are zero iff the square
//                around tile pixel (y,x) holds one label: the pixel is in the band iff they are not.  The centre label is v(y+d,x) without BD_MIX.
// Positions outside the image carry BD_OUT, so crossing the image edge is a difference like any other, and a block reads its own image only.  Labels are bytes:
// 0..63 a class, BD_IGN, BD_OUT (all below BD_MIX).  The T region is loaded first and run through the row pass, then every thread turns ITS bytes of the region into
// P in place (P = BD_IGN where T is): one region buffer serves both maps.  Dynamic LDS at d = 32, K = 64: histogram (3K + K^2) x 4 = 17 152 B, region 128 x 128 =
// 16 384 B, two v arrays 128 x BD_VP = 17 408 B: 50 944 B, below the 64 KiB that need no opt-in.  At d = 3, K = 12: 720 + 5 040 + 9 520 = 15 280 B, and the 32 waves of
// a CU, not the LDS, bound the blocks per CU.  Only band pixels touch the histogram.  Integer atomics throughout: the sums do not depend on the block order.
constexpr int BD_TILE = 64;            // a wave's 64 lanes are the columns of a tile row (row pass) and the rows of a tile column (column pass)
constexpr int BD_VP = BD_TILE + 4;     // pitch of v in bytes: 17 words, so the column pass (lane = row) reads 32 different banks per lane group
constexpr int BD_DMAX = 32;            // 2d <= 64: a window's pair bits fit one 64-bit word cut out of the two ballots
constexpr int BD_IGN = 64, BD_OUT = 65, BD_MIX = 0x80;

// bits [i, i + 2d) of the 128-bit word (hi, lo), i in [0, 64): any set?  mask = the low 2d bits.
__device__ __forceinline__ bool bd_window(unsigned long long lo, unsigned long long hi, int i, unsigned long long mask) {
  const unsigned long long w = (lo >> i) | (i ? hi << (64 - i) : 0ull);
  return (w & mask) != 0ull;
}

__device__ __forceinline__ void bd_row_pass(const uint8_t* __restrict__ reg, uint8_t* __restrict__ v, int RW, int RP, int d, unsigned long long mask) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int r = wave; r < RW; r += 4) {                              // the region is square: RW rows too
    const uint8_t* row = reg + r * RP;
    const unsigned long long lo = __ballot(row[lane] != row[lane + 1]);                                         // RW >= 66: column lane + 1 exists
    const unsigned long long hi = __ballot(lane + 65 < RW && row[lane + 64] != row[lane + 65]);
    v[r * BD_VP + lane] = (uint8_t)(row[lane + d] | (bd_window(lo, hi, lane, mask) ? BD_MIX : 0));
  }
}

__device__ __forceinline__ bool bd_pair(const uint8_t* __restrict__ v, int r, int x) {
  const int a = v[r * BD_VP + x], b = v[(r + 1) * BD_VP + x];
  return a != b || ((a | b) & BD_MIX);
}

__global__ __launch_bounds__(256) void boundary_counts_kernel(const uint8_t* __restrict__ pred, const int64_t* __restrict__ tgt, int H, int W, int K, int ignore, int d,
                                                              int tiles_x, int tiles_y, unsigned long long* __restrict__ counts,
                                                              unsigned long long* __restrict__ band_cm) {
  extern __shared__ unsigned int bd_lds[];
  const int nh = 3 * K + K * K, RW = BD_TILE + 2 * d, RP = (RW + 3) & ~3;
  unsigned int* hb = bd_lds;                                         // [3][K] counts, then [K][K] band_cm
  uint8_t* reg = (uint8_t*)(hb + nh);                                // [RW][RP]
  uint8_t* vT = reg + RW * RP;                                       // [RW][BD_VP]
  uint8_t* vP = vT + RW * BD_VP;
  int tile = blockIdx.x;
  const int tx = tile % tiles_x; tile /= tiles_x;
  const int ty = tile % tiles_y, b = tile / tiles_y;
  const int x0 = tx * BD_TILE - d, y0 = ty * BD_TILE - d;            // image position of region (0, 0)
  const size_t img = (size_t)b * H * W;
  const unsigned long long mask = 2 * d == 64 ? ~0ull : (1ull << (2 * d)) - 1ull;
  for (int i = threadIdx.x; i < nh; i += 256) hb[i] = 0;
  for (int i = threadIdx.x; i < RW * RW; i += 256) {
    const int r = i / RW, c = i - r * RW, gy = y0 + r, gx = x0 + c;
    int code = BD_OUT;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
      const long long t = tgt[img + (size_t)gy * W + gx];
      code = (t >= 0 && t < K && t != ignore) ? (int)t : BD_IGN;
    }
    reg[r * RP + c] = (uint8_t)code;
  }
  __syncthreads();
  bd_row_pass(reg, vT, RW, RP, d, mask);
  __syncthreads();
  for (int i = threadIdx.x; i < RW * RW; i += 256) {                 // the same thread owns the same bytes as above: T -> P in place
    const int r = i / RW, c = i - r * RW, gy = y0 + r, gx = x0 + c;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
      const int p = pred[img + (size_t)gy * W + gx];
      if (reg[r * RP + c] == BD_IGN || p >= K) reg[r * RP + c] = BD_IGN; else reg[r * RP + c] = (uint8_t)p;
    }
  }
  __syncthreads();
  bd_row_pass(reg, vP, RW, RP, d, mask);
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  // x and the loop bound are the same in every lane of a wave, so each iteration is entered by whole waves and the four ballots see all 64 lanes.  Everything that depends
  // on the lane (the rows past H, the ignored pixels: the `continue`s below) must stay BELOW the ballots: a lane that left before them would drop its pair bit.
  for (int x = wave; x < BD_TILE && tx * BD_TILE + x < W; x += 4) {
    const unsigned long long gl = __ballot(bd_pair(vT, lane, x)), gh = __ballot(lane + 65 < RW && bd_pair(vT, lane + 64, x));
    const unsigned long long pl = __ballot(bd_pair(vP, lane, x)), ph = __ballot(lane + 65 < RW && bd_pair(vP, lane + 64, x));
    if (ty * BD_TILE + lane >= H) continue;
    const int t = vT[(lane + d) * BD_VP + x] & (BD_MIX - 1), p = vP[(lane + d) * BD_VP + x] & (BD_MIX - 1);
    if (t == BD_IGN) continue;                                       // then P is BD_IGN too: the pixel is in no count
    const bool gb = bd_window(gl, gh, lane, mask), pb = bd_window(pl, ph, lane, mask);
    if (gb) {
      atomicAdd(&hb[K + t], 1u);
      if (p < K) atomicAdd(&hb[3 * K + t * K + p], 1u);
    }
    if (pb && p < K) atomicAdd(&hb[2 * K + p], 1u);
    if (gb && pb && p == t) atomicAdd(&hb[t], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nh; i += 256)
    if (hb[i]) atomicAdd(i < 3 * K ? &counts[i] : &band_cm[i - 3 * K], (unsigned long long)hb[i]);
}

template <typename T>
__global__ void masked_avg_pool_kernel(const T* __restrict__ feat, const float* __restrict__ mask, int B, int h, int w, int C, int H, int W,
                                       float sy, float sx, float* __restrict__ proto) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  float total = 0.f;
  for (int b = 0; b < B; ++b) {
    float sf = 0.f, sm = 0.f;
    for (int y = 0; y < h; ++y) {
      int y0, y1; float ly;
      src_index_ac1(y, H, sy, y0, y1, ly);
      for (int x = 0; x < w; ++x) {
        int x0, x1; float lx;
        src_index_ac1(x, W, sx, x0, x1, lx);
        const float* mb = mask + (size_t)b * H * W;
        const float m = (1.f - ly) * ((1.f - lx) * mb[y0 * W + x0] + lx * mb[y0 * W + x1]) + ly * ((1.f - lx) * mb[y1 * W + x0] + lx * mb[y1 * W + x1]);
        sf += to_f<T>(feat[((size_t)(b * h + y) * w + x) * C + c]) * m;
        sm += m;
      }
    }
    total += sf / (sm + 1e-5f);
  }
  proto[c] = total / (float)B;
}

template <typename T>
__global__ void nhwc_to_nchw_kernel(const T* __restrict__ src, float* __restrict__ dst, int B, int HW, int C) {
  const long long total = (long long)B * HW * C;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int p = (int)(i % HW); const long long r = i / HW;     // i enumerates the NCHW destination
    const int c = (int)(r % C), b = (int)(r / C);
    dst[i] = to_f<T>(src[((size_t)b * HW + p) * C + c]);
  }
}
template <typename T>
__global__ void nchw_to_nhwc_kernel(const float* __restrict__ src, T* __restrict__ dst, int B, int HW, int C) {
  const long long total = (long long)B * HW * C;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % C); const long long r = i / C;       // i enumerates the NHWC destination
    const int p = (int)(r % HW), b = (int)(r / HW);
    dst[i] = from_f<T>(src[((size_t)b * C + c) * HW + p]);
  }
}

// ---- Online hard-pixel mining (OHEM, bootstrapped cross-entropy; the contract is in include/segland_hip.h).  Three passes in front of the unchanged loss kernels:
//   1. upsample_ohem_prob_kernel: p = softmax probability of the true class of every valid pixel (the forward kernel's arithmetic), OHEM_SENTINEL elsewhere;
//   2. an exact radix select of the k-th smallest p: probabilities are non-negative floats, so their bit patterns order as unsigned integers.  OHEM_PASSES digits of 8
//      bits from the top; per digit ohem_hist_kernel counts the values under the prefix found so far (LDS histogram, then one integer global atomic per non-empty bin
//      and block) and the one-block ohem_select_kernel takes the bin that holds the k-th value.  Integer counts only: two runs give the same bits;
//   3. ohem_mine_kernel: the mined label map from the STORED p and the theta of pass 2.
// k, q, theta and the counts never leave the device (no synchronisation: capturable).
constexpr float OHEM_SENTINEL = 2.0f;                // prob of a pixel that is not valid: above every probability, so its top digit (0x40) lies above every valid one (<= 0x3f)
constexpr int OHEM_PASSES = 4, OHEM_BINS = 256;
constexpr int OHEM_TOP_VALID = 0x3f;                 // top digit of 1.0f (0x3f800000): the valid pixels are the bins 0 .. OHEM_TOP_VALID of pass 0
// workspace: unsigned hist[OHEM_PASSES][OHEM_BINS], then the select state
enum OhemState { OS_PREFIX, OS_KREM, OS_LESS, OS_N, OS_K, OS_LE_THRESH, OS_NWORDS = 8 };
constexpr int OHEM_WS_WORDS = OHEM_PASSES * OHEM_BINS + OS_NWORDS;

template <int KW>
__global__ __launch_bounds__(256) void upsample_ohem_prob_kernel(UpGeom g, const float* __restrict__ lg, const int64_t* __restrict__ tgt, int ignore, float* __restrict__ prob) {
  const long long total = (long long)g.B * g.H * g.W;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += gridDim.x * 256LL) {
    const long long t = tgt[i];
    if (t == ignore || t < 0 || t >= g.K) { prob[i] = OHEM_SENTINEL; continue; }
    const int X = (int)(i % g.W); const long long r = i / g.W;
    const int Y = (int)(r % g.H), b = (int)(r / g.H);
    float v[KW];
    pixel_logits<KW>(g, lg, b, Y, X, v);
    float vt;
    const float m = ce_max<KW>(v, (int)t, vt);
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < KW; ++k) if (k < g.K) s += expf(v[k] - m);
    prob[i] = expf(vt - m) / s;
  }
}

__global__ __launch_bounds__(256) void ohem_init_kernel(unsigned* __restrict__ ws) {
  for (int i = threadIdx.x; i < OHEM_WS_WORDS; i += 256) ws[i] = 0u;
}

// digit `pass` (8 bits, from the top) of every value whose higher digits equal the prefix selected so far; pass 0 also counts the values <= thresh
__global__ __launch_bounds__(256) void ohem_hist_kernel(const float* __restrict__ prob, long long n, int pass, float thresh, unsigned* __restrict__ ws) {
  __shared__ unsigned h[OHEM_BINS];
  __shared__ unsigned le[4];
  const int tid = threadIdx.x;
  h[tid] = 0u;
  __syncthreads();
  const int shift = 24 - 8 * pass;
  const unsigned* st = ws + OHEM_PASSES * OHEM_BINS;
  const unsigned prefix = pass ? st[OS_PREFIX] : 0u;
  const unsigned himask = pass ? 0xffffffffu << (shift + 8) : 0u;
  unsigned nle = 0u;
  for (long long i = blockIdx.x * 256LL + tid; i < n; i += gridDim.x * 256LL) {
    const float p = prob[i];
    const unsigned u = __float_as_uint(p);
    if (pass == 0) nle += p <= thresh ? 1u : 0u;       // the sentinel is above every threshold
    if ((u & himask) == prefix) atomicAdd(&h[(u >> shift) & (OHEM_BINS - 1)], 1u);
  }
  __syncthreads();
  if (h[tid]) atomicAdd(&ws[pass * OHEM_BINS + tid], h[tid]);
  if (pass == 0) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nle += __shfl_xor(nle, o, 64);
    if ((tid & 63) == 0) le[tid >> 6] = nle;
    __syncthreads();
    if (tid == 0 && le[0] + le[1] + le[2] + le[3]) atomicAdd(&ws[OHEM_PASSES * OHEM_BINS + OS_LE_THRESH], le[0] + le[1] + le[2] + le[3]);
  }
}

// One block, one thread per bin: the bin of digit `pass` that holds the k-th smallest value extends the prefix.  Pass 0 fixes n (the values below the sentinel's digit)
// and k = min(min_kept, n); the last pass has the k-th smallest value q itself and writes theta = max(thresh, q) and counts = (n, k, number of values <= theta).
// n == 0: theta = thresh, counts = 0, and the later passes find k == 0 and write nothing.
__global__ __launch_bounds__(OHEM_BINS) void ohem_select_kernel(int pass, long long min_kept, float thresh, unsigned* __restrict__ ws, float* __restrict__ theta,
                                                                long long* __restrict__ counts) {
  __shared__ unsigned inc[OHEM_BINS];
  const int tid = threadIdx.x;
  unsigned* st = ws + OHEM_PASSES * OHEM_BINS;
  const unsigned c = ws[pass * OHEM_BINS + tid];
  inc[tid] = c;
  __syncthreads();
  for (int o = 1; o < OHEM_BINS; o <<= 1) {             // inclusive prefix sums of the bins
    const unsigned a = tid >= o ? inc[tid - o] : 0u;
    __syncthreads();
    inc[tid] += a;
    __syncthreads();
  }
  const unsigned n = pass == 0 ? inc[OHEM_TOP_VALID] : st[OS_N];
  const unsigned k = pass == 0 ? (unsigned)(min_kept < (long long)n ? min_kept : (long long)n) : st[OS_K];
  const unsigned krem = pass == 0 ? k : st[OS_KREM];
  const unsigned prefix = pass == 0 ? 0u : st[OS_PREFIX], less = pass == 0 ? 0u : st[OS_LESS], le_thresh = st[OS_LE_THRESH];
  __syncthreads();                                      // every thread has read the state before one of them writes it
  const unsigned excl = inc[tid] - c;
  if (krem >= 1u && excl < krem && krem <= inc[tid]) {  // exactly one thread: its bin is not empty
    const unsigned pre = prefix | ((unsigned)tid << (24 - 8 * pass));
    st[OS_PREFIX] = pre; st[OS_KREM] = krem - excl; st[OS_LESS] = less + excl;
    if (pass == 0) { st[OS_N] = n; st[OS_K] = k; }
    if (pass == OHEM_PASSES - 1) {
      const float q = __uint_as_float(pre);
      const unsigned le_q = less + excl + c;            // values <= q: all ties at q are kept
      theta[0] = fmaxf(thresh, q);
      counts[0] = n; counts[1] = k; counts[2] = le_q > le_thresh ? le_q : le_thresh;
    }
  }
  if (pass == 0 && n == 0u && tid == 0) { theta[0] = thresh; counts[0] = 0; counts[1] = 0; counts[2] = 0; }
}

// mined = target where the stored p <= theta (the sentinel never is) and ignore elsewhere; without a valid pixel the map is the target
__global__ __launch_bounds__(256) void ohem_mine_kernel(const float* __restrict__ prob, const int64_t* __restrict__ tgt, const float* __restrict__ theta,
                                                        const long long* __restrict__ counts, long long n, int ignore, int64_t* __restrict__ mined) {
  const float th = theta[0];
  const bool none = counts[0] == 0;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n; i += gridDim.x * 256LL) mined[i] = (none || prob[i] <= th) ? tgt[i] : (int64_t)ignore;
}

// ---- Lovasz-softmax forward (the contract is in include/segland_hip.h): no sort.  The Lovasz extension does not depend on the order inside ties, so with every class's
// errors quantised to LOV_NB bins the loss and a subgradient follow from two integer histograms per class and one scan over the bins:
//   1. upsample_lovasz_hist_kernel: one softmax per valid pixel (the arithmetic of upsample_ohem_prob_kernel), one increment per class into the block's LDS histograms
//      [classes of the slice][LOV_NB][2] (foreground, background), then one integer global atomic per non-empty bin and block.  Integer sums: two runs give the same bits.
//      A block holds LOV_KC classes (64 KiB of LDS, two blocks per CU); wider K runs cdiv(K, LOV_KC) slices side by side in gridDim.y, each evaluating the softmax again.
//   2. lovasz_scan_kernel: one block per class, one thread per bin, integer suffix sums, then the Jaccard steps, the table row and the class's partial in double;
//   3. lovasz_sum_kernel: one thread adds the present classes in index order.
// workspace: unsigned hist[K][LOV_NB][2], then double part[K][2] = (sum_j centre_j dJ_c[j], class is present)
constexpr int LOV_KC = 8, LOV_HT = 512;
inline size_t lov_ws_bytes(int K) { return (size_t)K * LOV_NB * 2 * sizeof(unsigned) + (size_t)K * 2 * sizeof(double); }

__global__ __launch_bounds__(256) void lovasz_zero_kernel(unsigned* __restrict__ ws, int n) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) ws[i] = 0u;
}

template <int KW>
__global__ __launch_bounds__(LOV_HT) void upsample_lovasz_hist_kernel(UpGeom g, const float* __restrict__ lg, const int64_t* __restrict__ tgt, int ignore, unsigned* __restrict__ hist) {
  extern __shared__ unsigned lovh[];                     // [kn][LOV_NB][2]
  const int tid = threadIdx.x;
  const int k0 = blockIdx.y * LOV_KC, kn = min(LOV_KC, g.K - k0);
  for (int i = tid; i < kn * LOV_NB * 2; i += LOV_HT) lovh[i] = 0u;
  __syncthreads();
  const long long total = (long long)g.B * g.H * g.W;
  for (long long i = blockIdx.x * (long long)LOV_HT + tid; i < total; i += gridDim.x * (long long)LOV_HT) {
    const long long t = tgt[i];
    if (t == ignore || t < 0 || t >= g.K) continue;
    const int X = (int)(i % g.W); const long long r = i / g.W;
    const int Y = (int)(r % g.H), b = (int)(r / g.H);
    float v[KW];
    pixel_logits<KW>(g, lg, b, Y, X, v);
    float vt;
    const float m = ce_max<KW>(v, (int)t, vt);
    float s = 0.f, so = 0.f;
#pragma unroll
    for (int k = 0; k < KW; ++k) if (k < g.K) { v[k] = expf(v[k] - m); s += v[k]; if (k != (int)t) so += v[k]; }
#pragma unroll
    for (int k = 0; k < KW; ++k) {
      if (k >= k0 && k < k0 + kn) {                       // k0 is the same in every lane
        const bool fg = k == (int)t;
        const float e = (fg ? so : v[k]) / s;
        atomicAdd(&lovh[((k - k0) * LOV_NB + lov_bin(e)) * 2 + (fg ? 0 : 1)], 1u);
      }
    }
  }
  __syncthreads();
  unsigned* hs = hist + (size_t)k0 * LOV_NB * 2;
  for (int i = tid; i < kn * LOV_NB * 2; i += LOV_HT) if (lovh[i]) atomicAdd(&hs[i], lovh[i]);
}

// Block c, thread j = bin j.  Walking the bins from the top, f and b are the foreground and background counts of the bins >= j (inclusive suffix sums, integers):
//   J(j) = 1 - (G - f) / (G + b),  dJ[j] = J(j) - J(j + 1),  J(LOV_NB) = 0;  an empty bin has dJ == 0 exactly.  Every block counts the present classes itself (K * LOV_NB
// words from the L2) so that the table needs no second pass.
__global__ __launch_bounds__(LOV_NB) void lovasz_scan_kernel(const unsigned* __restrict__ hist, int K, float* __restrict__ tab, double* __restrict__ part) {
  __shared__ unsigned sf[LOV_NB], sb[LOV_NB];
  __shared__ double sj[LOV_NB];
  __shared__ int flag[KMAXC];
  const int c = blockIdx.x, j = threadIdx.x;
  if (j < KMAXC) flag[j] = 0;
  __syncthreads();
  for (int k = 0; k < K; ++k) if (hist[((size_t)k * LOV_NB + j) * 2]) flag[k] = 1;
  const unsigned F = hist[((size_t)c * LOV_NB + j) * 2], Bk = hist[((size_t)c * LOV_NB + j) * 2 + 1];
  sf[j] = F; sb[j] = Bk;
  __syncthreads();
  int np = 0;
  for (int k = 0; k < K; ++k) np += flag[k];
  for (int o = 1; o < LOV_NB; o <<= 1) {
    const unsigned a = j + o < LOV_NB ? sf[j + o] : 0u, d = j + o < LOV_NB ? sb[j + o] : 0u;
    __syncthreads();
    sf[j] += a; sb[j] += d;
    __syncthreads();
  }
  const unsigned G = sf[0];
  const bool present = G > 0u;
  const double J = present ? 1.0 - (double)(G - sf[j]) / ((double)G + (double)sb[j]) : 0.0;
  sj[j] = J;
  __syncthreads();
  const double dJ = J - (j + 1 < LOV_NB ? sj[j + 1] : 0.0);
  const double cnt = (double)F + (double)Bk;
  tab[(size_t)c * LOV_NB + j] = present && cnt > 0.0 ? (float)(dJ / (cnt * (double)np)) : 0.f;
  __syncthreads();
  sj[j] = present ? ((double)j + 0.5) / (double)LOV_NB * dJ : 0.0;
  __syncthreads();
  for (int o = LOV_NB / 2; o > 0; o >>= 1) {
    if (j < o) sj[j] += sj[j + o];
    __syncthreads();
  }
  if (j == 0) { part[2 * c] = sj[0]; part[2 * c + 1] = present ? 1.0 : 0.0; }
}

// out = (mean over the present classes, in index order; number of present classes); (0, 0) without one
__global__ void lovasz_sum_kernel(const double* __restrict__ part, int K, float* __restrict__ out) {
  if (threadIdx.x || blockIdx.x) return;
  double L = 0.0, np = 0.0;
  for (int c = 0; c < K; ++c) { L += part[2 * c]; np += part[2 * c + 1]; }
  out[0] = np > 0.0 ? (float)(L / np) : 0.f;
  out[1] = (float)np;
}

inline UpGeom make_up(int B, int K, int h, int w, int H, int W) {
  UpGeom g; g.B = B; g.K = K; g.h = h; g.w = w; g.H = H; g.W = W; g.sy = ac1_scale(h, H); g.sx = ac1_scale(w, W);
  return g;
}
inline int ce_blocks(long long total) { long long b = (total + 255) / 256; return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b)); }

// One launch plan for the plain (WT = false) and the weighted (WT = true) forms: which kernel runs depends on K, the scale and the hook only.
// FC (the focal forms): the same plan, rows and partial layout; gamma rides in cf.
template <bool WT, bool FC = false>
int launch_ce_fwd(const UpGeom& g, const float* logits, const int64_t* target, int ignore_index, float* partial, hipStream_t stream, CeW<WT> cw, CeF<FC> cf = CeF<FC>()) {
  const int nblk = ce_blocks((long long)g.B * g.H * g.W);
  return sl_launch("upsample_ce_fwd_kernel", g.K <= KNC ? upsample_ce_fwd_kernel<KNC, WT, FC> : upsample_ce_fwd_kernel<KMAXC, WT, FC>, dim3(nblk), dim3(256), 0, stream, g, logits, target, ignore_index, cf, partial, cw);
}

// nbs: blocks per sample of the hybrid forward (its partial buffer has B * nbs rows).  About 1024 blocks in all, a quarter of the plain forward's: a block ends in 3 K wave
// reductions and the one finalize block reads every row, so a thread takes ~16 pixels at the bench shape instead of 4.
inline int ce_dice_blocks(int B, long long hw) {
  const long long need = (hw + 255) / 256, cap = 1024 / B;
  return (int)(need < 1 ? 1 : (need > cap ? (cap < 1 ? 1 : cap) : need));
}

template <bool WT, bool FC = false>
int launch_ce_dice_fwd(const UpGeom& g, const float* logits, const int64_t* target, int ignore_index, float* partial, hipStream_t stream, CeW<WT> cw, CeF<FC> cf = CeF<FC>()) {
  const int nbs = ce_dice_blocks(g.B, (long long)g.H * g.W);
  // three per-thread accumulators per channel: a width of 8 (the bench head) keeps the kernel at twice the waves per SIMD of the width of 16
  return sl_launch("upsample_ce_dice_fwd_kernel", g.K <= 8 ? upsample_ce_dice_fwd_kernel<8, WT, FC> : g.K <= KNC ? upsample_ce_dice_fwd_kernel<KNC, WT, FC> : upsample_ce_dice_fwd_kernel<KMAXC, WT, FC>,
                   dim3((unsigned)(g.B * nbs)), dim3(256), 0, stream,
                   g, nbs, logits, target, ignore_index, partial, cw, cf);
}

// DC (the hybrid form): the tiled kernels keep 2 K coefficients more in the LDS and the channel-sliced one a fourth word per footprint pixel; the same 150 KiB limit decides
// (more slices, then the gather kernel).  loss_and_count is then the finalize's (cross-entropy, denominator, dice) and gscale holds two values.
// FC (the focal forms): two words more per footprint pixel in the channel-sliced kernel's statistics, decided by the same list and limit.
// LV (the Lovasz term): two words more per footprint pixel in the channel-sliced kernel's statistics, by the same list and limit; gscale then holds three values.
template <bool WT, bool DC = false, bool FC = false, bool LV = false>
int launch_ce_bwd(const UpGeom& g, const float* logits, const int64_t* target, const float* loss_and_count, const float* gscale, int ignore_index, float* dlogits,
                  hipStream_t stream, CeW<WT> cw, CeD<DC> cd = CeD<DC>(), CeF<FC> cf = CeF<FC>(), CeL<LV> cl = CeL<LV>()) {
  const int B = g.B, K = g.K, h = g.h, w = g.w, H = g.H, W = g.W;
  const long long cells = (long long)B * h * w;
  // tiled kernel when the joint footprint of a CT x CT cell tile fits the LDS (always for an upsampling factor <= ~12 at K <= 16); test hook sl_debug_ce_tiled(0): never
  if (g.sy > 0.f && g.sx > 0.f && g_sl_debug.ce_tiled) {
#ifndef SL_UPCE_NT
#define SL_UPCE_NT 512      // threads per block of the one-pass tiled kernel (A/B build: 256)
#endif
    const bool wide = K > KNC;
    const dim3 tiles((unsigned)(B * cdiv(h, CT) * cdiv(w, CT)));
    UpTile ut;
    ut.NYmax = (int)ceilf((float)(CT + 1) / g.sy) + 3; if (ut.NYmax > H) ut.NYmax = H;
    ut.NXmax = (int)ceilf((float)(CT + 1) / g.sx) + 3; if (ut.NXmax > W) ut.NXmax = W;
    const size_t limit = 150 * 1024;
    if (!wide) {                                     // all K channels in one pass, or not tiled
      ut.KS = K;
      const size_t lds = tile_lds_bytes(K, ut, WT, DC, FC, LV, false);
      if (lds <= limit)
        return sl_launch("upsample_ce_bwd_tiled_kernel", upsample_ce_bwd_tiled_kernel<SL_UPCE_NT, WT, DC, FC, LV>, tiles, dim3(SL_UPCE_NT), lds, stream, g, ut, logits, target, loss_and_count, gscale, ignore_index, dlogits, cw, cd, cf, cl);
    } else {
      // channel-sliced form: the fewest slices (of at most KNC channels) whose G and H1 fit next to the per-pixel statistics
      for (int ns = cdiv(K, KNC); ns <= K; ++ns) {
        ut.KS = cdiv(K, ns);
        const size_t lds = tile_lds_bytes(K, ut, WT, DC, FC, LV, true);
        if (lds > limit) continue;
        return sl_launch("upsample_ce_bwd_tiled_wide_kernel", upsample_ce_bwd_tiled_wide_kernel<512, WT, DC, FC, LV>, tiles, dim3(512), lds, stream, g, ut, logits, target, loss_and_count, gscale, ignore_index, dlogits, cw, cd, cf, cl);
      }
    }
  }
  return sl_launch("upsample_ce_bwd_kernel", K <= KNC ? upsample_ce_bwd_kernel<KNC, WT, DC, FC, LV> : upsample_ce_bwd_kernel<KMAXC, WT, DC, FC, LV>, dim3((unsigned)((cells * 4 + 255) / 256)), dim3(256), 0, stream, g, logits, target,
                   loss_and_count, gscale, ignore_index, dlogits, cw, cd, cf, cl);
}

inline CeW<true> make_cew(const float* class_weight, float label_smoothing, int K) {
  CeW<true> cw; cw.w = class_weight; cw.keep = 1.f - label_smoothing; cw.epsk = label_smoothing / (float)K;
  return cw;
}

}  // namespace

extern "C" int sl_upsample_ce_rows(int B, int H, int W) { return ce_blocks((long long)B * H * W); }

extern "C" int sl_upsample_ce_fwd(const float* logits, const int64_t* target, int B, int K, int h, int w, int H, int W,
                                  int ignore_index, float* partial, sl_stream_t stream) {
  SL_REQUIRE(logits && target && partial && B > 0 && K >= 1 && h > 0 && w > 0 && H > 0 && W > 0, "upsample_ce_fwd: bad args");
  SL_REQUIRE(K <= KMAXC, "upsample_ce_fwd: %d logit channels; this build holds at most %d", K, KMAXC);
  return launch_ce_fwd<false>(make_up(B, K, h, w, H, W), logits, target, ignore_index, partial, (hipStream_t)stream, CeW<false>());
}

// loss/criterion.py:33,51-52 with nn.CrossEntropyLoss(weight=class_weight, label_smoothing): partial[blk] = (sum of pixel numerators, sum of w_t)
extern "C" int sl_upsample_ce_weighted_fwd(const float* logits, const int64_t* target, const float* class_weight, float label_smoothing,
                                           int B, int K, int h, int w, int H, int W, int ignore_index, float* partial, sl_stream_t stream) {
  SL_REQUIRE(logits && target && partial && B > 0 && h > 0 && w > 0 && H > 0 && W > 0, "upsample_ce_weighted_fwd: bad args");
  SL_REQUIRE(K >= 1 && K <= KMAXC, "upsample_ce_weighted_fwd: %d logit channels; this build holds at most %d", K, KMAXC);
  SL_REQUIRE(class_weight, "upsample_ce_weighted_fwd: class_weight is null (K floats on the device)");
  SL_REQUIRE(label_smoothing >= 0.f && label_smoothing <= 1.f, "upsample_ce_weighted_fwd: label_smoothing %g outside [0, 1]", (double)label_smoothing);
  return launch_ce_fwd<true>(make_up(B, K, h, w, H, W), logits, target, ignore_index, partial, (hipStream_t)stream, make_cew(class_weight, label_smoothing, K));
}

extern "C" int sl_upsample_ce_finalize(const float* partial, int nblk, float* loss_and_count, sl_stream_t stream) {
  SL_REQUIRE(partial && loss_and_count && nblk > 0, "upsample_ce_finalize: bad args");
  return sl_launch("upsample_ce_finalize_kernel", upsample_ce_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partial, nblk, loss_and_count);
}

extern "C" int sl_upsample_ce_bwd(const float* logits, const int64_t* target, const float* loss_and_count, const float* gscale,
                                  int B, int K, int h, int w, int H, int W, int ignore_index, float* dlogits,
                                  sl_stream_t stream) {
  SL_REQUIRE(logits && target && loss_and_count && gscale && dlogits && K >= 1, "upsample_ce_bwd: bad args");
  SL_REQUIRE(K <= KMAXC, "upsample_ce_bwd: %d logit channels; this build holds at most %d", K, KMAXC);
  return launch_ce_bwd<false>(make_up(B, K, h, w, H, W), logits, target, loss_and_count, gscale, ignore_index, dlogits, (hipStream_t)stream, CeW<false>());
}

// loss/criterion.py:33,51-52, gradient of the weighted form: loss_and_count[1] is the weight sum of the valid pixels (from the weighted forward + finalize)
extern "C" int sl_upsample_ce_weighted_bwd(const float* logits, const int64_t* target, const float* class_weight, float label_smoothing,
                                           const float* loss_and_count, const float* gscale, int B, int K, int h, int w, int H, int W,
                                           int ignore_index, float* dlogits, sl_stream_t stream) {
  SL_REQUIRE(logits && target && loss_and_count && gscale && dlogits && B > 0 && h > 0 && w > 0 && H > 0 && W > 0, "upsample_ce_weighted_bwd: bad args");
  SL_REQUIRE(K >= 1 && K <= KMAXC, "upsample_ce_weighted_bwd: %d logit channels; this build holds at most %d", K, KMAXC);
  SL_REQUIRE(class_weight, "upsample_ce_weighted_bwd: class_weight is null (K floats on the device)");
  SL_REQUIRE(label_smoothing >= 0.f && label_smoothing <= 1.f, "upsample_ce_weighted_bwd: label_smoothing %g outside [0, 1]", (double)label_smoothing);
  return launch_ce_bwd<true>(make_up(B, K, h, w, H, W), logits, target, loss_and_count, gscale, ignore_index, dlogits, (hipStream_t)stream,
                             make_cew(class_weight, label_smoothing, K));
}

// ---- hybrid cross-entropy + soft Dice (loss/criterion.py:34).  class_weight may be null: weights of one; with label_smoothing == 0 the cross-entropy part is then the plain form.
#define SL_CE_DICE_COMMON(what)                                                                                                                  \
  SL_REQUIRE(K >= 1 && K <= KMAXC, what ": %d logit channels; this build holds at most %d", K, KMAXC);                                          \
  SL_REQUIRE(label_smoothing >= 0.f && label_smoothing <= 1.f, what ": label_smoothing %g outside [0, 1]", (double)label_smoothing);             \
  SL_REQUIRE(B > 0 && h > 0 && w > 0 && H > 0 && W > 0 && (long long)H * W < (1LL << 30), what ": bad shape")

extern "C" int sl_upsample_ce_dice_rows(int B, int H, int W) { return B > 0 && H > 0 && W > 0 ? B * ce_dice_blocks(B, (long long)H * W) : 0; }

extern "C" int sl_upsample_ce_dice_fwd(const float* logits, const int64_t* target, const float* class_weight, float label_smoothing,
                                       int B, int K, int h, int w, int H, int W, int ignore_index, float* partial, sl_stream_t stream) {
  SL_CE_DICE_COMMON("upsample_ce_dice_fwd");
  SL_REQUIRE(logits && target && partial, "upsample_ce_dice_fwd: null buffer");
  const UpGeom g = make_up(B, K, h, w, H, W);
  if (!class_weight && label_smoothing == 0.f) return launch_ce_dice_fwd<false>(g, logits, target, ignore_index, partial, (hipStream_t)stream, CeW<false>());
  return launch_ce_dice_fwd<true>(g, logits, target, ignore_index, partial, (hipStream_t)stream, make_cew(class_weight, label_smoothing, K));
}

extern "C" int sl_upsample_ce_dice_finalize(const float* partial, const float* class_weight, float smooth, int B, int K, int H, int W,
                                            float* loss3, float* coef, sl_stream_t stream) {
  SL_REQUIRE(K >= 1 && K <= KMAXC, "upsample_ce_dice_finalize: %d logit channels; this build holds at most %d", K, KMAXC);
  SL_REQUIRE(smooth > 0.f && smooth <= 3.402823466e38f, "upsample_ce_dice_finalize: smooth %g is not a finite value > 0", (double)smooth);
  SL_REQUIRE(B > 0 && H > 0 && W > 0, "upsample_ce_dice_finalize: bad shape");
  SL_REQUIRE(partial && loss3 && coef, "upsample_ce_dice_finalize: null buffer");
  return sl_launch("upsample_ce_dice_finalize_kernel", upsample_ce_dice_finalize_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, partial, B, K, ce_dice_blocks(B, (long long)H * W),
                   class_weight, (double)smooth, loss3, coef);
}

extern "C" int sl_upsample_ce_dice_bwd(const float* logits, const int64_t* target, const float* class_weight, float label_smoothing,
                                       const float* loss3, const float* coef, const float* gscale, int B, int K, int h, int w, int H, int W,
                                       int ignore_index, float* dlogits, sl_stream_t stream) {
  SL_CE_DICE_COMMON("upsample_ce_dice_bwd");
  SL_REQUIRE(logits && target && loss3 && coef && gscale && dlogits, "upsample_ce_dice_bwd: null buffer");
  const UpGeom g = make_up(B, K, h, w, H, W);
  CeD<true> cd; cd.coef = coef;
  if (!class_weight && label_smoothing == 0.f)
    return launch_ce_bwd<false, true>(g, logits, target, loss3, gscale, ignore_index, dlogits, (hipStream_t)stream, CeW<false>(), cd);
  return launch_ce_bwd<true, true>(g, logits, target, loss3, gscale, ignore_index, dlogits, (hipStream_t)stream, make_cew(class_weight, label_smoothing, K), cd);
}

// ---- focal modulation of the cross-entropy term (CeF above; the contract is in the header).  class_weight may be null: weights of one, as in the hybrid pair.
#define SL_FOCAL_COMMON(what)                                                                                                                       \
  SL_CE_DICE_COMMON(what);                                                                                                                          \
  SL_REQUIRE(gamma >= 1.f && gamma <= 3.402823466e38f, what ": gamma %g is not a finite value >= 1 (u^(gamma - 1) is unbounded below 1)", (double)gamma)

inline CeF<true> make_cef(float gamma) { CeF<true> cf; cf.gamma = gamma; return cf; }

extern "C" int sl_upsample_focal_fwd(const float* logits, const int64_t* target, const float* class_weight, float label_smoothing, float gamma,
                                     int B, int K, int h, int w, int H, int W, int ignore_index, float* partial, sl_stream_t stream) {
  SL_FOCAL_COMMON("upsample_focal_fwd");
  SL_REQUIRE(logits && target && partial, "upsample_focal_fwd: null buffer");
  const UpGeom g = make_up(B, K, h, w, H, W);
  if (!class_weight && label_smoothing == 0.f) return launch_ce_fwd<false, true>(g, logits, target, ignore_index, partial, (hipStream_t)stream, CeW<false>(), make_cef(gamma));
  return launch_ce_fwd<true, true>(g, logits, target, ignore_index, partial, (hipStream_t)stream, make_cew(class_weight, label_smoothing, K), make_cef(gamma));
}

extern "C" int sl_upsample_focal_bwd(const float* logits, const int64_t* target, const float* class_weight, float label_smoothing, float gamma,
                                     const float* loss_and_count, const float* gscale, int B, int K, int h, int w, int H, int W,
                                     int ignore_index, float* dlogits, sl_stream_t stream) {
  SL_FOCAL_COMMON("upsample_focal_bwd");
  SL_REQUIRE(logits && target && loss_and_count && gscale && dlogits, "upsample_focal_bwd: null buffer");
  const UpGeom g = make_up(B, K, h, w, H, W);
  if (!class_weight && label_smoothing == 0.f)
    return launch_ce_bwd<false, false, true>(g, logits, target, loss_and_count, gscale, ignore_index, dlogits, (hipStream_t)stream, CeW<false>(), CeD<false>(), make_cef(gamma));
  return launch_ce_bwd<true, false, true>(g, logits, target, loss_and_count, gscale, ignore_index, dlogits, (hipStream_t)stream, make_cew(class_weight, label_smoothing, K),
                                          CeD<false>(), make_cef(gamma));
}

extern "C" int sl_upsample_focal_dice_fwd(const float* logits, const int64_t* target, const float* class_weight, float label_smoothing, float gamma,
                                          int B, int K, int h, int w, int H, int W, int ignore_index, float* partial, sl_stream_t stream) {
  SL_FOCAL_COMMON("upsample_focal_dice_fwd");
  SL_REQUIRE(logits && target && partial, "upsample_focal_dice_fwd: null buffer");
  const UpGeom g = make_up(B, K, h, w, H, W);
  if (!class_weight && label_smoothing == 0.f) return launch_ce_dice_fwd<false, true>(g, logits, target, ignore_index, partial, (hipStream_t)stream, CeW<false>(), make_cef(gamma));
  return launch_ce_dice_fwd<true, true>(g, logits, target, ignore_index, partial, (hipStream_t)stream, make_cew(class_weight, label_smoothing, K), make_cef(gamma));
}

extern "C" int sl_upsample_focal_dice_bwd(const float* logits, const int64_t* target, const float* class_weight, float label_smoothing, float gamma,
                                          const float* loss3, const float* coef, const float* gscale, int B, int K, int h, int w, int H, int W,
                                          int ignore_index, float* dlogits, sl_stream_t stream) {
  SL_FOCAL_COMMON("upsample_focal_dice_bwd");
  SL_REQUIRE(logits && target && loss3 && coef && gscale && dlogits, "upsample_focal_dice_bwd: null buffer");
  const UpGeom g = make_up(B, K, h, w, H, W);
  CeD<true> cd; cd.coef = coef;
  if (!class_weight && label_smoothing == 0.f)
    return launch_ce_bwd<false, true, true>(g, logits, target, loss3, gscale, ignore_index, dlogits, (hipStream_t)stream, CeW<false>(), cd, make_cef(gamma));
  return launch_ce_bwd<true, true, true>(g, logits, target, loss3, gscale, ignore_index, dlogits, (hipStream_t)stream, make_cew(class_weight, label_smoothing, K), cd, make_cef(gamma));
}

// ---- online hard-pixel mining: probability pass, exact k-th smallest selection, mined label map (the kernels above; one call of each per head)
extern "C" int sl_upsample_ohem_prob(const float* logits, const int64_t* target, int B, int K, int h, int w, int H, int W, int ignore_index, float* prob,
                                     sl_stream_t stream) {
  SL_REQUIRE(K >= 1 && K <= KMAXC, "upsample_ohem_prob: %d logit channels; this build holds at most %d", K, KMAXC);
  SL_REQUIRE(B > 0 && h > 0 && w > 0 && H > 0 && W > 0 && (long long)B * H * W < (1LL << 31), "upsample_ohem_prob: bad shape");
  SL_REQUIRE(logits && target && prob, "upsample_ohem_prob: null buffer");
  const UpGeom g = make_up(B, K, h, w, H, W);
  return sl_launch("upsample_ohem_prob_kernel", K <= KNC ? upsample_ohem_prob_kernel<KNC> : upsample_ohem_prob_kernel<KMAXC>, dim3(ce_blocks((long long)B * H * W)), dim3(256), 0,
                   (hipStream_t)stream, g, logits, target, ignore_index, prob);
}

extern "C" size_t sl_ohem_workspace(int B, int H, int W) { return B > 0 && H > 0 && W > 0 ? OHEM_WS_WORDS * sizeof(unsigned) : 0; }

extern "C" int sl_ohem_threshold(const float* prob, long long n_pix, float thresh, long long min_kept, void* workspace, size_t ws_bytes, float* theta, long long* counts,
                                 sl_stream_t stream) {
  SL_REQUIRE(thresh > 0.f && thresh <= 1.f, "ohem_threshold: thresh %g outside (0, 1]", (double)thresh);
  SL_REQUIRE(min_kept >= 1, "ohem_threshold: min_kept %lld is not >= 1", min_kept);
  SL_REQUIRE(n_pix > 0 && n_pix < (1LL << 31), "ohem_threshold: %lld pixels; one call selects among 1 to 2^31 - 1", n_pix);
  SL_REQUIRE(prob && workspace && theta && counts, "ohem_threshold: null buffer");
  SL_REQUIRE(ws_bytes >= OHEM_WS_WORDS * sizeof(unsigned), "ohem_threshold: workspace %zu < %zu (sl_ohem_workspace)", ws_bytes, OHEM_WS_WORDS * sizeof(unsigned));
  unsigned* ws = (unsigned*)workspace;
  const hipStream_t s = (hipStream_t)stream;
  // 8 values per thread: a block ends in up to OHEM_BINS global atomics
  const long long nb = (n_pix + 2047) / 2048;
  const dim3 grid((unsigned)(nb < 1 ? 1 : (nb > 1024 ? 1024 : nb)));
  SL_TRY(sl_launch("ohem_init_kernel", ohem_init_kernel, dim3(1), dim3(256), 0, s, ws));
  for (int pass = 0; pass < OHEM_PASSES; ++pass) {
    SL_TRY(sl_launch("ohem_hist_kernel", ohem_hist_kernel, grid, dim3(256), 0, s, prob, n_pix, pass, thresh, ws));
    SL_TRY(sl_launch("ohem_select_kernel", ohem_select_kernel, dim3(1), dim3(OHEM_BINS), 0, s, pass, min_kept, thresh, ws, theta, counts));
  }
  return 0;
}

extern "C" int sl_ohem_mine(const float* prob, const int64_t* target, const float* theta, const long long* counts, long long n_pix, int ignore_index, int64_t* mined,
                            sl_stream_t stream) {
  SL_REQUIRE(n_pix > 0 && n_pix < (1LL << 31), "ohem_mine: %lld pixels; one call takes 1 to 2^31 - 1", n_pix);
  SL_REQUIRE(prob && target && theta && counts && mined, "ohem_mine: null buffer");
  return sl_launch("ohem_mine_kernel", ohem_mine_kernel, dim3(ce_blocks(n_pix)), dim3(256), 0, (hipStream_t)stream, prob, target, theta, counts, n_pix, ignore_index, mined);
}

// ---- Lovasz-softmax term: histogram pass, scan, and the one backward launch for cross-entropy (plain, weighted, focal) [+ Dice] + Lovasz (the kernels above)
extern "C" int sl_lovasz_bins(void) { return LOV_NB; }

extern "C" size_t sl_lovasz_workspace(int K) { return K >= 1 && K <= KMAXC ? lov_ws_bytes(K) : 0; }

extern "C" int sl_upsample_lovasz_hist(const float* logits, const int64_t* target, int B, int K, int h, int w, int H, int W, int ignore_index, void* workspace,
                                       size_t ws_bytes, sl_stream_t stream) {
  SL_REQUIRE(K >= 1 && K <= KMAXC, "upsample_lovasz_hist: %d logit channels; this build holds at most %d", K, KMAXC);
  SL_REQUIRE(B > 0 && h > 0 && w > 0 && H > 0 && W > 0, "upsample_lovasz_hist: bad shape");
  SL_REQUIRE((long long)B * H * W < (1LL << 32), "upsample_lovasz_hist: %lld pixels; the bin counts are 32-bit, one call takes fewer than 2^32", (long long)B * H * W);
  SL_REQUIRE(logits && target && workspace, "upsample_lovasz_hist: null buffer");
  SL_REQUIRE(ws_bytes >= lov_ws_bytes(K), "upsample_lovasz_hist: workspace %zu < %zu (sl_lovasz_workspace)", ws_bytes, lov_ws_bytes(K));
  const UpGeom g = make_up(B, K, h, w, H, W);
  const hipStream_t s = (hipStream_t)stream;
  const int words = (int)(lov_ws_bytes(K) / sizeof(unsigned));
  SL_TRY(sl_launch("lovasz_zero_kernel", lovasz_zero_kernel, dim3((unsigned)cdiv(words, 256 * 8)), dim3(256), 0, s, (unsigned*)workspace, words));
  // 8 pixels per thread and at most 512 blocks per slice: a block ends in up to LOV_KC * LOV_NB * 2 global atomics
  const long long nb = ((long long)B * H * W + LOV_HT * 8 - 1) / (LOV_HT * 8);
  const dim3 grid((unsigned)(nb < 1 ? 1 : (nb > 512 ? 512 : nb)), (unsigned)cdiv(K, LOV_KC));
  const size_t lds = (size_t)(K < LOV_KC ? K : LOV_KC) * LOV_NB * 2 * sizeof(unsigned);
  return sl_launch("upsample_lovasz_hist_kernel", K <= LOV_KC ? upsample_lovasz_hist_kernel<LOV_KC> : K <= KNC ? upsample_lovasz_hist_kernel<KNC> : upsample_lovasz_hist_kernel<KMAXC>,
                   grid, dim3(LOV_HT), lds, s, g, logits, target, ignore_index, (unsigned*)workspace);
}

extern "C" int sl_lovasz_scan(const void* workspace, int K, float* out, float* table, sl_stream_t stream) {
  SL_REQUIRE(K >= 1 && K <= KMAXC, "lovasz_scan: %d classes; this build holds at most %d", K, KMAXC);
  SL_REQUIRE(workspace && out && table, "lovasz_scan: null buffer");
  const hipStream_t s = (hipStream_t)stream;
  const unsigned* hist = (const unsigned*)workspace;
  double* part = (double*)(hist + (size_t)K * LOV_NB * 2);
  SL_TRY(sl_launch("lovasz_scan_kernel", lovasz_scan_kernel, dim3((unsigned)K), dim3(LOV_NB), 0, s, hist, K, table, part));
  return sl_launch("lovasz_sum_kernel", lovasz_sum_kernel, dim3(1), dim3(64), 0, s, part, K, out);
}

extern "C" int sl_upsample_lovasz_bwd(const float* logits, const int64_t* target, const float* class_weight, float label_smoothing, float gamma, const float* loss_out,
                                      const float* coef, const float* table, const float* gscale, int B, int K, int h, int w, int H, int W, int ignore_index,
                                      float* dlogits, sl_stream_t stream) {
  SL_CE_DICE_COMMON("upsample_lovasz_bwd");
  SL_REQUIRE(gamma == 0.f || (gamma >= 1.f && gamma <= 3.402823466e38f), "upsample_lovasz_bwd: gamma %g is neither 0 (no focal modulation) nor a finite value >= 1", (double)gamma);
  SL_REQUIRE(logits && target && loss_out && table && gscale && dlogits, "upsample_lovasz_bwd: null buffer");
  const UpGeom g = make_up(B, K, h, w, H, W);
  const hipStream_t s = (hipStream_t)stream;
  const bool wt = class_weight || label_smoothing != 0.f, dc = coef != nullptr, fc = gamma != 0.f;
  CeD<true> cd; cd.coef = coef;
  CeL<true> cl; cl.tab = table;
  const CeW<true> cw = make_cew(class_weight, label_smoothing, K);
#define SL_LOV_BWD(WT, DC, FC, cw_, cd_, cf_) \
  return launch_ce_bwd<WT, DC, FC, true>(g, logits, target, loss_out, gscale, ignore_index, dlogits, s, cw_, cd_, cf_, cl)
  if (!wt && !dc && !fc) SL_LOV_BWD(false, false, false, CeW<false>(), CeD<false>(), CeF<false>());
  if (!wt && !dc && fc) SL_LOV_BWD(false, false, true, CeW<false>(), CeD<false>(), make_cef(gamma));
  if (!wt && dc && !fc) SL_LOV_BWD(false, true, false, CeW<false>(), cd, CeF<false>());
  if (!wt && dc && fc) SL_LOV_BWD(false, true, true, CeW<false>(), cd, make_cef(gamma));
  if (wt && !dc && !fc) SL_LOV_BWD(true, false, false, cw, CeD<false>(), CeF<false>());
  if (wt && !dc && fc) SL_LOV_BWD(true, false, true, cw, CeD<false>(), make_cef(gamma));
  if (wt && dc && !fc) SL_LOV_BWD(true, true, false, cw, cd, CeF<false>());
  SL_LOV_BWD(true, true, true, cw, cd, make_cef(gamma));
#undef SL_LOV_BWD
}

extern "C" int sl_pseudo_label(const float* logits, int K2, int h, int w, int64_t* mask, int B, int H, int W, int n_base,
                               sl_stream_t stream) {
  SL_REQUIRE(logits && mask && K2 >= 1 && B > 0, "pseudo_label: bad args");
  SL_REQUIRE(K2 <= KMAXC, "pseudo_label: %d logit channels; this build holds at most %d", K2, KMAXC);
  const UpGeom g = make_up(B, K2, h, w, H, W);
  return sl_launch("upsample_argmax_kernel", K2 <= KNC ? upsample_argmax_kernel<true, KNC> : upsample_argmax_kernel<true, KMAXC>, dim3(ce_blocks((long long)B * H * W)), dim3(256), 0, (hipStream_t)stream,
                   g, logits, nullptr, mask, n_base);
}

extern "C" int sl_upsample_argmax(const float* logits, int B, int K, int h, int w, int H, int W, uint8_t* labels,
                                  sl_stream_t stream) {
  SL_REQUIRE(logits && labels && K >= 1 && B > 0, "upsample_argmax: bad args");
  SL_REQUIRE(K <= KMAXC, "upsample_argmax: %d logit channels; this build holds at most %d", K, KMAXC);
  const UpGeom g = make_up(B, K, h, w, H, W);
  return sl_launch("upsample_argmax_kernel", K <= KNC ? upsample_argmax_kernel<false, KNC> : upsample_argmax_kernel<false, KMAXC>, dim3(ce_blocks((long long)B * H * W)), dim3(256), 0, (hipStream_t)stream,
                   g, logits, labels, nullptr, 0);
}

extern "C" int sl_upsample_logits(const float* logits, int B, int K, int h, int w, int H, int W, float* out, sl_stream_t stream) {
  SL_REQUIRE(logits && out && K >= 1 && B > 0, "upsample_logits: bad args");
  SL_REQUIRE(K <= KMAXC, "upsample_logits: %d logit channels; this build holds at most %d", K, KMAXC);
  const UpGeom g = make_up(B, K, h, w, H, W);
  return sl_launch("upsample_logits_kernel", K <= KNC ? upsample_logits_kernel<KNC> : upsample_logits_kernel<KMAXC>, dim3(ce_blocks((long long)B * H * W)), dim3(256), 0, (hipStream_t)stream, g, logits, out);
}

extern "C" int sl_tta_fuse(const SlTtaViews* views, int B, int K, int H, int W, int mode, uint8_t* labels, float* fused, sl_stream_t stream) {
  SL_REQUIRE(views && labels && B > 0 && H > 0 && W > 0, "tta_fuse: bad args");
  SL_REQUIRE(K >= 1 && K <= KMAXC, "tta_fuse: %d logit channels; this build holds at most %d", K, KMAXC);
  SL_REQUIRE(mode == 0 || mode == 1, "tta_fuse: mode %d is neither 0 (mean of the softmax probabilities) nor 1 (mean of the upsampled logits)", mode);
  SL_REQUIRE(views->n >= 1 && views->n <= SL_TTA_MAX_VIEWS, "tta_fuse: %d views; one call fuses 1 to %d", views->n, SL_TTA_MAX_VIEWS);
  TtaViews a = {};                                         // the unused slots stay zero: every word of the kernel argument is defined
  a.n = views->n;
  for (int i = 0; i < a.n; ++i) {
    SL_REQUIRE(views->logits[i] && views->h[i] > 0 && views->w[i] > 0, "tta_fuse: view %d: bad args", i);
    SL_REQUIRE(views->flip[i] >= 0 && views->flip[i] <= 3, "tta_fuse: view %d: flip %d outside [0, 3] (bit 0 horizontal, bit 1 vertical)", i, views->flip[i]);
    SL_REQUIRE(views->weight[i] > 0.f && views->weight[i] <= 3.402823466e38f, "tta_fuse: view %d: weight %g is not a finite value > 0", i, (double)views->weight[i]);
    a.lg[i] = views->logits[i]; a.h[i] = views->h[i]; a.w[i] = views->w[i]; a.flip[i] = views->flip[i]; a.wt[i] = views->weight[i];
    a.sy[i] = ac1_scale(a.h[i], H); a.sx[i] = ac1_scale(a.w[i], W);
    a.wsum = i == 0 ? a.wt[0] : a.wsum + a.wt[i];        // list order, term 0 starts the sum
  }
  SL_REQUIRE(a.wsum <= 3.402823466e38f, "tta_fuse: the weights sum to %g", (double)a.wsum);
  return sl_launch("tta_fuse_kernel", K <= KNC ? tta_fuse_kernel<KNC> : tta_fuse_kernel<KMAXC>, dim3(ce_blocks((long long)B * H * W)), dim3(256), 0, (hipStream_t)stream, a, B, K, H, W, mode,
                   labels, fused);
}

extern "C" int sl_slide_windows(int L, int crop, int stride) {
  if (L < 1 || crop < 1 || stride < 1 || stride > crop) return -1;
  return (int)slide_count(L, crop, stride);                 // at most L
}

extern "C" int sl_slide_fuse(const SlSlide* s, const float* logits, uint8_t* labels, float* fused, sl_stream_t stream) {
  SL_REQUIRE(s, "slide_fuse: null descriptor");
  SL_REQUIRE(logits, "slide_fuse: null logits");
  SL_REQUIRE(labels, "slide_fuse: null labels");
  SL_REQUIRE(s->B >= 1 && s->H >= 1 && s->W >= 1 && s->h >= 1 && s->w >= 1 && s->crop_h >= 1 && s->crop_w >= 1,
             "slide_fuse: B %d, H %d, W %d, h %d, w %d, crop_h %d, crop_w %d must all be at least 1", s->B, s->H, s->W, s->h, s->w, s->crop_h, s->crop_w);
  SL_REQUIRE(s->stride_h >= 1 && s->stride_h <= s->crop_h && s->stride_w >= 1 && s->stride_w <= s->crop_w,
             "slide_fuse: stride_h %d, stride_w %d outside [1, crop] (crop_h %d, crop_w %d): a stride above the crop leaves holes", s->stride_h, s->stride_w, s->crop_h, s->crop_w);
  SL_REQUIRE(s->K >= 1 && s->K <= KMAXC, "slide_fuse: %d logit channels; this build holds at most %d", s->K, KMAXC);
  SL_REQUIRE(s->mode == SL_SLIDE_PROB || s->mode == SL_SLIDE_LOGIT, "slide_fuse: mode %d is neither 0 (mean of the softmax probabilities) nor 1 (mean of the upsampled logits)", s->mode);
  SL_REQUIRE(s->blend == SL_SLIDE_UNIFORM || s->blend == SL_SLIDE_TENT, "slide_fuse: blend %d is neither 0 (uniform weights) nor 1 (tent weights)", s->blend);
  const long long ny = slide_count(s->H, s->crop_h, s->stride_h), nx = slide_count(s->W, s->crop_w, s->stride_w);       // each at most its side
  SL_REQUIRE((double)s->B * (double)ny * (double)nx <= 2147483647.0, "slide_fuse: %.0f windows (B %d x %lld x %lld) do not fit an int", (double)s->B * (double)ny * (double)nx, s->B, ny, nx);
  SlideGeom a;
  a.B = s->B; a.K = s->K; a.H = s->H; a.W = s->W; a.h = s->h; a.w = s->w; a.mode = s->mode; a.blend = s->blend;
  a.ch = s->crop_h < s->H ? s->crop_h : s->H; a.cw = s->crop_w < s->W ? s->crop_w : s->W;
  a.sh = s->stride_h; a.sw = s->stride_w; a.ny = (int)ny; a.nx = (int)nx;
  a.sy = ac1_scale(a.h, a.ch); a.sx = ac1_scale(a.w, a.cw);
  return sl_launch("slide_fuse_kernel", s->K <= KNC ? slide_fuse_kernel<KNC> : slide_fuse_kernel<KMAXC>, dim3(ce_blocks((long long)s->B * s->H * s->W)), dim3(256), 0, (hipStream_t)stream, a,
                   logits, labels, fused);
}

extern "C" int sl_fuse_argmax(const void* mats_dev, int n_models, int K, long long hw, uint8_t* labels, sl_stream_t stream) {
  SL_REQUIRE(mats_dev && labels && n_models >= 1 && K >= 1 && K <= 255 && hw > 0, "fuse_argmax: bad args");
  return sl_launch("fuse_argmax_kernel", fuse_argmax_kernel, dim3(ce_blocks(hw)), dim3(256), 0, (hipStream_t)stream, (const float* const*)mats_dev, n_models, K, hw, labels);
}

extern "C" int sl_iou_hist(const uint8_t* pred, const int64_t* target, long long n, int K, int ignore_index, long long* hist,
                           sl_stream_t stream) {
  SL_REQUIRE(pred && target && hist && n > 0 && K >= 1 && K <= 256, "iou_hist: bad args");
  return sl_launch("iou_hist_kernel", iou_hist_kernel, dim3(ce_blocks(n)), dim3(256), 0, (hipStream_t)stream, pred, target, n, K, ignore_index, (unsigned long long*)hist);
}

extern "C" int sl_confusion_matrix(const uint8_t* pred, const int64_t* target, long long n, int K, int ignore_index, long long* cm,
                                   sl_stream_t stream) {
  SL_REQUIRE(pred && target && cm && n > 0 && K >= 1 && K <= 64, "confusion_matrix: bad args");
  return sl_launch("confusion_kernel", confusion_kernel, dim3(ce_blocks(n)), dim3(256), (size_t)K * K * sizeof(unsigned), (hipStream_t)stream, pred, target, n, K, ignore_index,
                   (unsigned long long*)cm);
}

extern "C" int sl_boundary_counts(const uint8_t* pred, const int64_t* target, int B, int H, int W, int K, int ignore_index, int d, long long* counts,
                                  long long* band_cm, sl_stream_t stream) {
  SL_REQUIRE(pred && target && counts && band_cm, "boundary_counts: NULL pointer (pred %p, target %p, counts %p, band_cm %p)", (const void*)pred, (const void*)target,
             (const void*)counts, (const void*)band_cm);
  SL_REQUIRE(B >= 1 && H >= 1 && W >= 1, "boundary_counts: B %d, H %d, W %d must all be at least 1", B, H, W);
  SL_REQUIRE(K >= 1 && K <= 64, "boundary_counts: %d classes outside [1, 64]", K);
  SL_REQUIRE(d >= 1 && d <= BD_DMAX, "boundary_counts: band width %d outside [1, %d] pixels", d, BD_DMAX);
  const int tiles_x = cdiv(W, BD_TILE), tiles_y = cdiv(H, BD_TILE);
  const double blocks = (double)B * (double)tiles_x * (double)tiles_y;
  SL_REQUIRE(blocks <= 2147483647.0, "boundary_counts: %.0f tiles (B %d x %d x %d) do not fit an int", blocks, B, tiles_y, tiles_x);
  const int RW = BD_TILE + 2 * d, RP = (RW + 3) & ~3;
  const size_t lds = (size_t)(3 * K + K * K) * sizeof(unsigned) + (size_t)RW * RP + 2 * (size_t)RW * BD_VP;       // at most 50 944 B
  return sl_launch("boundary_counts_kernel", boundary_counts_kernel, dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, pred, target, H, W, K, ignore_index, d,
                   tiles_x, tiles_y, (unsigned long long*)counts, (unsigned long long*)band_cm);
}

extern "C" int sl_masked_avg_pool(int dtype, const void* feature, const float* mask, int B, int h, int w, int C, int H, int W,
                                  float* proto, sl_stream_t stream) {
  SL_REQUIRE(feature && mask && proto && B > 0 && C > 0, "masked_avg_pool: bad args");
  const float sy = ac1_scale(H, h), sx = ac1_scale(W, w);
  return sl_by_dtype(dtype, "masked_avg_pool", [&](auto t) -> int {
    using T = decltype(t);
    return sl_launch("masked_avg_pool_kernel", masked_avg_pool_kernel<T>, dim3(cdiv(C, 64)), dim3(64), 0, (hipStream_t)stream, (const T*)feature, mask, B, h, w, C, H, W, sy, sx, proto);
  });
}

extern "C" int sl_nhwc_to_nchw_f32(int dtype, const void* src, float* dst, int B, int H, int W, int C, sl_stream_t stream) {
  SL_REQUIRE(src && dst && B > 0, "nhwc_to_nchw: bad args");
  const long long total = (long long)B * H * W * C;
  const int blocks = (int)((total + 255) / 256 < 16384 ? (total + 255) / 256 : 16384);
  return sl_by_dtype(dtype, "nhwc_to_nchw", [&](auto t) -> int {
    using T = decltype(t);
    return sl_launch("nhwc_to_nchw_kernel", nhwc_to_nchw_kernel<T>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const T*)src, dst, B, H * W, C);
  });
}

extern "C" int sl_nchw_f32_to_nhwc(int dtype, const float* src, void* dst, int B, int H, int W, int C, sl_stream_t stream) {
  SL_REQUIRE(src && dst && B > 0, "nchw_to_nhwc: bad args");
  const long long total = (long long)B * H * W * C;
  const int blocks = (int)((total + 255) / 256 < 16384 ? (total + 255) / 256 : 16384);
  return sl_by_dtype(dtype, "nchw_to_nhwc", [&](auto t) -> int {
    using T = decltype(t);
    return sl_launch("nchw_to_nhwc_kernel", nchw_to_nhwc_kernel<T>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, src, (T*)dst, B, H * W, C);
  });
}
