// Normalization kernels, bf16 in/out, f32 compute, gfx950.
//
// All are HBM-bound: per guide Appendix B, loads are vectorized bf16x8
// (16 B/lane) and each op is fused with its adjacent elementwise work so the
// tensor is read once (SiLU into GroupNorm for the SDXL UNet/VAE resnets,
// affine into LayerNorm/RMSNorm).
//
// Serves: GroupNorm+SiLU — K3 VAE/UNet resnet blocks
// (reference trigger: diffusers pipelines, text_to_image.py:114-120);
// LayerNorm — Whisper/GPT blocks (hp_sweep_gpt src/model.py); RMSNorm — Llama.
#include "common.h"

// ---------------------------------------------------------------- GroupNorm(+SiLU)
// x: [N, C, H*W] contiguous (NCHW). groups divide C. One workgroup per (n, g):
// the group's slab is C/G * HW contiguous elements — two-pass (sum/sqsum, then
// normalize+affine+optional SiLU).

__global__ __launch_bounds__(256) void gn_partial_kernel(
    const short* __restrict__ X, float* __restrict__ WS, int N, int C,
    long long HW, int G, int split) {
  const int blk = blockIdx.x;
  const int ng = blk / split;
  const int sp = blk % split;
  const int n = ng / G, g = ng % G;
  const int cpg = C / G;
  const short* x = X + ((long long)n * C + (long long)g * cpg) * HW;
  long long per = (((HW + split - 1) / split) + 7) & ~7LL;  // 16B-aligned lo
  long long lo = sp * per, hi = min(HW, lo + per);
  if (lo >= HW) return;
  float s = 0.f, ss = 0.f;
  for (int c = 0; c < cpg; ++c) {
    const short* xc = x + (long long)c * HW;
    long long i = lo + (long long)threadIdx.x * 8;
    for (; i + 8 <= hi; i += 256 * 8) {
      bf16x8 v = *(const bf16x8*)&xc[i];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float f = bf2f(v[j]);
        s += f;
        ss += f * f;
      }
    }
    // ragged tail of this slice
    long long tail = hi - ((hi - lo) % 8);
    for (long long t = tail + threadIdx.x; t < hi; t += 256) {
      if (t >= lo) {
        float f = bf2f(xc[t]);
        s += f;
        ss += f * f;
      }
    }
  }
  s = wave_sum(s);
  ss = wave_sum(ss);
  if ((threadIdx.x & (WAVE - 1)) == 0) {
    atomicAdd(&WS[ng * 2], s);
    atomicAdd(&WS[ng * 2 + 1], ss);
  }
}

// The coefficient and element math of every apply kernel (gn_norm_kernel,
// gn_norm_nhwc_kernel), written with explicit fmaf so that no two of them can
// contract differently: their outputs are bit-identical for the same sums.
DEV_INLINE void gn_stats(const float* __restrict__ WS, int ng, float slab,
                         float eps, float& mean, float& rstd) {
  mean = WS[ng * 2] / slab;
  const float var = fmaf(-mean, mean, WS[ng * 2 + 1] / slab);
  rstd = rsqrtf(var + eps);
}

DEV_INLINE void gn_coeff(float gamma_c, float beta_c, float mean, float rstd,
                         float& gam, float& bet) {
  gam = gamma_c * rstd;
  bet = fmaf(-mean, gam, beta_c);
}

DEV_INLINE float gn_elem(short x, float gam, float bet, int do_silu) {
  float f = fmaf(bf2f(x), gam, bet);
  if (do_silu) f = f / (1.f + __expf(-f));
  return f;
}

__global__ __launch_bounds__(256) void gn_norm_kernel(
    const short* __restrict__ X, short* __restrict__ Y,
    const float* __restrict__ WS, const float* __restrict__ gamma,
    const float* __restrict__ beta, int N, int C, long long HW, int G,
    float eps, int do_silu, int split) {
  const int blk = blockIdx.x;
  const int ng = blk / split;
  const int sp = blk % split;
  const int n = ng / G, g = ng % G;
  const int cpg = C / G;
  const long long slab = (long long)cpg * HW;
  const short* x = X + ((long long)n * C + (long long)g * cpg) * HW;
  short* y = Y + ((long long)n * C + (long long)g * cpg) * HW;
  float mean, rstd;
  gn_stats(WS, ng, (float)slab, eps, mean, rstd);
  long long per = (((HW + split - 1) / split) + 7) & ~7LL;
  long long lo = sp * per, hi = min(HW, lo + per);
  if (lo >= HW) return;
  for (int c = 0; c < cpg; ++c) {
    const short* xc = x + (long long)c * HW;
    short* yc = y + (long long)c * HW;
    float gam, bet;
    gn_coeff(gamma[g * cpg + c], beta[g * cpg + c], mean, rstd, gam, bet);
    long long i = lo + (long long)threadIdx.x * 8;
    for (; i + 8 <= hi; i += 256 * 8) {
      bf16x8 v = *(const bf16x8*)&xc[i];
      bf16x8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = f2bf(gn_elem(v[j], gam, bet, do_silu));
      *(bf16x8*)&yc[i] = o;
    }
    long long tail = hi - ((hi - lo) % 8);
    for (long long t = tail + threadIdx.x; t < hi; t += 256) {
      if (t >= lo) yc[t] = f2bf(gn_elem(xc[t], gam, bet, do_silu));
    }
  }
}

// GroupNorm apply with an NHWC result: y[n, hw, c] from x[n, c, hw].  One
// block moves a 64-channel x 64-pixel tile through LDS, so the NCHW read is
// 16-byte vectors along hw and the NHWC write 16-byte vectors along c (the
// sequence-major layout the transformer blocks and the VAE mid attention
// take; GroupNorm to NCHW followed by a transposing copy wrote and read the
// tensor once more).  A side whose row length is no multiple of 8 (rows
// then start unaligned) moves element by element, bounds-checked.
//
// LDS image: [64 pixels][64 channels] bf16, rows padded to 33 dwords.  The
// transposed side moves one dword = a channel pair per pixel with lanes as
// (pixel group = lane / 8, channel pair = lane % 8 + 8 * wave): the 32 lanes
// of a half-wave hit 32 different banks.
#define TT 64            // tile edge, both ways
#define TT_LD (TT + 2)   // padded LDS row, bf16 elements (33 dwords)

__global__ __launch_bounds__(256) void gn_norm_nhwc_kernel(
    const short* __restrict__ X, short* __restrict__ Y,
    const float* __restrict__ WS, const float* __restrict__ gamma,
    const float* __restrict__ beta, int C, int HW, int G, float eps,
    int do_silu) {
  __shared__ alignas(16) unsigned tile[TT * TT_LD / 2];
  const int n = blockIdx.z;
  const int c0 = blockIdx.y * TT, p0 = blockIdx.x * TT;
  const int cpg = C / G;
  const int lane = threadIdx.x % WAVE, wv = threadIdx.x / WAVE;
  {
    // NCHW side: channels (ca, ca + 1), pixels pa .. pa + 7
    const int ca = c0 + 2 * (lane % 8 + 8 * wv);
    const int pl = (lane / 8) * 8, pa = p0 + pl;
    short v[2][8];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int c = ca + h;
      const short* xr = X + ((long long)n * C + c) * HW;
      if (c < C && (HW % 8) == 0 && pa < HW) {
        const bf16x8 t = *(const bf16x8*)&xr[pa];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[h][j] = t[j];
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          v[h][j] = (c < C && pa + j < HW) ? xr[pa + j] : (short)0;
      }
    }
    float gam[2], bet[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int c = min(ca + h, C - 1);
      float mean, rstd;
      gn_stats(WS, n * G + c / cpg, (float)((long long)cpg * HW), eps, mean,
               rstd);
      gn_coeff(gamma[c], beta[c], mean, rstd, gam[h], bet[h]);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const unsigned lo =
          (unsigned short)f2bf(gn_elem(v[0][j], gam[0], bet[0], do_silu));
      const unsigned hi =
          (unsigned short)f2bf(gn_elem(v[1][j], gam[1], bet[1], do_silu));
      tile[((pl + j) * TT_LD + (ca - c0)) / 2] = lo | (hi << 16);
    }
  }
  __syncthreads();
  // NHWC side: pixel pb, channels cb .. cb + 7
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int pr = threadIdx.x / 8 + 32 * i, pb = p0 + pr;
    const int cl = (threadIdx.x % 8) * 8, cb = c0 + cl;
    if (pb >= HW || cb >= C) continue;
    unsigned d[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) d[q] = tile[(pr * TT_LD + cl) / 2 + q];
    short* yr = Y + ((long long)n * HW + pb) * C;
    if ((C % 8) == 0) {
      i32x4 o = {(int)d[0], (int)d[1], (int)d[2], (int)d[3]};
      *(i32x4*)&yr[cb] = o;
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (cb + j < C) yr[cb + j] = (short)(d[j / 2] >> (16 * (j & 1)));
    }
  }
}

// fill the chip: split each (n, group) slab so total blocks >= ~1024
static int gn_split(int N, int G, long long HW) {
  int split = 1;
  while (N * G * split < 1024 && (long long)split * 2048 < HW) split *= 2;
  return split;
}

// y: [N, HW, C].  HW < 2^31 (checked by the binding).
extern "C" void groupnorm_silu_nhwc_bf16(const void* x, void* y, float* ws,
                                         const float* gamma, const float* beta,
                                         int N, int C, long long HW, int G,
                                         float eps, int do_silu,
                                         hipStream_t stream) {
  if (N == 0 || C == 0 || HW == 0) return;
  const int split = gn_split(N, G, HW);
  hipLaunchKernelGGL(gn_partial_kernel, dim3(N * G * split), dim3(256), 0,
                     stream, (const short*)x, ws, N, C, HW, G, split);
  dim3 grid((unsigned)((HW + TT - 1) / TT), (C + TT - 1) / TT, N);
  hipLaunchKernelGGL(gn_norm_nhwc_kernel, grid, dim3(256), 0, stream,
                     (const short*)x, (short*)y, ws, gamma, beta, C, (int)HW,
                     G, eps, do_silu);
}

extern "C" void groupnorm_silu_bf16(const void* x, void* y, float* ws,
                                    const float* gamma, const float* beta,
                                    int N, int C, long long HW, int G,
                                    float eps, int do_silu,
                                    hipStream_t stream) {
  const int split = gn_split(N, G, HW);
  dim3 grid(N * G * split);
  hipLaunchKernelGGL(gn_partial_kernel, grid, dim3(256), 0, stream,
                     (const short*)x, ws, N, C, HW, G, split);
  hipLaunchKernelGGL(gn_norm_kernel, grid, dim3(256), 0, stream,
                     (const short*)x, (short*)y, ws, gamma, beta, N, C, HW, G,
                     eps, do_silu, split);
}

// ---------------------------------------------------------------- LayerNorm
// x: [rows, D]; one wave per row for D<=4096 (bf16x8 loads), block = 4 rows.
//
// ln_row is the row body of layernorm_kernel and add_layernorm_kernel.  Src
// yields the row: vec(i, first) its elements i .. i+7, one(i, first) a single
// element of the tail past the last whole vector; `first` is true on the
// statistics pass, false on the normalise pass.  The first NV vectors of each
// lane stay in registers between the passes, the rest are fetched again.

struct LnSrcPlain {
  const short* x;
  DEV_INLINE bf16x8 vec(int i, bool) const { return *(const bf16x8*)&x[i]; }
  DEV_INLINE short one(int i, bool) const { return x[i]; }
};

// the row is bf16(x + y): a float add rounded once; the first visit of an
// element also stores it to s
struct LnSrcAdd {
  const short* x;
  const short* y;
  short* s;
  DEV_INLINE bf16x8 vec(int i, bool first) const {
    const bf16x8 a = *(const bf16x8*)&x[i];
    const bf16x8 b = *(const bf16x8*)&y[i];
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = f2bf(bf2f(a[j]) + bf2f(b[j]));
    if (first) *(bf16x8*)&s[i] = o;
    return o;
  }
  DEV_INLINE short one(int i, bool first) const {
    const short o = f2bf(bf2f(x[i]) + bf2f(y[i]));
    if (first) s[i] = o;
    return o;
  }
};

template <int NV, class Src>
DEV_INLINE void ln_row(const Src& src, short* __restrict__ y,
                       const float* __restrict__ gamma,
                       const float* __restrict__ beta, int D, float eps,
                       int l) {
  bf16x8 keep[NV > 0 ? NV : 1];
  float s = 0.f, ss = 0.f;
  auto stat = [&](const bf16x8& v) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float f = bf2f(v[j]);
      s += f;
      ss += f * f;
    }
  };
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int i = l * 8 + k * WAVE * 8;
    if (i + 8 <= D) {
      keep[k] = src.vec(i, true);
      stat(keep[k]);
    }
  }
  for (int i = l * 8 + NV * WAVE * 8; i + 8 <= D; i += WAVE * 8)
    stat(src.vec(i, true));
  for (int i = (D / 8) * 8 + l; i < D; i += WAVE) {
    float f = bf2f(src.one(i, true));
    s += f;
    ss += f * f;
  }
  s = wave_sum(s);
  ss = wave_sum(ss);
  float mean = s / D, var = ss / D - mean * mean;
  float rstd = rsqrtf(var + eps);
  auto norm = [&](const bf16x8& v, int i) {
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      o[j] = f2bf((bf2f(v[j]) - mean) * rstd * gamma[i + j] + beta[i + j]);
    *(bf16x8*)&y[i] = o;
  };
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int i = l * 8 + k * WAVE * 8;
    if (i + 8 <= D) norm(keep[k], i);
  }
  for (int i = l * 8 + NV * WAVE * 8; i + 8 <= D; i += WAVE * 8)
    norm(src.vec(i, false), i);
  for (int i = (D / 8) * 8 + l; i < D; i += WAVE)
    y[i] = f2bf((bf2f(src.one(i, false)) - mean) * rstd * gamma[i] + beta[i]);
}

__global__ __launch_bounds__(256) void layernorm_kernel(
    const short* __restrict__ X, short* __restrict__ Y,
    const float* __restrict__ gamma, const float* __restrict__ beta,
    long long rows, int D, float eps) {
  int w = threadIdx.x / WAVE, l = threadIdx.x % WAVE;
  long long row = (long long)blockIdx.x * 4 + w;
  if (row >= rows) return;
  ln_row<0>(LnSrcPlain{X + row * D}, Y + row * D, gamma, beta, D, eps, l);
}

extern "C" void layernorm_bf16(const void* x, void* y, const float* gamma,
                               const float* beta, long long rows, int D,
                               float eps, hipStream_t stream) {
  long long blocks = (rows + 3) / 4;
  hipLaunchKernelGGL(layernorm_kernel, dim3((unsigned)blocks), dim3(256), 0,
                     stream, (const short*)x, (short*)y, gamma, beta, rows, D,
                     eps);
}

// s = bf16(x + y) and ln = LayerNorm(s) from one read of x and y: the
// residual add of a pre-norm transformer sub-layer and the norm of the next
// one.  The statistics and the normalisation work on the rounded sum, in
// layernorm_kernel's order, so (s, ln) equals the add followed by
// layernorm_bf16 bit for bit.  NV * 512 columns of a row stay in registers.

template <int NV>
__global__ __launch_bounds__(256) void add_layernorm_kernel(
    const short* __restrict__ X, const short* __restrict__ Yin,
    short* __restrict__ S, short* __restrict__ LN,
    const float* __restrict__ gamma, const float* __restrict__ beta,
    long long rows, int D, float eps) {
  int w = threadIdx.x / WAVE, l = threadIdx.x % WAVE;
  long long row = (long long)blockIdx.x * 4 + w;
  if (row >= rows) return;
  ln_row<NV>(LnSrcAdd{X + row * D, Yin + row * D, S + row * D}, LN + row * D,
             gamma, beta, D, eps, l);
}

extern "C" void add_layernorm_bf16(const void* x, const void* y, void* s,
                                   void* ln, const float* gamma,
                                   const float* beta, long long rows, int D,
                                   float eps, hipStream_t stream) {
  if (rows == 0 || D == 0) return;
  long long blocks = (rows + 3) / 4;
  const int nv = (D / 8 + WAVE - 1) / WAVE;
#define ALN(NVV) \
  hipLaunchKernelGGL(add_layernorm_kernel<NVV>, dim3((unsigned)blocks), \
                     dim3(256), 0, stream, (const short*)x, (const short*)y, \
                     (short*)s, (short*)ln, gamma, beta, rows, D, eps)
  if (nv <= 1) ALN(1);
  else if (nv <= 2) ALN(2);
  else if (nv <= 3) ALN(3);
  else ALN(4);
#undef ALN
}

// ---------------------------------------------------------------- RMSNorm

__global__ __launch_bounds__(256) void rmsnorm_kernel(
    const short* __restrict__ X, short* __restrict__ Y,
    const float* __restrict__ gamma, long long rows, int D, float eps) {
  int w = threadIdx.x / WAVE, l = threadIdx.x % WAVE;
  long long row = (long long)blockIdx.x * 4 + w;
  if (row >= rows) return;
  const short* x = X + row * D;
  short* y = Y + row * D;
  float ss = 0.f;
  for (int i = l * 8; i + 8 <= D; i += WAVE * 8) {
    bf16x8 v = *(const bf16x8*)&x[i];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float f = bf2f(v[j]);
      ss += f * f;
    }
  }
  ss = wave_sum(ss);
  float rstd = rsqrtf(ss / D + eps);
  for (int i = l * 8; i + 8 <= D; i += WAVE * 8) {
    bf16x8 v = *(const bf16x8*)&x[i];
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = f2bf(bf2f(v[j]) * rstd * gamma[i + j]);
    *(bf16x8*)&y[i] = o;
  }
}

extern "C" void rmsnorm_bf16(const void* x, void* y, const float* gamma,
                             long long rows, int D, float eps,
                             hipStream_t stream) {
  long long blocks = (rows + 3) / 4;
  hipLaunchKernelGGL(rmsnorm_kernel, dim3((unsigned)blocks), dim3(256), 0,
                     stream, (const short*)x, (short*)y, gamma, rows, D, eps);
}


// ---- GN stats only + per-(n,c) affine coefficients (conv-fusion path) ----
// The fused conv (conv3x3.hip GN variant) applies silu(x*scale + shift)
// during its staging read, so gn_norm's full write+read pass disappears.
// scale[n*Cpad + c] = gamma[c]*rstd(n,g);  shift = beta[c] - mean*scale.

__global__ __launch_bounds__(256) void gn_coeff_kernel(
    const float* __restrict__ WS, const float* __restrict__ gamma,
    const float* __restrict__ beta, float* __restrict__ scale,
    float* __restrict__ shift, int N, int C, int Cpad, long long HW, int G,
    float eps) {
  int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N * Cpad) return;
  int n = i / Cpad, c = i % Cpad;
  if (c >= C) {
    scale[i] = 0.f;
    shift[i] = 0.f;
    return;
  }
  int cpg = C / G, g = c / cpg;
  long long slab = (long long)cpg * HW;
  float mean = WS[(n * G + g) * 2] / (float)slab;
  float var = WS[(n * G + g) * 2 + 1] / (float)slab - mean * mean;
  float rstd = rsqrtf(var + eps);
  float sc = gamma[c] * rstd;
  scale[i] = sc;
  shift[i] = beta[c] - mean * sc;
}

extern "C" void gn_conv_coeffs_bf16(const void* x, float* ws,
                                    const float* gamma, const float* beta,
                                    float* scale, float* shift, int N, int C,
                                    int Cpad, long long HW, int G, float eps,
                                    hipStream_t stream) {
  const int split = gn_split(N, G, HW);
  hipLaunchKernelGGL(gn_partial_kernel, dim3(N * G * split), dim3(256), 0,
                     stream, (const short*)x, ws, N, C, HW, G, split);
  hipLaunchKernelGGL(gn_coeff_kernel, dim3((N * Cpad + 255) / 256), dim3(256),
                     0, stream, ws, gamma, beta, scale, shift, N, C, Cpad, HW,
                     G, eps);
}
