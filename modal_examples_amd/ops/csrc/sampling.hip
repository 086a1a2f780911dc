// Fused LLM sampling, gfx950.  Serves K8: logits → token
// without materializing softmax (reference trigger: the generate loops of
// transformers/vLLM at batched_whisper.py:133, vllm_inference.py:158-209, and
// the explicit sampling loop at hp_sweep_gpt/src/model.py:148-157).
//
// Gumbel-max trick: argmax(logits/T + G_i), G_i = -log(-log(u_i)) samples the
// softmax(logits/T) distribution in ONE read of the logits row — no max pass,
// no sum pass, no CDF scan over a 128k vocab.  u_i comes from a counter-based
// hash (philox-lite) of (seed, row, i) → deterministic per seed. T=0 → argmax:
// "greedy" is its own flag — every seed value, 0 included, samples at T > 0.
#include "common.h"

#define SMP_BLOCK 256

DEV_INLINE unsigned int hash3(unsigned int a, unsigned int b, unsigned int c) {
  // xxhash-style avalanche mix of three words
  unsigned int h = a * 0x9E3779B1u ^ b * 0x85EBCA77u ^ c * 0xC2B2AE3Du;
  h ^= h >> 15;
  h *= 0x2C1B3C6Du;
  h ^= h >> 12;
  h *= 0x297A2D39u;
  h ^= h >> 15;
  return h;
}

__global__ __launch_bounds__(SMP_BLOCK) void gumbel_sample_kernel(
    const float* __restrict__ Logits,  // [rows, V] f32 (final-layer output)
    unsigned long long* __restrict__ Keys,  // [rows] packed argmax workspace
    int rows, int V, int splits, float inv_temp, unsigned long long seed,
    int greedy) {
  int row = blockIdx.x / splits;
  int split = blockIdx.x % splits;
  if (row >= rows) return;
  const float* lg = Logits + (long long)row * V;
  int chunk = (V + splits - 1) / splits;
  int lo = split * chunk, hi = min(V, lo + chunk);
  float best = -1e30f;
  int best_i = lo;
  for (int i = lo + threadIdx.x; i < hi; i += SMP_BLOCK) {
    float s = lg[i] * inv_temp;
    if (!greedy) {
      unsigned int u = hash3((unsigned int)seed, (unsigned int)(seed >> 32) ^ row, i);
      float uf = (u >> 8) * (1.f / 16777216.f) + 1e-10f;
      s += -__logf(-__logf(uf));
    }
    if (s > best || (s == best && i < best_i)) {
      best = s;
      best_i = i;
    }
  }
#pragma unroll
  for (int s_ = 1; s_ < WAVE; s_ <<= 1) {
    float ov = __shfl_xor(best, s_, WAVE);
    int oi = __shfl_xor(best_i, s_, WAVE);
    if (ov > best || (ov == best && oi < best_i)) {
      best = ov;
      best_i = oi;
    }
  }
  __shared__ float sv[SMP_BLOCK / WAVE];
  __shared__ int si[SMP_BLOCK / WAVE];
  int w = threadIdx.x / WAVE;
  if (threadIdx.x % WAVE == 0) {
    sv[w] = best;
    si[w] = best_i;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int j = 1; j < SMP_BLOCK / WAVE; ++j)
      if (sv[j] > best || (sv[j] == best && si[j] < best_i)) {
        best = sv[j];
        best_i = si[j];
      }
    // pack (orderable float, ~idx) so atomicMax picks max value, min index.
    // -0.0 == +0.0 in the compares above, so it must not order below +0.0
    // here either: two splits whose maxima are zeros of unlike sign tie.
    unsigned int ub = __float_as_uint(best);
    if ((ub << 1) == 0u) ub = 0u;
    ub = (ub & 0x80000000u) ? ~ub : (ub | 0x80000000u);
    unsigned long long key =
        ((unsigned long long)ub << 32) | (unsigned int)(~best_i);
    atomicMax(Keys + row, key);
  }
}

__global__ void gumbel_unpack_kernel(const unsigned long long* __restrict__ Keys,
                                     int* __restrict__ Out, int rows) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < rows) Out[i] = (int)(~(unsigned int)(Keys[i] & 0xFFFFFFFFull));
}

extern "C" void gumbel_sample(const float* logits, unsigned long long* keys,
                              int* out, int rows, int V, float temperature,
                              unsigned long long seed, hipStream_t stream) {
  const int greedy = temperature > 0.f ? 0 : 1;
  float inv_t = greedy ? 1.f : 1.f / temperature;
  // fill the chip: aim for >=512 blocks (256 CUs), split each row's vocab
  int splits = 1;
  while (rows * splits < 512 && splits * SMP_BLOCK * 4 < V) splits *= 2;
  hipLaunchKernelGGL(gumbel_sample_kernel, dim3(rows * splits),
                     dim3(SMP_BLOCK), 0, stream, logits, keys, rows, V, splits,
                     inv_t, seed, greedy);
  hipLaunchKernelGGL(gumbel_unpack_kernel, dim3((rows + 255) / 256), dim3(256),
                     0, stream, keys, out, rows);
}

// ---------------------------------------------------------------- row softmax
// Plain row softmax (f32 in/out) for probability outputs / tests: online
// single-pass per wave using running max+sum, then a normalize pass.

__global__ __launch_bounds__(SMP_BLOCK) void softmax_rows_kernel(
    const float* __restrict__ X, float* __restrict__ Y, int rows, int V) {
  int row = blockIdx.x;
  if (row >= rows) return;
  const float* x = X + (long long)row * V;
  float* y = Y + (long long)row * V;
  float m = -1e30f, l = 0.f;
  for (int i = threadIdx.x; i < V; i += SMP_BLOCK) {
    float v = x[i];
    float m_new = fmaxf(m, v);
    l = l * __expf(m - m_new) + __expf(v - m_new);
    m = m_new;
  }
  // block-combine (m, l)
  __shared__ float sm[SMP_BLOCK / WAVE], sl[SMP_BLOCK / WAVE];
#pragma unroll
  for (int s_ = 1; s_ < WAVE; s_ <<= 1) {
    float om = __shfl_xor(m, s_, WAVE);
    float ol = __shfl_xor(l, s_, WAVE);
    float mn = fmaxf(m, om);
    l = l * __expf(m - mn) + ol * __expf(om - mn);
    m = mn;
  }
  int w = threadIdx.x / WAVE;
  if (threadIdx.x % WAVE == 0) {
    sm[w] = m;
    sl[w] = l;
  }
  __syncthreads();
  float M = sm[0], L = sl[0];
  for (int j = 1; j < SMP_BLOCK / WAVE; ++j) {
    float mn = fmaxf(M, sm[j]);
    L = L * __expf(M - mn) + sl[j] * __expf(sm[j] - mn);
    M = mn;
  }
  float inv = 1.f / L;
  for (int i = threadIdx.x; i < V; i += SMP_BLOCK)
    y[i] = __expf(x[i] - M) * inv;
}

extern "C" void softmax_rows(const float* x, float* y, int rows, int V,
                             hipStream_t stream) {
  hipLaunchKernelGGL(softmax_rows_kernel, dim3(rows), dim3(SMP_BLOCK), 0,
                     stream, x, y, rows, V);
}

// ------------------------------------------- scaled row softmax, bf16 -> bf16
// softmax((s * scale).float(), -1).to(bf16) in one pass over HBM (the VAE
// mid-attention score chunks, [16, 2048, 16384]: the four-kernel torch chain
// moves 12.8 GB per chunk, this moves 4.3).  The product is rounded to bf16
// first - `s * scale` is a bf16 tensor in the chain this replaces - then max,
// exponential and sum are fp32.  One block per row; V % 8 == 0.
//
// Rows up to SSM_NV * 2048 columns stay in registers between the read and
// the write; longer rows run an online (max, sum) pass and read the row a
// second time.

#define SSM_MAX_NV 8  // bf16x8 vectors per thread held in registers

DEV_INLINE float ssm_block_max(float v, float* sh) {
  v = wave_max(v);
  const int w = threadIdx.x / WAVE;
  if (threadIdx.x % WAVE == 0) sh[w] = v;
  __syncthreads();
  float r = sh[0];
#pragma unroll
  for (int j = 1; j < SMP_BLOCK / WAVE; ++j) r = fmaxf(r, sh[j]);
  return r;
}

DEV_INLINE float ssm_block_sum(float v, float* sh) {
  v = wave_sum(v);
  const int w = threadIdx.x / WAVE;
  if (threadIdx.x % WAVE == 0) sh[w] = v;
  __syncthreads();
  float r = sh[0];
#pragma unroll
  for (int j = 1; j < SMP_BLOCK / WAVE; ++j) r += sh[j];
  return r;
}

// the bf16-rounded product, as the float the softmax works on
DEV_INLINE float ssm_scaled(short s, float scale) {
  return bf2f(f2bf(bf2f(s) * scale));
}

template <int NV>
__global__ __launch_bounds__(SMP_BLOCK) void scaled_softmax_kernel(
    const short* __restrict__ X, short* __restrict__ Y, int V, float scale) {
  __shared__ float shm[SMP_BLOCK / WAVE], shs[SMP_BLOCK / WAVE];
  const long long row = blockIdx.x;
  const short* x = X + row * V;
  short* y = Y + row * V;
  const int nvec = V / 8;
  float f[NV][8];
  float m = -INFINITY;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int vi = k * SMP_BLOCK + threadIdx.x;
    if (vi < nvec) {
      const bf16x8 v = *(const bf16x8*)&x[vi * 8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        f[k][j] = ssm_scaled(v[j], scale);
        m = fmaxf(m, f[k][j]);
      }
    }
  }
  m = ssm_block_max(m, shm);
  float l = 0.f;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int vi = k * SMP_BLOCK + threadIdx.x;
    if (vi < nvec) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        f[k][j] = __expf(f[k][j] - m);
        l += f[k][j];
      }
    }
  }
  l = ssm_block_sum(l, shs);
  const float inv = 1.f / l;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int vi = k * SMP_BLOCK + threadIdx.x;
    if (vi < nvec) {
      bf16x8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = f2bf(f[k][j] * inv);
      *(bf16x8*)&y[vi * 8] = o;
    }
  }
}

__global__ __launch_bounds__(SMP_BLOCK) void scaled_softmax_long_kernel(
    const short* __restrict__ X, short* __restrict__ Y, int V, float scale) {
  __shared__ float shm[SMP_BLOCK / WAVE], shs[SMP_BLOCK / WAVE];
  const long long row = blockIdx.x;
  const short* x = X + row * V;
  short* y = Y + row * V;
  const int nvec = V / 8;
  float m = -INFINITY;
  for (int vi = threadIdx.x; vi < nvec; vi += SMP_BLOCK) {
    const bf16x8 v = *(const bf16x8*)&x[vi * 8];
#pragma unroll
    for (int j = 0; j < 8; ++j) m = fmaxf(m, ssm_scaled(v[j], scale));
  }
  m = ssm_block_max(m, shm);
  float l = 0.f;
  for (int vi = threadIdx.x; vi < nvec; vi += SMP_BLOCK) {
    const bf16x8 v = *(const bf16x8*)&x[vi * 8];
#pragma unroll
    for (int j = 0; j < 8; ++j) l += __expf(ssm_scaled(v[j], scale) - m);
  }
  l = ssm_block_sum(l, shs);
  const float inv = 1.f / l;
  for (int vi = threadIdx.x; vi < nvec; vi += SMP_BLOCK) {
    const bf16x8 v = *(const bf16x8*)&x[vi * 8];
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      o[j] = f2bf(__expf(ssm_scaled(v[j], scale) - m) * inv);
    *(bf16x8*)&y[vi * 8] = o;
  }
}

// x, y: [rows, V] contiguous bf16, V % 8 == 0, rows < 2^31 (checked by the
// binding).
extern "C" void scaled_softmax_bf16(const void* x, void* y, long long rows,
                                    int V, float scale, hipStream_t stream) {
  if (rows == 0 || V == 0) return;
  const int nv = (V / 8 + SMP_BLOCK - 1) / SMP_BLOCK;
#define SSM(NVV) \
  hipLaunchKernelGGL(scaled_softmax_kernel<NVV>, dim3((unsigned)rows), \
                     dim3(SMP_BLOCK), 0, stream, (const short*)x, (short*)y, \
                     V, scale)
  if (nv <= 1) SSM(1);
  else if (nv <= 2) SSM(2);
  else if (nv <= 4) SSM(4);
  else if (nv <= SSM_MAX_NV) SSM(SSM_MAX_NV);
  else
    hipLaunchKernelGGL(scaled_softmax_long_kernel, dim3((unsigned)rows),
                       dim3(SMP_BLOCK), 0, stream, (const short*)x, (short*)y,
                       V, scale);
#undef SSM
}

// ------------------------------------------------- per-row filtered sampling
// Batched sampling with per-row temperature, top-k / top-p / min-p, seed and
// counter, all read from device arrays (nothing comes back to the host).
//
// All three filters are monotone in the logit, so together they are ONE value
// threshold per row: the kept set is {i : logit_i >= cutoff}.  The cutoff
// kernel finds that threshold without sorting (radix select over the
// order-preserving unsigned image of the float, most significant digits
// first, LDS histograms); the draw kernel is the gumbel arg-max above with
// the compare `logit >= cutoff` in front.
//
// Determinism: counts are integers and probability mass is accumulated in
// fixed point (e_i * 2^32 in 64-bit integer LDS atomics), so every sum is
// associative: a row gives the bit-identical cutoff whatever its index, the
// batch around it, or the order the atomics arrive in.

#define CUT_BLOCK 1024
#define CUT_WAVES (CUT_BLOCK / WAVE)
#define CUT_BINS 4096            // 12-bit first digit, then 10 + 10
#define CUT_PER_THREAD (CUT_BINS / CUT_BLOCK)
#define CUT_NONE 0x7fffffff
#define KEY_NEG_INF 0x007FFFFFu  // fkey(-inf): every finite key is above it

// order-preserving float -> uint; -0.0 maps onto +0.0 so the zeros tie
DEV_INLINE unsigned int fkey(float x) {
  unsigned int u = __float_as_uint(x);
  if ((u << 1) == 0u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

DEV_INLINE float fkey_inv(unsigned int k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// e_i = exp(logit_i * inv_t - m), rounded step by step (no fma contraction)
// so that a host emulation reproduces it
DEV_INLINE float row_exp(float x, float inv_t, float m) {
  return expf(__fsub_rn(__fmul_rn(x, inv_t), m));
}

DEV_INLINE unsigned long long mass_fx(float e) {
  return (unsigned long long)(e * 4294967296.f);  // e in [0,1] -> <= 2^32
}

// f(x) for every element of the row; 16-byte loads where the row allows
template <class F>
DEV_INLINE void row_foreach(const float* __restrict__ lg, int V, F f) {
  if ((V & 3) == 0 && ((unsigned long long)lg & 15) == 0) {
    const float4* lg4 = reinterpret_cast<const float4*>(lg);
    const int n4 = V >> 2;
    int i = threadIdx.x;
    // one block streams the whole row: keep four loads in flight per lane
    for (; i + 3 * CUT_BLOCK < n4; i += 4 * CUT_BLOCK) {
      float4 a = lg4[i], b = lg4[i + CUT_BLOCK], c = lg4[i + 2 * CUT_BLOCK],
             d = lg4[i + 3 * CUT_BLOCK];
      f(a.x); f(a.y); f(a.z); f(a.w);
      f(b.x); f(b.y); f(b.z); f(b.w);
      f(c.x); f(c.y); f(c.z); f(c.w);
      f(d.x); f(d.y); f(d.z); f(d.w);
    }
    for (; i < n4; i += CUT_BLOCK) {
      float4 x = lg4[i];
      f(x.x);
      f(x.y);
      f(x.z);
      f(x.w);
    }
  } else {
    for (int i = threadIdx.x; i < V; i += CUT_BLOCK) f(lg[i]);
  }
}

// block-wide max / min of a u32 and sum of an int; `red` is CUT_WAVES words.
// Every thread returns the result.
DEV_INLINE unsigned int block_max_u32(unsigned int v, unsigned int* red) {
#pragma unroll
  for (int s = 1; s < WAVE; s <<= 1) v = max(v, (unsigned int)__shfl_xor((int)v, s, WAVE));
  __syncthreads();
  if (threadIdx.x % WAVE == 0) red[threadIdx.x / WAVE] = v;
  __syncthreads();
  unsigned int r = red[0];
  for (int j = 1; j < CUT_WAVES; ++j) r = max(r, red[j]);
  return r;
}

DEV_INLINE unsigned int block_min_u32(unsigned int v, unsigned int* red) {
  return ~block_max_u32(~v, red);
}

DEV_INLINE int block_sum_i32(int v, unsigned int* red) {
#pragma unroll
  for (int s = 1; s < WAVE; s <<= 1) v += __shfl_xor(v, s, WAVE);
  __syncthreads();
  if (threadIdx.x % WAVE == 0) red[threadIdx.x / WAVE] = (unsigned int)v;
  __syncthreads();
  int r = 0;
  for (int j = 0; j < CUT_WAVES; ++j) r += (int)red[j];
  return r;
}

struct CutShared {
  unsigned long long hist[CUT_BINS];
  unsigned long long wtot[CUT_WAVES];
  unsigned long long sel_above;
  int sel_bin;
  unsigned int red[CUT_WAVES];
};

// Radix select.  Over the elements with key >= kmin, each weighing 1
// (MASS = false) or its fixed-point e_i (MASS = true), return the smallest
// key v with  weight{key > v} <= limit  among keys of non-zero weight.
// MASS: limit = trunc(p * total weight), the total read off the first
// histogram.  Returns false when nothing qualifies (no finite element).
template <bool MASS>
DEV_INLINE bool radix_select(const float* __restrict__ lg, int V,
                             unsigned int kmin, float inv_t, float m,
                             unsigned long long limit, float p,
                             CutShared& sh, unsigned int* out_key) {
  unsigned int prefix = 0;
  unsigned long long above = 0;
  const int tid = threadIdx.x;
#pragma unroll 1
  for (int level = 0; level < 3; ++level) {
    const int shift = level == 0 ? 20 : level == 1 ? 10 : 0;
    const int bits = level == 0 ? 12 : 10;
    const unsigned int dmask = (1u << bits) - 1u;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < CUT_PER_THREAD; ++j) sh.hist[tid * CUT_PER_THREAD + j] = 0ull;
    if (tid == 0) sh.sel_bin = CUT_NONE;
    __syncthreads();
    row_foreach(lg, V, [&](float x) {
      unsigned int key = fkey(x);
      // (key >> shift) >> bits: a 32-bit shift is never issued at level 0
      if (key >= kmin && (level == 0 || ((key >> shift) >> bits) == prefix)) {
        unsigned long long w = MASS ? mass_fx(row_exp(x, inv_t, m)) : 1ull;
        if (w) atomicAdd(&sh.hist[(key >> shift) & dmask], w);
      }
    });
    __syncthreads();
    // suffix sums: thread t owns bins [4t, 4t+4)
    unsigned long long h[CUT_PER_THREAD];
    unsigned long long ls = 0;
#pragma unroll
    for (int j = 0; j < CUT_PER_THREAD; ++j) {
      h[j] = sh.hist[tid * CUT_PER_THREAD + j];
      ls += h[j];
    }
    unsigned long long incl = ls;  // inclusive prefix over threads
#pragma unroll
    for (int s = 1; s < WAVE; s <<= 1) {
      unsigned long long o = __shfl_up(incl, s, WAVE);
      if ((tid % WAVE) >= s) incl += o;
    }
    if (tid % WAVE == WAVE - 1) sh.wtot[tid / WAVE] = incl;
    __syncthreads();
    unsigned long long total = 0;
    for (int j = 0; j < CUT_WAVES; ++j) {
      if (j < tid / WAVE) incl += sh.wtot[j];
      total += sh.wtot[j];
    }
    if (MASS && level == 0)
      limit = (unsigned long long)((double)p * (double)total);
    // weight above this thread's highest bin, then walk its bins downwards
    unsigned long long u = above + (total - incl);
    int mine = CUT_NONE;
    unsigned long long mine_u = 0;
#pragma unroll
    for (int j = CUT_PER_THREAD - 1; j >= 0; --j) {
      if (h[j] != 0ull && u <= limit) {
        mine = tid * CUT_PER_THREAD + j;
        mine_u = u;
      }
      u += h[j];
    }
    if (mine != CUT_NONE) atomicMin(&sh.sel_bin, mine);
    __syncthreads();
    const int sel = sh.sel_bin;
    if (sel == CUT_NONE) return false;
    if (sel / CUT_PER_THREAD == tid) {
      // u <= limit is monotone, so `mine` is this thread's lowest such bin
      sh.sel_above = mine_u;
    }
    __syncthreads();
    above = sh.sel_above;
    prefix = (prefix << bits) | (unsigned int)sel;
  }
  *out_key = prefix;
  return true;
}

__global__ __launch_bounds__(CUT_BLOCK) void sampling_cutoff_kernel(
    const float* __restrict__ Logits,  // [rows, V]
    const float* __restrict__ Temps,   // [rows]
    const int* __restrict__ TopK,      // [rows] 0 or >= V: off
    const float* __restrict__ TopP,    // [rows] >= 1: off
    const float* __restrict__ MinP,    // [rows] <= 0: off
    float* __restrict__ Cut,           // [rows]
    int rows, int V) {
  __shared__ CutShared sh;
  const int row = blockIdx.x;
  if (row >= rows) return;
  const float T = Temps[row];
  const int k = TopK[row];
  const float p = TopP[row];
  const float q = MinP[row];
  const bool k_on = k > 0 && k < V;
  const bool p_on = p < 1.f;
  const bool q_on = q > 0.f;
  const float NEG_INF = __uint_as_float(0xFF800000u);
  if (!(T > 0.f) || !(k_on || p_on || q_on)) {
    if (threadIdx.x == 0) Cut[row] = NEG_INF;
    return;
  }
  const float* lg = Logits + (long long)row * V;
  const float inv_t = 1.f / T;

  // pass 0: row maximum and the number of finite logits
  unsigned int kmax = 0;
  int nfin = 0;
  row_foreach(lg, V, [&](float x) {
    unsigned int key = fkey(x);
    kmax = max(kmax, key);
    nfin += key > KEY_NEG_INF ? 1 : 0;
  });
  kmax = block_max_u32(kmax, sh.red);
  nfin = block_sum_i32(nfin, sh.red);
  if (nfin == 0 || kmax <= KEY_NEG_INF) {  // no finite logit: nothing to cut
    if (threadIdx.x == 0) Cut[row] = NEG_INF;
    return;
  }
  const float m = __fmul_rn(fkey_inv(kmax), inv_t);

  unsigned int cut = KEY_NEG_INF + 1u;  // filters never keep -inf
  bool ok = true;
  if (k_on) {
    unsigned int kk;
    int keff = min(k, nfin);
    ok = radix_select<false>(lg, V, KEY_NEG_INF + 1u, inv_t, m,
                             (unsigned long long)(keff - 1), 0.f, sh, &kk);
    if (ok) cut = max(cut, kk);
  }
  if (ok && p_on) {
    unsigned int kp;
    ok = radix_select<true>(lg, V, cut, inv_t, m, 0ull, fmaxf(p, 0.f), sh, &kp);
    if (ok) cut = max(cut, kp);
  }
  if (ok && q_on) {
    unsigned int kq = 0xFFFFFFFFu;
    row_foreach(lg, V, [&](float x) {
      unsigned int key = fkey(x);
      if (key > KEY_NEG_INF && row_exp(x, inv_t, m) >= q) kq = min(kq, key);
    });
    kq = block_min_u32(kq, sh.red);
    if (kq != 0xFFFFFFFFu) cut = max(cut, kq);
  }
  // a failed select (no usable weight, e.g. NaN input) keeps the arg-max only
  if (threadIdx.x == 0) Cut[row] = ok ? fkey_inv(cut) : fkey_inv(kmax);
}

// One split's scan of gumbel_sample_batch_kernel.  FILTER: a token below the
// cutoff scores -inf, never above `best` (a select, not a branch).
template <bool FILTER>
DEV_INLINE void gumbel_scan(const float* __restrict__ lg, int lo, int hi,
                            float inv_temp, int greedy,
                            unsigned long long seed, unsigned int ctr,
                            float cut, float& best, int& best_i) {
  for (int i = lo + threadIdx.x; i < hi; i += SMP_BLOCK) {
    float x = lg[i];
    float s = x * inv_temp;
    if (!greedy) {
      unsigned int u = hash3((unsigned int)seed, (unsigned int)(seed >> 32) ^ ctr, i);
      float uf = (u >> 8) * (1.f / 16777216.f) + 1e-10f;
      s += -__logf(-__logf(uf));
    }
    if (FILTER) s = x >= cut ? s : __uint_as_float(0xFF800000u);
    if (s > best || (s == best && i < best_i)) {
      best = s;
      best_i = i;
    }
  }
}

// The split-vocabulary gumbel arg-max of gumbel_sample_kernel with per-row
// temperature, seed, counter and cutoff.  Per-element arithmetic is the same,
// so with Cutoff = -inf and counter = row it returns the same tokens.
__global__ __launch_bounds__(SMP_BLOCK) void gumbel_sample_batch_kernel(
    const float* __restrict__ Logits,       // [rows, V]
    const float* __restrict__ Temps,        // [rows]
    const long long* __restrict__ Seeds,    // [rows]
    const long long* __restrict__ Counters, // [rows] low 32 bits used
    const float* __restrict__ Cutoff,       // [rows] or null (= -inf)
    unsigned long long* __restrict__ Keys,  // [rows] packed argmax workspace
    int rows, int V, int splits) {
  int row = blockIdx.x / splits;
  int split = blockIdx.x % splits;
  if (row >= rows) return;
  const float* lg = Logits + (long long)row * V;
  const float T = Temps[row];
  const int greedy = T > 0.f ? 0 : 1;
  const float inv_temp = greedy ? 1.f : 1.f / T;
  const unsigned long long seed = (unsigned long long)Seeds[row];
  const unsigned int ctr = (unsigned int)(unsigned long long)Counters[row];
  const float NEG_INF = __uint_as_float(0xFF800000u);
  const float cut = (Cutoff != nullptr && !greedy) ? Cutoff[row] : NEG_INF;
  int chunk = (V + splits - 1) / splits;
  int lo = split * chunk, hi = min(V, lo + chunk);
  float best = -1e30f;
  int best_i = lo;
  if (cut == NEG_INF)  // block-uniform: unfiltered rows run the plain loop
    gumbel_scan<false>(lg, lo, hi, inv_temp, greedy, seed, ctr, cut, best, best_i);
  else
    gumbel_scan<true>(lg, lo, hi, inv_temp, greedy, seed, ctr, cut, best, best_i);
#pragma unroll
  for (int s_ = 1; s_ < WAVE; s_ <<= 1) {
    float ov = __shfl_xor(best, s_, WAVE);
    int oi = __shfl_xor(best_i, s_, WAVE);
    if (ov > best || (ov == best && oi < best_i)) {
      best = ov;
      best_i = oi;
    }
  }
  __shared__ float sv[SMP_BLOCK / WAVE];
  __shared__ int si[SMP_BLOCK / WAVE];
  int w = threadIdx.x / WAVE;
  if (threadIdx.x % WAVE == 0) {
    sv[w] = best;
    si[w] = best_i;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int j = 1; j < SMP_BLOCK / WAVE; ++j)
      if (sv[j] > best || (sv[j] == best && si[j] < best_i)) {
        best = sv[j];
        best_i = si[j];
      }
    // same packing as gumbel_sample_kernel (zeros of either sign tie)
    unsigned int ub = __float_as_uint(best);
    if ((ub << 1) == 0u) ub = 0u;
    ub = (ub & 0x80000000u) ? ~ub : (ub | 0x80000000u);
    unsigned long long key =
        ((unsigned long long)ub << 32) | (unsigned int)(~best_i);
    atomicMax(Keys + row, key);
  }
}

extern "C" void sampling_cutoff(const float* logits, const float* temps,
                                const int* top_k, const float* top_p,
                                const float* min_p, float* cut, int rows,
                                int V, hipStream_t stream) {
  hipLaunchKernelGGL(sampling_cutoff_kernel, dim3(rows), dim3(CUT_BLOCK), 0,
                     stream, logits, temps, top_k, top_p, min_p, cut, rows, V);
}

extern "C" void gumbel_sample_batch(const float* logits, const float* temps,
                                    const long long* seeds,
                                    const long long* counters,
                                    const float* cutoff,
                                    unsigned long long* keys, int* out,
                                    int rows, int V, hipStream_t stream) {
  // the split rule of gumbel_sample
  int splits = 1;
  while (rows * splits < 512 && splits * SMP_BLOCK * 4 < V) splits *= 2;
  hipLaunchKernelGGL(gumbel_sample_batch_kernel, dim3(rows * splits),
                     dim3(SMP_BLOCK), 0, stream, logits, temps, seeds,
                     counters, cutoff, keys, rows, V, splits);
  hipLaunchKernelGGL(gumbel_unpack_kernel, dim3((rows + 255) / 256), dim3(256),
                     0, stream, keys, out, rows);
}
