// Fused mixture-of-experts FFN, bf16, gfx950: on-device routing, a grouped
// GEMM schedule built on the device, two MFMA grouped GEMMs and a weighted
// combine.  Nothing on the host depends on routing data — every grid and
// workspace size is a function of (N, top_k, E, dim, ffn_dim) only — so the
// whole FFN is sync-free and captures into a hipGraph.
//
//   route    logits [N,E] f32 -> idx [N,k] i32 (descending logit, ties to the
//            lower expert), weights [N,k] f32 = softmax over the k logits
//   align    idx -> per-expert segments of (token, j) pairs, each padded to
//            the 32-row M-tile so a tile belongs to one expert:
//            slot_map [tiles*32] (pair id, -1 = pad), tile_expert, num_tiles
//   up GEMM  h[slot] = silu(x[tok] . gate[e]^T) * (x[tok] . up[e]^T), the
//            SwiGLU applied to the f32 accumulators; h is bf16 [slots, F]
//   down     y[pair] = h[slot] . down[e]^T, f32 [N*k, d]
//   combine  out[t] = sum_j weights[t,j] * y[t*k+j], f32 in j order, one
//            rounding to bf16
//
// No float atomics anywhere, and each GEMM sums K in one fixed order, so an
// output row depends only on its own inputs: results are bitwise
// reproducible and independent of how rows fall into tiles.  (The integer
// atomics of align only decide which slot of its expert's segment a pair
// takes.)
//
// GEMM shape: the decode case has <= ~32 rows per expert and streams every
// weight once, so a block is ONE wave that owns a 32-row M-tile and two
// 32-column N-tiles (gate+up columns n0.. and F+n0.. in the up GEMM, 64
// adjacent columns in the down GEMM) over the whole K.  Both operands have K
// contiguous, so the 32x32x16 fragments (layouts: attention_mfma32.h) are
// plain 16 B loads straight to registers, one K-chunk ahead of the MFMAs
// (guide §5, the "GEMV / M <= 16" row: no LDS round trip for weights that
// are read once).  y is f32: 4 B * N*k*d written and read once, against
// 6 B * E*F*d of weights — 0.25 % of the bytes at N=64, and one rounding
// fewer than a bf16 y.
//
// Preconditions the device cannot report: idx values in [0,E), distinct per
// token (moe_route always produces that).  A pair with an id outside [0,E)
// is skipped by align — its y row is never written — rather than indexed.
#include "attention_mfma32.h"

#define MOE_BM 32          // rows per M-tile = one 32x32 MFMA tile
#define MOE_MAX_E 128
#define MOE_MAX_K 8
#define MOE_ALIGN_NT 1024

// ---------------------------------------------------------------- route

__global__ __launch_bounds__(256) void moe_route_kernel(
    const float* __restrict__ logits, float* __restrict__ weights,
    int* __restrict__ idx, int N, int E, int top_k) {
  int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= N) return;
  const float* row = logits + (size_t)t * E;
  unsigned long long taken_lo = 0, taken_hi = 0;  // experts already chosen
  float sel[MOE_MAX_K];
  int sid[MOE_MAX_K];
#pragma unroll
  for (int j = 0; j < MOE_MAX_K; ++j) {
    sel[j] = 0.f;
    sid[j] = 0;
    if (j < top_k) {
      // first not-yet-taken maximum: a strict > keeps the lower index on ties
      float best = 0.f;
      int bi = -1;
      for (int e = 0; e < E; ++e) {
        bool taken = ((e < 64 ? taken_lo >> e : taken_hi >> (e - 64)) & 1ull);
        float v = row[e];
        if (!taken && (bi < 0 || v > best)) {
          best = v;
          bi = e;
        }
      }
      if (bi < 64) taken_lo |= 1ull << bi;
      else taken_hi |= 1ull << (bi - 64);
      sel[j] = best;
      sid[j] = bi;
    }
  }
  float ex[MOE_MAX_K];
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < MOE_MAX_K; ++j) {
    ex[j] = j < top_k ? expf(sel[j] - sel[0]) : 0.f;
    sum += ex[j];
  }
#pragma unroll
  for (int j = 0; j < MOE_MAX_K; ++j)
    if (j < top_k) {
      weights[(size_t)t * top_k + j] = ex[j] / sum;
      idx[(size_t)t * top_k + j] = sid[j];
    }
}

// ---------------------------------------------------------------- align
// One block.  P = N*top_k pairs; max_tiles = P/32 + E bounds the tiles in
// use (sum of ceil(c_e/32) <= floor(P/32) + E), so every index written here
// stays inside slot_map [max_tiles*32] and tile_expert [max_tiles].

__global__ __launch_bounds__(MOE_ALIGN_NT) void moe_align_kernel(
    const int* __restrict__ idx, int P, int E, int* __restrict__ slot_map,
    int* __restrict__ tile_expert, int* __restrict__ num_tiles) {
  __shared__ int cnt[MOE_MAX_E], start[MOE_MAX_E], fill[MOE_MAX_E];
  const int tid = threadIdx.x;
  if (tid < MOE_MAX_E) {
    cnt[tid] = 0;
    fill[tid] = 0;
  }
  __syncthreads();
  for (int p = tid; p < P; p += MOE_ALIGN_NT) {
    int e = idx[p];
    if ((unsigned)e < (unsigned)E) atomicAdd(&cnt[e], 1);
  }
  __syncthreads();
  if (tid == 0) {
    int tile = 0;
    for (int e = 0; e < E; ++e) {
      start[e] = tile * MOE_BM;
      int nt = (cnt[e] + MOE_BM - 1) / MOE_BM;
      for (int i = 0; i < nt; ++i) tile_expert[tile + i] = e;
      tile += nt;
    }
    *num_tiles = tile;
  }
  __syncthreads();
  // the pad slots behind each expert's rows (fewer than 32 per expert)
  for (int e = tid >> 5; e < E; e += MOE_ALIGN_NT / 32) {
    int c = cnt[e];
    int end = start[e] + (c + MOE_BM - 1) / MOE_BM * MOE_BM;
    int s = start[e] + c + (tid & 31);
    if (s < end) slot_map[s] = -1;
  }
  for (int p = tid; p < P; p += MOE_ALIGN_NT) {
    int e = idx[p];
    if ((unsigned)e < (unsigned)E)
      slot_map[start[e] + atomicAdd(&fill[e], 1)] = p;
  }
}

// ---------------------------------------------------------------- grouped GEMM
// One wave per block: M-tile mtile (32 slots of one expert) x two 32-column
// N-tiles, over all of K.  UP: A rows are x rows gathered through the slot
// map (pad rows read as zero), the N-tiles are gate columns n0.. and up
// columns F+n0.., the epilogue stores silu(gate)*up to H.  !UP: A rows are
// H rows in slot order, the N-tiles are columns n0.. and n0+32.., the
// epilogue stores each row to its pair's row of Y.
//
// NF = 16-wide k-steps per chunk; the loads of chunk i+1 are issued before
// the MFMAs of chunk i.

template <int NF>
struct MoeFrags {
  bf16x8 a[NF], b0[NF], b1[NF];
};

template <int NF>
DEV_INLINE void moe_load(MoeFrags<NF>& f, const short* pa, const short* p0,
                         const short* p1, int k0, short keep) {
#pragma unroll
  for (int c = 0; c < NF; ++c) {
    f.b0[c] = *(const bf16x8*)(p0 + k0 + c * 16);
    f.b1[c] = *(const bf16x8*)(p1 + k0 + c * 16);
    // keep is all ones, or zero on a pad row: a mask, not a select, so the
    // load itself stays unconditional
    f.a[c] = *(const bf16x8*)(pa + k0 + c * 16) & keep;
  }
}

template <int NF>
DEV_INLINE void moe_mma(const MoeFrags<NF>& f, f32x16& acc0, f32x16& acc1) {
#pragma unroll
  for (int c = 0; c < NF; ++c) {
    acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.a[c], f.b0[c], acc0, 0,
                                                   0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.a[c], f.b1[c], acc1, 0,
                                                   0, 0);
  }
}

template <bool UP, int NF>
__global__ __launch_bounds__(WAVE) void moe_gemm_kernel(
    const short* __restrict__ A, const short* __restrict__ W,
    const int* __restrict__ slot_map, const int* __restrict__ tile_expert,
    const int* __restrict__ num_tiles, short* __restrict__ H,
    float* __restrict__ Y, int K, int Nout, int top_k, int max_tiles) {
  const int mtile = blockIdx.x % max_tiles;
  const int nb = blockIdx.x / max_tiles;
  if (mtile >= *num_tiles) return;  // tiles past the device-side count
  const int lane = threadIdx.x, l31 = lane & 31, hi5 = lane >> 5;
  const int e = tile_expert[mtile];
  const int slot = mtile * MOE_BM + l31;
  const int pair = slot_map[slot];
  const short keep = (UP && pair < 0) ? 0 : -1;

  int n0, n1;  // first column of the two N-tiles, as rows of W[e]
  size_t a_row;
  if (UP) {
    n0 = nb * 32;
    n1 = Nout + nb * 32;
    a_row = pair < 0 ? 0 : (size_t)(pair / top_k);
  } else {
    n0 = nb * 64;
    n1 = nb * 64 + 32;
    a_row = (size_t)slot;
  }
  const size_t w_rows = UP ? 2 * (size_t)Nout : (size_t)Nout;
  const short* we = W + (size_t)e * w_rows * K;
  const short* pa = A + a_row * K + hi5 * 8;
  const short* p0 = we + (size_t)(n0 + l31) * K + hi5 * 8;
  const short* p1 = we + (size_t)(n1 + l31) * K + hi5 * 8;

  f32x16 acc0, acc1;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.f;

  // two register sets in turn, K ascending: f0 holds chunk k0, f1 k0 + KC
  constexpr int KC = NF * 16;
  MoeFrags<NF> f0, f1;
  moe_load<NF>(f0, pa, p0, p1, 0, keep);
  int k0 = 0;
  for (; k0 + 2 * KC < K; k0 += 2 * KC) {
    moe_load<NF>(f1, pa, p0, p1, k0 + KC, keep);
    moe_mma<NF>(f0, acc0, acc1);
    moe_load<NF>(f0, pa, p0, p1, k0 + 2 * KC, keep);
    moe_mma<NF>(f1, acc0, acc1);
  }
  if (k0 + KC < K) {
    moe_load<NF>(f1, pa, p0, p1, k0 + KC, keep);
    moe_mma<NF>(f0, acc0, acc1);
    moe_mma<NF>(f1, acc0, acc1);
  } else {
    moe_mma<NF>(f0, acc0, acc1);
  }

  // C fragment: register r of this lane is row c_row(r, hi5), column l31
  if (UP) {
    short* hrow = H + (size_t)mtile * MOE_BM * Nout + n0 + l31;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float g = acc0[r], u = acc1[r];
      float h = g / (1.f + __expf(-g)) * u;
      hrow[(size_t)c_row(r, hi5) * Nout] = f2bf(h);
    }
  } else {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      int p = slot_map[mtile * MOE_BM + c_row(r, hi5)];
      if (p >= 0) {
        float* yrow = Y + (size_t)p * Nout + l31;
        yrow[n0] = acc0[r];
        yrow[n1] = acc1[r];
      }
    }
  }
}

// ---------------------------------------------------------------- combine

__global__ __launch_bounds__(256) void moe_combine_kernel(
    const float* __restrict__ Y, const float* __restrict__ weights,
    short* __restrict__ out, long long n4, int d4, int top_k) {
  long long stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4;
       i += stride) {
    long long t = i / d4;
    int c4 = (int)(i % d4);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < top_k; ++j) {
      float w = weights[t * top_k + j];
      f32x4 y = *(const f32x4*)&Y[((t * top_k + j) * d4 + c4) * 4];
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[q] += w * y[q];
    }
    bf16x4 o;
#pragma unroll
    for (int q = 0; q < 4; ++q) o[q] = f2bf(acc[q]);
    *(bf16x4*)&out[i * 4] = o;
  }
}

// ---------------------------------------------------------------- launchers
// Both return 0 once launched, non-zero (nothing launched) for a
// configuration outside what the kernels support.

static bool moe_shape_ok(long long N, int E, int top_k) {
  return N >= 1 && E >= 1 && E <= MOE_MAX_E && top_k >= 1 &&
         top_k <= MOE_MAX_K && top_k <= E && N * top_k < (1ll << 30);
}

extern "C" int moe_max_tiles(long long N, int top_k, int E) {
  return (int)(N * top_k / MOE_BM) + E;
}

extern "C" int moe_route_f32(const float* logits, float* weights, int* idx,
                             long long N, int E, int top_k,
                             hipStream_t stream) {
  if (!moe_shape_ok(N, E, top_k)) return 1;
  int grid = (int)((N + 255) / 256);
  hipLaunchKernelGGL(moe_route_kernel, dim3(grid), dim3(256), 0, stream,
                     logits, weights, idx, (int)N, E, top_k);
  return 0;
}

// sched is int32 [max_tiles*32 + max_tiles + 1]: slot_map, tile_expert,
// num_tiles; h bf16 [max_tiles*32, F]; y f32 [N*top_k, d]; out bf16 [N, d].
extern "C" int moe_ffn_bf16(const void* x, const void* gate_up,
                            const void* down, const float* weights,
                            const int* idx, int* sched, void* h, float* y,
                            void* out, long long N, int d, int F, int E,
                            int top_k, hipStream_t stream) {
  if (!moe_shape_ok(N, E, top_k) || d < 64 || F < 64 || d % 64 || F % 64)
    return 1;
  const int max_tiles = moe_max_tiles(N, top_k, E);
  const long long up_blocks = (long long)max_tiles * (F / 32);
  const long long down_blocks = (long long)max_tiles * (d / 64);
  if (up_blocks >= (1ll << 31) || down_blocks >= (1ll << 31)) return 1;
  int* slot_map = sched;
  int* tile_expert = sched + (size_t)max_tiles * MOE_BM;
  int* num_tiles = tile_expert + max_tiles;
  const int P = (int)(N * top_k);

  hipLaunchKernelGGL(moe_align_kernel, dim3(1), dim3(MOE_ALIGN_NT), 0, stream,
                     idx, P, E, slot_map, tile_expert, num_tiles);
  // a 128-deep chunk keeps twice the weight bytes in flight per wave
  if (d % 128 == 0)
    hipLaunchKernelGGL((moe_gemm_kernel<true, 8>), dim3((unsigned)up_blocks),
                       dim3(WAVE), 0, stream, (const short*)x,
                       (const short*)gate_up, slot_map, tile_expert,
                       num_tiles, (short*)h, (float*)nullptr, d, F, top_k,
                       max_tiles);
  else
    hipLaunchKernelGGL((moe_gemm_kernel<true, 4>), dim3((unsigned)up_blocks),
                       dim3(WAVE), 0, stream, (const short*)x,
                       (const short*)gate_up, slot_map, tile_expert,
                       num_tiles, (short*)h, (float*)nullptr, d, F, top_k,
                       max_tiles);
  if (F % 128 == 0)
    hipLaunchKernelGGL((moe_gemm_kernel<false, 8>),
                       dim3((unsigned)down_blocks), dim3(WAVE), 0, stream,
                       (const short*)h, (const short*)down, slot_map,
                       tile_expert, num_tiles, (short*)nullptr, y, F, d,
                       top_k, max_tiles);
  else
    hipLaunchKernelGGL((moe_gemm_kernel<false, 4>),
                       dim3((unsigned)down_blocks), dim3(WAVE), 0, stream,
                       (const short*)h, (const short*)down, slot_map,
                       tile_expert, num_tiles, (short*)nullptr, y, F, d,
                       top_k, max_tiles);
  const long long n4 = N * (d / 4);
  int grid = (int)((n4 + 255) / 256 > 4096 ? 4096 : (n4 + 255) / 256);
  hipLaunchKernelGGL(moe_combine_kernel, dim3(grid), dim3(256), 0, stream,
                     (const float*)y, weights, (short*)out, n4, d / 4, top_k);
  return 0;
}
