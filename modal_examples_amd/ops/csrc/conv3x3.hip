// K3: hand-written NCHW implicit-GEMM 3x3 conv (stride 1, pad 1) on MFMA.
//
// Replaces MIOpen/CK for the SDXL VAE/UNet conv pyramid (reference trigger:
// 06_gpu_and_ml/stable_diffusion/text_to_image.py:114 VAE decode path,
// flux.py:259-261).  MIOpen's fastest solvers insert NCHW<->NHWC transpose
// pairs (~19 ms of the 390 ms SDXL step); this kernel consumes NCHW directly
// and does its one unavoidable transpose (x-contiguous -> c-contiguous) in
// LDS during staging.
//
// Formulation: 9 shifted GEMMs.  out[k][p] = sum_tap sum_c W[tap][k][c] *
// in[c][p+tap].  M = 64 out-channels, N = 256 or 512 pixels (8 or 16 rows x
// 32 cols, chosen per call: conv3x3_tile_rule), K-dim = C in chunks of 16
// (mfma_f32_32x32x16_bf16).
//
//  - Input patch staged per 16-channel chunk as LDS [rows+2][34 cols][16 c]
//    (c innermost): the MFMA B-fragment read (8 consecutive c at the lane's
//    pixel) is one ds_read_b128 at 32 B col-stride -> 64 lanes cover a
//    contiguous span, every bank hit evenly (conflict-free; guide §6 G4
//    applies to same-column strides, not contiguous spans).
//  - Weights repacked on host to [9][Kpad][C16] (c contiguous).  The block
//    stages the chunk's [9][64][16] tile into LDS once (one bf16x8 global
//    read per slot, shared by the four waves) and the MFMA A-fragment is one
//    ds_read_b128 from it; per-k-tile weight working set (64 x C x 9 x 2B
//    <= 590 KB) stays L2-resident across the XCD-chunked run of pixel tiles
//    (bijective chunk swizzle, guide §5 T1/m204).
//  - Wave w owns RPW output rows and BOTH 32-k fragments.  Per chunk it
//    reads 18 weight fragments (9 taps x 2) and 3 * (RPW + 2) input
//    fragments - each patch row x column offset once, shared by the taps
//    that use it -: RPW = 2 runs 36 MFMA per 30 ds_read_b128 (1.2:1),
//    RPW = 4 runs 72 per 36 (2:1).
//  - Staging is software-pipelined: chunk cc+1's input and weight loads
//    issue back to back right after chunk cc's second barrier and are first
//    waited for after chunk cc's last MFMA.  Every input load is
//    UNCONDITIONAL from a clamped, always-valid address (row/col clamped into
//    the image, channel clamped to C-1, slot clamped to the last one); the
//    zero fill for padding pixels, spare slots and channels past C is an AND
//    with a 0/-1 mask when the values are packed for the LDS write.  A
//    `cond ? load : 0` per element makes hipcc branch around each load and
//    wait vmcnt(0) per element (guide §5 trap 4(c)), which serialised the
//    whole chunk in front of its MFMAs.
//  - Epilogue fuses bias add and an optional residual add (VAEResnet skip).
//    The block's 64 bias values sit in LDS from the prologue; residual loads
//    are unconditional (clamped on edge tiles) and issue 16 at a time with
//    one wait per batch; interior tiles carry no per-element condition, edge
//    tiles mask only the stores.
//  - Optional per-(n, k) addend (the UNet resnets' time-embedding
//    projection, broadcast over the pixels): out = bf16(bf16(acc + bias) +
//    addend[n][k]) - two roundings, the arithmetic of the separate broadcast
//    add over the conv's bf16 output that it replaces.  The block's 64 values
//    sit in LDS beside the bias.  Not combined with a residual.
//  - Offsets inside one image are 32-bit: the host checks C16*Hs*Ws and
//    64*H*W below 2^31 elements (bindings.cpp check_conv).
//
//  - Optional GroupNorm statistics (`stats` non-null): the epilogue also sums
//    the values AS STORED (the bf16 result widened back to f32) and their
//    squares per aligned channel quad, for the GroupNorm that reads this
//    tensor next.  A lane's 8 quads x (sum, sumsq) are summed over its rows
//    in registers, halved across the 32 lanes of its half-wave (per
//    k-fragment 4, 2, 1 values exchanged, then two butterflies: 18 cross-lane
//    moves for 16 statistics), and the four
//    waves meet in the LDS of the finished main loop.  The block writes its
//    16 quad partials with plain stores to stats[n][pixel tile][quad][2]
//    (32 consecutive floats);
//    gn_stats_finalize_kernel (norms.hip) sums them per (n, group) in a fixed
//    order.  No atomics: the statistics are deterministic.  Masked pixels
//    and channels past K add nothing; the stored output is that of a call
//    without statistics (same arithmetic, a separate epilogue instance).
//
// The kernel is stride-1/pad-1 only; stride-2 downsample convs (3 per UNet
// fwd) stay on the library path.
#include "common.h"

#include <cstdio>
#include <cstdlib>
#include <type_traits>

#define CV_NW 4      // waves per block
#define CV_COLS 32   // output cols per block
#define CV_BK 64     // output channels per block
#define CV_CC 16     // input-channel chunk (MFMA K)

typedef __attribute__((ext_vector_type(16))) float f32x16c;

// GN staging value: silu(x*scale+shift) of one bf16, back to bf16 bits.
DEV_INLINE unsigned gn_silu_bf16(unsigned raw, float sc, float sh) {
  float f = bf2f((short)raw) * sc + sh;
  f = f / (1.f + __expf(-f));
  return (unsigned)(unsigned short)f2bf(f);
}

// A wave-uniform value moved to an SGPR.  The builtin readfirstlane is folded
// away when the compiler can prove the value uniform - and then leaves it in
// a VGPR; the s_nop covers the VALU-write -> readfirstlane hazard.
DEV_INLINE int to_sgpr(int v) {
  int s;
  asm volatile("s_nop 0\n\tv_readfirstlane_b32 %0, %1" : "=s"(s) : "v"(v));
  return s;
}

// RPW = output rows per wave (block rows = CV_NW*RPW).  RPW=2 runs 3
// waves/SIMD (64 accumulators in a 168-register budget); RPW=4 doubles the
// MFMAs per staged byte and per weight read at 2 waves/SIMD: 128 accumulators
// and everything else within 256 registers, every MFMA in its VGPR form (the
// budgets: __launch_bounds__ below, held by check_kernel_resources.py).
// LDS patch: [rows+2][CV_COLS+2][CV_CC] bf16, c innermost.
#define PATCH_C (CV_COLS + 2)

// weight tile in LDS: [9 taps][CV_BK k][CV_CC c], staged once per c-chunk and
// shared by all 4 waves (per-wave global A-reads were 4x-redundant L2
// traffic — the v1 bottleneck).
#define WLDS_ELEMS (9 * CV_BK * CV_CC)
#define WSLOTS (WLDS_ELEMS / 8)  // bf16x8 units
#define WSLOTS_PER_T ((WSLOTS + CV_NW * WAVE - 1) / (CV_NW * WAVE))

// UP: fused nearest-2x upsample — the conv reads the half-res source
// directly (out pixel (y,x) <- src[y/2][x/2]), eliminating the materialized
// F.interpolate pass before every Upsample conv.  H/W are OUTPUT dims;
// Hs/Ws the source's.
// GN: fuse GroupNorm+SiLU into the staging read — silu(x*scale[c]+shift[c])
// with per-(n,c) coefficients from gn_conv_coeffs_bf16 (norms.hip).  The
// gn_norm write+read pass over the full tensor disappears.
template <bool UP, bool GN, int RPW>
__global__ __launch_bounds__(CV_NW * WAVE, RPW == 2 ? 3 : 2)
void conv3x3_kernel(
    const short* __restrict__ in, const short* __restrict__ wr,
    const float* __restrict__ bias, const short* __restrict__ res,
    const short* __restrict__ addend, short* __restrict__ out, const float* __restrict__ gn_scale,
    const float* __restrict__ gn_shift, float* __restrict__ stats, int C,
    int H, int W, int Hs, int Ws,
    int K, int C16, int Kpad, int npix_x, int npix, int nk) {
  constexpr int CV_ROWS = CV_NW * RPW;
  constexpr int PATCH_R = CV_ROWS + 2;
  constexpr int PATCH_ELEMS = PATCH_R * PATCH_C * CV_CC;
  constexpr int STAGE_SLOTS = PATCH_R * PATCH_C * 2;  // (row, col, c-oct)
  constexpr int SLOTS_PER_T =
      (STAGE_SLOTS + CV_NW * WAVE - 1) / (CV_NW * WAVE);
  __shared__ alignas(16) short patch[PATCH_ELEMS];
  __shared__ alignas(16) short wlds[WLDS_ELEMS];
  __shared__ alignas(16) float bias_s[CV_BK];
  __shared__ alignas(16) float addend_s[CV_BK];
  __shared__ unsigned long long stat_dst_s;

  const int tid = threadIdx.x;
  const int w = tid / WAVE;
  const int l = tid % WAVE;
  const int l31 = l & 31;
  const int hi5 = l >> 5;
  const int n = blockIdx.y;

  // bijective XCD-chunk swizzle (m204): each XCD runs a contiguous range of
  // block ids = consecutive pixel tiles of ONE k-tile -> weights L2-hit.
  int bid = blockIdx.x;
  {
    int nwg = npix * nk;
    int q = nwg >> 3, r = nwg & 7;
    int xcd = bid & 7, pos = bid >> 3;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + pos;
  }
  // the division runs on the VALU and its (block-uniform) result would stay
  // in VGPRs, with every tile coordinate and address base built on it
  const int ktile = to_sgpr(bid / npix);
  const int pix = bid - ktile * npix;
  const int pix_y = pix / npix_x;
  const int y0 = pix_y * CV_ROWS;
  const int x0 = (pix - pix_y * npix_x) * CV_COLS;
  const int k0 = ktile * CV_BK;

  const long long in_n = (long long)n * C * Hs * Ws;
  const int nc = C16 / CV_CC;

  // bias: the block's 64 values go to LDS once (index clamped to K-1; the
  // loop's first barrier orders this write before the epilogue's reads).
  if (tid < CV_BK) {
    const int kc = min(k0 + tid, K - 1);
    bias_s[tid] = bias[kc];
    if (addend != nullptr) addend_s[tid] = bf2f(addend[(long long)n * K + kc]);
  }

  // statistics: where this block's 16 quad partials go (0: none asked for).
  // Parked in LDS so that neither the pointer nor the tile counts stay in
  // scalar registers across the main loop, which has none to spare.
  if (tid == 0) {
    const long long e = ((long long)n * npix + pix) * (nk * (CV_BK / 4)) +
                        ktile * (CV_BK / 4);
    stat_dst_s = stats != nullptr ? (unsigned long long)(stats + e * 2) : 0ull;
  }

  // ---- staging: slot s = (row, col, c-oct); thread gathers 8 strided
  // channel values (coalesced across lanes: consecutive threads read
  // consecutive x) and writes ONE bf16x8 to the c-contiguous LDS slot.
  // Fixed per slot for the whole kernel: the byte offset inside image n of
  // (clamped pixel, next chunk's channel oct*8) - advanced by 16 channels per
  // stage_load -, the pixel's last valid offset (channel C-1), the LDS
  // element offset, and a 0/-1 mask that is 0 for padding pixels and for the
  // slots past STAGE_SLOTS.
  const char* in_img = (const char*)(in + in_n);
  const unsigned hwb = (unsigned)Hs * (unsigned)Ws * 2u;  // channel stride, B
  unsigned soff[SLOTS_PER_T], soff_max[SLOTS_PER_T];
  int slds[SLOTS_PER_T], smask[SLOTS_PER_T];
#pragma unroll
  for (int i = 0; i < SLOTS_PER_T; ++i) {
    const int s_raw = i * CV_NW * WAVE + tid;
    const int s = min(s_raw, STAGE_SLOTS - 1);
    const int col = s % PATCH_C;
    const int u = s / PATCH_C;
    const int oct = u & 1;
    const int row = u >> 1;
    const int y = y0 + row - 1;
    const int x = x0 + col - 1;
    const bool live =
        s_raw < STAGE_SLOTS && y >= 0 && y < H && x >= 0 && x < W;
    const int yc = min(max(y, 0), H - 1);
    const int xc = min(max(x, 0), W - 1);
    const unsigned sy = UP ? (yc >> 1) : yc;
    const unsigned sx = UP ? (xc >> 1) : xc;
    const unsigned pix = (sy * (unsigned)Ws + sx) * 2u;
    soff[i] = pix + (unsigned)(oct * 8) * hwb;
    soff_max[i] = pix + (unsigned)(C - 1) * hwb;
    slds[i] = (row * PATCH_C + col) * CV_CC + oct * 8;
    // opaque to the optimiser: as a visible `live ? v : 0` the zero fill
    // turns back into a branch around every load
    int m = live ? -1 : 0;
    asm volatile("" : "+v"(m));
    smask[i] = m;
  }

  // All of a chunk's loads are unconditional and independent, so they issue
  // back to back; nothing here consumes a loaded value.
  unsigned sraw[SLOTS_PER_T][8];
  float gsc[GN ? CV_CC : 1], gsh[GN ? CV_CC : 1];  // chunk's GN coeffs
  auto stage_load = [&](int cc) {
#pragma unroll
    for (int i = 0; i < SLOTS_PER_T; ++i) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const unsigned o = min(soff[i] + (unsigned)j * hwb, soff_max[i]);
        sraw[i][j] = *(const unsigned short*)(in_img + o);
      }
      soff[i] += CV_CC * hwb;
    }
    if constexpr (GN) {
      // tiny [N, C16] arrays at a block-uniform address
      const float* ps = gn_scale + (long long)n * C16 + cc * CV_CC;
      const float* ph = gn_shift + (long long)n * C16 + cc * CV_CC;
#pragma unroll
      for (int j = 0; j < CV_CC; ++j) {
        gsc[j] = ps[j];
        gsh[j] = ph[j];
      }
    }
  };
  // The first use of the loaded values: (GN: normalise + SiLU,) pack pairs,
  // AND with the slot mask and the channel-tail mask, one 16-byte LDS write.
  auto stage_write = [&](int cc) {
    const int nv = C - cc * CV_CC;  // channels of this chunk below C (uniform)
#pragma unroll
    for (int i = 0; i < SLOTS_PER_T; ++i) {
      const int o8 = slds[i] & 8;  // oct * 8
      i32x4 pk;
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        unsigned lo = sraw[i][2 * d], hi = sraw[i][2 * d + 1];
        // pin the first use here: left alone, hipcc hoists the pair packing
        // (and with it the wait for these loads) above the MFMA block
        asm volatile("" : "+v"(lo), "+v"(hi));
        if constexpr (GN) {
          lo = gn_silu_bf16(lo, o8 ? gsc[8 + 2 * d] : gsc[2 * d],
                            o8 ? gsh[8 + 2 * d] : gsh[2 * d]);
          hi = gn_silu_bf16(hi, o8 ? gsc[9 + 2 * d] : gsc[1 + 2 * d],
                            o8 ? gsh[9 + 2 * d] : gsh[1 + 2 * d]);
        }
        pk[d] = (int)((lo | (hi << 16)) & (unsigned)smask[i]);
      }
      // channel tail, last chunk only: a block-uniform branch round pure
      // ALU work; the masks are sign-bit arithmetic, never a select
      if (nv < CV_CC) {
        const int nvl = nv - o8;  // this oct's channels below C
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          const unsigned lo = (unsigned)((2 * d - nvl) >> 31);
          const unsigned hi = (unsigned)((2 * d + 1 - nvl) >> 31);
          pk[d] &= (int)((lo & 0xffffu) | (hi & 0xffff0000u));
        }
      }
      // only the last round has spare slots
      if ((i + 1) * CV_NW * WAVE <= STAGE_SLOTS ||
          i * CV_NW * WAVE + tid < STAGE_SLOTS)
        *(i32x4*)&patch[slds[i]] = pk;
    }
  };

  // weight staging: slot = (tap, k-row, c-oct); one bf16x8 each.  The spare
  // slots of the last round re-read the last slot (no branch round a load).
  // Per-thread 32-bit byte offsets from the k-tile's (block-uniform) base.
  bf16x8 wreg[WSLOTS_PER_T];
  unsigned woff[WSLOTS_PER_T];
#pragma unroll
  for (int i = 0; i < WSLOTS_PER_T; ++i) {
    const int s = min(i * CV_NW * WAVE + tid, WSLOTS - 1);
    const int oct = s & 1;
    const int kr = (s >> 1) & (CV_BK - 1);
    const int tap = (s >> 1) >> 6;  // 64 k-rows per tap
    woff[i] = ((unsigned)(tap * Kpad + kr) * (unsigned)C16 + oct * 8) * 2u;
  }
  const char* w_tile = (const char*)(wr + (long long)k0 * C16);
  auto wstage_load = [&](int cc) {
    const char* wb = w_tile + cc * (CV_CC * 2);
#pragma unroll
    for (int i = 0; i < WSLOTS_PER_T; ++i)
      wreg[i] = *(const bf16x8*)(wb + woff[i]);
  };
  auto wstage_write = [&]() {
#pragma unroll
    for (int i = 0; i < WSLOTS_PER_T; ++i) {
      const int s = i * CV_NW * WAVE + tid;
      if ((i + 1) * CV_NW * WAVE <= WSLOTS || s < WSLOTS)
        *(bf16x8*)&wlds[s * 8] = wreg[i];
    }
  };

  // accumulators: [wave-row rr][k-fragment mf]
  f32x16c acc[RPW][2];
#pragma unroll
  for (int a = 0; a < RPW; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  stage_load(0);
  wstage_load(0);
  for (int cc = 0; cc < nc; ++cc) {
    __syncthreads();  // previous compute done; LDS free
    stage_write(cc);
    wstage_write();
    __syncthreads();  // patch + weights ready
    if (cc + 1 < nc) {
      stage_load(cc + 1);
      wstage_load(cc + 1);
    }

    // one base per operand; every tap/row is a compile-time LDS offset
    const short* wl = &wlds[l31 * CV_CC + hi5 * 8];
    const short* pl = &patch[(w * RPW * PATCH_C + l31) * CV_CC + hi5 * 8];
    // dx outer, then a window of RPW patch rows that slides down by one per
    // dy: the B-fragment of tap (dy, dx) for output row rr is patch row
    // rr + dy at column offset dx, so every fragment is read ONCE and feeds
    // each (row, k-fragment) MFMA that uses it - 3 * (RPW + 2) input reads
    // per chunk instead of 9 * RPW, beside the 18 weight reads.  Live at a
    // time: the two A-fragments of one tap and RPW B-fragments.
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      bf16x8 b[RPW + 2];
#pragma unroll
      for (int dy = 0; dy < 3; ++dy) {
        const int tap = dy * 3 + dx;
        bf16x8 a0 = *(const bf16x8*)&wl[tap * CV_BK * CV_CC];
        bf16x8 a1 = *(const bf16x8*)&wl[(tap * CV_BK + 32) * CV_CC];
#pragma unroll
        for (int rr = 0; rr < RPW; ++rr) {
          const int pr = rr + dy;  // patch row
          if (dy == 0 || rr == RPW - 1)
            b[pr] = *(const bf16x8*)&pl[(pr * PATCH_C + dx) * CV_CC];
          __builtin_amdgcn_s_setprio(1);
          acc[rr][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b[pr], acc[rr][0], 0, 0, 0);
          acc[rr][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b[pr], acc[rr][1], 0, 0, 0);
          __builtin_amdgcn_s_setprio(0);
        }
      }
    }
  }

  // ---- epilogue: bias (+ residual) add, NCHW store.  RES / EDGE are
  // block-uniform and decided once, outside: no load sits behind a
  // per-element condition.  Edge tiles clamp (y, x, k) for the residual
  // loads and mask the stores; interior tiles have no condition at all.
  // Offsets inside the block's (n, k0) slab of 64 planes are 32-bit.
  auto epilogue = [&](auto res_c, auto add_c, auto edge_c, auto stat_c,
                      float* stat_dst) {
    constexpr bool RES = decltype(res_c)::value;
    constexpr bool ADD = decltype(add_c)::value;
    constexpr bool EDGE = decltype(edge_c)::value;
    constexpr bool STAT = decltype(stat_c)::value;
    // lane coordinates rebuilt from an opaque copy of tid: kept live across
    // the main loop they cost registers the loop has not got
    int t = tid;
    asm volatile("" : "+v"(t));
    const int w = t / WAVE, l31 = t & 31, hi5 = (t >> 5) & 1;
    const unsigned hw = (unsigned)H * (unsigned)W;
    const long long slab = ((long long)n * K + k0) * hw;
    // block-uniform bases, 32-bit byte offsets
    const char* resb = RES ? (const char*)(res + slab) : nullptr;
    char* outb = (char*)(out + slab);
    const int x = x0 + l31;
    const int kmax = K - 1 - k0;  // last valid k of this tile (EDGE)
    // st[i], i = 4*{sum, sumsq} + q: the lane's quad sums of one k-fragment
    // over its rows
    float st[STAT ? 8 : 1];
    // edge tiles: a 0/-1 mask ANDed onto the bits of a counted value, sign-bit
    // arithmetic like the staging masks.  As a second use of the stores'
    // condition every element's lane mask stays live in scalar registers.
    // K is a multiple of 4 here, so a quad is below K as a whole.
    const int kq = 4 * hi5 - kmax - 1;  // + the quad's mf*32 + 8*q: < 0 below K
    // one (row, k-fragment) of the wave's tile: 16 values per lane
    auto frag = [&](int rr, int mf) {
      const int y = y0 + w * RPW + rr;
      const bool pix_ok = !EDGE || (y < H && x < W);
      const unsigned po = EDGE ? (unsigned)min(y, H - 1) * W + min(x, W - 1)
                               : (unsigned)y * W + x;
      int pmask = -1;  // STAT && EDGE: 0 for a pixel past H or W
      if constexpr (STAT && EDGE)
        pmask = (((y - H) >> 31) & ((x - W) >> 31));
      unsigned rv[16];
      if constexpr (RES) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kl = mf * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi5;
          const unsigned ke = EDGE ? min(kl, kmax) : kl;
          rv[r] = *(const unsigned short*)(resb + (po + ke * hw) * 2u);
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4 b4 = *(const f32x4*)&bias_s[mf * 32 + 8 * q + 4 * hi5];
        f32x4 a4;
        int qm = -1;  // STAT && EDGE: 0 for a quad past K or a pixel outside
        if constexpr (STAT && EDGE)
          qm = ((mf * 32 + 8 * q + kq) >> 31) & pmask;
        if constexpr (ADD)
          a4 = *(const f32x4*)&addend_s[mf * 32 + 8 * q + 4 * hi5];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int r = q * 4 + j;
          const int kl = mf * 32 + j + 8 * q + 4 * hi5;
          float v = acc[rr][mf][r] + b4[j];
          if constexpr (RES) v += bf2f((short)rv[r]);
          if constexpr (ADD) v = bf2f(f2bf(v)) + a4[j];
          const short o = f2bf(v);
          if (!EDGE || (pix_ok && kl <= kmax))
            *(short*)(outb + (po + (unsigned)kl * hw) * 2u) = o;
          if constexpr (STAT) {
            float f = bf2f(o);
            if constexpr (EDGE) f = __int_as_float(__float_as_int(f) & qm);
            st[q] += f;
            st[4 + q] = fmaf(f, f, st[4 + q]);
          }
        }
        // one quad at a time: scheduled as a whole, the 64 rounded values
        // and their widened copies are all live at once and spill
        if constexpr (STAT) __builtin_amdgcn_sched_barrier(0);
      }
    };
    if constexpr (!STAT) {
#pragma unroll
      for (int rr = 0; rr < RPW; ++rr)
#pragma unroll
        for (int mf = 0; mf < 2; ++mf) frag(rr, mf);
    } else {
      // k-fragment by k-fragment, so that 8 sums are live at a time and the
      // first fragment's accumulators are dead during the second.  Halving
      // exchange inside the half-wave: at lane bit b a lane keeps the upper
      // half of its values if the bit is set, else the lower, and adds the
      // partner's copy of that half; after bits 4..2 one value is left,
      // st index (l31 >> 2), and bits 1, 0 are plain butterflies: 9 moves
      // for a fragment's 8 statistics.
      const bool b4 = l31 & 16, b3 = l31 & 8, b2 = l31 & 4;
      float sred[2];
#pragma unroll
      for (int mf = 0; mf < 2; ++mf) {
#pragma unroll
        for (int i = 0; i < 8; ++i) st[i] = 0.f;
#pragma unroll
        for (int rr = 0; rr < RPW; ++rr) frag(rr, mf);
        float s4[4], s2[2], s1;
#pragma unroll
        for (int i = 0; i < 4; ++i)
          s4[i] = (b4 ? st[4 + i] : st[i]) +
                  __shfl_xor(b4 ? st[i] : st[4 + i], 16, WAVE);
#pragma unroll
        for (int i = 0; i < 2; ++i)
          s2[i] = (b3 ? s4[2 + i] : s4[i]) +
                  __shfl_xor(b3 ? s4[i] : s4[2 + i], 8, WAVE);
        s1 = (b2 ? s2[1] : s2[0]) + __shfl_xor(b2 ? s2[0] : s2[1], 4, WAVE);
        s1 += __shfl_xor(s1, 2, WAVE);
        s1 += __shfl_xor(s1, 1, WAVE);
        sred[mf] = s1;
      }
      // the four waves meet in the patch's LDS: every wave has left the main
      // loop once it is past this barrier
      float* red = (float*)patch;  // [wave][hi5][mf][8]
      __syncthreads();
      if ((l31 & 3) == 0) {
        red[((w * 2 + hi5) * 2 + 0) * 8 + (l31 >> 2)] = sred[0];
        red[((w * 2 + hi5) * 2 + 1) * 8 + (l31 >> 2)] = sred[1];
      }
      __syncthreads();
      if (t < 32) {
        // thread = (quad of the tile, statistic); quad cq covers channels
        // k0 + 4*cq .. +3 = mf*32 + 8*q + 4*hi5
        const int cq = t >> 1, sq = t & 1;
        const int i = (((cq & 1) * 2 + (cq >> 3)) * 8) + sq * 4 + ((cq >> 1) & 3);
        float a = 0.f;
#pragma unroll
        for (int ww = 0; ww < CV_NW; ++ww) a += red[ww * 32 + i];
        stat_dst[t] = a;  // t = 2 * cq + sq
      }
    }
  };
  const bool edge =
      y0 + CV_ROWS > H || x0 + CV_COLS > W || k0 + CV_BK > K;
  const std::true_type yes{};
  const std::false_type no{};
  const unsigned long long sd = stat_dst_s;  // written before the loop
  float* const stat_dst = (float*)(((unsigned long long)(unsigned)to_sgpr(
                                        (int)(sd >> 32)) << 32) |
                                   (unsigned)to_sgpr((int)sd));
  auto dispatch = [&](auto stat_c) {
    if (res != nullptr) {
      if (edge) epilogue(yes, no, yes, stat_c, stat_dst);
      else epilogue(yes, no, no, stat_c, stat_dst);
    } else if (addend != nullptr) {
      if (edge) epilogue(no, yes, yes, stat_c, stat_dst);
      else epilogue(no, yes, no, stat_c, stat_dst);
    } else {
      if (edge) epilogue(no, no, yes, stat_c, stat_dst);
      else epilogue(no, no, no, stat_c, stat_dst);
    }
  };
  if (stat_dst != nullptr) dispatch(yes);
  else dispatch(no);
}

// Blocks of a call at `rpw` rows per wave (grid x * y).
static long long conv_blocks(int rpw, int N, int H, int W, int K) {
  const int rows = CV_NW * rpw;
  return (long long)((W + CV_COLS - 1) / CV_COLS) * ((H + rows - 1) / rows) *
         ((K + CV_BK - 1) / CV_BK) * N;
}

// The tile rule: rows per wave (2: 8-row tile, 4: 16-row tile) as a pure
// function of the call's shape; H, W are the OUTPUT dims.  PERF.md, "conv3x3:
// input fragments shared between taps, 16-row tile per call", has the table
// it rests on.
extern "C" int conv3x3_tile_rule(int N, int C, int H, int W, int K,
                                 int upsample, int gn) {
  (void)upsample;  // both upsample shapes of the table fall on the same side
  // GroupNorm in the staging: not timed with the 16-row tile, stays at 8
  if (gn) return 2;
  // a few chunks only: the block is mostly epilogue and gains nothing from
  // fewer LDS reads per MFMA (4 -> 512 @128^2: no faster, +res slower)
  if (C < 128) return 2;
  // the 16-row tiling may round H up by 8 rows more than the 8-row tiling:
  // taken only where those are no rows at all or under 1/16 of the image
  const int rows16 = (H + 15) / 16 * 16, rows8 = (H + 7) / 8 * 8;
  if (rows16 != rows8 && H < 128) return 2;
  // two blocks of the 16-row tile are resident per CU, 512 on the 256 CUs:
  // faster from two such rounds of blocks on (1024: 512 -> 512 @128^2 x 4),
  // level at 640 blocks, slower at 320 and 160
  return conv_blocks(4, N, H, W, K) >= 2 * 2 * 256 ? 4 : 2;
}

// The tile of one call: the rule, or MODAL_AMD_CONV_RPW=2|4 (read once per
// process) for A/B runs.  The launcher, conv3x3_stats_dims and the caller of
// gn_stats_finalize all take the value this returns.
extern "C" int conv3x3_tile_rpw(int N, int C, int H, int W, int K,
                                int upsample, int gn) {
  static const int forced = [] {
    const char* e = getenv("MODAL_AMD_CONV_RPW");
    const int v = e ? atoi(e) : 0;
    return (v == 2 || v == 4) ? v : 0;
  }();
  return forced ? forced : conv3x3_tile_rule(N, C, H, W, K, upsample, gn);
}

// The statistics workspace of an H x W x K output written at `rpw` rows per
// wave: [N][npix][nquads][2] f32.
extern "C" void conv3x3_stats_dims(int rpw, int H, int W, int K, int* npix,
                                   int* nquads) {
  const int rows = CV_NW * rpw;
  *npix = ((W + CV_COLS - 1) / CV_COLS) * ((H + rows - 1) / rows);
  *nquads = ((K + CV_BK - 1) / CV_BK) * (CV_BK / 4);
}

// rpw: conv3x3_tile_rpw() of this call (the caller sized `stats` from it).
extern "C" void conv3x3_bf16(const void* in, const void* wrepack,
                             const void* bias, const void* residual,
                             const void* addend, void* out,
                             const float* gn_scale, const float* gn_shift,
                             float* stats, int N, int C, int H, int W, int K,
                             int C16,
                             int Kpad, int upsample, int rpw,
                             hipStream_t stream) {
  // H/W are the OUTPUT dims; with upsample the source is H/2 x W/2.
  const int Hs = upsample ? H / 2 : H;
  const int Ws = upsample ? W / 2 : W;
  const int rows = CV_NW * rpw;
  const int npix_x = (W + CV_COLS - 1) / CV_COLS;
  const int npix_y = (H + rows - 1) / rows;
  const int npix = npix_x * npix_y;
  const int nk = (K + CV_BK - 1) / CV_BK;
  dim3 grid(npix * nk, N);
  dim3 block(CV_NW * WAVE);
  const bool gn = gn_scale != nullptr;
#define CVL(UPV, GNV, RPWV) \
  hipLaunchKernelGGL((conv3x3_kernel<UPV, GNV, RPWV>), grid, block, 0, \
                     stream, (const short*)in, (const short*)wrepack, \
                     (const float*)bias, (const short*)residual, \
                     (const short*)addend, (short*)out, \
                     gn_scale, gn_shift, stats, C, H, W, Hs, Ws, K, C16, \
                     Kpad, \
                     npix_x, npix, nk)
  if (rpw == 4) {
    if (upsample) {
      if (gn) CVL(true, true, 4); else CVL(true, false, 4);
    } else {
      if (gn) CVL(false, true, 4); else CVL(false, false, 4);
    }
  } else {
    if (upsample) {
      if (gn) CVL(true, true, 2); else CVL(true, false, 2);
    } else {
      if (gn) CVL(false, true, 2); else CVL(false, false, 2);
    }
  }
#undef CVL
}
