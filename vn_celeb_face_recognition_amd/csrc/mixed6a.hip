// mixed_6a branch 1 (inception_resnet_v1.py:137-141) as ONE launch on gfx950: 1x1 256 -> 192, 3x3 pad 1 192 -> 192 and
// 3x3 stride 2 192 -> 256 on one 17 x 17 image, written as channels [coff, coff + 256) of the 8 x 8 mixed_6a output.
// The plan runs them as three convolutions with two 17 x 17 x 192 tensors through memory between them; the last one
// (M = 64 per image) fills half the chip and the first one (four K tiles) mostly fills and drains its ring.  This kernel
// takes the form of trunk17.hip / block8.hip instead: one workgroup (8 waves) = one image, resident on its CU.
//
// What stays where
//   * the image lives in LDS in the K-tile image of fused_device.h ([k-tile][pixel row][128 B], 16-byte slots XOR-swizzled
//     by row & 7), a tile being M6_ROWS = 296 pixel rows (289, rounded up to the 8-row pieces of the LDS-DMA).  X is four
//     tiles; the 1x1 output (three tiles) is written over it once every wave has read its last X fragment, the 3x3 p1
//     output over that in the same way.  The nine taps of a 3x3 are shifted row reads of the image; a tap outside the
//     image reads one zero chunk (fed to the MFMA, not skipped, as the plan's gather does);
//   * every accumulator lives in registers.  1x1 and 3x3 p1: wave = (channel group cg = wave & 3, pixel half ph =
//     wave >> 2) holds channel tiles 3cg .. 3cg + 2 x pixel tiles 10ph .. 10ph + 9 = 30 MFMA tiles (the 20th pixel tile
//     is padding; the 19th holds pixel 288 alone).  A B fragment read from LDS feeds 3 MFMAs, an A fragment 10.
//     3x3 s2: wave holds channel tiles 2 wave, 2 wave + 1 x the four pixel tiles of the 8 x 8 output;
//   * weights stream L2 -> registers, one contiguous stream per wave in consumption order (mixed6a_repack), M6_RING = 9
//     fragments in flight per wave across the phase boundaries (72 KiB per CU).  The two pixel halves fetch the same 1x1
//     and 3x3 p1 fragments: 2 x (96 + 648) KiB + 864 KiB = 2.3 MiB ingested per image.  9 divides the fragments of one tap
//     (18) and of one tap row of the last convolution (36), so the tap loops stay rolled with compile-time ring slots.
//
// Rows 289..295 of a tile are loaded as copies of row 288 and never written afterwards; pixel tiles reach rows up to
// 319, which in the 1x1 phase are the next tile's first rows or the bytes behind the image (inside this workgroup's
// LDS): a pixel is one MFMA column, so they cannot reach another pixel's sum, and they are never stored.  In the 3x3 p1
// phase those pixels take every tap from the zero chunk, and a live pixel's in-image neighbour is always a row < 289.
//
// Barriers: X resident | 1x1 done | m6a written | 3x3 p1 done | m6b written | output tile written.
//
// Numerics: bit-identical to the three plan convolutions.  Same MFMA (v_mfma_f32_16x16x32, weights as A, pixels as B),
// every convolution from a zero accumulator in ascending 32-deep k steps with k = (kh, kw, c), then the plan's fast
// epilogue (conv_device.h): v = acc + bias, max(v, 0), round to T -- at the same three points.
#include "mixed6a.h"
#include "fused_device.h"

namespace vnf {

namespace {

constexpr int M6_PX = 289;                         // 17 x 17
constexpr int M6_ROWS = 296;                       // pixel rows of one K tile
constexpr int M6_RING = 9;                         // weight fragments in flight per wave
constexpr int M6_KS1 = 8;                          // 32-deep k steps of the 1x1 (K = 256)
constexpr int M6_KS3 = 54;                         // of a 3x3 (K = 9 x 192)
constexpr int M6_F1 = 3 * M6_KS1;                  // fragments per wave: 1x1 (3 channel tiles)
constexpr int M6_F2 = 3 * M6_KS3;                  // 3x3 p1 (3 channel tiles)
constexpr int M6_F3 = 2 * M6_KS3;                  // 3x3 s2 (2 channel tiles)
constexpr int M6_FRAGS = M6_F1 + M6_F2 + M6_F3;
constexpr int M6_SLOT = M6_FRAGS + M6_RING;        // stream slots per wave: the ring's read-ahead lands in zero padding
constexpr int M6_STREAM_FRAGS = 8 * M6_SLOT;
constexpr int KT_BYTES = M6_ROWS * 128;            // one K tile (64 channels) of the image
constexpr int OFF_X = 0;                           // 4 K tiles: the block input
constexpr int OFF_A = 0;                           // 3 K tiles over X: the 1x1 output, then the 3x3 p1 output
constexpr int OFF_OUT = 3 * KT_BYTES;              // [4 tiles][64 rows][128 B] over X's last tile: the 8 x 8 x 256 output
constexpr int OFF_ZERO = 4 * KT_BYTES;             // 256 zero bytes: out-of-image taps
constexpr int OFF_REACH = 3 * KT_BYTES + 320 * 128;   // end of what the 1x1 phase's 20 pixel tiles address in the last tile
constexpr int OFF_BIAS = OFF_REACH;                // the M6_BIAS biases (a global load would queue behind the ring)
constexpr int M6_LDS = OFF_BIAS + M6_BIAS * 4;
static_assert(M6_ROWS % 8 == 0 && M6_ROWS >= M6_PX, "a tile is whole 8-row LDS-DMA pieces");
static_assert(4 * 64 * 128 <= KT_BYTES, "the output tile fits X's last K tile");
static_assert(OFF_ZERO + 256 <= OFF_REACH, "the zero chunk lies inside the allocation");
static_assert(M6_LDS <= 160 * 1024, "one workgroup's LDS");
static_assert(M6_F1 % M6_RING == 6 && 18 % M6_RING == 0 && (M6_F1 + M6_F2) % M6_RING == 6 && 36 % M6_RING == 0,
              "the ring slot of a step must not depend on the tap");

// the plan's fast epilogue on one accumulator quad: v = acc + bias, max(v, 0), round to T
template <typename T>
__device__ __forceinline__ uint2 bias_relu_round(const f32x4_t& acc, const f32x4_t& bias) {
  f32x4_t v;
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = fmaxf(acc[e] + bias[e], 0.f);
  return pack4<T>(v);
}

}  // namespace

template <typename T>
__global__ __launch_bounds__(512) void mixed6a_chain_kernel(const Mixed6aArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int frow = lane & 15, fgrp = lane >> 4;
  const int cg = wave & 3, ph = wave >> 2;
  const int img = blockIdx.x;
  const unsigned lds0 = lds_dma_base(smem);

  // ---- weight stream of this wave: fragment f at wp + f * 64 (uint4 units); the first M6_RING go out before the input
  const uint4* wp = reinterpret_cast<const uint4*>(a.wstream) + (size_t)wave * M6_SLOT * 64 + lane;
  uint4 wq[M6_RING];
  ring_prime(wq, wp);

  // ---- image -> LDS by LDS-DMA: piece = 8 pixel rows x 128 B of one K tile, 4 x 37 pieces over the 8 waves
  {
    const char* src = (const char*)a.x + (size_t)img * M6_PX * a.ldx * 2;
    const int r = lane >> 3, slot = lane & 7;
    constexpr int PIECES = 4 * (M6_ROWS / 8);
#pragma unroll
    for (int i = 0; i < (PIECES + 7) / 8; ++i) {
      const int piece = wave + i * 8;              // [kt 0..3][row group 0..36]
      if (piece < PIECES) {
        const int kt = piece / (M6_ROWS / 8), rg = piece - kt * (M6_ROWS / 8);
        const int p = min(rg * 8 + r, M6_PX - 1);  // rows behind the image's last: that row again
        glds16(src + ((size_t)p * a.ldx + kt * 64 + ((slot ^ r) << 3)) * 2, lds0 + OFF_X + kt * KT_BYTES + rg * 1024);
      }
    }
    if (tid < 16) reinterpret_cast<uint4*>(smem + OFF_ZERO)[tid] = uint4{0u, 0u, 0u, 0u};
    if (tid < M6_BIAS / 4) reinterpret_cast<f32x4_t*>(smem + OFF_BIAS)[tid] = reinterpret_cast<const f32x4_t*>(a.bias)[tid];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __syncthreads();

  // Per-lane LDS offsets inside the K-tile image (fused_device.h).  Pixel tile i of this wave is pixels p0 + 16 i + frow,
  // p0 = 160 ph; all of them share row & 7 = frow & 7.  B-fragment read of k step ks of K tile kt:
  // kt * KT_BYTES + rowb + i * 2048 + (ks & 1 ? rb1 : rb0).  Accumulator quad of channel tile ct: quad(ct) + rowb + i * 2048.
  const int p0 = 160 * ph + frow;
  const int rowb = p0 * 128;
  const int rb0 = (fgrp ^ (frow & 7)) << 4, rb1 = rb0 ^ 64;
  auto quad = [&](int c, int row7) {               // ktile_quad without the row term; c = first of the lane's 4 channels
    return (c >> 6) * KT_BYTES + ((((c & 63) >> 3) ^ row7) << 4) + (c & 4) * 2;
  };

  f32x4_t acc[3][10];
  auto clear = [&]() {
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int i = 0; i < 10; ++i) acc[j][i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  };
  // bias + ReLU + round of the 30 tiles into the image at OFF_A (rows of the image only); bias0 = the convolution's first bias
  auto store_image = [&](int bias0) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int c = 16 * (3 * cg + j) + 4 * fgrp;
      const f32x4_t bv = *reinterpret_cast<const f32x4_t*>(smem + OFF_BIAS + (bias0 + c) * 4);
      const int qb = OFF_A + quad(c, frow & 7) + rowb;
#pragma unroll
      for (int i = 0; i < 10; ++i)
        if (p0 + 16 * i < M6_PX) *reinterpret_cast<uint2*>(smem + qb + i * 2048) = bias_relu_round<T>(acc[j][i], bv);
    }
  };

  // ---------------------------------------------------------------- 1x1, 256 -> 192
  clear();
#pragma unroll
  for (int ks = 0; ks < M6_KS1; ++ks) {
    uint4 xf[10];
#pragma unroll
    for (int i = 0; i < 10; ++i)
      xf[i] = *reinterpret_cast<const uint4*>(smem + OFF_X + (ks >> 1) * KT_BYTES + rowb + i * 2048 + ((ks & 1) ? rb1 : rb0));
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int s = ks * 3 + j;
#pragma unroll
      for (int i = 0; i < 10; ++i) mma_chunk<T>(acc[j][i], wq[s % M6_RING], xf[i]);
      ring_refill(wq, s, wp);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  __syncthreads();   // X is dead only now: every wave has read its last fragment
  store_image(0);
  __syncthreads();

  // ---------------------------------------------------------------- 3x3 pad 1, 192 -> 192, k = tap * 192 + c
  {
    int yx[10];      // (y << 8) | x of the tile's pixel; a padding pixel sits far outside, so every tap of it is out of the image
#pragma unroll
    for (int i = 0; i < 10; ++i) {
      const int p = p0 + 16 * i, y = (p * 241) >> 12;   // p / 17 for p < 4096
      yx[i] = p < M6_PX ? (y << 8) | (p - 17 * y) : 0x4040;
    }
    clear();
#pragma unroll 1
    for (int tap = 0; tap < 9; ++tap) {
      const int dy = tap / 3 - 1, dx = tap - 3 * (tap / 3) - 1;
      int tb[10];    // the tap's fragment base in K tile 0, first half; < 0: outside the image
#pragma unroll
      for (int i = 0; i < 10; ++i) {
        const bool ok = (unsigned)((yx[i] >> 8) + dy) < 17u && (unsigned)((yx[i] & 255) + dx) < 17u;
        const int row = p0 + 16 * i + 17 * dy + dx;
        tb[i] = ok ? row * 128 + ((fgrp ^ (row & 7)) << 4) : -1;
      }
#pragma unroll
      for (int kk = 0; kk < 6; ++kk) {
        uint4 xf[10];
#pragma unroll
        for (int i = 0; i < 10; ++i) {
          const int off = OFF_A + (((kk >> 1) * KT_BYTES + tb[i]) ^ ((kk & 1) * 64));
          xf[i] = *reinterpret_cast<const uint4*>(smem + (tb[i] >= 0 ? off : OFF_ZERO));
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const int s = M6_F1 + kk * 3 + j;        // + 18 tap: a multiple of the ring
#pragma unroll
          for (int i = 0; i < 10; ++i) mma_chunk<T>(acc[j][i], wq[s % M6_RING], xf[i]);
          ring_refill(wq, s, wp);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
  __syncthreads();   // every wave is done reading the 1x1 output
  store_image(192);
  __syncthreads();

  // ---------------------------------------------------------------- 3x3 stride 2 pad 0, 192 -> 256, to 8 x 8
  {
    f32x4_t o[2][4];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) o[j][i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    // output pixel q = 16 i + frow = (oy, ox) = (2 i + (frow >> 3), frow & 7) reads input pixel (2 oy + dy, 2 ox + dx)
    const int in0 = 34 * (frow >> 3) + 2 * (frow & 7);   // input row of tap (0, 0) for i = 0; + 68 i
#pragma unroll 1
    for (int dy = 0; dy < 3; ++dy) {
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        int tb[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int row = in0 + 68 * i + 17 * dy + dx;
          tb[i] = row * 128 + ((fgrp ^ (row & 7)) << 4);
        }
#pragma unroll
        for (int kk = 0; kk < 6; ++kk) {
          uint4 xf[4];
#pragma unroll
          for (int i = 0; i < 4; ++i)
            xf[i] = *reinterpret_cast<const uint4*>(smem + OFF_A + (((kk >> 1) * KT_BYTES + tb[i]) ^ ((kk & 1) * 64)));
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            const int s = M6_F1 + M6_F2 + dx * 12 + kk * 2 + j;   // + 36 dy: a multiple of the ring
#pragma unroll
            for (int i = 0; i < 4; ++i) mma_chunk<T>(o[j][i], wq[s % M6_RING], xf[i]);
            ring_refill(wq, s, wp);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
    // bias + ReLU + round into the output tile (X's last K tile: dead since the 1x1, untouched by the two images since)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int c = 32 * wave + 16 * j + 4 * fgrp;
      const f32x4_t bv = *reinterpret_cast<const f32x4_t*>(smem + OFF_BIAS + (384 + c) * 4);
      const int qb = OFF_OUT + (c >> 6) * 8192 + frow * 128 + ((((c & 63) >> 3) ^ (frow & 7)) << 4) + (c & 4) * 2;
#pragma unroll
      for (int i = 0; i < 4; ++i) *reinterpret_cast<uint2*>(smem + qb + i * 2048) = bias_relu_round<T>(o[j][i], bv);
    }
  }
  __syncthreads();
  // ---- output tile -> channels [coff, coff + 256) of the image's 64 output rows, 16 bytes per lane
  {
    char* dst = (char*)a.y + ((size_t)img * 64 * a.ldy + a.coff) * 2;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int idx = it * 512 + tid;               // 2048 16-byte chunks: [pixel][32 chunks]
      const int q = idx >> 5, ch = idx & 31;        // chunk ch = channels 8 ch .. 8 ch + 7
      const uint4 v = *reinterpret_cast<const uint4*>(smem + OFF_OUT + (ch >> 3) * 8192 + q * 128 + (((ch & 7) ^ (q & 7)) << 4));
      *reinterpret_cast<uint4*>(dst + ((size_t)q * a.ldy + ch * 8) * 2) = v;
    }
  }
}

// ---------------------------------------------------------------------------------------------- weight stream
// One stream of M6_SLOT fragments per wave (cg = wave & 3): fragment s, in the kernel's consumption order,
//   s 0..23      1x1 rows 16 (3 cg + j) .. + 15,     k = 32 ks .. + 31,  s = 3 ks + j
//   s 24..185    3x3 p1 rows 16 (3 cg + j) .. + 15,  k = 32 ks .. + 31,  s - 24 = 3 ks + j
//   s 186..293   3x3 s2 rows 16 (2 wave + j) .. + 15, k = 32 ks .. + 31, s - 186 = 2 ks + j
// then M6_RING zero fragments for the ring's read-ahead.
__global__ void mixed6a_repack_kernel(Mixed6aPack p, uint4* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int frag = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (frag >= M6_STREAM_FRAGS) return;
  const int wave = frag / M6_SLOT, s = frag - wave * M6_SLOT, cg = wave & 3;
  int conv = -1, r0 = 0, k0 = 0;
  if (s < M6_F1) { conv = 0; r0 = 16 * (3 * cg + s % 3); k0 = 32 * (s / 3); }
  else if (s < M6_F1 + M6_F2) { const int t = s - M6_F1; conv = 1; r0 = 16 * (3 * cg + t % 3); k0 = 32 * (t / 3); }
  else if (s < M6_FRAGS) { const int t = s - M6_F1 - M6_F2; conv = 2; r0 = 16 * (2 * wave + t % 2); k0 = 32 * (t / 2); }
  uint4 v = {0u, 0u, 0u, 0u};
  if (conv >= 0) v = GatherA16::load(p.w[conv], p.kpad[conv], r0, k0, lane, 0);
  out[(size_t)frag * 64 + lane] = v;
}

size_t mixed6a_stream_bytes() { return (size_t)M6_STREAM_FRAGS * 1024; }

hipError_t mixed6a_repack(const Mixed6aPack& p, void* out, hipStream_t s) {
  hipLaunchKernelGGL(mixed6a_repack_kernel, dim3((M6_STREAM_FRAGS + 3) / 4), dim3(256), 0, s, p, (uint4*)out);
  return hipGetLastError();
}

hipError_t launch_mixed6a(const Mixed6aArgs& a, int dtype, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  if (dtype == BF16) return launch_with_lds<mixed6a_chain_kernel<__bf16>>(a.n, 512, M6_LDS, s, a);
  if (dtype == F16) return launch_with_lds<mixed6a_chain_kernel<_Float16>>(a.n, 512, M6_LDS, s, a);
  return hipErrorInvalidValue;
}

}  // namespace vnf
