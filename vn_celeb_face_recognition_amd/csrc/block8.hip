// Block8 branch chain (inception_resnet_v1.py:98-126) as ONE launch on gfx950: the fused reducer 1x1 1792 -> (192 | 192)
// and, behind its second half, the 1x3 and 3x1 192 -> 192 convolutions, written as the 384-channel concat the block's
// up-projection reads.  The tensors are 3 x 3 pixels, so the three plan convolutions are pure weight traffic
// (1.38 + 0.22 + 0.22 MB against 32 KB of activations per image) behind a serial K loop; this kernel takes the form of
// trunk17.hip instead.
//
// Work split
//   * blockIdx.x = a group of B8_G = 3 whole images: 27 pixel rows of the 32 (two MFMA pixel tiles) a workgroup
//     addresses.  Rows past the group's last valid row are loaded from that row (in bounds, finite or not: a pixel is one
//     MFMA column, so it cannot reach another pixel's sum) and are never stored;
//   * blockIdx.y selects the role (role = 1 - blockIdx.y: the longer one is dispatched first).  Role 0 computes reducer rows 0..191 (branch0) and stores concat channels 0..191.  Role 1 computes
//     reducer rows 192..383 (branch1.0) into LDS, then 1x3 and 3x1 out of LDS, and stores concat channels 192..383.
//     The roles share nothing but their input, so no flag or grid-wide barrier couples them.
//
// What stays where
//   * the group's input rows go to LDS once at full depth, by LDS-DMA: 28 K tiles of [32 rows][128 B] = 112 KiB, 16-byte
//     slots XOR-swizzled by row & 7 (the image of trunk17.hip / conv_igemm.hip: conflict-free ds_read_b128).  The
//     branch1.0 and 1x3 outputs of role 1 are 3 K tiles (12 KiB) each in the same image; 1x3 / 3x1 taps are rows +-1 /
//     +-3 of it, and a tap that leaves its own image reads one zero chunk (fed to the MFMA, not skipped);
//   * weights stream L2 -> registers.  The 12 waves split the 192 output channels of every convolution (one 16-channel
//     tile each), so a 1-KiB weight fragment is used by exactly one wave; block8_repack lays every wave's fragments out
//     in the order the wave consumes them (56 reducer steps, then 18 + 18 for role 1), and the wave keeps a ring of
//     B8_RING = 8 of them in flight, across the phase boundaries.  No LDS-DMA and no barrier inside a K loop.
//
// Bytes in flight: 12 waves x 8 fragments x 1 KiB = 96 KiB per workgroup and CU (LDS admits one workgroup per CU), above
// the ~70 KB that Little's law asks for at ~70 GB/s per-CU L2 ingest and ~1 us of latency.  Barriers: input resident |
// reduce done | 1x3 done.
//
// Numerics: bit-identical to the per-convolution plan.  Same MFMA (v_mfma_f32_16x16x32, weights as A, pixels as B), every
// convolution from a zero accumulator in ascending 32-deep k steps with k = (kh, kw, c), then the plan's fast epilogue
// (conv_device.h): v = acc + bias, max(v, 0), round to T -- at the same four points (t8a, t8b, both concat halves).
#include "block8.h"
#include "fused_device.h"

namespace vnf {

namespace {

constexpr int B8_ROWS = 32;                        // pixel rows addressed per workgroup
constexpr int B8_WAVES = 12;                       // one 16-channel output tile of every convolution per wave
constexpr int B8_RING = 8;                         // weight fragments in flight per wave
constexpr int B8_KS_RED = 56;                      // 32-deep k steps of the reducer (K = 1792)
constexpr int B8_KS_TAP = 18;                      // of 1x3 / 3x1 (K = 3 x 192)
constexpr int B8_FRAGS0 = B8_KS_RED;               // fragments per wave, role 0
constexpr int B8_FRAGS1 = B8_KS_RED + 2 * B8_KS_TAP;   // role 1
constexpr int B8_SLOT0 = B8_FRAGS0 + B8_RING;      // stream slots per wave: the ring's read-ahead lands in zero padding
constexpr int B8_SLOT1 = B8_FRAGS1 + B8_RING;
constexpr int B8_STREAM_FRAGS = B8_WAVES * (B8_SLOT0 + B8_SLOT1);
constexpr int KT_BYTES = B8_ROWS * 128;            // one K tile (64 channels) of the 32 rows
constexpr int OFF_X = 0;                           // 28 K tiles: the block input
constexpr int OFF_TA = 28 * KT_BYTES;              // 3 K tiles: branch1.0 output
constexpr int OFF_TB = 31 * KT_BYTES;              // 3 K tiles: 1x3 output
constexpr int OFF_ZERO = 34 * KT_BYTES;            // 256 zero bytes: out-of-image taps
constexpr int B8_LDS = 34 * KT_BYTES + 256;
static_assert(B8_G * 9 <= B8_ROWS, "the group's rows fit the two pixel tiles");
static_assert(B8_LDS <= 160 * 1024, "one workgroup's LDS");

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
__global__ __launch_bounds__(B8_WAVES * 64) void block8_chain_kernel(const Block8Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int frow = lane & 15, fgrp = lane >> 4;
  const int role = 1 - (int)blockIdx.y;            // the longer role's workgroups are dispatched first
  const int img0 = blockIdx.x * B8_G;
  const int nrows = 9 * min(B8_G, a.n - img0);   // valid pixel rows of this group (>= 9: the grid has no empty group)
  const unsigned lds0 = lds_dma_base(smem);

  // ---- weight stream of this wave: fragment f at wp + f * 64 (uint4 units); the first B8_RING go out before the input
  const uint4* wp = reinterpret_cast<const uint4*>(a.wstream) +
                    (size_t)(role == 0 ? wave * B8_SLOT0 : B8_WAVES * B8_SLOT0 + wave * B8_SLOT1) * 64 + lane;
  uint4 wq[B8_RING];
  ring_prime(wq, wp);
  // the wave's biases, ahead of the stream: a load issued at a phase boundary would be waited for behind the whole ring
  const int cw = 16 * wave + 4 * fgrp;             // first of the lane's 4 output channels inside a 192-channel convolution
  const f32x4_t bv_red = *reinterpret_cast<const f32x4_t*>(a.bias + role * 192 + cw);
  f32x4_t bv_tap[2] = {bv_red, bv_red};
  if (role == 1) {
    bv_tap[0] = *reinterpret_cast<const f32x4_t*>(a.bias + 384 + cw);
    bv_tap[1] = *reinterpret_cast<const f32x4_t*>(a.bias + 576 + cw);
  }

  // ---- input rows -> LDS by LDS-DMA: piece = 8 pixel rows x 128 B of one K tile, 112 pieces over the 12 waves
  {
    const char* src = (const char*)a.x + (size_t)img0 * 9 * a.ldx * 2;
    const int r = lane >> 3, slot = lane & 7;
#pragma unroll
    for (int i = 0; i < (112 + B8_WAVES - 1) / B8_WAVES; ++i) {
      const int piece = wave + i * B8_WAVES;       // [kt 0..27][row group 0..3]
      if (piece < 112) {
        const int kt = piece >> 2, rg = piece & 3;
        const int p = min(rg * 8 + r, nrows - 1);  // rows behind the group's last: that row again
        glds16(src + ((size_t)p * a.ldx + kt * 64 + ((slot ^ r) << 3)) * 2, lds0 + OFF_X + kt * KT_BYTES + rg * 1024);
      }
    }
    if (tid < 16) reinterpret_cast<uint4*>(smem + OFF_ZERO)[tid] = uint4{0u, 0u, 0u, 0u};
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __syncthreads();

  // Per-lane LDS offsets inside the K-tile image (fused_device.h).  B-fragment read of pixel 16*i + frow, k step ks of
  // K tile kt: kt * KT_BYTES + i * 2048 + (ks & 1 ? rb1 : rb0).  This wave's accumulator quad of that pixel: wb + i * 2048.
  const int rb0 = ktile_slot(frow, fgrp), rb1 = rb0 ^ 64;
  const int wb = (cw >> 6) * KT_BYTES + frow * 128 + ((((cw & 63) >> 3) ^ (frow & 7)) << 4) + (cw & 4) * 2;   // ktile_quad, written out (trunk17.hip)
  char* yrow = (char*)a.y + ((size_t)(img0 * 9 + frow) * a.ldy + role * 192 + cw) * 2;   // pixel tile i: + i * 16 rows

  // ---------------------------------------------------------------- reduce 1x1: rows role * 192 + 16 * wave .. + 15
  {
    f32x4_t acc[2] = {f32x4_t{0.f, 0.f, 0.f, 0.f}, f32x4_t{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int ks = 0; ks < B8_KS_RED; ++ks) {
      uint4 xf[2];
#pragma unroll
      for (int i = 0; i < 2; ++i)
        xf[i] = *reinterpret_cast<const uint4*>(smem + OFF_X + (ks >> 1) * KT_BYTES + i * 2048 + ((ks & 1) ? rb1 : rb0));
#pragma unroll
      for (int i = 0; i < 2; ++i) mma_chunk<T>(acc[i], wq[ks % B8_RING], xf[i]);
      ring_refill(wq, ks, wp);
      __builtin_amdgcn_sched_barrier(0);
    }
    const f32x4_t bv = bv_red;
    if (role == 0) {   // branch0: concat channels 0..191, valid rows only
#pragma unroll
      for (int i = 0; i < 2; ++i)
        if (16 * i + frow < nrows) *reinterpret_cast<uint2*>(yrow + (size_t)i * 16 * a.ldy * 2) = bias_relu_round<T>(acc[i], bv);
      return;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) *reinterpret_cast<uint2*>(smem + OFF_TA + wb + i * 2048) = bias_relu_round<T>(acc[i], bv);
  }
  __syncthreads();

  // ---------------------------------------------------------------- 1x3 (pad 0,1) then 3x1 (pad 1,0), k = tap * 192 + c
  int px[2], py[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int p = 16 * i + frow, q = p % 9;
    const bool live = p < 9 * B8_G;                // the tile's padding rows take every tap from the zero chunk
    py[i] = live ? q / 3 : -8;
    px[i] = live ? q % 3 : -8;
  }
#pragma unroll
  for (int ph = 0; ph < 2; ++ph) {
    const int src_off = ph == 0 ? OFF_TA : OFF_TB;
    f32x4_t acc[2] = {f32x4_t{0.f, 0.f, 0.f, 0.f}, f32x4_t{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int ks = 0; ks < B8_KS_TAP; ++ks) {
      const int tap = ks / 6, kt = (ks % 6) >> 1, half = ks & 1;
      uint4 xf[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        // the tap's pixel inside the lane's own image, or outside it: never a neighbouring image of the group
        const bool ok = (unsigned)((ph == 0 ? px[i] : py[i]) + tap - 1) < 3u;
        const int row = 16 * i + frow + (ph == 0 ? tap - 1 : 3 * (tap - 1));
        const int off = src_off + kt * KT_BYTES + row * 128 + (((half * 4 + fgrp) ^ (row & 7)) << 4);
        xf[i] = *reinterpret_cast<const uint4*>(smem + (ok ? off : OFF_ZERO));
      }
      const int s = B8_KS_RED + B8_KS_TAP * ph + ks;
#pragma unroll
      for (int i = 0; i < 2; ++i) mma_chunk<T>(acc[i], wq[s % B8_RING], xf[i]);
      ring_refill(wq, s, wp);
      __builtin_amdgcn_sched_barrier(0);
    }
    const f32x4_t bv = bv_tap[ph];
    if (ph == 0) {
#pragma unroll
      for (int i = 0; i < 2; ++i) *reinterpret_cast<uint2*>(smem + OFF_TB + wb + i * 2048) = bias_relu_round<T>(acc[i], bv);
      __syncthreads();
    } else {           // concat channels 192..383, valid rows only
#pragma unroll
      for (int i = 0; i < 2; ++i)
        if (16 * i + frow < nrows) *reinterpret_cast<uint2*>(yrow + (size_t)i * 16 * a.ldy * 2) = bias_relu_round<T>(acc[i], bv);
    }
  }
}

// ---------------------------------------------------------------------------------------------- weight stream
// Slot order: the 12 waves of role 0 (B8_SLOT0 fragments each), then the 12 waves of role 1 (B8_SLOT1 each); behind a
// wave's fragments, B8_RING zero fragments for the ring's read-ahead.  Fragment s of wave w (the kernel's consumption order):
//   role 0   s 0..55    reducer rows 16w .. +15,        k = 32s .. +31
//   role 1   s 0..55    reducer rows 192 + 16w .. +15,  k = 32s .. +31
//            s 56..73   1x3 rows 16w .. +15,            k = 32(s - 56) .. +31
//            s 74..91   3x1 rows 16w .. +15,            k = 32(s - 74) .. +31
__global__ void block8_repack_kernel(Block8Pack p, uint4* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int frag = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (frag >= B8_STREAM_FRAGS) return;
  int conv = -1, r0 = 0, k0 = 0;
  if (frag < B8_WAVES * B8_SLOT0) {
    const int wave = frag / B8_SLOT0, s = frag - wave * B8_SLOT0;
    if (s < B8_FRAGS0) { conv = 0; r0 = 16 * wave; k0 = 32 * s; }
  } else {
    const int f = frag - B8_WAVES * B8_SLOT0;
    const int wave = f / B8_SLOT1, s = f - wave * B8_SLOT1;
    if (s < B8_KS_RED) { conv = 0; r0 = 192 + 16 * wave; k0 = 32 * s; }
    else if (s < B8_KS_RED + B8_KS_TAP) { conv = 1; r0 = 16 * wave; k0 = 32 * (s - B8_KS_RED); }
    else if (s < B8_FRAGS1) { conv = 2; r0 = 16 * wave; k0 = 32 * (s - B8_KS_RED - B8_KS_TAP); }
  }
  uint4 v = {0u, 0u, 0u, 0u};
  if (conv >= 0) v = GatherA16::load(p.w[conv], p.kpad[conv], r0, k0, lane, 0);
  out[(size_t)frag * 64 + lane] = v;
}

size_t block8_stream_bytes() { return (size_t)B8_STREAM_FRAGS * 1024; }

hipError_t block8_repack(const Block8Pack& p, void* out, hipStream_t s) {
  hipLaunchKernelGGL(block8_repack_kernel, dim3((B8_STREAM_FRAGS + 3) / 4), dim3(256), 0, s, p, (uint4*)out);
  return hipGetLastError();
}

hipError_t launch_block8(const Block8Args& a, int dtype, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  const dim3 grid((a.n + B8_G - 1) / B8_G, 2);
  if (dtype == BF16) return launch_with_lds<block8_chain_kernel<__bf16>>(grid, B8_WAVES * 64, B8_LDS, s, a);
  if (dtype == F16) return launch_with_lds<block8_chain_kernel<_Float16>>(grid, B8_WAVES * 64, B8_LDS, s, a);
  return hipErrorInvalidValue;
}

}  // namespace vnf
