// Device-side pieces shared by the fused-stack kernels (stem_mid*.hip, block35*.hip, trunk35.hip, trunk17*.hip,
// block8.hip).  The MFMA itself is mma_chunk<T> / mfma_f16 of conv_device.h.  Everything here is inlined: a kernel that
// uses a helper compiles to the code it had with the helper's body written out.
//
// Lane roles.  Every kernel runs 64-lane waves on v_mfma_f32_16x16x32 with the weights as A and the pixels as B:
//   * lane l of an A or B fragment holds the 8 k values 8 * (l >> 4) .. + 7 of row / pixel l & 15;
//   * lane l of an accumulator holds the 4 output channels 4 * (l >> 4) .. + 3 of pixel l & 15 (a "quad").
// frow = l & 15 and fgrp = l >> 4 are those two coordinates.
//
// LDS images.
//   * K-tile image: [tile][row][128 B].  A row is a pixel, its 128 bytes eight 16-byte slots, slot s stored at
//     s ^ (row & 7): the 16 rows x 4 slots of one ds_read_b128 B-fragment read fall on different banks.  In a 16-bit
//     image a tile is 64 channels and slot s holds channels 8s .. 8s + 7; k step ks of the tile reads slot
//     4 * (ks & 1) + fgrp.  In a planar split-f16 image a tile is 32 channels: slots 0..3 hold the hi planes of the four
//     8-channel units, slots 4..7 their lo planes, so the lo half of anything sits at the hi address ^ 64.
//   * 64-byte-row image: [row][64 B] = 32 channels of 16 bits, four 16-byte chunks, chunk c stored at
//     c ^ ((-(row >> 2)) & 3).
//
// Weight streams.  A fragment is 1 KiB = 64 lanes x 16 bytes in MFMA A order, written by a repack kernel at create time
// in the order its consumer reads it (GatherA16 / GatherA16P); the kernels that stream weights to registers keep a
// ring of fragments per wave (ring_prime / ring_refill), and every stream ends in RING zero fragments for the ring's
// read-ahead.
//
// These kernels sit at their register limits and the compiler folds address arithmetic differently through a call
// than written out, so a kernel uses a helper only where its assembly is the same with it.  What stayed written out:
// every kernel's opening tid / lane / wave / frow / fgrp lines, ktile_quad in trunk17.hip and block8.hip, and the
// input-rows-to-image LDS-DMA loops (each clamps and groups its rows its own way).
#pragma once
#include "conv_device.h"

namespace vnf {

// the workgroup's dynamic LDS as an LDS-DMA base (glds16)
__device__ __forceinline__ unsigned lds_dma_base(char* smem) {
  return (unsigned)reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) char*)smem);
}

// an accumulator quad rounded to T (8 bytes), and back
template <typename T>
__device__ __forceinline__ uint2 pack4(const f32x4_t& v) {
  typedef T t4 __attribute__((ext_vector_type(4)));
  t4 r = {(T)v[0], (T)v[1], (T)v[2], (T)v[3]};
  return __builtin_bit_cast(uint2, r);
}
template <typename T>
__device__ __forceinline__ f32x4_t unpack4(const uint2& u) {
  typedef T t4 __attribute__((ext_vector_type(4)));
  const t4 r = __builtin_bit_cast(t4, u);
  return f32x4_t{(float)r[0], (float)r[1], (float)r[2], (float)r[3]};
}

// a quad as planar split-f16 (hi, lo) halves (split_f16.h), and back
__device__ __forceinline__ void split4(const f32x4_t& v, uint2& hi, uint2& lo) {
  typedef _Float16 h4 __attribute__((ext_vector_type(4)));
  h4 h, l;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const sf16 s(v[e]);
    h[e] = s.hi; l[e] = s.lo;
  }
  hi = __builtin_bit_cast(uint2, h);
  lo = __builtin_bit_cast(uint2, l);
}
__device__ __forceinline__ f32x4_t join4(const uint2& hi, const uint2& lo) {
  typedef _Float16 h4 __attribute__((ext_vector_type(4)));
  const h4 h = __builtin_bit_cast(h4, hi), l = __builtin_bit_cast(h4, lo);
  return f32x4_t{(float)h[0] + (float)l[0], (float)h[1] + (float)l[1], (float)h[2] + (float)l[2], (float)h[3] + (float)l[3]};
}

template <int N>
__device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// 64-byte-row image: byte offset of the 16-byte chunk `chunk` (0..3) of row q
__device__ __forceinline__ int row64_chunk(int q, int chunk) { return q * 64 + ((chunk ^ ((0 - (q >> 2)) & 3)) << 4); }

// K-tile image: byte offset of 16-byte slot `slot` (0..7) of row `row` inside a tile.  The B-fragment read of pixel
// 16 * i + frow, k step ks of a 16-bit tile is at i * 2048 + (ks & 1 ? rb ^ 64 : rb) with rb = ktile_slot(frow, fgrp); of
// a planar tile, rb is the hi plane and rb ^ 64 the lo plane.
__device__ __forceinline__ int ktile_slot(int row, int slot) { return row * 128 + ((slot ^ (row & 7)) << 4); }
// ... and of the accumulator quad of channels cw .. cw + 3 of pixel frow (+ i * 2048 for pixel 16 * i + frow) in an image
// of TILE_BYTES per tile and CH channels per tile (64: 16-bit, 8 bytes per quad; 32: planar, the hi half)
template <int TILE_BYTES, int CH>
__device__ __forceinline__ int ktile_quad(int cw, int frow) {
  static_assert(CH == 64 || CH == 32, "channels per tile");
  return (cw >> (CH == 64 ? 6 : 5)) * TILE_BYTES + frow * 128 + ((((cw & (CH - 1)) >> 3) ^ (frow & 7)) << 4) + (cw & 4) * 2;
}

// per-wave weight ring: fragment f of the wave's stream at wp + f * 64 (wp includes the lane).  Prime fetches the first
// RING; the consumer of fragment s uses wq[s % RING], then refills that slot with fragment s + RING.
template <int RING>
__device__ __forceinline__ void ring_prime(uint4 (&wq)[RING], const uint4*& wp) {
#pragma unroll
  for (int r = 0; r < RING; ++r) wq[r] = wp[r * 64];
  wp += RING * 64;
}
template <int RING>
__device__ __forceinline__ void ring_refill(uint4 (&wq)[RING], int s, const uint4*& wp) {
  wq[s % RING] = *wp;
  wp += 64;
}

// The repack kernels' gather of one MFMA A fragment from packed engine weights [rows][kpad] (k = (kh, kw, c)): lane l
// takes the 8 k values k0 + 8 * (l >> 4) .. + 7 of row r0 + (l & 15).  16-bit weights; and one plane (0 hi, 1 lo) of
// F16P weights, which keep a K tile of 32 k values as [32 hi halves][32 lo halves] (k0 a multiple of 32).
struct GatherA16 {
  static constexpr int PLANES = 1;
  static __device__ __forceinline__ uint4 load(const void* w, int kpad, int r0, int k0, int lane, int) {
    return *reinterpret_cast<const uint4*>((const char*)w + ((size_t)(r0 + (lane & 15)) * kpad + k0 + 8 * (lane >> 4)) * 2);
  }
};
struct GatherA16P {
  static constexpr int PLANES = 2;
  static __device__ __forceinline__ uint4 load(const void* w, int kpad, int r0, int k0, int lane, int plane) {
    return *reinterpret_cast<const uint4*>((const char*)w + ((size_t)(r0 + (lane & 15)) * kpad + k0) * 4 + plane * 64 + (lane >> 4) * 16);
  }
};

}  // namespace vnf
