// The one-workgroup exclusive scan: the device Huffman coder and decoder (jpeg_huff_device.hip, jpeg_huff_decode.hip)
// and cluster_number_kernel (gallery_cluster.hip), which numbers the clusters of f-17 and the tracks of f-18.  Device
// code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vnf {

constexpr int kScanLanes = 1024;    // one workgroup per frame, four entries per lane and step

// Exclusive scan of a[0, count) in place by one workgroup of kScanLanes lanes -> the sum.  a is 16-byte aligned and
// readable and writable up to the next multiple of 4 entries.  Steps of 4 * kScanLanes entries: a lane sums its four,
// a wave scans its lanes' sums with shuffles, LDS carries the waves' sums, a register the steps'.
__device__ inline uint32_t block_scan(uint32_t* a, uint32_t count) {
  __shared__ uint32_t wsum[kScanLanes / 64];
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t carry = 0;
  for (uint32_t base = 0; base < count; base += 4 * kScanLanes) {
    const uint32_t i = base + 4 * threadIdx.x;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (i < count) v = *reinterpret_cast<const uint4*>(a + i);
    if (i + 1 >= count) v.y = 0;
    if (i + 2 >= count) v.z = 0;
    if (i + 3 >= count) v.w = 0;
    const uint32_t s0 = v.x, s1 = s0 + v.y, s2 = s1 + v.z, s3 = s2 + v.w;
    uint32_t incl = s3;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t up = __shfl_up(incl, d, 64);
      if ((int)lane >= d) incl += up;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (unsigned w = 0; w < kScanLanes / 64; ++w) {
      const uint32_t x = wsum[w];
      if (w < wave) before += x;
      all += x;
    }
    const uint32_t excl = carry + before + incl - s3;
    if (i < count) *reinterpret_cast<uint4*>(a + i) = make_uint4(excl, excl + s0, excl + s1, excl + s2);
    carry += all;
    __syncthreads();   // wsum is written again in the next step
  }
  return carry;
}

}  // namespace vnf
