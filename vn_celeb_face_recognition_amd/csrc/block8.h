// Launch interface of the Block8 branch-chain kernel (block8.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace vnf {

constexpr int B8_G = 3;          // whole 3x3 images per workgroup: 27 of the 32 pixel rows it addresses
constexpr int B8_BIAS = 768;     // fp32 biases per block: 384 reduce (branch0 | branch1.0) | 192 (1x3) | 192 (3x1)

struct Block8Args {
  const void* x;        // (n, 9, ldx) 16-bit NHWC block input (first 1792 channels of each pixel row)
  void* y;              // (n, 9, ldy) the 384-channel concat: [branch0 | branch1 chain]
  int ldx, ldy, n;
  const void* wstream;  // block8_repack output
  const float* bias;    // [B8_BIAS]
};

// packed per-convolution weights [rows][kpad] (engine layout, k = (kh, kw, c)), device pointers
struct Block8Pack {
  const void* w[3];     // reduce (384 rows, K 1792), 1x3 (192, 576), 3x1 (192, 576)
  int kpad[3];
};

size_t block8_stream_bytes();
hipError_t block8_repack(const Block8Pack& p, void* out, hipStream_t s);
hipError_t launch_block8(const Block8Args& a, int dtype, hipStream_t s);

}  // namespace vnf
