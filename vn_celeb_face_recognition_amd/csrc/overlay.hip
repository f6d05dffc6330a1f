// Boxes and names drawn on frames that live in HBM: what cli_utils.draw_boxes_on_image (Pillow's ImageDraw.rectangle
// with width 2 and ImageDraw.text; /root/reference/demo_image.py:150-158) paints, in place, in one launch, so that an
// annotated video frame never has to visit the host as pixels.
//
// A thread owns one pixel and walks the op table in order, applying the ops of its frame that cover it: later ops
// paint over earlier ones exactly as consecutive Pillow calls do, and no two threads touch the same byte.  The faces
// of a batch are few (the table is tens of entries), every lane of a wave reads the same entry, and a pixel nothing
// covers -- nearly all of them -- is neither read nor written.
//   * rectangle: the pixels of [x0..x1] x [y0..y1] outside [x0+2..x1-2] x [y0+2..y1-2], opaque;
//   * label: a tw x th u8 coverage mask the host rendered with the font (FreeType's sub-pixel placement stays
//     Pillow's), blended per channel as Pillow's paste does: v = bg (255 - m) + c m + 128, out = ((v >> 8) + v) >> 8.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "engine.h"

namespace vnf {

__global__ void __launch_bounds__(256) overlay_kernel(uint8_t* __restrict__ frames, int b, int H, int W,
                                                      const vnf_overlay_op* __restrict__ ops, int n_ops,
                                                      const uint8_t* __restrict__ masks, long long masks_bytes) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)b * H * W) return;
  const long long row = t / W;
  const int x = (int)(t - row * W);
  const int f = (int)(row / H), y = (int)(row - (long long)f * H);
  int r = 0, g = 0, bl = 0;
  bool have = false, dirty = false;
  uint8_t* px = frames + (size_t)t * 3;
  for (int k = 0; k < n_ops; ++k) {
    const vnf_overlay_op op = ops[k];
    if (op.frame != f) continue;              // also: a frame index outside 0..b-1 belongs to nobody
    const int cr = op.rgb & 255, cg = (op.rgb >> 8) & 255, cb = (op.rgb >> 16) & 255;
    if (op.kind == VNF_OVERLAY_RECT) {
      if (x < op.x0 || x > op.x1 || y < op.y0 || y > op.y1) continue;
      // the hole, in 64 bits: a corner near INT_MAX must not wrap
      if (x >= (long long)op.x0 + 2 && x <= (long long)op.x1 - 2 && y >= (long long)op.y0 + 2 && y <= (long long)op.y1 - 2) continue;
      r = cr; g = cg; bl = cb;
      have = dirty = true;
    } else if (op.kind == VNF_OVERLAY_LABEL) {
      const long long tx = (long long)x - op.x0, ty = (long long)y - op.y0;   // x1, y1 hold the mask's width and height
      if (tx < 0 || ty < 0 || tx >= op.x1 || ty >= op.y1) continue;
      const long long at = (long long)op.mask_offset + ty * op.x1 + tx;
      if (op.mask_offset < 0 || (long long)op.mask_offset + (long long)op.x1 * op.y1 > masks_bytes) continue;
      const int m = masks[at];
      if (!m) continue;
      if (!have) { r = px[0]; g = px[1]; bl = px[2]; have = true; }
      int v = r * (255 - m) + cr * m + 128;
      r = ((v >> 8) + v) >> 8;
      v = g * (255 - m) + cg * m + 128;
      g = ((v >> 8) + v) >> 8;
      v = bl * (255 - m) + cb * m + 128;
      bl = ((v >> 8) + v) >> 8;
      dirty = true;
    }
  }
  if (dirty) {
    px[0] = (uint8_t)r;
    px[1] = (uint8_t)g;
    px[2] = (uint8_t)bl;
  }
}

}  // namespace vnf

using namespace vnf;

extern "C" int vnf_overlay_draw(uint8_t* frames_dev, int b, int height, int width, const vnf_overlay_op* ops_dev,
                                int n_ops, const uint8_t* masks_dev, int64_t masks_bytes, void* stream) {
  if (b == 0 || n_ops == 0) return VNF_OK;
  if (b < 0 || n_ops < 0 || height < 1 || width < 1 || height > 65535 || width > 65535 || !frames_dev || !ops_dev ||
      masks_bytes < 0 || (masks_bytes > 0 && !masks_dev))
    return fail(VNF_E_INVALID, "vnf_overlay_draw: bad argument");
  if ((uintptr_t)ops_dev & 3) return fail(VNF_E_INVALID, "vnf_overlay_draw: ops_dev must be 4-byte aligned");
  const long long blocks = ((long long)b * height * width + 255) / 256;
  if (blocks > 0x7fffffffLL) return fail(VNF_E_CAPACITY, "vnf_overlay_draw: batch too large for one grid");
  hipLaunchKernelGGL(overlay_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, frames_dev, b, height,
                     width, ops_dev, n_ops, masks_dev, (long long)masks_bytes);
  VNF_HIP(hipGetLastError());
  return VNF_OK;
}
