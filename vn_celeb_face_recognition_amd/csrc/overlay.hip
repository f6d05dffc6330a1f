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

// Text runs: what consecutive ImageDraw.text((x, y), s, fill=colour) calls with integer anchors and the default font
// paint (cli_utils.draw_emotions: '<tag> - <percent>%' lines that differ per face and per frame, so no mask can be
// cached).  One workgroup owns one run; its threads cover the run's ink rectangle, clipped to the frame, so the work
// follows the text's area and not frame pixels x table length.
//   * the glyphs of the run are placed at pen positions equal to the sum of the preceding advances (the font's layout
//     is Pillow's BASIC one: integer advances, no kerning -- the host checks that before it builds an atlas);
//   * where glyphs overlap ('ff', 'fi') their coverages combine as Pillow's font renderer combines them,
//     dst += round(src (255 - dst) / 255), left to right;
//   * the coverage is pasted with the LABEL formula above.
// The runs of ONE launch must not intersect on a frame (two workgroups would race for the pixel); the host puts a run
// that intersects an earlier one into a later launch (vnf_overlay_draw_text's launch_ends).
__global__ void __launch_bounds__(256) overlay_text_kernel(uint8_t* __restrict__ frames, int b, int H, int W,
                                                           const vnf_text_run* __restrict__ runs,
                                                           const uint8_t* __restrict__ chars, long long chars_bytes,
                                                           const uint8_t* __restrict__ atlas, long long atlas_bytes) {
  __shared__ int g_x[VNF_TEXT_RUN_MAX], g_y[VNF_TEXT_RUN_MAX], g_w[VNF_TEXT_RUN_MAX], g_h[VNF_TEXT_RUN_MAX];
  __shared__ int g_at[VNF_TEXT_RUN_MAX], g_adv[VNF_TEXT_RUN_MAX];
  __shared__ int box[4];
  const vnf_text_run run = runs[blockIdx.x];
  // everything below up to the barrier is uniform over the workgroup: a run the table should not hold paints nothing
  if (run.frame < 0 || run.frame >= b || run.length < 1 || run.length > VNF_TEXT_RUN_MAX || run.first < 0 ||
      (long long)run.first + run.length > chars_bytes)
    return;
  const vnf_text_atlas hd = *reinterpret_cast<const vnf_text_atlas*>(atlas);
  if (hd.n_glyphs < 1 || hd.n_glyphs > 256) return;
  const long long cov0 = (long long)sizeof(vnf_text_atlas) + (long long)hd.n_glyphs * (long long)sizeof(vnf_text_glyph);
  if (cov0 > atlas_bytes) return;
  const vnf_text_glyph* glyphs = reinterpret_cast<const vnf_text_glyph*>(atlas + sizeof(vnf_text_atlas));
  const int t = threadIdx.x;
  if (t < run.length) {
    const int c = (int)chars[run.first + t] - hd.first_char;
    vnf_text_glyph g = {0, 0, 0, 0, 0, 0};
    if (c >= 0 && c < hd.n_glyphs) g = glyphs[c];
    // a glyph outside the atlas's own limits has no ink and does not move the pen
    const bool ok = g.w >= 0 && g.h >= 0 && g.w <= VNF_TEXT_GLYPH_MAX && g.h <= VNF_TEXT_GLYPH_MAX && g.offset >= 0 &&
                    cov0 + g.offset + (long long)g.w * g.h <= atlas_bytes && g.advance >= 0 && g.advance <= VNF_TEXT_GLYPH_MAX &&
                    g.ox >= -VNF_TEXT_GLYPH_MAX && g.ox <= VNF_TEXT_GLYPH_MAX && g.oy >= -VNF_TEXT_GLYPH_MAX && g.oy <= VNF_TEXT_GLYPH_MAX;
    g_x[t] = ok ? g.ox : 0;
    g_y[t] = ok ? g.oy : 0;
    g_w[t] = ok && g.h > 0 ? g.w : 0;
    g_h[t] = ok && g.w > 0 ? g.h : 0;
    g_at[t] = ok ? g.offset : 0;
    g_adv[t] = ok ? g.advance : 0;
  }
  __syncthreads();
  if (t == 0) {
    int pen = 0, x0 = 0x7fffffff, y0 = 0x7fffffff, x1 = -0x7fffffff, y1 = -0x7fffffff;   // at most 64 * 128 away from 0
    for (int k = 0; k < run.length; ++k) {
      const int gx = pen + g_x[k];
      g_x[k] = gx;
      pen += g_adv[k];
      if (!g_w[k]) continue;
      x0 = min(x0, gx);
      x1 = max(x1, gx + g_w[k]);
      y0 = min(y0, g_y[k]);
      y1 = max(y1, g_y[k] + g_h[k]);
    }
    box[0] = x0; box[1] = y0; box[2] = x1; box[3] = y1;
  }
  __syncthreads();
  if (box[2] <= box[0]) return;                                 // no ink (spaces only)
  // the ink rectangle in frame coordinates, in 64 bits (an anchor may sit anywhere in int32), clipped to the frame
  const long long fx0 = max(0LL, (long long)run.x + box[0]), fx1 = min((long long)W, (long long)run.x + box[2]);
  const long long fy0 = max(0LL, (long long)run.y + box[1]), fy1 = min((long long)H, (long long)run.y + box[3]);
  if (fx1 <= fx0 || fy1 <= fy0) return;
  const int rw = (int)(fx1 - fx0), rh = (int)(fy1 - fy0);       // at most 64 * 128 + 64 by 128
  const int cr = run.rgb & 255, cg = (run.rgb >> 8) & 255, cb = (run.rgb >> 16) & 255;
  const uint8_t* cov = atlas + cov0;
  for (int p = t; p < rw * rh; p += 256) {
    const int py = p / rw, px = p - py * rw;
    const int lx = (int)(fx0 + px - run.x), ly = (int)(fy0 + py - run.y);   // relative to the anchor: inside the box
    int m = 0;
    for (int k = 0; k < run.length; ++k) {
      const int tx = lx - g_x[k], ty = ly - g_y[k];
      if (tx < 0 || ty < 0 || tx >= g_w[k] || ty >= g_h[k]) continue;
      const int v = cov[g_at[k] + ty * g_w[k] + tx] * (255 - m) + 128;
      m += ((v >> 8) + v) >> 8;
    }
    if (!m) continue;
    uint8_t* q = frames + (((size_t)run.frame * H + (size_t)(fy0 + py)) * W + (size_t)(fx0 + px)) * 3;
    int v = q[0] * (255 - m) + cr * m + 128;
    q[0] = (uint8_t)(((v >> 8) + v) >> 8);
    v = q[1] * (255 - m) + cg * m + 128;
    q[1] = (uint8_t)(((v >> 8) + v) >> 8);
    v = q[2] * (255 - m) + cb * m + 128;
    q[2] = (uint8_t)(((v >> 8) + v) >> 8);
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

extern "C" int vnf_overlay_draw_text(uint8_t* frames_dev, int b, int height, int width, const vnf_text_run* runs_dev,
                                     int n_runs, const int32_t* launch_ends, int n_launches, const uint8_t* chars_dev,
                                     int64_t chars_bytes, const void* atlas_dev, int64_t atlas_bytes, void* stream) {
  if (b == 0 || n_runs == 0) return VNF_OK;
  if (b < 0 || n_runs < 0 || height < 1 || width < 1 || height > 65535 || width > 65535 || !frames_dev || !runs_dev ||
      chars_bytes < 0 || (chars_bytes > 0 && !chars_dev) || !atlas_dev || atlas_bytes < (int64_t)sizeof(vnf_text_atlas))
    return fail(VNF_E_INVALID, "vnf_overlay_draw_text: bad argument");
  if (((uintptr_t)runs_dev & 3) || ((uintptr_t)atlas_dev & 3))
    return fail(VNF_E_INVALID, "vnf_overlay_draw_text: runs_dev and atlas_dev must be 4-byte aligned");
  const int32_t one = n_runs;
  if (!launch_ends) {
    launch_ends = &one;
    n_launches = 1;
  }
  if (n_launches < 1 || launch_ends[n_launches - 1] != n_runs)
    return fail(VNF_E_INVALID, "vnf_overlay_draw_text: launch_ends must end at n_runs");
  for (int i = 0, at = 0; i < n_launches; at = launch_ends[i++])
    if (launch_ends[i] <= at) return fail(VNF_E_INVALID, "vnf_overlay_draw_text: launch_ends must ascend from above 0");
  for (int i = 0, at = 0; i < n_launches; at = launch_ends[i++]) {
    hipLaunchKernelGGL(overlay_text_kernel, dim3((unsigned)(launch_ends[i] - at)), dim3(256), 0, (hipStream_t)stream,
                       frames_dev, b, height, width, runs_dev + at, chars_dev, (long long)chars_bytes,
                       (const uint8_t*)atlas_dev, (long long)atlas_bytes);
    VNF_HIP(hipGetLastError());
  }
  return VNF_OK;
}
