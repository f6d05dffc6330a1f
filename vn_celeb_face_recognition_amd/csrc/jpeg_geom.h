// Geometry of a baseline JPEG frame as the device kernels of jpeg_decode.hip and jpeg_encode.hip see it: the MCU-padded
// block grid of every component plane.  A plane's samples (one byte each) and its coefficients (64 int16 per block)
// share one set of offsets.
#pragma once
#include "../../include/vnface.h"

namespace vnf {

struct JpegGeom {
  int ncomp;
  int bw[3], bh[3];          // blocks per row / column of each plane
  long long plane_off[3];    // of a plane inside a frame's planes, in bytes (and, times 64 int16, its coefficients)
  long long plane_frame;     // bytes of a frame's planes = coefficients of a frame
  long long blocks;          // per frame
  int cw, chh;               // real chroma samples per row / rows
};

static inline bool jpeg_geom(int width, int height, int sampling, JpegGeom* g) {
  int h0, v0;
  switch (sampling) {
    case VNF_JPEG_GRAY: g->ncomp = 1; h0 = 1; v0 = 1; break;
    case VNF_JPEG_444: g->ncomp = 3; h0 = 1; v0 = 1; break;
    case VNF_JPEG_422: g->ncomp = 3; h0 = 2; v0 = 1; break;
    case VNF_JPEG_420: g->ncomp = 3; h0 = 2; v0 = 2; break;
    default: return false;
  }
  const int mx = (width + 8 * h0 - 1) / (8 * h0), my = (height + 8 * v0 - 1) / (8 * v0);
  long long co = 0;
  for (int c = 0; c < 3; ++c) {
    const bool on = c < g->ncomp;
    g->bw[c] = on ? mx * (c ? 1 : h0) : 0;
    g->bh[c] = on ? my * (c ? 1 : v0) : 0;
    g->plane_off[c] = co;  // 64 coefficients become 64 bytes
    co += 64LL * g->bw[c] * g->bh[c];
  }
  g->plane_frame = co;
  g->blocks = co / 64;
  g->cw = (width + h0 - 1) / h0;
  g->chh = (height + v0 - 1) / v0;
  return true;
}

}  // namespace vnf
