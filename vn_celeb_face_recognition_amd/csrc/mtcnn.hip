// MTCNN P/R/O-Net cascade on the device (gfx950), restating
//   /root/reference/models/mtcnn_utils/detect_face.py:25-185 (detect_face) and helpers 188-306,
//   /root/reference/models/mtcnn.py:38-49, 84-99, 138-157 (the three nets), 326-347 (area ordering).
//
// Everything between "frames are in HBM" and "final boxes" stays on the device: the image pyramid,
// the three nets, threshold + compaction, all four NMS passes, box regression / squaring / padding
// and the per-candidate crop+resize that the reference does in Python loops.  fp32 everywhere
// (thin channels: 3..128; the path is HBM / latency bound, not FLOP bound), explicit op order
// (built with -ffp-contract=off, FMAs only where written) so box arithmetic and IoU tests are
// bit-identical to the fp32 numpy / torch-CPU statements of the oracle.
//
// Kernel map:
//   K1 pyramid_rows_kernel   u8 frame -> all pyramid levels (area bins of area_sum.h, normalised); pyramid_kernel for
//      frames whose rows or base address are not 16-byte aligned, or whose rows exceed 64 KiB of LDS as fp32
//   K2 pnet_conv1_pool_direct / pnet_conv2 / pnet_conv3_heads   (all levels and frames per launch)
//   K3 threshold + compaction fused into pnet_conv3_heads (wave-aggregated atomic slots;
//      order restored by the sort keys, which carry the cell index)
//   K4 nms_scale_kernel (per level x frame, IoU 0.5), nms_image_kernel (per frame, IoU 0.7,
//      + regress, rerec, pad), stage2_post_kernel (IoU 0.7 + bbreg + rerec + pad)
//   K5 crop_resize_rows_kernel   box table -> N x {24,48}^2 x 4 (the same area bins, also up-sampling); unaligned
//      frames and crops wider than a strip of column sums take its per-pixel branch
//   K6 net_front_kernel (conv1 + pool1), net_mid_kernel (conv2 + pool2), then the rest of R-Net / O-Net as MFMA plans
//      of the conv core (plan_mtcnn.cpp build_rnet / build_onet) over the dense batch of all frames' candidates
//   K7 stage3_post_kernel    landmarks, bbreg, "Min" NMS, area-descending order
//
// The host layer (handle, create, the cascade's control, the C ABI) is mtcnn_host.cpp; it reaches these kernels through the
// launchers at the end of this file, declared in mtcnn.h with the types both sides share.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "area_sum.h"
#include "conv_device.h"
#include "mtcnn.h"
#include "nms_device.h"
#include "split_f16.h"

namespace vnf {

typedef float float2_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ int find_level(const LevelTable& t, int idx, int which) {
  int l = 0;
#pragma unroll 1
  for (int i = 1; i < t.n; ++i) {
    const int off = which == 0 ? t.l[i].off_px : which == 1 ? t.l[i].off_p1 : which == 2 ? t.l[i].off_c2 : t.l[i].off_out;
    if (idx >= off) l = i;
  }
  return l;
}

// --------------------------------------------------------------------------------------------- K1
// detect_face.py:71-72: imresample(imgs, (int(h*s+1), int(w*s+1))) then (x-127.5)*0.0078125: the bins, sums and finish
// of area_sum.h.  This form gathers every output pixel's bin byte by byte: the only one for frames whose rows or base
// address are not 16-byte aligned, or whose rows exceed 64 KiB of LDS as fp32.
__global__ void pyramid_kernel(const uint8_t* __restrict__ frames, int H, int W, LevelTable t, float* __restrict__ lvl) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= t.tot_px) return;
  const int img = blockIdx.y;
  const int li = find_level(t, idx, 0);
  const LevelDesc L = t.l[li];
  const int p = idx - L.off_px, y = p / L.Ws, x = p - y * L.Ws;
  const AreaBin bh = area_bin(y, H, L.Hs), bw = area_bin(x, W, L.Ws);
  unsigned s[3];
  area_gather(frames + (size_t)img * H * W * 3, (size_t)W * 3, bh.lo, bh.hi, bw.lo, bw.hi, s);
  float* o = lvl + ((size_t)img * 3) * t.tot_px + L.off_px + p;
#pragma unroll
  for (int c = 0; c < 3; ++c) o[c * (size_t)t.tot_px] = area_norm(s[c], bh.hi - bh.lo, bw.hi - bw.lo);
}

// The row form of K1 for rows that are a whole number of 16-byte chunks (W*3 % 16 == 0: 1920, 1280, 640 ...).
// One workgroup per (output row of any level, frame): every lane streams 16-byte chunks of the input
// rows of that bin row (fully coalesced; each level re-reads the u8 frame once, from L2 / Infinity
// Cache after the first), keeps per-byte column sums in registers, parks them in LDS, and the
// output pixels then add their horizontal spans.
__global__ void __launch_bounds__(256) pyramid_rows_kernel(const uint8_t* __restrict__ frames, int H, int W,
                                                            LevelTable t, float* __restrict__ lvl, const int* __restrict__ row_order) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned* colsum = reinterpret_cast<unsigned*>(smem);  // W*3 entries
  // XCD-aware dispatch: blockIdx.x is the FRAME (workgroups go to the 8 XCDs round-robin in linear order, so with a
  // multiple of 8 frames every frame stays on one XCD and its private L2), blockIdx.y walks the output rows of ALL levels
  // in the order of the frame rows they read (row_order: sorted by the bin's first input row, tall bins first on ties):
  // the nine levels' readers of a band of the frame run together and the band is fetched from beyond L2 once, not 9x
  const int packed = row_order[blockIdx.y];
  const int li = packed >> 16, r = packed & 0xFFFF;
  const LevelDesc L = t.l[li];
  const int img = blockIdx.x, i = r;
  const AreaBin bh = area_bin(i, H, L.Hs);
  const int h0 = bh.lo, h1 = bh.hi;
  const int rowb = W * 3, nchunk = rowb >> 4;
  const uint8_t* base = frames + (size_t)img * H * rowb;
  for (int c0 = 0; c0 < nchunk; c0 += 512) {   // 2 chunks per thread per sweep
    unsigned acc[2][16];
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int j = 0; j < 16; ++j) acc[q][j] = 0u;
    const int ca = c0 + threadIdx.x, cb = ca + 256;
    const int cac = min(ca, nchunk - 1), cbc = min(cb, nchunk - 1);   // clamped: unconditional loads, results dropped below
    // the packed sums of area_colsum16, on this kernel's own load schedule; 256 rows of 255 fit in 16 bits, then the
    // packed sums are flushed into the 32-bit ones
    for (int y0 = h0; y0 < h1; y0 += 256) {
      const int y1 = min(h1, y0 + 256);
      unsigned pe[2][4], po[2][4];
#pragma unroll
      for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int d = 0; d < 4; ++d) { pe[q][d] = 0u; po[q][d] = 0u; }
      // two rows per round, four 16-byte loads in flight; the second row is clamped and masked at an odd tail
      // (slower: four rows per round -- the bins of the first level are only 4-5 rows tall; six-row rounds for the
      // tall bins of the small levels, 0.154 ms -- more requests in flight only crowd the memory system)
      for (int yy = y0; yy < y1; yy += 2) {
        const int yb = min(yy + 1, y1 - 1);
        const unsigned mb = (yy + 1 < y1) ? 0x00FF00FFu : 0u;
        const uint4* r0 = reinterpret_cast<const uint4*>(base + (size_t)yy * rowb);
        const uint4* r1 = reinterpret_cast<const uint4*>(base + (size_t)yb * rowb);
        const uint4 v00 = r0[cac], v01 = r0[cbc], v10 = r1[cac], v11 = r1[cbc];
        const unsigned w0[2][4] = {{v00.x, v00.y, v00.z, v00.w}, {v01.x, v01.y, v01.z, v01.w}};
        const unsigned w1[2][4] = {{v10.x, v10.y, v10.z, v10.w}, {v11.x, v11.y, v11.z, v11.w}};
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
          for (int d = 0; d < 4; ++d) {
            pe[q][d] += (w0[q][d] & 0x00FF00FFu) + (w1[q][d] & mb);
            po[q][d] += ((w0[q][d] >> 8) & 0x00FF00FFu) + ((w1[q][d] >> 8) & mb);
          }
      }
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        unsigned u[16];
        area_unpack(pe[q], po[q], u);
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[q][j] += u[j];
      }
    }
    if (ca < nchunk) {
#pragma unroll
      for (int j = 0; j < 16; ++j) colsum[ca * 16 + j] = acc[0][j];
    }
    if (cb < nchunk) {
#pragma unroll
      for (int j = 0; j < 16; ++j) colsum[cb * 16 + j] = acc[1][j];
    }
  }
  __syncthreads();
  for (int x = threadIdx.x; x < L.Ws; x += blockDim.x) {
    const AreaBin bw = area_bin(x, W, L.Ws);
    unsigned s[3] = {0u, 0u, 0u};
    area_span(colsum + 3 * bw.lo, bw.hi - bw.lo, s);
    float* o = lvl + ((size_t)img * 3) * t.tot_px + L.off_px + i * L.Ws + x;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c * (size_t)t.tot_px] = area_norm(s[c], h1 - h0, bw.hi - bw.lo);
  }
}

// --------------------------------------------------------------------------------------------- K2
// mtcnn.py:39-41: conv1 3->10 (3x3) + PReLU, then MaxPool2d(2,2,ceil_mode=True), on the matrix pipe: the 270 weights
// are an MFMA operand (9 VGPRs per lane, loaded once), not wave-uniform scalars (those do not fit the SGPR file, and a
// per-pixel VALU kernel waits on fetching them again and again).  One workgroup per (pooled row of any level, frame); a
// wave takes tiles of 2 conv rows x 8 conv columns = 16 pixels, one v_mfma_f32_16x16x4_f32 per tap (A = weights [16 ch
// pad][4 ch pad], B = pixels, accumulator preset with the bias), PReLU, the 2x2 max over the lane quartet {l, l^1, l^8,
// l^9} by DPP.  Every lane fetches its nine B values straight from the level (the 9-fold reuse between taps and the
// 2-column overlap of neighbouring tiles are L1 hits), two tiles in flight per wave so the two accumulator chains
// interleave, the next pair's loads issued before the current pair's MFMAs.  No barrier at all.
typedef float f32x4p_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float dpp_xor1(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));   // quad_perm [1,0,3,2]
}
__device__ __forceinline__ float dpp_xor8(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x128, 0xF, 0xF, true));  // row_ror:8
}
__global__ void __launch_bounds__(256) pnet_conv1_pool_direct_kernel(const float* __restrict__ lvl, LevelTable t, PNetW w,
                                                                      float* __restrict__ p1) {
  int li = 0, py = blockIdx.y;   // frame on x: one XCD (and its L2) per frame, see pyramid_rows_kernel
  while (li + 1 < t.n && py >= t.l[li].Hp) { py -= t.l[li].Hp; ++li; }
  const LevelDesc L = t.l[li];
  const int img = blockIdx.x, tid = threadIdx.x;
  const int Hc = L.Hs - 2, Wc = L.Ws - 2;
  const int wave = tid >> 6, lane = tid & 63, lg = lane >> 4, lm = lane & 15, dy = lm >> 3, dx = lm & 7;
  float wa[9];
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) wa[tap] = (lm < 10 && lg < 3) ? w.w1[(lg * 9 + tap) * 10 + lm] : 0.f;
  float bias[4], slope[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int ch = lg * 4 + e;
    bias[e] = ch < 10 ? w.b1[ch] : 0.f;
    slope[e] = ch < 10 ? w.a1[ch] : 0.f;
  }
  const float* g0 = lvl + ((size_t)img * 3 + min(lg, 2)) * t.tot_px + L.off_px;
  const float* rowp[3];
#pragma unroll
  for (int kh = 0; kh < 3; ++kh) rowp[kh] = g0 + (size_t)min(2 * py + dy + kh, L.Hs - 1) * L.Ws;
  const bool row_ok = 2 * py + dy < Hc;
  const int ntile = (L.Wp + 3) >> 2;
  float* o = p1 + ((size_t)img * 10) * t.tot_p1 + L.off_p1 + (size_t)py * L.Wp;
  auto fetch = [&](int tx, float (&xb)[9]) {
    const int x0 = min(8 * tx + dx, L.Ws - 3);
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) xb[kh * 3 + kw] = rowp[kh][x0 + kw];
  };
  auto finish = [&](int tx, f32x4p_t acc) {
    const bool ok = row_ok && 8 * tx + dx < Wc;
    const int pxx = 4 * tx + (dx >> 1);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float v = acc[e] > 0.f ? acc[e] : acc[e] * slope[e];
      v = ok ? v : -INFINITY;
      v = fmaxf(v, dpp_xor1(v));
      v = fmaxf(v, dpp_xor8(v));
      if ((lm & 9) == 0 && pxx < L.Wp && lg * 4 + e < 10) o[(size_t)(lg * 4 + e) * t.tot_p1 + pxx] = v;
    }
  };
  // tiles wave, wave+4 form the first pair, then +8 ...; a tile index beyond ntile is clamped for the loads and skipped
  // (one pooled row per WAVE instead of per workgroup was slower: the long rows of the first level then set the time)
  float xa[9], xb[9];
  int tx = wave;
  if (tx >= ntile) return;
  fetch(tx, xa);
  fetch(min(tx + 4, ntile - 1), xb);
  for (; tx < ntile; tx += 8) {
    float na[9], nb[9];
    const int nx = tx + 8;
    if (nx < ntile) { fetch(nx, na); fetch(min(nx + 4, ntile - 1), nb); }
    f32x4p_t a0 = {bias[0], bias[1], bias[2], bias[3]}, a1 = a0;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[tap], xa[tap], a0, 0, 0, 0);
      a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[tap], xb[tap], a1, 0, 0, 0);
    }
    finish(tx, a0);
    if (tx + 4 < ntile) finish(tx + 4, a1);
    if (nx < ntile) {
#pragma unroll
      for (int i = 0; i < 9; ++i) { xa[i] = na[i]; xb[i] = nb[i]; }
    }
  }
}

// mtcnn.py:42-43: conv2 10->16 (3x3) + PReLU
__global__ void pnet_conv2_kernel(const float* __restrict__ p1, LevelTable t, PNetW w, float* __restrict__ c2) {
  const int idx = blockIdx.y * blockDim.x + threadIdx.x;
  if (idx >= t.tot_c2) return;
  const int img = blockIdx.x;
  const int li = find_level(t, idx, 2);
  const LevelDesc L = t.l[li];
  const int p = idx - L.off_c2, y = p / L.W2, x = p - y * L.W2;
  const float* src = p1 + ((size_t)img * 10) * t.tot_p1 + L.off_p1;
  float2_t acc2[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc2[j] = float2_t{w.b2[2 * j], w.b2[2 * j + 1]};
#pragma unroll 1
  for (int c = 0; c < 10; ++c) {
    const float* sc = src + (size_t)c * t.tot_p1 + y * L.Wp + x;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const float v = sc[kh * L.Wp + kw];
        const float2_t v2 = {v, v};
        const float* ww = w.w2 + ((c * 3 + kh) * 3 + kw) * 16;
#pragma unroll
        for (int j = 0; j < 8; ++j) acc2[j] = __builtin_elementwise_fma(v2, float2_t{ww[2 * j], ww[2 * j + 1]}, acc2[j]);
      }
  }
  float* o = c2 + ((size_t)img * 16) * t.tot_c2 + L.off_c2 + p;
#pragma unroll
  for (int co = 0; co < 16; ++co) {
    const float a = acc2[co >> 1][co & 1];
    o[(size_t)co * t.tot_c2] = a > 0.f ? a : a * w.a2[co];
  }
}

// mtcnn.py:44-49: conv3 16->32 + PReLU, conv4_1 (1x1 ->2) + softmax, conv4_2 (1x1 -> 4);
// detect_face.py:209: mask = prob[:,1] >= thr, fused: survivors are appended to the
// (level, frame) candidate list.  prob_dbg / reg_dbg (optional) receive the dense maps.
__global__ void pnet_conv3_heads_kernel(const float* __restrict__ c2, LevelTable t, PNetW w, float thr, int B, int cap_out,
                                        Cand* __restrict__ cand, int* __restrict__ cells, int* __restrict__ cand_cnt,
                                        float* __restrict__ prob_dbg, float* __restrict__ reg_dbg) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= t.tot_out) return;
  const int img = blockIdx.y;
  const int li = find_level(t, idx, 3);
  const LevelDesc L = t.l[li];
  const int p = idx - L.off_out, y = p / L.ow, x = p - y * L.ow;
  const float* src = c2 + ((size_t)img * 16) * t.tot_c2 + L.off_c2;
  // two output channels per v_pk_fma_f32: the same IEEE fma per channel in the same (c,kh,kw) order, at twice
  // the scalar-FMA rate (this kernel is FMA-bound: 4608 FMAs per output cell)
  float2_t acc2[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) acc2[j] = float2_t{w.b3[2 * j], w.b3[2 * j + 1]};
#pragma unroll 1
  for (int c = 0; c < 16; ++c) {
    const float* sc = src + (size_t)c * t.tot_c2 + y * L.W2 + x;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const float v = sc[kh * L.W2 + kw];
        const float2_t v2 = {v, v};
        const float* ww = w.w3 + ((c * 3 + kh) * 3 + kw) * 32;
#pragma unroll
        for (int j = 0; j < 16; ++j) acc2[j] = __builtin_elementwise_fma(v2, float2_t{ww[2 * j], ww[2 * j + 1]}, acc2[j]);
      }
  }
  float acc[32];
#pragma unroll
  for (int j = 0; j < 16; ++j) { acc[2 * j] = acc2[j][0]; acc[2 * j + 1] = acc2[j][1]; }
  float a0 = w.b41[0], a1 = w.b41[1], r0 = w.b42[0], r1 = w.b42[1], r2 = w.b42[2], r3 = w.b42[3];
#pragma unroll
  for (int c = 0; c < 32; ++c) {
    const float v = acc[c] > 0.f ? acc[c] : acc[c] * w.a3[c];
    a0 = fmaf(v, w.w41[c * 2 + 0], a0);
    a1 = fmaf(v, w.w41[c * 2 + 1], a1);
    r0 = fmaf(v, w.w42[c * 4 + 0], r0);
    r1 = fmaf(v, w.w42[c * 4 + 1], r1);
    r2 = fmaf(v, w.w42[c * 4 + 2], r2);
    r3 = fmaf(v, w.w42[c * 4 + 3], r3);
  }
  const float m = fmaxf(a0, a1);
  const float e0 = expf(a0 - m), e1 = expf(a1 - m);
  const float prob = e1 / (e0 + e1);
  if (prob_dbg) {
    prob_dbg[(size_t)img * t.tot_out + idx] = prob;
    float* rd = reg_dbg + ((size_t)img * 4) * t.tot_out + idx;
    rd[0] = r0; rd[(size_t)t.tot_out] = r1; rd[2 * (size_t)t.tot_out] = r2; rd[3 * (size_t)t.tot_out] = r3;
  }
  if (prob >= thr) {
    // the record goes to its cell's slot of a dense per-frame table, the cell index to the level's compact list (one
    // entry per cell at most: the list cannot overflow)
    const int slot = atomicAdd(&cand_cnt[li * B + img], 1);
    Cand c;
    c.score = prob; c.r0 = r0; c.r1 = r1; c.r2 = r2; c.r3 = r3; c.cell = p;
    cand[(size_t)img * cap_out + idx] = c;
    cells[(size_t)img * cap_out + L.off_out + slot] = p;
  }
}

__device__ __forceinline__ float4 cell_box(int cell, int ow, float scale) {
  // detect_face.py:214-216: stride 2, cellsize 12; fp32 division by the fp32-rounded scale
  const int y = cell / ow, x = cell - y * ow;
  const float fx = (float)x, fy = (float)y;
  return float4{floorf((2.f * fx + 1.f) / scale), floorf((2.f * fy + 1.f) / scale),
                floorf((2.f * fx + 12.f) / scale), floorf((2.f * fy + 12.f) / scale)};
}

// --------------------------------------------------------------------------------------------- K4a
// detect_face.py:79: batched_nms(..., 0.5) within each (scale, image).  Visiting order = stable
// score-descending over nonzero() order (y, x): key = (inverted score | cell | slot).

template <bool KEYS_G, bool KEPT_G>
__device__ __forceinline__ void nms_scale_body(const Cand* __restrict__ cd, const int* __restrict__ cl, int n, int ow, float scale,
                                               float thr, unsigned long long* keys, float4* kbox, int* keepl, float4* s_cbox,
                                               int* s_alive, int* __restrict__ out_cells, int* __restrict__ out_cnt, int* status) {
  const int npad = next_pow2(n);
  // visiting order = stable score-descending over nonzero() order (y, x): key = (inverted score | cell); cells are unique
  for (int i = threadIdx.x; i < npad; i += blockDim.x)
    keys[i] = i < n ? ((unsigned long long)inv_score_bits(cd[cl[i]].score) << 32) | (unsigned)cl[i] : ~0ull;
  __syncthreads();
  block_sort(keys, n, npad);
  auto getbox = [&](int r) { return cell_box((int)(keys[r] & 0xFFFFFFFFu), ow, scale); };
  const int nk = block_greedy_nms<NMS_TV>(n, thr, getbox, keepl, kbox, n, s_cbox, s_alive, status);
  for (int k = threadIdx.x; k < nk; k += blockDim.x) out_cells[k] = (int)(keys[keepl[k]] & 0xFFFFFFFFu);
  if (threadIdx.x == 0) *out_cnt = nk;
}

__global__ void __launch_bounds__(256) nms_scale_kernel(const Cand* __restrict__ cand, const int* __restrict__ cells,
                                                         const int* __restrict__ cand_cnt, LevelTable t, int B, int cap_out, float thr,
                                                         int* __restrict__ keep1c, int* __restrict__ keep_cnt, int* __restrict__ status,
                                                         NmsScratch g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(smem);              // CAP_LDS_KEYS * 8
  float4* s_kbox = reinterpret_cast<float4*>(smem + CAP_LDS_KEYS * 8);                  // KEEP * 16
  int* s_keep = reinterpret_cast<int*>(smem + CAP_LDS_KEYS * 8 + KEEP * 16);            // KEEP * 4
  float4* s_cbox = reinterpret_cast<float4*>(smem + CAP_LDS_KEYS * 8 + KEEP * 20);      // 256 * 16
  int* s_alive = reinterpret_cast<int*>(smem + CAP_LDS_KEYS * 8 + KEEP * 20 + 256 * 16);
  const int li = blockIdx.x, img = blockIdx.y, seg = li * B + img;
  const int n = cand_cnt[seg];
  if (n == 0) {
    if (threadIdx.x == 0) keep_cnt[seg] = 0;
    return;
  }
  const LevelDesc& L = t.l[li];
  const size_t base = (size_t)img * cap_out + L.off_out;
  const Cand* cd = cand + base;
  const int* cl = cells + base;
  int* oc = keep1c + base;
  const size_t gb = (size_t)img * g.stride + L.off_out;
  // LDS while the list fits; a level with more candidates than the LDS tables hold takes global-memory scratch
  if (n <= KEEP) nms_scale_body<false, false>(cd, cl, n, L.ow, L.scale, thr, keys, s_kbox, s_keep, s_cbox, s_alive, oc, keep_cnt + seg, status);
  else if (n <= CAP_LDS_KEYS) nms_scale_body<false, true>(cd, cl, n, L.ow, L.scale, thr, keys, g.kbox + gb, g.keep + gb, s_cbox, s_alive, oc, keep_cnt + seg, status);
  else nms_scale_body<true, true>(cd, cl, n, L.ow, L.scale, thr, g.keys + gb, g.kbox + gb, g.keep + gb, s_cbox, s_alive, oc, keep_cnt + seg, status);
}

// --------------------------------------------------------------------------------------------- K4b
// detect_face.py:83-104: concatenate the per-scale survivors, batched_nms(..., 0.7) per image,
// regress with (w,h) WITHOUT +1, rerec (square), pad (trunc + clamp).  Table order = visiting
// order (score descending; ties: scale order, then within-scale order).
__device__ __forceinline__ void rerec_pad(float& x1, float& y1, float& x2, float& y2, int W, int H, Row& r) {
  const float h = y2 - y1, w = x2 - x1;
  const float l = fmaxf(w, h);
  x1 = x1 + w * 0.5f - l * 0.5f;
  y1 = y1 + h * 0.5f - l * 0.5f;
  x2 = x1 + l;
  y2 = y1 + l;
  int ix = (int)truncf(x1), iy = (int)truncf(y1), iex = (int)truncf(x2), iey = (int)truncf(y2);
  if (ix < 1) ix = 1;
  if (iy < 1) iy = 1;
  if (iex > W) iex = W;
  if (iey > H) iey = H;
  r.x1 = x1; r.y1 = y1; r.x2 = x2; r.y2 = y2;
  r.x = ix; r.y = iy; r.ex = iex; r.ey = iey;
}

template <bool KEYS_G, bool KEPT_G, typename Locate>
__device__ __forceinline__ void nms_image_body(Locate locate, const LevelTable& t, int n, float thr, int W, int H, int KR,
                                               unsigned long long* keys, float4* kbox, int* keepl, float4* s_cbox, int* s_alive,
                                               Row* __restrict__ rows_img, int* __restrict__ row_cnt_img, int* status) {
  const int npad = next_pow2(n);
  for (int i = threadIdx.x; i < npad; i += blockDim.x) {
    if (i < n) {
      int l;
      const Cand* c = locate(i, l);
      keys[i] = ((unsigned long long)inv_score_bits(c->score) << 32) | (unsigned)i;
    } else {
      keys[i] = ~0ull;
    }
  }
  __syncthreads();
  block_sort(keys, n, npad);
  auto getbox = [&](int r) {
    int l;
    const Cand* c = locate((int)(keys[r] & 0xFFFFFFFFu), l);
    return cell_box(c->cell, t.l[l].ow, t.l[l].scale);
  };
  int nk = block_greedy_nms<NMS_TV>(n, thr, getbox, keepl, kbox, n, s_cbox, s_alive, status);
  if (nk > KR) {     // more survivors than the stage-2 table has rows: the call fails (the host layer grows the table)
    if (threadIdx.x == 0) atomicOr(status, ST_OVER_KEEP);
    nk = KR;
  }
  for (int k = threadIdx.x; k < nk; k += blockDim.x) {
    int l;
    const Cand* c = locate((int)(keys[keepl[k]] & 0xFFFFFFFFu), l);
    const float4 b = kbox[k];
    const float regw = b.z - b.x, regh = b.w - b.y;
    float x1 = b.x + c->r0 * regw, y1 = b.y + c->r1 * regh, x2 = b.z + c->r2 * regw, y2 = b.w + c->r3 * regh;
    Row r;
    rerec_pad(x1, y1, x2, y2, W, H, r);
    r.score = c->score;
    rows_img[k] = r;
  }
  if (threadIdx.x == 0) *row_cnt_img = nk;
}

__global__ void __launch_bounds__(256) nms_image_kernel(const Cand* __restrict__ cand, const int* __restrict__ keep1c,
                                                         const int* __restrict__ keep1_cnt, LevelTable t, int B, int cap_out,
                                                         float thr, int W, int H, int KR, Row* __restrict__ rows,
                                                         int* __restrict__ row_cnt, int* __restrict__ status, NmsScratch g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(smem);           // CAP_LDS_KEYS * 8
  float4* s_kbox = reinterpret_cast<float4*>(smem + CAP_LDS_KEYS * 8);
  int* s_keep = reinterpret_cast<int*>(smem + CAP_LDS_KEYS * 8 + KEEP * 16);
  float4* s_cbox = reinterpret_cast<float4*>(smem + CAP_LDS_KEYS * 8 + KEEP * 20);
  int* s_alive = reinterpret_cast<int*>(smem + CAP_LDS_KEYS * 8 + KEEP * 20 + 256 * 16);
  __shared__ int s_off[MAX_LEVELS + 1];
  const int img = blockIdx.x;
  if (threadIdx.x == 0) {
    int acc = 0;
    for (int l = 0; l < t.n; ++l) { s_off[l] = acc; acc += keep1_cnt[l * B + img]; }
    s_off[t.n] = acc;
  }
  __syncthreads();
  const int n = s_off[t.n];
  if (n == 0) {
    if (threadIdx.x == 0) row_cnt[img] = 0;
    return;
  }
  const size_t base = (size_t)img * cap_out;
  auto locate = [&](int gi, int& l) -> const Cand* {  // gathered index -> record (per-scale survivors are lists of cells)
    l = 0;
    for (int i = 1; i < t.n; ++i)
      if (gi >= s_off[i]) l = i;
    return cand + base + t.l[l].off_out + keep1c[base + t.l[l].off_out + (gi - s_off[l])];
  };
  Row* ro = rows + (size_t)img * KR;
  const size_t gb = (size_t)img * g.stride;
  if (n <= KEEP) nms_image_body<false, false>(locate, t, n, thr, W, H, KR, keys, s_kbox, s_keep, s_cbox, s_alive, ro, row_cnt + img, status);
  else if (n <= CAP_LDS_KEYS) nms_image_body<false, true>(locate, t, n, thr, W, H, KR, keys, g.kbox + gb, g.keep + gb, s_cbox, s_alive, ro, row_cnt + img, status);
  else nms_image_body<true, true>(locate, t, n, thr, W, H, KR, g.keys + gb, g.kbox + gb, g.keep + gb, s_cbox, s_alive, ro, row_cnt + img, status);
}

// --------------------------------------------------------------------------------------------- K5
// detect_face.py:109-114 / 138-143: imgs[i, :, y-1:ey, x-1:ex] -> imresample(S,S) -> normalise (area_sum.h).
// Degenerate rectangles (the reference silently drops them from im_data, which would desynchronise its tables) are
// flagged and zeroed.
// Where candidate k of frame img goes: slot offs[img] + k - c0 of the dense batch, compact NHWC4 (RGB + 0, the input
// layout of the MFMA R/O-Net plans); nullptr for a candidate outside this chunk [c0, c0 + cap).
__device__ __forceinline__ float* crop_dst(float* out, const int* offs, int c0, int cap, int img, int k, int S) {
  const int ci = offs[img] + k - c0;
  return ci < 0 || ci >= cap ? nullptr : out + (size_t)ci * S * S * 4;
}

constexpr int CROP_MAXB = 4096;  // bytes of crop row per strip (1365 px)

// grid (candidate, frame, row group).  Each wave owns output rows wave, wave+4, ... of its group; its lanes stream the
// 16-byte chunks that cover the crop's byte span of every input row of the bin row (coalesced dwordx4 loads instead of
// per-pixel byte loads), keep per-byte column sums in registers, park them in a wave-private LDS strip, and then add the
// horizontal bin spans.  A candidate the strips cannot serve is gathered pixel by pixel by its first row group.
__global__ void __launch_bounds__(256) crop_resize_rows_kernel(const uint8_t* __restrict__ frames, int H, int W,
                                                                const Row* __restrict__ rows, const int* __restrict__ row_cnt,
                                                                int S, float* __restrict__ out, int* __restrict__ status,
                                                                const int* __restrict__ offs, int c0, int cap, int KR) {
  // per-byte column sums of one bin row are at most (rows of a bin) x 255: 16 bits hold 257 rows.  Half the LDS of
  // 32-bit sums -> twice the resident waves.
  __shared__ __attribute__((aligned(16))) unsigned short strips[4][CROP_MAXB + 32];
  const int k = blockIdx.x, img = blockIdx.y;
  if (k >= row_cnt[img]) return;
  float* o = crop_dst(out, offs, c0, cap, img, k, S);
  if (!o) return;
  const Row r = rows[(size_t)img * KR + k];
  const int y0 = r.y - 1, x0 = r.x - 1, ch = r.ey - y0, cw = r.ex - x0;
  if (blockIdx.z == 0)
    for (int i = threadIdx.x; i < S * S; i += blockDim.x) o[i * 4 + 3] = 0.f;
  if ((ch <= 0 || cw <= 0) && blockIdx.z != 0) return;
  if (ch <= 0 || cw <= 0) {
    for (int i = threadIdx.x; i < S * S; i += blockDim.x) { o[i * 4] = 0.f; o[i * 4 + 1] = 0.f; o[i * 4 + 2] = 0.f; }
    if (threadIdx.x == 0) atomicOr(status, ST_DEGENERATE);
    return;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rowb = W * 3, bs = x0 * 3, be = (x0 + cw) * 3;
  const int c_lo = bs >> 4, nch = ((be + 15) >> 4) - c_lo, off = bs - (c_lo << 4);
  const uint8_t* fbase = frames + (size_t)img * H * rowb;
  // the strips need 16-byte chunks of the frame (rows and base address aligned: the launcher then sends one row group
  // only), a crop no wider than a strip and bins of at most 257 rows (frames taller than ~6000 px at S = 24)
  const bool gather = (rowb & 15) != 0 || (reinterpret_cast<uintptr_t>(frames) & 15) != 0 || nch * 16 > CROP_MAXB + 32 ||
                      (ch + S - 1) / S + 1 > 257;
  if (gather && blockIdx.z != 0) return;
  if (gather) {
    const uint8_t* base = fbase + (size_t)y0 * rowb + (size_t)x0 * 3;
    for (int i = threadIdx.x; i < S * S; i += blockDim.x) {
      const int oy = i / S, ox = i - oy * S;
      const AreaBin bh = area_bin(oy, ch, S), bw = area_bin(ox, cw, S);
      unsigned s[3];
      area_gather(base, (size_t)rowb, bh.lo, bh.hi, bw.lo, bw.hi, s);
#pragma unroll
      for (int c = 0; c < 3; ++c) o[i * 4 + c] = area_norm(s[c], bh.hi - bh.lo, bw.hi - bw.lo);
    }
    return;
  }
  unsigned short* cs = strips[wave];
  // blockIdx.z splits the S output rows into gridDim.z groups, so one large box (its bins are tens of input rows
  // deep) is spread over several workgroups instead of setting the duration of the whole launch
  const int zrows = (S + (int)gridDim.z - 1) / (int)gridDim.z;
  const int oy_lo = (int)blockIdx.z * zrows, oy_hi = min(S, oy_lo + zrows);
  // per-byte column sums of input rows [h0,h1) of chunk column c, as 16-bit pairs into the strip at dst.  Two rounds
  // per trip, eight loads in flight: the kernel waits on L2 latency, not on bandwidth.
  auto colsum = [&](int c, AreaBin bh, unsigned short* dst) {
    unsigned pe[4], po[4], acc[16];
    area_colsum16<true, 2>(fbase + (size_t)y0 * rowb + ((size_t)(c_lo + c) << 4), (size_t)rowb, bh.lo, bh.hi, pe, po);
    area_unpack(pe, po, acc);
#pragma unroll
    for (int j = 0; j < 2; ++j)
      reinterpret_cast<uint4*>(dst)[j] = uint4{acc[8 * j] | (acc[8 * j + 1] << 16), acc[8 * j + 2] | (acc[8 * j + 3] << 16),
                                               acc[8 * j + 4] | (acc[8 * j + 5] << 16), acc[8 * j + 6] | (acc[8 * j + 7] << 16)};
  };
  // channel cch of output (oy, ox) from the strip row `row` (its byte 0 = the crop's first byte)
  auto finish = [&](const unsigned short* row, int oy, int ox, int cch, AreaBin bh) {
    const AreaBin bw = area_bin(ox, cw, S);
    unsigned sum = 0;
    for (int xx = bw.lo; xx < bw.hi; ++xx) sum += row[xx * 3 + cch];
    o[(oy * S + ox) * 4 + cch] = area_norm(sum, bh.hi - bh.lo, bw.hi - bw.lo);
  };
  if (nch <= 32) {
    // narrow crops (the common case: a 100-px box spans ~20 chunks): a wave takes R = 64/nch output rows at
    // once, lane -> (row sub, chunk c), so the loads keep the whole wave busy
    // R rows per wave and pass, but no more than spreads the group's rows over the four waves
    const int R = min(64 / nch, (oy_hi - oy_lo + 3) / 4), sub = lane / nch, c = lane - sub * nch;
    for (int oy0 = oy_lo + wave * R; oy0 < oy_hi; oy0 += 4 * R) {
      const int oy = oy0 + sub;
      if (sub < R && oy < oy_hi) colsum(c, area_bin(oy, ch, S), cs + (sub * nch + c) * 16);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      for (int q = lane; q < R * 3 * S; q += 64) {
        const int s2 = q / (3 * S), q2 = q - s2 * 3 * S;
        const int oy2 = oy0 + s2;
        if (oy2 < oy_hi) {
          const int cch = q2 / S, ox = q2 - cch * S;
          finish(cs + s2 * nch * 16 + off, oy2, ox, cch, area_bin(oy2, ch, S));
        }
      }
      __builtin_amdgcn_wave_barrier();
    }
    return;
  }
  for (int oy = oy_lo + wave; oy < oy_hi; oy += 4) {
    const AreaBin bh = area_bin(oy, ch, S);
    for (int c = lane; c < nch; c += 64) colsum(c, bh, cs + c * 16);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int q = lane; q < 3 * S; q += 64) {
      const int cch = q / S, ox = q - cch * S;
      finish(cs + off, oy, ox, cch, bh);
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// --------------------------------------------------------------------------------------------- K6a
// R-Net / O-Net front: conv1 (3 -> 28 / 32, 3x3) + PReLU + MaxPool(3, 2, ceil_mode) in one kernel (mtcnn.py:84-87 /
// 138-141).  The conv1 map is the largest tensor of the cascade (46x46x32 floats per O-Net candidate, 208 MB for 767
// candidates); here it only ever exists in LDS.  One workgroup per (band of BANDP pooled rows, candidate): the crop
// rows the band needs go to LDS, every wave computes all 32 output channels of 16 conv pixels per round on the MFMA
// (weights stay in registers), the PReLU outputs are parked in LDS as [pixel][32] with the 16-byte chunk index
// XOR-swizzled by the pixel, and the pooled rows are reduced from there and written as whole NHWC rows.
typedef float f32x4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float split_pack(float v) {
  const sf16 h(v);
  return __builtin_bit_cast(float, h);
}
// SPLIT (the split-f16 plans): the pooled map is written as split-f16 (hi, lo) pairs, the storage of the F16X2 plans
// (split_f16.h), and conv1 itself runs on the 16-bit MFMA with split-f16 operands -- the crop pixels are split once when
// they are copied to LDS (a pixel's 3 + 1 channels as four (hi, lo) pairs are the same 16 bytes as its four floats), a
// k block is four taps x four channels, so the 9 taps are three MFMA pairs per 16-channel tile (96 cycles) instead of
// nine f32 MFMAs (288); ~22 significant bits per operand like every later layer of the split plans.  Without SPLIT (the
// exact-f32 plans) conv1 is nine exact-fp32 MFMAs per tile and the pooled map stays fp32.
template <int S, int BANDP, int NT, bool SPLIT>
__global__ void __launch_bounds__(NT) net_front_kernel(const float* __restrict__ crops, FrontW fw, float* __restrict__ p1) {
  constexpr int C = S - 2;                 // conv1 rows / cols
  constexpr int P = (C - 3 + 1) / 2 + 1;   // ceil((C - 3) / 2) + 1
  constexpr int CR = 2 * BANDP + 1;        // conv rows of a band
  constexpr int IR = CR + 2;               // crop rows of a band
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float4* s_in = reinterpret_cast<float4*>(smem);                    // [IR][S] NHWC4
  float4* s_cv = reinterpret_cast<float4*>(smem) + IR * S;           // [CR * C][8 chunks]
  const int band = blockIdx.x, cand = blockIdx.y, t = threadIdx.x;
  const int p0 = band * BANDP, np = min(BANDP, P - p0);
  const int cr0 = 2 * p0, ncr = min(CR, C - cr0), nir = ncr + 2;
  const float4* src = reinterpret_cast<const float4*>(crops) + ((size_t)cand * S + cr0) * S;
  for (int i = t; i < nir * S; i += NT) {
    float4 v = src[i];
    if constexpr (SPLIT) v = float4{split_pack(v.x), split_pack(v.y), split_pack(v.z), split_pack(v.w)};
    s_in[i] = v;
  }
  __syncthreads();
  // conv1 as 16x16x4 fp32 MFMAs, one per (tap, 16-channel tile): A = weights (lane: channel l&15, input channel l>>4),
  // B = crop pixels (lane: pixel l&15, input channel l>>4; channel 3 is the zero pad), D = 4 consecutive output
  // channels of one pixel per lane.  Same k order as the plan's implicit-GEMM conv (tap-major), bias after the sum.
  const int wave = t >> 6, lane = t & 63, lg = lane >> 4, lm = lane & 15;
  float wa[2][SPLIT ? 1 : 9];
  uint4 ws[2][SPLIT ? 3 : 1];   // SPLIT: A fragments, lane (channel lm, group lg) = tap 4 blk + lg, input channels 0..3 as (hi, lo) pairs
  if constexpr (SPLIT) {
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int blk = 0; blk < 3; ++blk) {
        const int tap = 4 * blk + lg;
        float4 w4 = float4{0.f, 0.f, 0.f, 0.f};
        if (tap < 9) w4 = *reinterpret_cast<const float4*>(fw.w + ((ct * 16 + lm) * 9 + tap) * 4);
        const float4 sp = float4{split_pack(w4.x), split_pack(w4.y), split_pack(w4.z), split_pack(w4.w)};
        ws[ct][blk] = __builtin_bit_cast(uint4, sp);
      }
  } else {
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) wa[ct][tap] = fw.w[((ct * 16 + lm) * 9 + tap) * 4 + lg];
  }
  float bias[2][4], slope[2][4];
#pragma unroll
  for (int ct = 0; ct < 2; ++ct)
#pragma unroll
    for (int e = 0; e < 4; ++e) { bias[ct][e] = fw.b[ct * 16 + lg * 4 + e]; slope[ct][e] = fw.a[ct * 16 + lg * 4 + e]; }
  const int npx = ncr * C;
  const float* s_inf = reinterpret_cast<const float*>(s_in);
  for (int tile = wave; tile * 16 < npx; tile += NT / 64) {
    const int px = tile * 16 + lm, pxc = min(px, npx - 1);
    const int r = pxc / C, x = pxc - r * C;
    f32x4_t acc[2] = {f32x4_t{0.f, 0.f, 0.f, 0.f}, f32x4_t{0.f, 0.f, 0.f, 0.f}};
    if constexpr (SPLIT) {
      typedef _Float16 f16x8f_t __attribute__((ext_vector_type(8)));
      const uint4* s_inu = reinterpret_cast<const uint4*>(s_in);
#pragma unroll
      for (int blk = 0; blk < 3; ++blk) {
        const int tap = 4 * blk + lg;
        uint4 xf = uint4{0u, 0u, 0u, 0u};
        if (tap < 9) xf = s_inu[(r + tap / 3) * S + x + tap % 3];
        const uint4 xr = {(xf.x >> 16) | (xf.x << 16), (xf.y >> 16) | (xf.y << 16), (xf.z >> 16) | (xf.z << 16),
                          (xf.w >> 16) | (xf.w << 16)};
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
          acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8f_t, ws[ct][blk]), __builtin_bit_cast(f16x8f_t, xf), acc[ct], 0, 0, 0);
          acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8f_t, ws[ct][blk]), __builtin_bit_cast(f16x8f_t, xr), acc[ct], 0, 0, 0);
        }
      }
    } else {
      float xb[9];
#pragma unroll
      for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) xb[kh * 3 + kw] = s_inf[((r + kh) * S + x + kw) * 4 + lg];
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[0][tap], xb[tap], acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[1][tap], xb[tap], acc[1], 0, 0, 0);
      }
    }
    if (px < npx) {
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) {
        float4 o;
        float* op = reinterpret_cast<float*>(&o);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float v = acc[ct][e] + bias[ct][e];
          op[e] = v > 0.f ? v : v * slope[ct][e];
        }
        s_cv[px * 8 + ((ct * 4 + lg) ^ (px & 7))] = o;
      }
    }
  }
  __syncthreads();
  float4* dst = reinterpret_cast<float4*>(p1) + ((size_t)cand * P + p0) * P * 8;
  for (int i = t; i < np * P * 8; i += NT) {
    const int q = i & 7, pp = i >> 3, py = pp / P, pxx = pp - py * P;
    float4 m = float4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        const int rr = 2 * py + dy, xx = 2 * pxx + dx;      // band-local conv row, conv col
        if (rr < ncr && xx < C) {
          const int px = rr * C + xx;
          const float4 v = s_cv[px * 8 + (q ^ (px & 7))];
          m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
        }
      }
    if (SPLIT) m = float4{split_pack(m.x), split_pack(m.y), split_pack(m.z), split_pack(m.w)};
    dst[i] = m;
  }
}

// --------------------------------------------------------------------------------------------- K6b
// R-Net / O-Net conv2 (32 -> 48 / 64, 3x3) + PReLU + MaxPool(3, 2, ceil_mode) in one kernel (mtcnn.py:88-90 / 142-144)
// for the split-f16 plans: one workgroup per candidate, the pooled conv1 map (net_front_kernel's output: [pixel][32
// channels] of (hi, lo) pairs) in LDS, the convolution as 16x16x32 f16 MFMAs on the interleaved split operands -- per
// 16 k values (one tap, 16 channels) the chunk pair and the pair with the activation's halves swapped, exactly
// mma_chunk<sf16>, in the plan's k order (tap-major) with its fp32 sum, bias and PReLU -- weights as 18 A-fragments per
// 16-channel tile in REGISTERS, the conv map ([pixel][channels of the pass] fp32) only ever in LDS, pooled from there
// in fp32 and written as split-f16 NHWC rows for the plan's conv3 (the plan splits the map first and pools the split
// values: the same up to the split format's 2^-22 rounding; detections agree to 1e-3 px / 1e-6, tested).  The unfused plan wrote and re-read that map (O-Net: 99 MB
// per 880 candidates) and paid two launches: 0.089 + 0.029 ms (O-Net), 0.057 + 0.017 ms (R-Net) per 16 frames.
typedef _Float16 f16x8m_t __attribute__((ext_vector_type(8)));

template <int PI, int CO, int NWAVE, int NPASS>
__global__ void __launch_bounds__(NWAVE * 64) net_mid_kernel(const float* __restrict__ p1, MidW mw, float* __restrict__ p2) {
  constexpr int C = PI - 2, NPX = C * C, PO = (C - 3 + 1) / 2 + 1;
  constexpr int NCT = CO / 16, CTP = NCT / NPASS, NMG = NWAVE / CTP, NMT = (NPX + 15) / 16;
  constexpr int CHP = CTP * 4;   // 16-byte fp32 chunks per conv pixel in one pass
  static_assert(NCT % NPASS == 0 && NWAVE % CTP == 0, "channel tiles divide over passes and waves");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint4* s_in = reinterpret_cast<uint4*>(smem);                       // [PI * PI][8 chunks of 4 (hi, lo) channels], chunk ^ (px & 7)
  float4* s_cv = reinterpret_cast<float4*>(smem + PI * PI * 128);    // [NPX][CHP]
  const int cand = blockIdx.x, t = threadIdx.x;
  const int wave = t >> 6, lane = t & 63, frow = lane & 15, g = lane >> 4;
  const int ctl = wave % CTP, mg = wave / CTP;
  // the first pass's weight fragments travel while the input map is copied to LDS; the next pass's while this one pools
  uint4 wf[18];
#pragma unroll
  for (int kb = 0; kb < 18; ++kb) wf[kb] = mw.w[((size_t)ctl * 18 + kb) * 64 + lane];
  {
    const uint4* src = reinterpret_cast<const uint4*>(p1) + (size_t)cand * PI * PI * 8;
    for (int i = t; i < PI * PI * 8; i += NWAVE * 64) {
      const int q = i >> 3, ch = i & 7;
      s_in[q * 8 + (ch ^ (q & 7))] = src[i];
    }
  }
  __syncthreads();
#pragma unroll 1
  for (int pass = 0; pass < NPASS; ++pass) {
    const int ct = pass * CTP + ctl;
    float bias[4], slope[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) { bias[e] = mw.b[ct * 16 + 4 * g + e]; slope[e] = mw.a[ct * 16 + 4 * g + e]; }
    for (int tile = mg; tile < NMT; tile += NMG) {
      const int px = tile * 16 + frow, pxc = min(px, NPX - 1);
      const int oy = pxc / C, ox = pxc - oy * C;
      const int q0 = oy * PI + ox;
      f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const int q = q0 + (tap / 3) * PI + tap % 3;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const uint4 xf = s_in[q * 8 + ((4 * h + g) ^ (q & 7))];
          const uint4 xr = {(xf.x >> 16) | (xf.x << 16), (xf.y >> 16) | (xf.y << 16), (xf.z >> 16) | (xf.z << 16),
                            (xf.w >> 16) | (xf.w << 16)};
          acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8m_t, wf[2 * tap + h]),
                                                       __builtin_bit_cast(f16x8m_t, xf), acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8m_t, wf[2 * tap + h]),
                                                       __builtin_bit_cast(f16x8m_t, xr), acc, 0, 0, 0);
        }
      }
      if (px < NPX) {
        float4 o;
        float* op = reinterpret_cast<float*>(&o);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float v = acc[e] + bias[e];
          op[e] = v > 0.f ? v : v * slope[e];
        }
        s_cv[px * CHP + ctl * 4 + g] = o;
      }
    }
    if (pass + 1 < NPASS) {
#pragma unroll
      for (int kb = 0; kb < 18; ++kb) wf[kb] = mw.w[((size_t)(ct + CTP) * 18 + kb) * 64 + lane];
    }
    __syncthreads();
    float4* dst = reinterpret_cast<float4*>(p2) + (size_t)cand * PO * PO * (CO / 4) + pass * CHP;
    for (int i = t; i < PO * PO * CHP; i += NWAVE * 64) {
      const int chunk = i % CHP, pp = i / CHP, py = pp / PO, pxx = pp - py * PO;
      float4 m = float4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
      for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
          const int rr = 2 * py + dy, xx = 2 * pxx + dx;
          if (rr < C && xx < C) {
            const float4 v = s_cv[(rr * C + xx) * CHP + chunk];
            m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
          }
        }
      dst[(size_t)pp * (CO / 4) + chunk] = float4{split_pack(m.x), split_pack(m.y), split_pack(m.z), split_pack(m.w)};
    }
    if (pass + 1 < NPASS) __syncthreads();
  }
}

// exclusive prefix of the per-frame candidate counts: compact batch index of (img, k) = offs[img] + k
__global__ void prefix_offsets_kernel(const int* __restrict__ cnt, int B, int* __restrict__ offs) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    int acc = 0;
    for (int i = 0; i < B; ++i) { offs[i] = acc; acc += cnt[i]; }
    offs[B] = acc;
  }
}

// head outputs of the MFMA plans (hw floats per candidate: a0, a1, then the regression / landmark
// values) -> the per-frame tables the post kernels read: [softmax prob of class 1, values...]
__global__ void heads_scatter_kernel(const float* __restrict__ heads, int hw, const int* __restrict__ offs,
                                     const int* __restrict__ cnt, int c0, int cap, float* __restrict__ dst, int nf, int split, int KR) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x, img = blockIdx.y;
  if (k >= cnt[img]) return;
  const int ci = offs[img] + k - c0;
  if (ci < 0 || ci >= cap) return;
  const float* hsrc = heads + (size_t)ci * hw;
  auto val = [&](int i) { return split ? (float)__builtin_bit_cast(sf16, hsrc[i]) : hsrc[i]; };
  float* o = dst + ((size_t)img * KR + k) * nf;
  const float a0 = val(0), a1 = val(1);
  const float m = fmaxf(a0, a1);
  const float e0 = expf(a0 - m), e1 = expf(a1 - m);
  o[0] = e1 / (e0 + e1);
  for (int i = 1; i < nf; ++i) o[i] = val(1 + i);
}

// --------------------------------------------------------------------------------------------- stage-2 post
// detect_face.py:119-131: keep score > thr, batched_nms(0.7) per image, bbreg (w,h WITH +1), rerec;
// then pad for stage 3 (136).  Visiting order: score descending, ties by stage-1 table order.
template <bool BIG>
__device__ __forceinline__ void stage2_post_body(const Row* __restrict__ r, const float* __restrict__ ro, int n0, float thr_score,
                                                 float thr_nms, int W, int H, unsigned long long* keys, float4* kbox, int* keepl,
                                                 float4* s_cbox, int* s_alive, Row* __restrict__ out, int* __restrict__ out_cnt,
                                                 int* status) {
  __shared__ int s_n;
  const int npad = next_pow2(max(n0, 1));
  for (int i = threadIdx.x; i < npad; i += blockDim.x)
    keys[i] = (i < n0 && ro[i * 5] > thr_score) ? ((unsigned long long)inv_score_bits(ro[i * 5]) << 32) | (unsigned)i : ~0ull;
  __syncthreads();
  block_sort(keys, n0, npad);
  if (threadIdx.x == 0) {
    int lo = 0, hi = n0;  // first padded key
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (keys[mid] == ~0ull) hi = mid; else lo = mid + 1; }
    s_n = lo;
  }
  __syncthreads();
  const int n = s_n;
  auto getbox = [&](int q) { const Row& b = r[(int)(keys[q] & 0xFFFFFFFFu)]; return float4{b.x1, b.y1, b.x2, b.y2}; };
  const int nk = block_greedy_nms<NMS_TV>(n, thr_nms, getbox, keepl, kbox, max(n, 1), s_cbox, s_alive, status);
  for (int k = threadIdx.x; k < nk; k += blockDim.x) {
    const int src = (int)(keys[keepl[k]] & 0xFFFFFFFFu);
    const float4 b = kbox[k];
    const float* mv = ro + src * 5 + 1;
    const float w = b.z - b.x + 1.f, h = b.w - b.y + 1.f;
    float x1 = b.x + mv[0] * w, y1 = b.y + mv[1] * h, x2 = b.z + mv[2] * w, y2 = b.w + mv[3] * h;
    Row o;
    rerec_pad(x1, y1, x2, y2, W, H, o);
    o.score = ro[src * 5];
    out[k] = o;
  }
  if (threadIdx.x == 0) *out_cnt = nk;
}

__global__ void __launch_bounds__(256) stage2_post_kernel(const Row* __restrict__ rows, const int* __restrict__ row_cnt,
                                                           const float* __restrict__ rout, float thr_score, float thr_nms,
                                                           int W, int H, int KR, Row* __restrict__ rows3, int* __restrict__ row3_cnt,
                                                           int* __restrict__ status, NmsScratch g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(smem);  // KEEP * 8
  float4* s_kbox = reinterpret_cast<float4*>(smem + KEEP * 8);
  int* s_keep = reinterpret_cast<int*>(smem + KEEP * 8 + KEEP * 16);
  float4* s_cbox = reinterpret_cast<float4*>(smem + KEEP * 28);
  int* s_alive = reinterpret_cast<int*>(smem + KEEP * 28 + 256 * 16);
  const int img = blockIdx.x;
  const int n0 = row_cnt[img];
  const Row* r = rows + (size_t)img * KR;
  const float* ro = rout + (size_t)img * KR * 5;
  Row* out = rows3 + (size_t)img * KR;     // survivors are a subset of the n0 <= KR input rows: no overflow
  const size_t gb = (size_t)img * g.stride;
  if (n0 <= KEEP) stage2_post_body<false>(r, ro, n0, thr_score, thr_nms, W, H, keys, s_kbox, s_keep, s_cbox, s_alive, out, row3_cnt + img, status);
  else stage2_post_body<true>(r, ro, n0, thr_score, thr_nms, W, H, g.keys + gb, g.kbox + gb, g.keep + gb, s_cbox, s_alive, out, row3_cnt + img, status);
}

// --------------------------------------------------------------------------------------------- K7
// detect_face.py:148-169: keep score > thr, landmarks, bbreg, nms_numpy(0.7, 'Min') per image
// (visit from the highest score; equal scores -- softmax saturates to exactly 1.0f on clear faces --
// are visited in table order: the reference leaves tie order to np.argsort's unstable default
// sort, which is implementation defined; the oracle pins the same rule), then mtcnn.py:334-340: order by box area
// descending (argsort ascending, reversed).  fin: [x1,y1,x2,y2,score, 10 landmark coords] rows.
template <bool BIG>
__device__ __forceinline__ void stage3_post_body(const Row* __restrict__ r, const float* __restrict__ oo, int n0, float thr_score,
                                                 float thr_nms, int select_largest, unsigned long long* keys, float4* kbox,
                                                 int* keepl, float4* reg, float4* s_cbox, int* s_alive, float* __restrict__ fo,
                                                 int* __restrict__ out_cnt, int* status) {
  __shared__ int s_n;
  for (int i = threadIdx.x; i < n0; i += blockDim.x) {  // bbreg of every row (w,h WITH +1)
    const Row& b = r[i];
    const float* mv = oo + i * 15 + 1;
    const float w = b.x2 - b.x1 + 1.f, h = b.y2 - b.y1 + 1.f;
    reg[i] = float4{b.x1 + mv[0] * w, b.y1 + mv[1] * h, b.x2 + mv[2] * w, b.y2 + mv[3] * h};
  }
  const int npad = next_pow2(max(n0, 1));
  for (int i = threadIdx.x; i < npad; i += blockDim.x)  // ties: earlier row first (see header note on ties)
    keys[i] = (i < n0 && oo[i * 15] > thr_score) ? ((unsigned long long)inv_score_bits(oo[i * 15]) << 32) | (unsigned)i : ~0ull;
  __syncthreads();
  block_sort(keys, n0, npad);
  if (threadIdx.x == 0) {
    int lo = 0, hi = n0;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (keys[mid] == ~0ull) hi = mid; else lo = mid + 1; }
    s_n = lo;
  }
  __syncthreads();
  const int n = s_n;
  auto srcof = [&](int q) { return (int)(keys[q] & 0xFFFFFFFFu); };
  auto getbox = [&](int q) { return reg[srcof(q)]; };
  const int nk = block_greedy_nms<NMS_MIN>(n, thr_nms, getbox, keepl, kbox, max(n, 1), s_cbox, s_alive, status);
  __syncthreads();
  // final order: area descending (argsort ascending reversed: ties -> later pick first)
  // the score-sorted keys are dead after this: resolve kept ranks to source rows, then reuse `keys`
  for (int k = threadIdx.x; k < nk; k += blockDim.x) keepl[k] = srcof(keepl[k]);
  __syncthreads();
  const int kpad = next_pow2(max(nk, 1));
  for (int k = threadIdx.x; k < kpad; k += blockDim.x) {
    if (k < nk) {
      const float4 b = kbox[k];
      const float area = (b.z - b.x) * (b.w - b.y);
      // areas may be negative in degenerate cases: map float to an order-preserving unsigned
      unsigned u = __float_as_uint(area);
      u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
      keys[k] = select_largest ? ((unsigned long long)(0xFFFFFFFFu - u) << 32) | (unsigned)(0x7FFFFFFF - k)
                               : (unsigned long long)k;
    } else {
      keys[k] = ~0ull;
    }
  }
  __syncthreads();
  block_sort(keys, nk, kpad);
  for (int q = threadIdx.x; q < nk; q += blockDim.x) {
    const int k = select_largest ? 0x7FFFFFFF - (int)(keys[q] & 0xFFFFFFFFu) : (int)keys[q];
    const int src = keepl[k];
    const Row& b = r[src];
    const float4 bb = kbox[k];
    float* o = fo + q * 15;
    o[0] = bb.x; o[1] = bb.y; o[2] = bb.z; o[3] = bb.w; o[4] = oo[src * 15];
    // detect_face.py:159-163 (boxes BEFORE bbreg): px = w_i * p + x1 - 1
    const float w_i = b.x2 - b.x1 + 1.f, h_i = b.y2 - b.y1 + 1.f;
    const float* lm = oo + src * 15 + 5;
    for (int j = 0; j < 5; ++j) {
      o[5 + 2 * j] = w_i * lm[j] + b.x1 - 1.f;
      o[6 + 2 * j] = h_i * lm[5 + j] + b.y1 - 1.f;
    }
  }
  if (threadIdx.x == 0) *out_cnt = nk;
}

__global__ void __launch_bounds__(256) stage3_post_kernel(const Row* __restrict__ rows3, const int* __restrict__ row3_cnt,
                                                           const float* __restrict__ oout, float thr_score, float thr_nms,
                                                           int select_largest, int KR, float* __restrict__ fin,
                                                           int* __restrict__ fin_cnt, int* __restrict__ status, NmsScratch g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(smem);
  float4* s_kbox = reinterpret_cast<float4*>(smem + KEEP * 8);
  int* s_keep = reinterpret_cast<int*>(smem + KEEP * 8 + KEEP * 16);
  float4* s_cbox = reinterpret_cast<float4*>(smem + KEEP * 28);
  int* s_alive = reinterpret_cast<int*>(smem + KEEP * 28 + 256 * 16);
  float4* s_reg = reinterpret_cast<float4*>(smem + KEEP * 28 + 256 * 20);  // KEEP * 16: boxes after bbreg
  const int img = blockIdx.x;
  const int n0 = row3_cnt[img];
  const Row* r = rows3 + (size_t)img * KR;
  const float* oo = oout + (size_t)img * KR * 15;
  float* fo = fin + (size_t)img * KR * 15;
  const size_t gb = (size_t)img * g.stride;
  if (n0 <= KEEP) stage3_post_body<false>(r, oo, n0, thr_score, thr_nms, select_largest, keys, s_kbox, s_keep, s_reg, s_cbox, s_alive, fo, fin_cnt + img, status);
  else stage3_post_body<true>(r, oo, n0, thr_score, thr_nms, select_largest, g.keys + gb, g.kbox + gb, g.keep + gb, g.reg + gb, s_cbox, s_alive, fo, fin_cnt + img, status);
}


// counts block (row_cnt .. status) followed by [B][FIN_FAST][15] result rows
__global__ void pack_results_kernel(const int* __restrict__ cnt_block, int ncnt, const float* __restrict__ fin,
                                    const int* __restrict__ fin_cnt, int B, int KR, float* __restrict__ stage) {
  int* so = reinterpret_cast<int*>(stage);
  for (int i = threadIdx.x + blockIdx.x * blockDim.x; i < ncnt; i += gridDim.x * blockDim.x) so[i] = cnt_block[i];
  float* ro = stage + ncnt;
  const int total = B * FIN_FAST * 15;
  for (int i = threadIdx.x + blockIdx.x * blockDim.x; i < total; i += gridDim.x * blockDim.x) {
    const int img = i / (FIN_FAST * 15), r = i - img * FIN_FAST * 15, k = r / 15;
    ro[i] = k < fin_cnt[img] ? fin[(size_t)img * KR * 15 + r] : 0.f;
  }
}

// =============================================================================================
// launchers (mtcnn.h)
hipError_t launch_pyramid(const uint8_t* frames, int B, int H, int W, const LevelTable& t, float* lvl, const int* row_order,
                          hipStream_t s) {
  if (row_order) {
    int rows = 0;
    for (int l = 0; l < t.n; ++l) rows += t.l[l].Hs;
    hipLaunchKernelGGL(pyramid_rows_kernel, dim3(B, rows), dim3(256), (size_t)W * 12, s, frames, H, W, t, lvl, row_order);
  } else {
    hipLaunchKernelGGL(pyramid_kernel, dim3((t.tot_px + 255) / 256, B), dim3(256), 0, s, frames, H, W, t, lvl);
  }
  return hipGetLastError();
}

hipError_t launch_pnet_conv1_pool(const float* lvl, int B, const LevelTable& t, const PNetW& w, float* p1, hipStream_t s) {
  int rows = 0;
  for (int l = 0; l < t.n; ++l) rows += t.l[l].Hp;
  hipLaunchKernelGGL(pnet_conv1_pool_direct_kernel, dim3(B, rows), dim3(256), 0, s, lvl, t, w, p1);
  return hipGetLastError();
}

hipError_t launch_pnet_conv2(const float* p1, int B, const LevelTable& t, const PNetW& w, float* c2, hipStream_t s) {
  hipLaunchKernelGGL(pnet_conv2_kernel, dim3(B, (t.tot_c2 + 255) / 256), dim3(256), 0, s, p1, t, w, c2);
  return hipGetLastError();
}

hipError_t launch_pnet_conv3_heads(const float* c2, int B, const LevelTable& t, const PNetW& w, float thr, int cap_out, Cand* cand,
                                   int* cells, int* cand_cnt, float* prob_dbg, float* reg_dbg, hipStream_t s) {
  hipLaunchKernelGGL(pnet_conv3_heads_kernel, dim3((t.tot_out + 255) / 256, B), dim3(256), 0, s, c2, t, w, thr, B, cap_out, cand,
                     cells, cand_cnt, prob_dbg, reg_dbg);
  return hipGetLastError();
}

hipError_t launch_nms_stage1(const Cand* cand, const int* cells, const int* cand_cnt, const LevelTable& t, int B, int cap_out, int H,
                             int W, int KR, int* keep1c, int* keep1_cnt, Row* rows, int* row_cnt, int* status, const NmsScratch& g,
                             hipStream_t s) {
  allow_dynamic_lds<nms_scale_kernel>(LDS_NMS);
  allow_dynamic_lds<nms_image_kernel>(LDS_NMS);
  hipLaunchKernelGGL(nms_scale_kernel, dim3(t.n, B), dim3(256), LDS_NMS, s, cand, cells, cand_cnt, t, B, cap_out, 0.5f, keep1c,
                     keep1_cnt, status, g);
  hipLaunchKernelGGL(nms_image_kernel, dim3(B), dim3(256), LDS_NMS, s, cand, keep1c, keep1_cnt, t, B, cap_out, 0.7f, W, H, KR, rows,
                     row_cnt, status, g);
  return hipGetLastError();
}

hipError_t launch_crop_resize(const uint8_t* frames, int B, int H, int W, const Row* rows, const int* row_cnt, int maxc, int S,
                              float* out, int* status, const int* offs, int c0, int cap, int KR, hipStream_t s) {
  // S / 8 row groups per candidate: 8 output rows per workgroup = 4 waves x 2 rows (measured best of 2..8 groups); one
  // where the kernel gathers every candidate in its first group
  const int groups = frames_aligned(frames, W) ? S / 8 : 1;
  hipLaunchKernelGGL(crop_resize_rows_kernel, dim3(maxc, B, groups), dim3(256), 0, s, frames, H, W, rows, row_cnt, S, out, status, offs, c0, cap, KR);
  return hipGetLastError();
}

template <int S, int BANDP, bool SPLIT>
static hipError_t launch_front(int bands, int lds, const float* crops, const FrontW& fw, float* p1, int n, hipStream_t s) {
  allow_dynamic_lds<net_front_kernel<S, BANDP, 512, SPLIT>>(lds);
  hipLaunchKernelGGL((net_front_kernel<S, BANDP, 512, SPLIT>), dim3(bands, n), dim3(512), lds, s, crops, fw, p1);
  return hipGetLastError();
}

hipError_t launch_net_front(int S, bool split, const float* crops, const FrontW& fw, float* p1, int n, hipStream_t s) {
  // R-Net: the whole candidate in one workgroup of 8 waves (no band overlap to recompute; measured 0.065 ms against
  // 0.074 for two bands x 4 waves); O-Net: bands of 4 pooled rows x 8 waves (larger bands / 16 waves were slower)
  if (S == 24) return split ? launch_front<24, 11, true>(1, LDS_RFRONT, crops, fw, p1, n, s) : launch_front<24, 11, false>(1, LDS_RFRONT, crops, fw, p1, n, s);
  return split ? launch_front<48, 4, true>(6, LDS_OFRONT, crops, fw, p1, n, s) : launch_front<48, 4, false>(6, LDS_OFRONT, crops, fw, p1, n, s);
}

hipError_t launch_net_mid(int S, const float* p1, const MidW& mw, float* p2, int n, hipStream_t s) {
  if (S == 24) {
    allow_dynamic_lds<net_mid_kernel<11, 48, 6, 1>>(LDS_RMID);
    hipLaunchKernelGGL((net_mid_kernel<11, 48, 6, 1>), dim3(n), dim3(384), LDS_RMID, s, p1, mw, p2);
  } else {
    allow_dynamic_lds<net_mid_kernel<23, 64, 8, 2>>(LDS_OMID);
    hipLaunchKernelGGL((net_mid_kernel<23, 64, 8, 2>), dim3(n), dim3(512), LDS_OMID, s, p1, mw, p2);
  }
  return hipGetLastError();
}

hipError_t launch_prefix_offsets(const int* cnt, int B, int* offs, hipStream_t s) {
  hipLaunchKernelGGL(prefix_offsets_kernel, dim3(1), dim3(64), 0, s, cnt, B, offs);
  return hipGetLastError();
}

hipError_t launch_heads_scatter(const float* heads, int hw, const int* offs, const int* cnt, int maxc, int B, int c0, int cap,
                                float* dst, int nf, bool split, int KR, hipStream_t s) {
  hipLaunchKernelGGL(heads_scatter_kernel, dim3((maxc + 63) / 64, B), dim3(64), 0, s, heads, hw, offs, cnt, c0, cap, dst, nf,
                     split ? 1 : 0, KR);
  return hipGetLastError();
}

hipError_t launch_stage2_post(const Row* rows, const int* row_cnt, const float* rout, float thr_score, int B, int H, int W, int KR,
                              Row* rows3, int* row3_cnt, int* status, const NmsScratch& g, hipStream_t s) {
  allow_dynamic_lds<stage2_post_kernel>(LDS_POST);
  hipLaunchKernelGGL(stage2_post_kernel, dim3(B), dim3(256), LDS_POST, s, rows, row_cnt, rout, thr_score, 0.7f, W, H, KR, rows3,
                     row3_cnt, status, g);
  return hipGetLastError();
}

hipError_t launch_stage3_post(const Row* rows3, const int* row3_cnt, const float* oout, float thr_score, int select_largest, int B,
                              int KR, float* fin, int* fin_cnt, int* status, const NmsScratch& g, hipStream_t s) {
  allow_dynamic_lds<stage3_post_kernel>(LDS_POST);
  hipLaunchKernelGGL(stage3_post_kernel, dim3(B), dim3(256), LDS_POST, s, rows3, row3_cnt, oout, thr_score, 0.7f, select_largest,
                     KR, fin, fin_cnt, status, g);
  return hipGetLastError();
}

hipError_t launch_pack_results(const int* cnt_block, int ncnt, const float* fin, const int* fin_cnt, int B, int KR, float* stage,
                               hipStream_t s) {
  hipLaunchKernelGGL(pack_results_kernel, dim3(B), dim3(256), 0, s, cnt_block, ncnt, fin, fin_cnt, B, KR, stage);
  return hipGetLastError();
}

bool stage_tables_overflowed(int status) { return (status & (ST_OVER_SCALE | ST_OVER_IMG | ST_OVER_KEEP)) != 0; }

}  // namespace vnf
