// Implicit-GEMM convolution for gfx950 (MI355X), NHWC activations, MFMA 16x16 tiles.
//
// GEMM view:  C[m][co] = sum_k A[m][k] * Wt[co][k]
//   m  = output pixel (n, ho, wo)          -> "pixel" axis, BM per workgroup
//   co = output channel                     -> "channel" axis, BN per workgroup
//   k  = (kh, kw, c) flattened, c fastest  -> walked in 128-byte K tiles
// A is never materialised: every 16-byte k-chunk (8 x 16-bit or 4 x f32 channels of one filter tap)
// is gathered straight from the NHWC input (tap and channel of each lane's chunk are tracked
// incrementally; the patch / wave-specialised kernels use the per-chunk offset table ktab);
// padded borders and rows past M read a 16-byte zero page instead.
//
// Main kernel (conv_igemm_dma_kernel): both operands go global -> LDS by LDS-DMA
// (global_load_lds_dwordx4, one 1-KiB piece = 8 rows x 128 B per wave instruction), never through
// VGPRs, into a ring of S stages.  The per-lane SOURCE address carries both the im2col gather and
// the bank swizzle (the LDS image must be lane-linear: physical 16-byte slot p of row r holds
// logical k-chunk p ^ (r & 7)), so the ds_read_b128 fragment reads are conflict-free on CDNA4's
// 64-bank LDS (checked exhaustively).  S-1 tiles are in flight under the MFMAs of the
// current one: counted s_waitcnt vmcnt(N) + one raw s_barrier per K tile, no VGPR staging cost,
// so bytes-in-flight per CU -- what bounds these small-K, small-N problems -- is set by LDS
// capacity (160 KiB) instead of by register pressure.
//
// The K loop itself -- fragment reads, MFMA order, software pipeline -- is conv_k_loop of
// conv_device.h, shared with the patch and wave-specialised kernels: the WEIGHT fragment is the A
// operand and the ACTIVATION fragment the B operand, so an accumulator register quad holds 4
// consecutive output channels of one pixel.  The epilogue (conv_epilogue, same header) stages fp32
// accumulators through LDS and writes whole NHWC rows with 16-byte stores: bias (folded BatchNorm;
// optionally one of 9 border classes), residual add, ReLU / PReLU, conversion, and routing of
// column ranges to different destination tensors (concat-free inception branches) all happen there.
//
// dtype paths: bf16 / f16 -> v_mfma_f32_16x16x32_{bf16,f16}; f32 -> v_mfma_f32_16x16x4_f32
// (exact f32 FMA chain; the <=1e-4 parity path).
#include <mutex>
#include <type_traits>
#include <utility>

#include "block35.h"
#include "conv_device.h"

namespace vnf {

template <typename T, int BM, int BN, int WM, int WN, int S>
__global__ __launch_bounds__(WM* WN * 64) void conv_igemm_dma_kernel(const KArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int ES = (int)sizeof(T);
  constexpr int BKE = 128 / ES;
  constexpr int WTM = BM / WM, WTN = BN / WN, TM = WTM / 16, TN = WTN / 16;
  constexpr int NW = WM * WN, NT = NW * 64, RS = NT / 8;  // waves, threads, tile rows covered per DMA pass
  constexpr int AP = BM / RS, BP = BN / RS, L = AP + BP;  // DMA pieces per wave per K tile
  constexpr int STAGE = (BM + BN) * 128;
  static_assert((NW == 4 || NW == 8) && S >= 3 && BM % RS == 0 && BN % RS == 0, "4 or 8 waves, ring of >= 3 stages");

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const int bid = xcd_remap(blockIdx.x, a.nblk);
  const int tile_m = bid / a.tiles_n, tile_n = bid - tile_m * a.tiles_n;
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const int nkt = a.nkt;

  const int lrow = tid >> 3, lcol = tid & 7;
  const int lchunk = lcol ^ (lrow & 7);  // logical k-chunk this lane fetches (physical slot = lcol)
  int abase[AP], ahi[AP], awi[AP];
  row_setup<AP, RS>(a, m0, lrow, abase, ahi, awi);
  const char* wsrc = a.w + (size_t)(n0 + lrow) * a.wrs + lchunk * 16;
  const unsigned lds0 = (unsigned)reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) char*)smem);  // LDS byte address of the ring

  f32x4_t acc[TM][TN];

  // This lane's k-chunk of the next K tile to issue, as (tap row, tap column, channel): advanced by one K tile per
  // issue() -- issue() is called with consecutive kt -- instead of looked up in the layer's gather table, so the
  // prologue has no table load and no barrier before the first DMA (the table's round trip was ~1.5 k cycles of
  // every workgroup; most launches of the inception blocks only live ~10 k).
  int g_c = chunk_chan<T>(lchunk), g_kh = 0, g_kw = 0;
  const int g_byte = chunk_byte<T>(lchunk);  // planar split-f16: the lo plane sits 16 bytes into its 8-channel unit
  auto g_norm = [&]() {
    while (g_c >= a.Cin) {
      g_c -= a.Cin;
      if (++g_kw == a.KW) { g_kw = 0; ++g_kh; }
    }
  };
  g_norm();
  auto issue = [&](int kt) {
    const unsigned sbase = __builtin_amdgcn_readfirstlane(lds0 + (unsigned)((kt % S) * STAGE) + (unsigned)(wave * 1024));
    const bool kvalid = g_kh < a.KH;  // k < K
    const int ex = (g_kh * a.W + g_kw) * a.ldx + g_c;
#pragma unroll
    for (int p = 0; p < AP; ++p) {
      const int hi = ahi[p] + g_kh, wi = awi[p] + g_kw;
      const bool ok = kvalid && (unsigned)hi < (unsigned)a.H && (unsigned)wi < (unsigned)a.W;
      const char* src = ok ? a.x + (size_t)(abase[p] + ex) * ES + g_byte : a.zero;
      glds16(src, sbase + p * (NW * 1024));
    }
#pragma unroll
    for (int p = 0; p < BP; ++p)
      glds16(wsrc + (size_t)(RS * p) * a.wrs + (size_t)kt * a.wts, sbase + BM * 128 + p * (NW * 1024));
    g_c += BKE;
    g_norm();
  };

#pragma unroll
  for (int t = 0; t < S - 1; ++t)
    if (t < nkt) issue(t);

  const int frow = lane & 15, fgrp = lane >> 4;
  auto sync_tile = [&](int kt) {
    // tile kt has landed once at most the S-2 younger tiles of this wave are still in flight
    if (kt + S - 2 < nkt)
      wait_dma_and_barrier<(S - 2) * L>();
    else
      wait_dma_and_barrier<0>();
    // every wave's pieces of tile kt have landed; stage (kt-1)%S is free for tile kt+S-1
    if (kt + S - 1 < nkt) issue(kt + S - 1);
  };
  conv_k_loop<T, TM, TN, true>(a.K, nkt, acc, sync_tile, [&](int kt, int ks, uint4 (&x)[TM], uint4 (&w)[TN]) {
    const char* sA = smem + (kt % S) * STAGE;
    read_rows(sA, wm * WTM, frow, fgrp, ks, x);
    read_rows(sA + BM * 128, wn * WTN, frow, fgrp, ks, w);
  });
  __syncthreads();
  conv_epilogue<T, BM, BN, WM, WN, S * STAGE>(a, acc, smem, m0, n0);
}

// ===================================================================== host launch
static const char* zero_page() {  // per-device 256 zero bytes for padded / out-of-range gather sources
  static char* z[16] = {nullptr};
  static std::once_flag once[16];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return nullptr;
  std::call_once(once[dev], [dev] {
    char* p = nullptr;
    if (hipMalloc((void**)&p, 256) != hipSuccess) return;
    (void)hipMemset(p, 0, 256);
    (void)hipDeviceSynchronize();  // once per device: the page must be zero before any stream reads it
    z[dev] = p;
  });
  return z[dev];
}

const char* conv_zero_page() { return zero_page(); }

template <typename T, int BM, int BN, int WM, int WN, int S>
static hipError_t launch_dma(const KArgs& k, hipStream_t s) {
  allow_dynamic_lds<conv_igemm_dma_kernel<T, BM, BN, WM, WN, S>>(160 * 1024);
  KArgs kk = k;
  const int lds = S * (BM + BN) * 128;
  const int tiles_m = (k.M + BM - 1) / BM;
  kk.tiles_n = (k.Cout + BN - 1) / BN;
  kk.nblk = tiles_m * kk.tiles_n;
  hipLaunchKernelGGL((conv_igemm_dma_kernel<T, BM, BN, WM, WN, S>), dim3(kk.nblk), dim3(WM * WN * 64), lds, s, kk);
  return hipGetLastError();
}

// Tile configurations of the LDS-DMA kernel: {BM, BN, waves along M, waves along N, ring stages}.
struct TileCfg { int bm, bn, wm, wn, s; };
static constexpr TileCfg kCfgs[] = {
    {128, 128, 2, 2, 3}, {128, 64, 2, 2, 3}, {128, 32, 4, 1, 3}, {64, 64, 2, 2, 4}, {64, 32, 2, 2, 4},
    {256, 32, 4, 1, 3},  {256, 64, 4, 1, 3}, {64, 128, 1, 4, 3}, {32, 64, 2, 2, 4}, {32, 128, 1, 4, 4},
    {128, 64, 2, 2, 4},  {64, 64, 2, 2, 3},  {128, 32, 4, 1, 4},
    // 8-wave workgroups: two waves per SIMD, so one wave's DMA issue / LDS reads hide under the other's MFMAs
    {128, 128, 2, 4, 3}, {256, 128, 4, 2, 3}, {256, 64, 4, 2, 3}, {128, 64, 4, 2, 3}, {128, 256, 2, 4, 3},
    {128, 128, 2, 4, 4},
    // deep rings for problems with about one workgroup per CU: the K loop is a serial chain of
    // L2 / Infinity-Cache round trips, so more tiles in flight shorten it directly
    {128, 64, 4, 2, 6},  {64, 64, 2, 2, 8},   {64, 32, 2, 2, 8},  {32, 64, 2, 2, 8},  {128, 32, 4, 1, 6},
    {64, 128, 2, 4, 5},  {128, 64, 2, 2, 6},
    // whole-N tiles: the activation operand (which comes from beyond L2) is read exactly once
    {64, 256, 1, 8, 3},  {64, 256, 1, 8, 4},  {128, 256, 2, 4, 3},
    // 96- and 192-channel tiles: the inception widths, so one tile spans the whole N and the gathered
    // activation operand crosses the L2 -> LDS path once per tap instead of once per tap and N tile
    {128, 96, 4, 1, 3},  {64, 96, 2, 2, 4},   {128, 192, 2, 4, 3}, {64, 192, 2, 4, 3},  {256, 96, 4, 1, 3},
    {64, 192, 2, 4, 4},
};
constexpr int kNumCfgs = (int)(sizeof(kCfgs) / sizeof(kCfgs[0]));

int conv_num_cfgs() { return kNumCfgs + patch_num_cfgs() + ws_num_cfgs(); }
void conv_family_sizes(int sizes[3]) { sizes[0] = kNumCfgs; sizes[1] = patch_num_cfgs(); sizes[2] = ws_num_cfgs(); }
bool conv_cfg_tile(int cfg, ConvTile& t) {
  if (cfg >= kNumCfgs + patch_num_cfgs()) return ws_cfg_tile(cfg - kNumCfgs - patch_num_cfgs(), t);
  if (cfg >= kNumCfgs) return patch_cfg_tile(cfg - kNumCfgs, t);
  if (cfg < 0) return false;
  t = ConvTile{0, kCfgs[cfg].bm, kCfgs[cfg].bn, kCfgs[cfg].wm, kCfgs[cfg].wn, kCfgs[cfg].s};
  return true;
}

static bool dma_capable(const ConvArgs& a) { return (a.Kpad / (128 / dtype_size(a.dtype))) * 8 * 16 <= 24 * 1024; }

bool conv_cfg_ok(const ConvArgs& a, int cfg) {
  if (cfg >= kNumCfgs + patch_num_cfgs()) return dma_capable(a) && ws_cfg_ok(a, cfg - kNumCfgs - patch_num_cfgs());
  if (cfg >= kNumCfgs) return dma_capable(a) && patch_cfg_ok(a, cfg - kNumCfgs);
  if (cfg < 0) return false;  // the ring kernel needs no table in LDS: any K
  const TileCfg& c = kCfgs[cfg];
  if (c.bn > 32 && a.Cout <= c.bn / 2) return false;  // more than half the tile would be padding
  if (((a.Cout + c.bn - 1) / c.bn) * c.bn > a.cout_pad) return false;  // weight rows n0..n0+BN-1 must exist in the packed buffer
  if ((c.bn % 64) && a.Cout % c.bn) return false;      // 96/192-wide tiles only where they divide N
  const int lds = c.s * (c.bm + c.bn) * 128;  // the ring (and, after the K loop, the epilogue staging)
  return lds <= 160 * 1024;
}

// cfg -> launch_dma<T, kCfgs[cfg]...>: entry I of the table is the template argument list of launcher I
template <typename T, size_t... I>
static hipError_t launch_cfg(int cfg, const KArgs& k, hipStream_t s, std::index_sequence<I...>) {
  static constexpr hipError_t (*kLaunch[])(const KArgs&, hipStream_t) = {
      launch_dma<T, kCfgs[I].bm, kCfgs[I].bn, kCfgs[I].wm, kCfgs[I].wn, kCfgs[I].s>...};
  return (unsigned)cfg < sizeof...(I) ? kLaunch[cfg](k, s) : hipErrorInvalidValue;
}
template <typename T>
static hipError_t launch_cfg(int cfg, const KArgs& k, hipStream_t s) {
  return launch_cfg<T>(cfg, k, s, std::make_index_sequence<kNumCfgs>{});
}

template <typename T>
static hipError_t launch_typed(const ConvArgs& a, const KArgs& k, hipStream_t s) {
  if (!k.zero) return hipErrorOutOfMemory;   // every kernel reads padded / out-of-range sources from the zero page
  if (a.cfg >= kNumCfgs + patch_num_cfgs() && conv_cfg_ok(a, a.cfg)) return launch_ws(a, k, a.cfg - kNumCfgs - patch_num_cfgs(), s);
  if (a.cfg >= kNumCfgs && conv_cfg_ok(a, a.cfg)) return launch_patch(a, k, a.cfg - kNumCfgs, s);
  if (a.cfg >= 0 && conv_cfg_ok(a, a.cfg)) return launch_cfg<T>(a.cfg, k, s);
  // heuristic: BN must divide every segment boundary; keep ~2 workgroups per CU when possible
  auto fits = [&](int) { return true; };
  int bn = 128;
  while (bn > 32 && !(fits(bn) && (a.Cout % bn == 0 || a.Cout > 2 * bn))) bn >>= 1;
  if (!fits(bn)) return hipErrorInvalidValue;
  auto blocks = [&](int bm_, int bn_) { return ((a.M + bm_ - 1) / bm_) * ((a.Cout + bn_ - 1) / bn_); };
  while (bn > 64 && blocks(128, bn) < 512) bn >>= 1;
  int bm = 128;
  if (bn <= 64 && blocks(128, bn) < 512) bm = 64;
  const int id = bm == 128 ? (bn == 128 ? 0 : bn == 64 ? 1 : 2) : (bn == 64 ? 3 : 4);
  return launch_cfg<T>(id, k, s);
}

hipError_t launch_conv(const ConvArgs& a, hipStream_t s) {
  if (a.M <= 0) return hipSuccess;
  const int es = dtype_size(a.dtype);
  const int bke = 128 / es;
  if (a.Cout % 8 || a.Kpad % bke || a.nseg < 1 || a.nseg > 4) return hipErrorInvalidValue;
  KArgs k;
  k.x = (const char*)a.x; k.w = (const char*)a.w; k.bias = a.bias; k.ktab = a.ktab;
  k.res = (const char*)a.res; k.slope = a.slope; k.zero = zero_page();
  k.ldx = a.ldx; k.H = a.H; k.W = a.W; k.Ho = a.Ho; k.Wo = a.Wo;
  k.sh = a.sh; k.sw = a.sw; k.ph = a.ph; k.pw = a.pw;
  k.K = a.K; k.Kpad = a.Kpad; k.nkt = a.Kpad / bke;
  k.wrs = a.Kpad * es; k.wts = 128;
  k.ncls = a.ncls; k.cout_pad = a.cout_pad;
  k.M = a.M; k.Cout = a.Cout; k.tiles_n = 0; k.nblk = 0;
  k.ldres = a.ldres; k.act = a.act; k.out_f32 = a.out_f32;
  k.nseg = a.nseg;
  k.KH = a.KH; k.KW = a.KW; k.Cin = a.Cin; k.pp = k.Wp = k.Hv = k.patch_bytes = k.lds_bytes = 0; k.dbg = nullptr;
  for (int i = 0; i < 4; ++i) {
    k.seg_c0[i] = i < a.nseg ? a.seg[i].c0 : 1 << 30;
    k.seg_c1[i] = i < a.nseg ? a.seg[i].c1 : 1 << 30;
    k.seg_ld[i] = i < a.nseg ? a.seg[i].ld : 0;
    k.seg_ptr[i] = i < a.nseg ? (char*)a.seg[i].ptr : nullptr;
  }
  switch (a.dtype) {
    case BF16: return launch_typed<__bf16>(a, k, s);
    case F16: return launch_typed<_Float16>(a, k, s);
    case F32: return launch_typed<float>(a, k, s);
    case F16X2: return launch_typed<sf16>(a, k, s);
    case F16P: return launch_typed<pf16>(a, k, s);
  }
  return hipErrorInvalidValue;
}

}  // namespace vnf
