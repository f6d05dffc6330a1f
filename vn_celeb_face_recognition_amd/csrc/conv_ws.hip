// Wave-specialised implicit-GEMM convolution for gfx950 (MI355X): big tiles at one workgroup per CU.
//
// With one 8-wave workgroup per CU the plain ring kernel (conv_igemm.hip) phase-locks: after the
// per-K-tile barrier every wave first queues its LDS-DMA pieces -- the texture path accepts about
// 28 B/clk/CU, so a 48-KiB K tile holds the waves ~1700 cycles at issue -- and only then
// multiplies, so the MFMA pipes idle during the issue phase and the DMA path idles during the
// MFMA phase.  Here the roles are split (MI355X_MICROARCH.md "ring-gemm"):
//   * WM x WN consumer waves (one per SIMD) only read fragments and issue MFMAs (conv_k_loop of
//     conv_device.h: LDS latency hides under the previous half K tile's MFMAs);
//   * LW loader waves only issue LDS-DMA pieces (im2col gather + swizzle in the source address,
//     exactly the ring kernel's image) and wait for them with counted vmcnt.
// One raw s_barrier per K tile joins both roles: after it tile kt has landed (the loaders waited
// for it) and stage (kt-1) % S is free (the consumers drained their reads of it), so the loaders
// refill it while the consumers multiply tile kt.  Same K order, operand roles and epilogue as the
// ring kernel, so results are bit-identical to it.
#include <type_traits>
#include <utility>

#include "conv_device.h"
#include "stamp.h"

namespace vnf {

// One K tile of a loader wave: its LA pixel pieces (im2col gather; e = the gather-table entry of this lane's k-chunk in K
// tile kt) and LB weight pieces, to the stage whose LDS byte address -- this wave's first piece -- is sbase.
template <typename T, int BM, int LW, int LA, int LB>
__device__ __forceinline__ void issue_pieces(const KArgs& a, const int4 e, unsigned sbase, int kt, const int (&abase)[LA],
                                             const int (&ahi)[LA], const int (&awi)[LA], const char* wsrc) {
#pragma unroll
  for (int p = 0; p < LA; ++p) {
    const int hi = ahi[p] + e.y, wi = awi[p] + e.z;
    const bool ok = e.w && (unsigned)hi < (unsigned)a.H && (unsigned)wi < (unsigned)a.W;
    const char* src = ok ? a.x + (size_t)(abase[p] + e.x) * sizeof(T) : a.zero;
    glds16(src, sbase + p * (LW * 1024));
  }
#pragma unroll
  for (int p = 0; p < LB; ++p)
    glds16(wsrc + (size_t)(p * LW * 8) * a.wrs + (size_t)kt * a.wts, sbase + BM * 128 + p * (LW * 1024));
}

// instrumented build: wait_dma_and_barrier<N> as two statements with a stamp in front of, between and behind them
// (N < 0: no wait for vector memory -- under stamps a consumer wave's only vector-memory operations are the stamps)
template <int N, class Stamp>
__device__ __forceinline__ void stamped_join(Stamp stamp) {
  stamp(0);
  if constexpr (N >= 0)
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(N) : "memory");
  else
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  stamp(1);
  asm volatile("s_barrier" ::: "memory");
  stamp(2);
}

template <typename T, int BM, int BN, int WM, int WN, int S, int LW, bool DBG = false>
__global__ __launch_bounds__((WM* WN + LW) * 64) void conv_igemm_ws_kernel(const KArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int WTM = BM / WM, WTN = BN / WN, TM = WTM / 16, TN = WTN / 16;
  constexpr int NC = WM * WN, NT = (NC + LW) * 64;
  constexpr int PA = BM / 8, PB = BN / 8;          // 1-KiB pieces (8 rows x 128 B) per K tile
  constexpr int LA = PA / LW, LB = PB / LW;        // pieces per loader wave
  constexpr int STAGE = (BM + BN) * 128;
  constexpr int CST = BN + 4;
  // epilogue staging budget handed to conv_epilogue: one pass over the whole tile only while its per-thread residual
  // prefetch (NIT x 8 floats, 256 consumer threads) stays within 64 registers -- beside 128 accumulators more spills
  constexpr int EPI_LDS = (BM * CST * 4 <= S * STAGE && (BM * (BN / 8)) / (NC * 64) <= 8) ? S * STAGE : (BM / WM) * CST * 4;
  constexpr int EPASS = (BM * CST * 4 <= EPI_LDS) ? 1 : WM;  // conv_epilogue's pass count
  static_assert(S >= 3 && PA % LW == 0 && PB % LW == 0, "pieces divide over the loader waves");

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int bid = xcd_remap(blockIdx.x, a.nblk);
  const int tile_m = bid / a.tiles_n, tile_n = bid - tile_m * a.tiles_n;
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const int nkt = a.nkt;
  // instrumented build (tools/stamp_ws.py): four cycle stamps per wave and K tile of workgroup 600, the first 64 K tiles
  auto stamp = [&](int kt, int slot) {
    if constexpr (DBG) {
      if (a.dbg && blockIdx.x == 600 && lane == 0 && kt < 64) a.dbg[(wave * 64 + kt) * 4 + slot] = __builtin_readcyclecounter();
    }
  };

  int4* sK = reinterpret_cast<int4*>(smem + S * STAGE);
  for (int i = tid; i < nkt * 8; i += NT) sK[i] = a.ktab[i];
  __syncthreads();  // gather table visible

  if (wave >= NC) {
    // ------------------------------------------------------------------ loader wave
    const int lw = wave - NC;
    const int prow = lane >> 3, lcol = lane & 7;
    const int lchunk = lcol ^ prow;  // piece rows start at multiples of 8: (row & 7) == prow
    int abase[LA], ahi[LA], awi[LA];
    row_setup<LA, LW * 8, true>(a, m0, lw * 8 + prow, abase, ahi, awi);
    const char* wsrc = a.w + (size_t)(n0 + lw * 8 + prow) * a.wrs + lchunk * 16;
    const unsigned lds0 = (unsigned)reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) char*)smem);
    auto issue = [&](int kt) {
      const unsigned sbase = __builtin_amdgcn_readfirstlane(lds0 + (unsigned)((kt % S) * STAGE) + (unsigned)(lw * 1024));
      issue_pieces<T, BM, LW, LA, LB>(a, sK[kt * 8 + lchunk], sbase, kt, abase, ahi, awi, wsrc);
    };
    auto wait_tile = [&](auto keep, int kt) {  // all but this wave's `keep` youngest pieces have landed; meet the others
      constexpr int N = decltype(keep)::value;
      if constexpr (DBG)
        stamped_join<N>([&](int slot) { stamp(kt, slot); });
      else
        wait_dma_and_barrier<N>();
    };
#pragma unroll
    for (int t = 0; t < S - 1; ++t)
      if (t < nkt) issue(t);
    for (int kt = 0; kt < nkt; ++kt) {
      if (kt + S - 2 < nkt)
        wait_tile(std::integral_constant<int, (S - 2) * (LA + LB)>{}, kt);
      else
        wait_tile(std::integral_constant<int, 0>{}, kt);
      if (kt + S - 1 < nkt) issue(kt + S - 1);
      stamp(kt, 3);
    }
    __syncthreads();
    if (conv_epilogue_is_fast<T, BM, BN>(a, S * STAGE)) {  // the consumers' epilogue barriers
      __syncthreads();
      return;
    }
    for (int pass = 0; pass < EPASS; ++pass) {
      __syncthreads();
      __syncthreads();
    }
    return;
  }

  // -------------------------------------------------------------------- consumer wave
  const int wm = wave / WN, wn = wave % WN;
  const int frow = lane & 15, fgrp = lane >> 4;
  f32x4_t acc[TM][TN];
  // Big wave tiles (8x4 MFMA tiles = 128 accumulator registers) keep ONE fragment set: two would spill.  Their 32
  // MFMAs per half K tile (512 cycles) dwarf the exposed read latency anyway; smaller tiles double-buffer.
  constexpr bool PIPE = (TM + TN) < 12;
  conv_k_loop<T, TM, TN, PIPE>(
      a.K, nkt, acc,
      [&](int kt) {
        if constexpr (DBG) {
          if (kt > 0) stamp(kt - 1, 3);  // the MFMAs of tile kt - 1 are issued (PIPE: but for its second half)
          stamped_join<-1>([&](int slot) { stamp(kt, slot); });
        } else {
          wait_dma_and_barrier<0>();  // no DMA of its own: drains this wave's fragment reads, then joins
        }
      },
      [&](int kt, int ks, uint4 (&x)[TM], uint4 (&w)[TN]) {
        const char* sA = smem + (kt % S) * STAGE;
        read_rows(sA, wm * WTM, frow, fgrp, ks, x);
        read_rows(sA + BM * 128, wn * WTN, frow, fgrp, ks, w);
      });
  stamp(nkt - 1, 3);
  __syncthreads();
  conv_epilogue<T, BM, BN, WM, WN, EPI_LDS>(a, acc, smem, m0, n0, S * STAGE);
}

// ---- persistent form -------------------------------------------------------------------------------------------
// One workgroup per CU walks the tiles blockIdx.x, blockIdx.x + gridDim.x, ...  The loader waves run the ring straight
// across tile boundaries (K tiles of the next output tile are in flight while the consumers finish this one), and the
// consumers store their accumulators from registers -- bias, ReLU, then swap_store: rounding to T and the lane-row swap
// that gives every lane 8 channels = one 16-byte store -- without touching LDS or a barrier.  In-kernel stamps of the
// one-tile-per-workgroup form (tools/stamp_patch.py): a workgroup spent 16 % of its life filling the pipeline and 18-29 %
// in the epilogue (the store burst of 256 workgroups in lockstep runs at HBM write speed); here both overlap the next
// tile's K loop.  Only for the layers of the fast epilogue (bias + ReLU, output in T, 2-byte T or planar split-f16).
// RES: a residual operand (Block8's up projection, small tiles only): its 16-byte chunks are fetched at the START of the
// tile -- behind the K loop they would wait, vmcnt being in issue order, for the previous tile's stores -- and un-swapped
// into the accumulator layout in the epilogue.  Same K order, operand roles, fp32 sum, bias add, residual add, max and
// rounding: bit-identical results.
template <typename T, int BM, int BN, int WM, int WN, int S, int LW, bool RES = false>
__global__ __launch_bounds__((WM* WN + LW) * 64) void conv_igemm_wsp_kernel(const KArgs a) {
  static_assert(sizeof(T) == 2 || is_planar<T>::value, "register epilogue: 2-byte elements or planar split-f16 units");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int ES = (int)sizeof(T);
  constexpr int WTM = BM / WM, WTN = BN / WN, TM = WTM / 16, TN = WTN / 16;
  constexpr int NC = WM * WN, NT = (NC + LW) * 64;
  constexpr int PA = BM / 8, PB = BN / 8;
  constexpr int LA = PA / LW, LB = PB / LW;
  constexpr int STAGE = (BM + BN) * 128;
  static_assert(S >= 3 && PA % LW == 0 && PB % LW == 0 && TN % 2 == 0, "pieces divide over the loader waves");

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nkt = a.nkt;
  const int G = (int)gridDim.x;
  const int ntile = (a.nblk - (int)blockIdx.x + G - 1) / G;  // this workgroup's tiles
  const int Q = ntile * nkt;                                   // ... and K tiles, one barrier each

  int4* sK = reinterpret_cast<int4*>(smem + S * STAGE);
  for (int i = tid; i < nkt * 8; i += NT) sK[i] = a.ktab[i];
  __syncthreads();

  if (wave >= NC) {
    // ------------------------------------------------------------------ loader wave
    const int lw = wave - NC;
    const int prow = lane >> 3, lcol = lane & 7;
    const int lchunk = lcol ^ prow;
    int abase[LA], ahi[LA], awi[LA];
    const char* wsrc = nullptr;
    auto setup = [&](int it) {
      const int bid = xcd_remap((int)blockIdx.x + it * G, a.nblk);
      const int tile_m = bid / a.tiles_n, tile_n = bid - tile_m * a.tiles_n;
      row_setup<LA, LW * 8, true>(a, tile_m * BM, lw * 8 + prow, abase, ahi, awi);
      wsrc = a.w + (size_t)(tile_n * BN + lw * 8 + prow) * a.wrs + lchunk * 16;
    };
    const unsigned lds0 = (unsigned)reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) char*)smem);
    int it_i = 0, kt_i = 0, st_i = 0;  // issue cursor: tile ordinal, K tile inside it, ring stage
    setup(0);
    auto issue = [&]() {
      const unsigned sbase = __builtin_amdgcn_readfirstlane(lds0 + (unsigned)(st_i * STAGE) + (unsigned)(lw * 1024));
      issue_pieces<T, BM, LW, LA, LB>(a, sK[kt_i * 8 + lchunk], sbase, kt_i, abase, ahi, awi, wsrc);
      st_i = st_i + 1 == S ? 0 : st_i + 1;
      if (++kt_i == nkt) {
        kt_i = 0;
        if (++it_i < ntile) setup(it_i);
      }
    };
#pragma unroll
    for (int t = 0; t < S - 1; ++t)
      if (t < Q) issue();
    for (int q = 0; q < Q; ++q) {
      if (q + S - 2 < Q)
        wait_dma_and_barrier<(S - 2) * (LA + LB)>();
      else
        wait_dma_and_barrier<0>();
      if (q + S - 1 < Q) issue();
    }
    return;
  }

  // -------------------------------------------------------------------- consumer wave
  const int wm = wave / WN, wn = wave % WN;
  const int frow = lane & 15, fgrp = lane >> 4;
  // no staging epilogue here: the 4 x 8 wave tile double-buffers too (2-byte dtypes; the planar hi/lo sets would spill)
  constexpr bool PIPE = (TM + TN) < 12 || ((TM + TN) == 12 && !is_planar<T>::value);
  const bool relu = a.act == ACT_RELU, prelu = a.act == ACT_PRELU;
  int st = 0;  // ring stage of the K tile being read: the ring runs on across output tiles
  for (int it = 0; it < ntile; ++it) {
    const int bid = xcd_remap((int)blockIdx.x + it * G, a.nblk);
    const int tile_m = bid / a.tiles_n, tile_n = bid - tile_m * a.tiles_n;
    const int m0 = tile_m * BM, n0 = tile_n * BN;
    f32x4_t acc[TM][TN];
    uint4 rres[RES ? TM : 1][RES ? TN / 2 : 1];
    if constexpr (RES) {
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int jp = 0; jp < TN / 2; ++jp) {
          const int c = n0 + wn * WTN + (2 * jp + (fgrp & 1)) * 16 + (fgrp >> 1) * 8;
          const int m = min(m0 + wm * WTM + i * 16 + frow, a.M - 1);
          rres[i][jp] = *reinterpret_cast<const uint4*>(a.res + ((size_t)m * a.ldres + (c < a.Cout ? c : 0)) * ES);
        }
    }
    conv_k_loop<T, TM, TN, PIPE>(
        a.K, nkt, acc,
        [&](int) {
          // no vmcnt here: this wave's only vector-memory operations are the previous tile's stores, which may still drain
          asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        },
        [&](int, int ks, uint4 (&x)[TM], uint4 (&w)[TN]) {
          const char* sA = smem + st * STAGE;
          read_rows(sA, wm * WTM, frow, fgrp, ks, x);
          read_rows(sA + BM * 128, wn * WTN, frow, fgrp, ks, w);
        },
        [&](int) { st = st + 1 == S ? 0 : st + 1; });

    // register epilogue: tiles j (even) and j+1 of a lane-row pair are exchanged so each lane holds 8 channels
#pragma unroll
    for (int j = 0; j < TN; j += 2) {
      const int cq = n0 + wn * WTN + j * 16 + fgrp * 4;  // this lane's channel quad in tile j; tile j+1: +16
      const f32x4_t b0 = cq < a.Cout ? *reinterpret_cast<const f32x4_t*>(a.bias + cq) : f32x4_t{0.f, 0.f, 0.f, 0.f};
      const f32x4_t b1 =
          cq + 16 < a.Cout ? *reinterpret_cast<const f32x4_t*>(a.bias + cq + 16) : f32x4_t{0.f, 0.f, 0.f, 0.f};
      f32x4_t s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0;
      if (prelu) {
        if (cq < a.Cout) s0 = *reinterpret_cast<const f32x4_t*>(a.slope + cq);
        if (cq + 16 < a.Cout) s1 = *reinterpret_cast<const f32x4_t*>(a.slope + cq + 16);
      }
      const int c = n0 + wn * WTN + (j + (fgrp & 1)) * 16 + (fgrp >> 1) * 8;  // the 8 channels it stores
      int sg = 0;
#pragma unroll
      for (int s2 = 1; s2 < 4; ++s2)
        if (s2 < a.nseg && c >= a.seg_c0[s2]) sg = s2;
      char* const dcol = a.seg_ptr[sg] + (size_t)(c - a.seg_c0[sg]) * ES;
      const int dld = a.seg_ld[sg];
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        float v0[4], v1[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v0[e] = acc[i][j][e] + b0[e];
          v1[e] = acc[i][j + 1][e] + b1[e];
        }
        if constexpr (RES) {
          // the chunk this lane will store holds, swapped, the residual of its two accumulator quads
          typedef T tx4 __attribute__((ext_vector_type(4)));
          const uint4 r = rres[i][j / 2];
          const auto rx = __builtin_amdgcn_permlane16_swap(r.x, r.z, false, false);
          const auto ry = __builtin_amdgcn_permlane16_swap(r.y, r.w, false, false);
          const tx4 q0 = __builtin_bit_cast(tx4, uint2{rx[0], ry[0]}), q1 = __builtin_bit_cast(tx4, uint2{rx[1], ry[1]});
#pragma unroll
          for (int e = 0; e < 4; ++e) { v0[e] += (float)q0[e]; v1[e] += (float)q1[e]; }
        }
        if (relu) {
#pragma unroll
          for (int e = 0; e < 4; ++e) { v0[e] = fmaxf(v0[e], 0.f); v1[e] = fmaxf(v1[e], 0.f); }
        }
        if (prelu) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            v0[e] = v0[e] > 0.f ? v0[e] : v0[e] * s0[e];
            v1[e] = v1[e] > 0.f ? v1[e] : v1[e] * s1[e];
          }
        }
        const int m = m0 + wm * WTM + i * 16 + frow;
        swap_store<T>(dcol + (size_t)m * dld * ES, m < a.M && c < a.Cout, f32x4_t{v0[0], v0[1], v0[2], v0[3]},
                      f32x4_t{v1[0], v1[1], v1[2], v1[3]});
      }
    }
  }
}

// ===================================================================== host side
struct WsCfg { int bm, bn, wm, wn, s, lw; };
static constexpr WsCfg kWs[] = {
    {256, 128, 2, 2, 3, 4}, {256, 128, 4, 1, 3, 4}, {128, 128, 2, 2, 3, 4}, {128, 128, 2, 2, 4, 4},
    {256, 64, 4, 1, 3, 4},  {128, 192, 2, 2, 3, 4}, {128, 256, 2, 2, 3, 4}, {128, 64, 2, 2, 4, 4},
    {256, 128, 2, 2, 3, 2}, {128, 128, 2, 2, 4, 2}, {128, 192, 2, 2, 3, 2}, {192, 128, 2, 2, 3, 4},
    // 160-row tiles: the 17x17 layers' 73,984 pixels are 578 tiles of 128 = 2.26 rounds over 256 CUs (a third round for a
    // quarter of them) but 463 tiles of 160 = 1.81
    {160, 256, 2, 2, 3, 4}, {160, 192, 2, 2, 3, 4},
    // small tiles for the 3x3-pixel tail (M = 9 rows per image): persistent, so their 6-28 K tiles per output tile run
    // back to back instead of each paying a pipeline fill and an epilogue
    {64, 64, 2, 2, 4, 4},   {64, 128, 2, 2, 4, 4},  {32, 64, 2, 2, 6, 4},   {32, 128, 2, 2, 4, 4},  {64, 64, 2, 2, 8, 4},
    // 224 rows beside BN = 192 (last, so every older id keeps its number): the tile height is capped by LDS, three
    // stages of (BM + BN) x 128 B plus the gather table within 160 KiB, and 3 x 416 x 128 + 12 x 128 = 161,280 B still
    // fits conv2d_4a's K = 720 (ws_cfg_ok refuses it past 32 K tiles: K = 2304).  A K tile moves 53,248 B through the ~28 B/clk
    // LDS-DMA path for 1.4 x the FLOPs of the 160 x 192 tile's 45,056 B: 15.6 % fewer bytes per FLOP on the path that
    // bounds the layer, and its 331,776 pixels are 1,482 tiles = 5.79 rounds of 256 CUs instead of 2,074 = 8.10.
    // TN = 6 per wave is even, so the persistent form exists (236 VGPRs, no scratch); 7 x 3 > 8: no RES form.  The
    // one-tile and planar forms spill (256 VGPRs + ~300 B/lane of scratch): correct, slow, never the tuner's choice.
    {224, 192, 2, 2, 3, 4},
};
constexpr int kNumWs = (int)(sizeof(kWs) / sizeof(kWs[0]));

int ws_num_cfgs() { return kNumWs; }
bool ws_cfg_tile(int wcfg, ConvTile& t) {
  if (wcfg < 0 || wcfg >= kNumWs) return false;
  t = ConvTile{2, kWs[wcfg].bm, kWs[wcfg].bn, kWs[wcfg].wm, kWs[wcfg].wn, kWs[wcfg].s};
  return true;
}

bool ws_cfg_ok(const ConvArgs& a, int wcfg) {
  if (wcfg < 0 || wcfg >= kNumWs) return false;
  const WsCfg& c = kWs[wcfg];
  if (a.Cout <= c.bn / 2) return false;
  if (((a.Cout + c.bn - 1) / c.bn) * c.bn > a.cout_pad) return false;
  if ((c.bn % 64) && a.Cout % c.bn) return false;
  const int lds = c.s * (c.bm + c.bn) * 128 + (a.Kpad / (128 / dtype_size(a.dtype))) * 8 * 16;
  return lds <= 160 * 1024;
}

// tile grid of a launch into kk; returns its dynamic LDS, the ring and the gather table
static int ws_geometry(KArgs& kk, int bm, int bn, int s) {
  kk.tiles_n = (kk.Cout + bn - 1) / bn;
  kk.nblk = ((kk.M + bm - 1) / bm) * kk.tiles_n;
  return s * (bm + bn) * 128 + kk.nkt * 8 * 16;
}

template <typename T, int BM, int BN, int WM, int WN, int S, int LW>
static hipError_t launch_one_tile(const KArgs& k, hipStream_t s) {
  allow_dynamic_lds<conv_igemm_ws_kernel<T, BM, BN, WM, WN, S, LW>>(160 * 1024);
  KArgs kk = k;
  const int lds = ws_geometry(kk, BM, BN, S);
  hipLaunchKernelGGL((conv_igemm_ws_kernel<T, BM, BN, WM, WN, S, LW>), dim3(kk.nblk), dim3((WM * WN + LW) * 64), lds, s,
                     kk);
  return hipGetLastError();
}

static int cu_count() {   // of the current device
  static std::atomic<int> n[16];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return 256;
  int c = n[dev].load(std::memory_order_relaxed);
  if (c) return c;
  hipDeviceProp_t p;
  if (hipGetDeviceProperties(&p, dev) != hipSuccess) return 256;
  n[dev].store(c = p.multiProcessorCount > 0 ? p.multiProcessorCount : 256, std::memory_order_relaxed);
  return c;
}

// the persistent form (bias + ReLU layers of the 2-byte plans; ConvArgs::ws_persist = 0, from VNF_WS_PERSIST=0 at the
// handle's create, keeps one tile per workgroup)
static bool ws_persistent(const ConvArgs& a, const KArgs& k) { return a.ws_persist && k.ncls == 1 && !k.out_f32; }

template <typename T, int BM, int BN, int WM, int WN, int S, int LW, bool RES>
static hipError_t launch_persistent(const KArgs& k, hipStream_t s) {
  allow_dynamic_lds<conv_igemm_wsp_kernel<T, BM, BN, WM, WN, S, LW, RES>>(160 * 1024);
  KArgs kk = k;
  const int lds = ws_geometry(kk, BM, BN, S);
  // one workgroup per CU per LDS-resident copy; whole rounds of 8 workgroups keep the blockIdx -> XCD map of xcd_remap
  // (tile t runs on XCD t % 8)
  const int per_cu = lds <= 80 * 1024 ? 2 : 1;
  const int slots = cu_count() * per_cu;
  int grid = kk.nblk < slots ? kk.nblk : slots & ~7;
  if (grid < 1) grid = kk.nblk;
  hipLaunchKernelGGL((conv_igemm_wsp_kernel<T, BM, BN, WM, WN, S, LW, RES>), dim3(grid), dim3((WM * WN + LW) * 64), lds, s,
                     kk);
  return hipGetLastError();
}

template <typename T, int BM, int BN, int WM, int WN, int S, int LW>
static hipError_t launch_one(const ConvArgs& a, const KArgs& k, hipStream_t s) {
  if constexpr ((sizeof(T) == 2 || is_planar<T>::value) && (BN / WN / 16) % 2 == 0) {
    if (ws_persistent(a, k)) {
      if (!k.res) return launch_persistent<T, BM, BN, WM, WN, S, LW, false>(k, s);
      // residual chunks live in registers for the whole K loop: small tiles only
      if constexpr (sizeof(T) == 2 && (BM / WM / 16) * (BN / WN / 32) <= 8)
        return launch_persistent<T, BM, BN, WM, WN, S, LW, true>(k, s);
    }
  }
  return launch_one_tile<T, BM, BN, WM, WN, S, LW>(k, s);
}

// wcfg -> launch_one<T, kWs[wcfg]...>: entry I of the table is the template argument list of launcher I
template <typename T, size_t... I>
static hipError_t launch_ws_typed(int wcfg, const ConvArgs& a, const KArgs& k, hipStream_t s, std::index_sequence<I...>) {
  static constexpr hipError_t (*kLaunch[])(const ConvArgs&, const KArgs&, hipStream_t) = {
      launch_one<T, kWs[I].bm, kWs[I].bn, kWs[I].wm, kWs[I].wn, kWs[I].s, kWs[I].lw>...};
  return (unsigned)wcfg < sizeof...(I) ? kLaunch[wcfg](a, k, s) : hipErrorInvalidValue;
}
template <typename T>
static hipError_t launch_ws_typed(int wcfg, const ConvArgs& a, const KArgs& k, hipStream_t s) {
  return launch_ws_typed<T>(wcfg, a, k, s, std::make_index_sequence<kNumWs>{});
}

// Instrumented launch (tools/stamp_ws.py): VNF_WS_STAMP=<file> dumps per-K-tile s_memtime stamps of workgroup 600
// of every bf16 launch of the tile kStamp with more than 600 workgroups.
#ifdef VNF_STAMPS
constexpr WsCfg kStamp = {128, 192, 2, 2, 3, 4};
constexpr int ws_cfg_id(const WsCfg& q) {
  for (int i = 0; i < kNumWs; ++i)
    if (kWs[i].bm == q.bm && kWs[i].bn == q.bn && kWs[i].wm == q.wm && kWs[i].wn == q.wn && kWs[i].s == q.s && kWs[i].lw == q.lw) return i;
  return -1;
}
constexpr int kStampId = ws_cfg_id(kStamp);
static_assert(kStampId >= 0, "the instrumented tile is one of kWs");

static hipError_t launch_stamped(const KArgs& k, hipStream_t s) {
  constexpr auto kernel = conv_igemm_ws_kernel<__bf16, kStamp.bm, kStamp.bn, kStamp.wm, kStamp.wn, kStamp.s, kStamp.lw, true>;
  KArgs kk = k;
  const int lds = ws_geometry(kk, kStamp.bm, kStamp.bn, kStamp.s);
  return stamped_launch(
      "VNF_WS_STAMP", 8 * 64 * 4, s,
      [&](long long* dbuf) {
        kk.dbg = dbuf;
        allow_dynamic_lds<kernel>(160 * 1024);
        hipLaunchKernelGGL(kernel, dim3(kk.nblk), dim3((kStamp.wm * kStamp.wn + kStamp.lw) * 64), lds, s, kk);
      },
      [&](FILE* f, const long long* host) {
        fprintf(f, "launch M=%d N=%d nkt=%d nblk=%d\n", k.M, k.Cout, k.nkt, kk.nblk);
        for (int w = 0; w < 8; ++w)
          for (int kt = 0; kt < k.nkt && kt < 64; ++kt)
            fprintf(f, "%d %d %lld %lld %lld %lld\n", w, kt, host[(w * 64 + kt) * 4], host[(w * 64 + kt) * 4 + 1],
                    host[(w * 64 + kt) * 4 + 2], host[(w * 64 + kt) * 4 + 3]);
      });
}
#endif

hipError_t launch_ws(const ConvArgs& a, const KArgs& k, int wcfg, hipStream_t s) {
  if (!ws_cfg_ok(a, wcfg) || !k.zero) return hipErrorInvalidValue;
#ifdef VNF_STAMPS
  if (getenv("VNF_WS_STAMP") && wcfg == kStampId && a.dtype == BF16 &&
      (k.M + kStamp.bm - 1) / kStamp.bm * ((k.Cout + kStamp.bn - 1) / kStamp.bn) > 600)
    return launch_stamped(k, s);
#endif
  switch (a.dtype) {
    case BF16: return launch_ws_typed<__bf16>(wcfg, a, k, s);
    case F16: return launch_ws_typed<_Float16>(wcfg, a, k, s);
    case F32: return launch_ws_typed<float>(wcfg, a, k, s);
    case F16X2: return launch_ws_typed<sf16>(wcfg, a, k, s);
    case F16P: return launch_ws_typed<pf16>(wcfg, a, k, s);
  }
  return hipErrorInvalidValue;
}

}  // namespace vnf
