// The device core the gallery kernels share: the handle, the 64-bit candidate key, the lane layout
// of a sum of squares, and the two pieces that decide a score's bits -- the load and normalisation of a wave's 16 queries
// into MFMA B fragments, and one 32-row tile of the exact-f32 MFMA stream.  gallery_search_kernel (gallery.hip) and
// gallery_mated_kernel (gallery_mated.hip) both call them, so the score of a (query, row) pair has the same bits in
// both: by construction, not by two copies that happen to agree.
#pragma once
#include "engine.h"

namespace vnf {

typedef float f32x4_t __attribute__((ext_vector_type(4)));

constexpr int GAL_MAX_KG = 32;      // dim <= 512: groups of 16 k
constexpr int GAL_MAX_K = 16;
constexpr float GAL_EPS = 1e-12f;   // F.normalize's eps
constexpr int64_t GAL_MAX_ROWS = 0x7FFFFFFF;

struct Gallery : HandleBase {
  static constexpr HandleKind KIND = HandleKind::Gallery;
  Gallery() : HandleBase(KIND) {}
  int dim = 0;
  int64_t rows = 0, cap = 0;
  float* mat = nullptr;        // (cap, dim), rows [0, rows) are unit vectors
  int32_t* labels = nullptr;   // (cap)
  ~Gallery() override {
    (void)hipFree(mat);
    (void)hipFree(labels);
  }
};

// ||x||^2 of the row a group of four lanes (lane & 15 equal, lane >> 4 = 0..3) holds: `part` is the lane's own sum, taken
// over its elements k = 16 kg + 4 (lane >> 4) + j in ascending (kg, j) as s = s + x * x from 0; the four are combined as
// (p0 + p1) + (p2 + p3).  Every lane of the group gets the same bits.
static __device__ __forceinline__ float sum_of_squares(float part) {
  part = part + __shfl_xor(part, 16);
  return part + __shfl_xor(part, 32);
}

static __device__ __forceinline__ uint64_t gallery_key(float s, uint32_t row) {
  const uint32_t u = __float_as_uint(s == 0.f ? 0.f : s);   // -0 ties with +0
  const uint32_t m = (s != s) ? 1u : ((u & 0x80000000u) ? ~u : (u | 0x80000000u));
  return ((uint64_t)m << 32) | (uint64_t)(0xFFFFFFFFu - row);
}

static __device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int mask) {
  const uint32_t lo = __shfl_xor((uint32_t)v, mask), hi = __shfl_xor((uint32_t)(v >> 32), mask);
  return ((uint64_t)hi << 32) | lo;
}

// The wave's 16 queries, normalised, as B fragments: lane (c = lane & 15, g = lane >> 4) holds elements
// k = 16 kg + 4 g + j of query qrow.  KG groups of 16 k are held; EXACT: dim == 16 KG, otherwise the groups at and beyond
// kgs = dim / 16 are zero.  A lane whose query does not exist (!qok) holds zeros.
template <int KG, bool EXACT>
static __device__ __forceinline__ void gallery_load_queries(const float* __restrict__ q, int qrow, bool qok, int dim, int g, int kgs,
                                                            f32x4_t (&qf)[KG]) {
  const float* qp = q + (size_t)(qok ? qrow : 0) * dim + 4 * g;
  float ss = 0.f;
#pragma unroll
  for (int kg = 0; kg < KG; ++kg) {
    f32x4_t v = {0.f, 0.f, 0.f, 0.f};
    if (EXACT || kg < kgs) v = *reinterpret_cast<const f32x4_t*>(qp + kg * 16);
    if (!qok) v = f32x4_t{0.f, 0.f, 0.f, 0.f};
    qf[kg] = v;
#pragma unroll
    for (int j = 0; j < 4; ++j) ss = ss + v[j] * v[j];   // + 0 past dim: the bits do not see KG
  }
  const float d = fmaxf(sqrtf(sum_of_squares(ss)), GAL_EPS);
#pragma unroll
  for (int kg = 0; kg < KG; ++kg)
#pragma unroll
    for (int j = 0; j < 4; ++j) qf[kg][j] = qf[kg][j] / d;
}

// gallery_load_queries' sibling for a self-join (gallery_cluster.hip, f-17): 16 STORED rows of the gallery as B fragments in
// the same lane layout, as they are -- no second normalisation, so the score of (row i, row j) is the sum of the same
// products in the same order whichever of the two is the B fragment.
template <int KG, bool EXACT>
static __device__ __forceinline__ void gallery_load_rows(const float* __restrict__ gal, int64_t row, bool ok, int dim, int g, int kgs,
                                                         f32x4_t (&qf)[KG]) {
  const float* qp = gal + (size_t)(ok ? row : 0) * dim + 4 * g;
#pragma unroll
  for (int kg = 0; kg < KG; ++kg) {
    f32x4_t v = {0.f, 0.f, 0.f, 0.f};
    if (EXACT || kg < kgs) v = *reinterpret_cast<const f32x4_t*>(qp + kg * 16);
    if (!ok) v = f32x4_t{0.f, 0.f, 0.f, 0.f};
    qf[kg] = v;
  }
}

// One step of the stream: the 16 queries against gallery rows [r0, r0 + 32) of the chunk [r_begin, r_end).  Lane (c, g)
// reads 16 contiguous bytes of row r0 + c (and r0 + 16 + c) per group of 16 k; a row past the chunk reads the chunk's first
// instead.  MFMA j takes element j of both operands: a fixed permutation of k inside each group of 16, the same for every
// (query, row) pair.  D[row = 4 g + r][col = c]: acc0[r] is this lane's query against row r0 + 4 g + r, acc1[r] against
// row r0 + 16 + 4 g + r.
template <int KG, bool EXACT>
static __device__ __forceinline__ void gallery_tile(const float* __restrict__ gal, int64_t r0, int64_t r_begin, int64_t r_end, int dim,
                                                    int c, int g, int kgs, const f32x4_t (&qf)[KG], f32x4_t& acc0, f32x4_t& acc1) {
  const int64_t ra = r0 + c, rb = r0 + 16 + c;
  const float* pa = gal + (size_t)(ra < r_end ? ra : r_begin) * dim + 4 * g;
  const float* pb = gal + (size_t)(rb < r_end ? rb : r_begin) * dim + 4 * g;
  acc0 = f32x4_t{0.f, 0.f, 0.f, 0.f};
  acc1 = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kg = 0; kg < KG; ++kg) {
    if (EXACT || kg < kgs) {   // wave-uniform
      const f32x4_t a = *reinterpret_cast<const f32x4_t*>(pa + kg * 16);
      const f32x4_t b = *reinterpret_cast<const f32x4_t*>(pb + kg * 16);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], qf[kg][j], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(b[j], qf[kg][j], acc1, 0, 0, 0);
      }
    }
  }
}

// chunk_rows == 0: about 2048 waves in flight however many queries there are, chunks of 64 rows at least (a wave's
// start-up -- 16 queries loaded and normalised -- costs about one step), whole steps of 32 rows.
static inline int64_t gallery_chunk_rows(int F, int64_t G, int64_t chunk_rows) {
  if (chunk_rows > 0) return chunk_rows;
  const int64_t nqg = F > 0 ? (F + 15) / 16 : 1;
  const int64_t target = 2048 / nqg > 0 ? 2048 / nqg : 1;
  int64_t c = (G + target - 1) / target;
  c = (c + 31) / 32 * 32;
  return c < 64 ? 64 : c;
}

// Stage two of both searches (gallery_merge_kernel, gallery.hip): partial (nchunks, F, k) descending key lists -> the k
// best of each of the F queries, decoded into idx / label / score (F, k).
hipError_t gallery_launch_merge(const uint64_t* partial, int64_t nchunks, int F, int k, const int32_t* labels, int32_t* idx_out,
                                int32_t* label_out, float* score_out, hipStream_t stream);

}  // namespace vnf
