// The streaming core under the five gallery kernels (DESIGN.md 1 f-15 .. f-18).  A wave holds 16 vectors as MFMA B
// fragments and streams gallery rows past them 32 at a time through the exact-f32 MFMA; a lane ends up with one vector's
// scores against eight rows of each tile and reduces them across the four lanes of its vector.  Here: the handle, the
// candidate key and its inverse, the lane descriptor, the loads that decide a score's bits (gallery_load_queries /
// gallery_load_rows, gallery_tile), the walk over a lane's (row, score) pairs, the keyed maximum over four lanes; for
// the host the chunk / grid plan, the EXACT dispatch and the workspace carver; and the stages every user ends with.
// The kernels add their epilogues, so a pair's score has the same bits in all: by construction, not by agreeing copies.
#pragma once
#include <type_traits>

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

// The total order (score descending, row ascending, a NaN below every number) as one unsigned comparison: the monotone
// image of the score << 32 | (0xFFFFFFFF - row).  0 is no candidate; gallery_key_row / gallery_key_score invert a real key.
static __device__ __forceinline__ uint64_t gallery_key(float s, uint32_t row) {
  const uint32_t u = __float_as_uint(s == 0.f ? 0.f : s);   // -0 ties with +0
  const uint32_t m = (s != s) ? 1u : ((u & 0x80000000u) ? ~u : (u | 0x80000000u));
  return ((uint64_t)m << 32) | (uint64_t)(0xFFFFFFFFu - row);
}

static __device__ __forceinline__ uint32_t gallery_key_row(uint64_t key) { return 0xFFFFFFFFu - (uint32_t)key; }

static __device__ __forceinline__ float gallery_key_score(uint64_t key) {
  const uint32_t m = (uint32_t)(key >> 32);
  return __uint_as_float(m == 1u ? 0x7FC00000u : ((m & 0x80000000u) ? (m ^ 0x80000000u) : ~m));
}

static __device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int mask) {
  const uint32_t lo = __shfl_xor((uint32_t)v, mask), hi = __shfl_xor((uint32_t)(v >> 32), mask);
  return ((uint64_t)hi << 32) | lo;
}

// The largest key of the four lanes of a vector, in all four.  They hold disjoint rows and real keys differ pairwise.
static __device__ __forceinline__ uint64_t gallery_max4(uint64_t key) {
  uint64_t o = shfl_xor_u64(key, 16);
  key = o > key ? o : key;
  o = shfl_xor_u64(key, 32);
  return o > key ? o : key;
}

// parent[] of a union-find or a pointer jump: written by atomics while other lanes read it.
static __device__ __forceinline__ int32_t gallery_load_relaxed(const int32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Where a lane stands.  c = lane & 15 is its vector among the wave's 16 and its row of a half tile's A fragment,
// g = lane >> 4 its quarter of each group of 16 k; qrow is its vector (a query, a probe, a stored row), qok whether that
// exists.  KG groups of 16 k are held; EXACT: dim == 16 KG, otherwise the groups at and beyond kgs = dim / 16 are skipped.
// The chunked kernels stream rows [r_begin, r_end) of chunk `chunk`; tracks_best_kernel sets its own window.  Row: int where
// the vectors are queries (F is an int), int64_t where they are rows of the gallery: the index arithmetic of each kind.
template <class Row>
struct GalleryLane {
  int c, g, kgs;
  Row qrow;
  int64_t chunk, r_begin, r_end;
  bool qok;
};

// The lane of the wave that holds vectors [16 qg, 16 qg + 16) of n.
template <int KG, bool EXACT, class Row, class Group>
static __device__ __forceinline__ void gallery_lane(GalleryLane<Row>& L, Group qg, Row n, int dim) {
  const int lane = threadIdx.x & 63;
  L.c = lane & 15;
  L.g = lane >> 4;
  L.kgs = EXACT ? KG : (dim >> 4);
  L.qrow = (Row)qg * 16 + L.c;
  L.qok = L.qrow < n;
}

// The four waves of a workgroup take consecutive (chunk, vector group) pairs of the nwork = nchunks * nqg, vector group
// fastest: with 64 vectors or fewer each chunk of the G rows is read by one workgroup.  A kernel takes w = gallery_wave()
// and leaves where w >= nwork itself: returned through this helper the test changes how the arguments are loaded.
static __device__ __forceinline__ int64_t gallery_wave() { return (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); }

template <int KG, bool EXACT, class Row>
static __device__ __forceinline__ void gallery_lane_chunked(GalleryLane<Row>& L, int64_t w, int nqg, Row n, int dim) {
  L.chunk = w / nqg;
  gallery_lane<KG, EXACT>(L, (int)(w % nqg), n, dim);
}

// The rows of the lane's chunk.  A call of its own, made where the stream begins: computed in the prologue the two bounds
// stay live across the load of the 16 vectors, which costs the query kernels registers and waits.
template <class Row>
static __device__ __forceinline__ void gallery_lane_rows(GalleryLane<Row>& L, int64_t chunk_rows, int64_t G) {
  L.r_begin = L.chunk * chunk_rows;
  L.r_end = (L.r_begin + chunk_rows < G) ? L.r_begin + chunk_rows : G;
}

// The wave's 16 queries, normalised, as B fragments: lane (c, g) holds elements k = 16 kg + 4 g + j of query qrow.
// The groups at and beyond kgs are zero, and so is a lane whose query does not exist (!qok).
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

// gallery_load_queries' sibling for a self-join (f-17, f-18): 16 STORED rows of the gallery as B fragments in the same
// lane layout, as they are -- no second normalisation, so the score of (row i, row j) is the sum of the same products in
// the same order whichever of the two is the B fragment.
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

// One step of the stream: the 16 vectors against gallery rows [r0, r0 + 32) of the chunk [r_begin, r_end).  Lane (c, g)
// reads 16 contiguous bytes of row r0 + c (and r0 + 16 + c) per group of 16 k; a row past the chunk reads the chunk's first
// instead.  MFMA j takes element j of both operands: a fixed permutation of k inside each group of 16, the same for every
// pair of vectors, so a score's bits depend on the two vectors alone: not on their number, not on the row's place in a
// tile, not on the chunking.  D[row = 4 g + r][col = c]: gallery_for_each walks it.
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

// A lane's eight (row, score) pairs of the tile at r0: fn(t, i, s, in) for t = 0 .. 7 in the order i = r0 + 4 g + r,
// then i + 16, r = 0 .. 3, with s the lane's vector against row i and in = i < r_end (s means nothing otherwise).
// tracks_best_kernel's epilogue is a call of this.  The four chunked kernels keep the same walk written out, two rows a
// step as their epilogues interleave them: handed their rows through a callable, one at a time or in pairs, the compiler
// orders their selects and branches differently and every one of them measured slower (profiles/gallery_core_ab.txt).
template <class Fn>
static __device__ __forceinline__ void gallery_for_each(int64_t r0, int g, int64_t r_end, const f32x4_t& acc0, const f32x4_t& acc1, Fn&& fn) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t i0 = r0 + 4 * g + r, i1 = i0 + 16;
    fn(r, i0, acc0[r], i0 < r_end);
    fn(4 + r, i1, acc1[r], i1 < r_end);
  }
}

// One int per row (a label, a core flag) of rows i0 .. i0 + 3, the lane's rows of a half tile; issued before gallery_tile
// so that the loads fly under the MFMAs.  A row at or past r_end reads the chunk's first row instead (its pair is never
// in).  vec: i0 is a multiple of 4 (wave-uniform: the chunk begins at one), so that 16 bytes can be read at once.
static __device__ __forceinline__ void gallery_int4(const int32_t* __restrict__ v, int64_t i0, int64_t r_begin, int64_t r_end, bool vec,
                                                    int32_t* out) {
  if (vec && i0 + 3 < r_end) {
    const int4 x = *reinterpret_cast<const int4*>(v + i0);
    out[0] = x.x; out[1] = x.y; out[2] = x.z; out[3] = x.w;
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r) out[r] = v[i0 + r < r_end ? i0 + r : r_begin];
  }
}

// chunk_rows == 0: about 2048 waves in flight however many vectors there are, chunks of 64 rows at least (a wave's
// start-up -- 16 vectors loaded and normalised -- costs about one step), whole steps of 32 rows.
static inline int64_t gallery_chunk_rows(int64_t F, int64_t G, int64_t chunk_rows) {
  if (chunk_rows > 0) return chunk_rows;
  const int64_t nqg = F > 0 ? (F + 15) / 16 : 1;
  const int64_t target = 2048 / nqg > 0 ? 2048 / nqg : 1;
  int64_t c = (G + target - 1) / target;
  c = (c + 31) / 32 * 32;
  return c < 64 ? 64 : c;
}

// The grid of a chunked kernel: F vectors in nqg groups of 16 against G rows in nchunks chunks, a wave per pair, four waves
// a workgroup.  !ok: more workgroups than a grid holds (the caller's "chunk_rows too small").  F, G <= GAL_MAX_ROWS.
struct GalleryPlan {
  int64_t chunk_rows, nchunks, nwork, blocks;
  int nqg;
  bool ok;
  GalleryPlan(int64_t F, int64_t G, int64_t chunk_rows_arg) {
    chunk_rows = gallery_chunk_rows(F, G, chunk_rows_arg);
    nchunks = (G + chunk_rows - 1) / chunk_rows;
    nqg = (int)((F + 15) / 16);
    nwork = nchunks * nqg;
    blocks = (nwork + 3) / 4;
    ok = blocks <= 0x7FFFFFFF;
  }
};

// fn(std::bool_constant<EXACT>) for the gallery's dim: a launch names its kernel<GAL_MAX_KG, decltype(exact)::value> once.
template <class Fn>
static inline void gallery_dispatch(int dim, Fn&& fn) {
  if (dim == 16 * GAL_MAX_KG) fn(std::true_type{});
  else fn(std::false_type{});
}

// Hands out the sections of a workspace in order, each rounded up to a multiple of 16 bytes; `bytes` is the total so far.
// A null base only counts.
struct GalleryCarver {
  char* base;
  int64_t bytes = 0;
  template <class T>
  T* take(int64_t nbytes) {
    T* p = base ? reinterpret_cast<T*>(base + bytes) : nullptr;
    bytes += (nbytes + 15) / 16 * 16;
    return p;
  }
};

// Stage two of the searches (gallery_merge_kernel, gallery.hip): partial (nchunks, F, k) descending key lists -> the k
// best of each of the F queries, decoded into idx / label / score (F, k).
hipError_t gallery_launch_merge(const uint64_t* partial, int64_t nchunks, int F, int k, const int32_t* labels, int32_t* idx_out,
                                int32_t* label_out, float* score_out, hipStream_t stream);

// Stage C of clustering and tracks, "roots to consecutive numbers" (cluster_number_kernel, cluster_write_kernel,
// gallery_cluster.hip): flag[i] = 1 where row i is a root and 0 elsewhere up to the next multiple of 4 entries, root[i] a
// root or negative -> flag's exclusive scan in place, *n_out = the number of roots, out[i] = the number of root[i] or -1.
hipError_t gallery_launch_number(const int32_t* root, uint32_t* flag, int64_t G, int32_t* n_out, int32_t* out, hipStream_t stream);

}  // namespace vnf
