// Gallery clustering: DBSCAN over the gallery's own stored rows, by an all-pairs cosine self-join.
//
//   s(i,j)     the fp32 dot of stored rows i and j: gallery_tile of gallery_core.h with row i among a wave's B fragments
//              (gallery_load_rows: the stored row as it is) and row j streaming past as an A fragment.  The products
//              commute and the k order is one, so s(i,j) and s(j,i) have the same bits.  NOT vnf_gallery_search's bits
//              for the pair: the search normalises its query once more.
//   N(i)       { j != i : s(i,j) >= t }, a NaN never; degree(i) = |N(i)|; core: degree(i) + 1 >= min_samples
//   clusters   connected components of the core rows, numbered by their smallest row
//   border     a non-core row with a core neighbour joins its best core neighbour's cluster (gallery_key order)
//
// Stage A (cluster_degree_kernel): the search's stream -- a wave owns 16 rows and a chunk, the chunk passes 32 rows a
// step, the four waves of a workgroup share a chunk.  A lane keeps one key (its best other row) and one count; the four
// lanes of a row combine by shuffle, the key goes to the workspace as a (chunk, G, 1) partial for the search's merge and
// the count to degree[] by one integer atomic add per (row, chunk) -- integer sums do not depend on their order.
// Stage B (cluster_link_kernel): the same pairs through the same adjacency test (cluster_adjacent on gallery_tile's
// output), so an edge exists in B exactly where A counted it.  A core row i unites with each core neighbour j < i in
// parent[] by a lock-free union-find: find both roots, compare-and-swap the larger root's parent from itself to the
// smaller root, start over if another lane got there first.  parent[x] <= x always and only ever decreases, so a find
// terminates, and the root a component ends with is its smallest row whatever the order of arrival.  No lane waits for
// another: a failed compare-and-swap means somebody else made progress.  A non-core row keeps the best key among its
// core neighbours in a register (gallery_mated_kernel's pattern with core[j] for the label predicate).  Rows without a
// neighbour have nothing to do in this stage and waves of only such rows leave at once; a wave of only core rows stops
// at its own last row, since its edges to later rows belong to those rows' waves.
// Stage C: roots flattened, numbered by one workgroup's exclusive scan (block_scan.h), clusters written.
// parent[] is initialised by a launch of its own, then written by atomics and read by relaxed agent-scope loads only.
#include <string>

#include "block_scan.h"
#include "gallery_core.h"

namespace vnf {

// Row j (of a chunk ending at r_end) is a neighbour of row i at score s.  NaN >= t is false.
static __device__ __forceinline__ bool cluster_adjacent(float s, float t, int64_t j, int64_t i, int64_t r_end) {
  return j < r_end && j != i && s >= t;
}

// core flags of rows i0 .. i0 + 3; a row at or past r_end reads the chunk's first row instead (it is never adjacent).
// vec: i0 is a multiple of 4 (wave-uniform), so that 16 bytes can be read at once.
static __device__ __forceinline__ void cluster_core4(const int32_t* __restrict__ core, int64_t i0, int64_t r_begin, int64_t r_end, bool vec,
                                                     int32_t (&out)[4]) {
  if (vec && i0 + 3 < r_end) {
    const int4 v = *reinterpret_cast<const int4*>(core + i0);
    out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = v.w;
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r) out[r] = core[i0 + r < r_end ? i0 + r : r_begin];
  }
}

static __device__ __forceinline__ int32_t parent_load(const int32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root of x's tree.  On the way a row whose parent is not a root is moved up to its grandparent (atomicMin: the
// entry only decreases, and only to an ancestor), which keeps later finds short.  parent[x] < x off the root: bounded.
static __device__ __forceinline__ int32_t cluster_find(int32_t* parent, int32_t x) {
  int32_t p = parent_load(parent + x);
  while (p != x) {
    const int32_t gp = parent_load(parent + p);
    if (gp != p) atomicMin(parent + x, gp);
    x = p;
    p = gp;
  }
  return x;
}

static __device__ __forceinline__ void cluster_unite(int32_t* parent, int32_t a, int32_t b) {
  for (;;) {
    a = cluster_find(parent, a);
    b = cluster_find(parent, b);
    if (a == b) return;
    const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
    if (atomicCAS(parent + hi, hi, lo) == hi) return;   // hi was still a root: hooked.  Otherwise somebody hooked it: again
  }
}

template <int KG, bool EXACT>
__global__ void __launch_bounds__(256) cluster_degree_kernel(const float* __restrict__ gal, int64_t G, int dim, float t, int64_t chunk_rows,
                                                             int nqg, int64_t nwork, uint64_t* __restrict__ partial,
                                                             int32_t* __restrict__ degree) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t w = (int64_t)blockIdx.x * 4 + wave;
  if (w >= nwork) return;
  const int64_t chunk = w / nqg;
  const int qg = (int)(w % nqg);
  const int c = lane & 15, g = lane >> 4;
  const int kgs = EXACT ? KG : (dim >> 4);
  const int64_t qrow = (int64_t)qg * 16 + c;
  const bool qok = qrow < G;

  f32x4_t qf[KG];   // the wave's 16 rows, as stored, as B fragments
  gallery_load_rows<KG, EXACT>(gal, qrow, qok, dim, g, kgs, qf);

  uint64_t best = 0;   // the lane's best other row so far; 0: none
  int32_t count = 0;   // its neighbours so far
  const int64_t r_begin = chunk * chunk_rows;
  const int64_t r_end = (r_begin + chunk_rows < G) ? r_begin + chunk_rows : G;
  for (int64_t r0 = r_begin; r0 < r_end; r0 += 32) {
    f32x4_t acc0, acc1;
    gallery_tile<KG, EXACT>(gal, r0, r_begin, r_end, dim, c, g, kgs, qf, acc0, acc1);
    // D[row = 4 g + r][col = c]: this lane's row against rows r0 + 4 g + r and r0 + 16 + 4 g + r
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t i0 = r0 + 4 * g + r, i1 = i0 + 16;
      const uint64_t k0 = (i0 < r_end && i0 != qrow) ? gallery_key(acc0[r], (uint32_t)i0) : 0;
      const uint64_t k1 = (i1 < r_end && i1 != qrow) ? gallery_key(acc1[r], (uint32_t)i1) : 0;
      best = k0 > best ? k0 : best;
      best = k1 > best ? k1 : best;
      count += (int32_t)cluster_adjacent(acc0[r], t, i0, qrow, r_end) + (int32_t)cluster_adjacent(acc1[r], t, i1, qrow, r_end);
    }
  }

  // the four lanes of a row hold disjoint rows of the chunk
  uint64_t o = shfl_xor_u64(best, 16);
  best = o > best ? o : best;
  o = shfl_xor_u64(best, 32);
  best = o > best ? o : best;
  count += __shfl_xor(count, 16);
  count += __shfl_xor(count, 32);
  if (g == 0 && qok) {
    partial[(size_t)chunk * G + qrow] = best;
    if (count) atomicAdd(degree + qrow, count);
  }
}

__global__ void __launch_bounds__(256) cluster_init_kernel(const int32_t* __restrict__ degree, int64_t G, int min_samples,
                                                           int32_t* __restrict__ parent, int32_t* __restrict__ core) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= G) return;
  parent[i] = (int32_t)i;
  core[i] = (int64_t)degree[i] + 1 >= min_samples;
}

template <int KG, bool EXACT>
__global__ void __launch_bounds__(256) cluster_link_kernel(const float* __restrict__ gal, int64_t G, int dim, float t, int64_t chunk_rows,
                                                           int nqg, int64_t nwork, const int32_t* __restrict__ degree,
                                                           const int32_t* __restrict__ core, int32_t* parent,
                                                           uint64_t* __restrict__ partial) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t w = (int64_t)blockIdx.x * 4 + wave;
  if (w >= nwork) return;
  const int64_t chunk = w / nqg;
  const int qg = (int)(w % nqg);
  const int c = lane & 15, g = lane >> 4;
  const int kgs = EXACT ? KG : (dim >> 4);
  const int64_t qrow = (int64_t)qg * 16 + c;
  const bool qok = qrow < G;
  const bool linked = qok && degree[qok ? qrow : 0] > 0;   // a row without a neighbour has no edge and no cluster to join
  const bool qcore = linked && core[qok ? qrow : 0] != 0;

  uint64_t best = 0;   // a non-core row's best core neighbour so far; 0: none
  const int64_t r_begin = chunk * chunk_rows;
  int64_t r_end = (r_begin + chunk_rows < G) ? r_begin + chunk_rows : G;
  if (__any(linked)) {
    // core rows take their edges to earlier rows only: a wave without a non-core row stops behind its own last row
    if (!__any(linked && !qcore) && (int64_t)qg * 16 + 16 < r_end) r_end = (int64_t)qg * 16 + 16;
    f32x4_t qf[KG];
    gallery_load_rows<KG, EXACT>(gal, qrow, qok, dim, g, kgs, qf);
    const bool vec = (r_begin & 3) == 0;   // r0 + 4 g (+ 16) is then a multiple of 4 at every step
    for (int64_t r0 = r_begin; r0 < r_end; r0 += 32) {
      int32_t c0[4], c1[4];
      cluster_core4(core, r0 + 4 * g, r_begin, r_end, vec, c0);
      cluster_core4(core, r0 + 16 + 4 * g, r_begin, r_end, vec, c1);
      f32x4_t acc0, acc1;
      gallery_tile<KG, EXACT>(gal, r0, r_begin, r_end, dim, c, g, kgs, qf, acc0, acc1);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t i0 = r0 + 4 * g + r, i1 = i0 + 16;
        const bool e0 = linked && c0[r] != 0 && cluster_adjacent(acc0[r], t, i0, qrow, r_end);
        const bool e1 = linked && c1[r] != 0 && cluster_adjacent(acc1[r], t, i1, qrow, r_end);
        if (qcore) {
          if (e0 && i0 < qrow) cluster_unite(parent, (int32_t)qrow, (int32_t)i0);
          if (e1 && i1 < qrow) cluster_unite(parent, (int32_t)qrow, (int32_t)i1);
        } else {
          const uint64_t k0 = e0 ? gallery_key(acc0[r], (uint32_t)i0) : 0;
          const uint64_t k1 = e1 ? gallery_key(acc1[r], (uint32_t)i1) : 0;
          best = k0 > best ? k0 : best;
          best = k1 > best ? k1 : best;
        }
      }
    }
  }
  uint64_t o = shfl_xor_u64(best, 16);
  best = o > best ? o : best;
  o = shfl_xor_u64(best, 32);
  best = o > best ? o : best;
  if (g == 0 && qok) partial[(size_t)chunk * G + qrow] = best;
}

// root[i]: the root of a core row's tree, of a border row's best core neighbour's tree, -1 for noise; flag[i] = 1 where
// row i is a root (a core row that is its own parent), 0 elsewhere, up to the next multiple of 4 entries.
__global__ void __launch_bounds__(256) cluster_flatten_kernel(int32_t* parent, const int32_t* __restrict__ core,
                                                              const int32_t* __restrict__ border_idx, int64_t G, int64_t padded,
                                                              int32_t* __restrict__ root, uint32_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= padded) return;
  if (i >= G) {
    flag[i] = 0;
    return;
  }
  const int32_t from = core[i] ? (int32_t)i : border_idx[i];   // border_idx: -1 without a core neighbour
  const int32_t r = from >= 0 ? cluster_find(parent, from) : -1;
  root[i] = r;
  flag[i] = r == (int32_t)i;
}

// flag -> its exclusive scan: at a root, the cluster's number.  One workgroup.
__global__ void __launch_bounds__(kScanLanes) cluster_number_kernel(uint32_t* flag, uint32_t G, int32_t* __restrict__ n_clusters) {
  const uint32_t n = block_scan(flag, G);
  if (threadIdx.x == 0) *n_clusters = (int32_t)n;
}

__global__ void __launch_bounds__(256) cluster_write_kernel(const int32_t* __restrict__ root, const uint32_t* __restrict__ number, int64_t G,
                                                            int32_t* __restrict__ cluster_out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= G) return;
  const int32_t r = root[i];
  cluster_out[i] = r >= 0 ? (int32_t)number[r] : -1;
}

static int64_t align16(int64_t bytes) { return (bytes + 15) / 16 * 16; }

// The workspace: (nchunks, G) keys, then six (G) 32-bit arrays, each section a multiple of 16 bytes.
struct ClusterWorkspace {
  int64_t chunk_rows, nchunks, padded, bytes;
  uint64_t* partial;
  int32_t *label_tmp, *border_idx, *parent, *core, *root;
  float* border_score;
  uint32_t* flag;
  ClusterWorkspace(int64_t G, int64_t cr_arg, void* base) {
    chunk_rows = gallery_chunk_rows((int)(G < 0x3FFFFFFF ? G : 0x3FFFFFFF), G, cr_arg);
    nchunks = (G + chunk_rows - 1) / chunk_rows;
    padded = (G + 3) / 4 * 4;
    char* p = (char*)base;
    const int64_t keys = align16(nchunks * G * 8), ints = align16(padded * 4);
    partial = (uint64_t*)p;
    label_tmp = (int32_t*)(p + keys);
    border_idx = (int32_t*)(p + keys + ints);
    border_score = (float*)(p + keys + 2 * ints);
    parent = (int32_t*)(p + keys + 3 * ints);
    core = (int32_t*)(p + keys + 4 * ints);
    root = (int32_t*)(p + keys + 5 * ints);
    flag = (uint32_t*)(p + keys + 6 * ints);
    bytes = keys + 7 * ints;
  }
};

}  // namespace vnf
using namespace vnf;

extern "C" int64_t vnf_gallery_cluster_workspace_bytes(int64_t G, int64_t chunk_rows) {
  if (G < 0 || G > GAL_MAX_ROWS || chunk_rows < 0) return VNF_E_INVALID;
  const int64_t cr = gallery_chunk_rows((int)(G < 0x3FFFFFFF ? G : 0x3FFFFFFF), G, chunk_rows);
  if (G > 0 && (G + cr - 1) / cr > ((int64_t)1 << 58) / G) return VNF_E_INVALID;   // the keys alone would not fit in 2^61 bytes
  const int64_t bytes = ClusterWorkspace(G, chunk_rows, nullptr).bytes;
  return bytes > 0 ? bytes : 16;
}

extern "C" int vnf_gallery_cluster(vnf_handle h, float threshold, int min_samples, int32_t* cluster_out, int32_t* degree_out,
                                   int32_t* nn_idx_out, float* nn_score_out, int32_t* n_clusters_out, int64_t chunk_rows, void* workspace,
                                   int64_t workspace_bytes, void* stream) {
  try {
    Gallery* t = handle_cast<Gallery>(h);
    if (!t) return fail(VNF_E_INVALID, "not a gallery handle");
    if (threshold != threshold || min_samples < 1 || chunk_rows < 0 || !n_clusters_out)
      return fail(VNF_E_INVALID, "vnf_gallery_cluster: bad argument (a NaN threshold, min_samples < 1, no n_clusters_out)");
    hipStream_t s = (hipStream_t)stream;
    const int64_t G = t->rows;
    if (G == 0) {
      VNF_HIP(hipMemsetAsync(n_clusters_out, 0, 4, s));
      return VNF_OK;
    }
    if (!cluster_out || !degree_out || !nn_idx_out || !nn_score_out || !workspace || ((uintptr_t)workspace & 15))
      return fail(VNF_E_INVALID, "vnf_gallery_cluster: null or misaligned pointer");
    const int64_t need = vnf_gallery_cluster_workspace_bytes(G, chunk_rows);
    if (need < 0) return fail(VNF_E_INVALID, "vnf_gallery_cluster: chunk_rows too small for this gallery");
    if (workspace_bytes < need)
      return fail(VNF_E_CAPACITY, "vnf_gallery_cluster: workspace smaller than vnf_gallery_cluster_workspace_bytes");
    const ClusterWorkspace ws(G, chunk_rows, workspace);
    const int64_t nqg64 = (G + 15) / 16;
    const int64_t nwork = ws.nchunks * nqg64, blocks = (nwork + 3) / 4;
    if (blocks > 0x7FFFFFFF) return fail(VNF_E_INVALID, "vnf_gallery_cluster: chunk_rows too small for this gallery");
    const int nqg = (int)nqg64;
    const dim3 grid((unsigned)blocks), rows_grid((unsigned)((ws.padded + 255) / 256));
    const bool exact = t->dim == 16 * GAL_MAX_KG;

    // A: degrees and nearest neighbours
    VNF_HIP(hipMemsetAsync(degree_out, 0, (size_t)G * 4, s));
    if (exact)
      hipLaunchKernelGGL((cluster_degree_kernel<GAL_MAX_KG, true>), grid, dim3(256), 0, s, t->mat, G, t->dim, threshold, ws.chunk_rows, nqg, nwork,
                         ws.partial, degree_out);
    else
      hipLaunchKernelGGL((cluster_degree_kernel<GAL_MAX_KG, false>), grid, dim3(256), 0, s, t->mat, G, t->dim, threshold, ws.chunk_rows, nqg, nwork,
                         ws.partial, degree_out);
    VNF_HIP(hipGetLastError());
    VNF_HIP(gallery_launch_merge(ws.partial, ws.nchunks, (int)G, 1, t->labels, nn_idx_out, ws.label_tmp, nn_score_out, s));
    hipLaunchKernelGGL(cluster_init_kernel, rows_grid, dim3(256), 0, s, degree_out, G, min_samples, ws.parent, ws.core);
    VNF_HIP(hipGetLastError());

    // B: links between core rows, best core neighbour of the others
    if (exact)
      hipLaunchKernelGGL((cluster_link_kernel<GAL_MAX_KG, true>), grid, dim3(256), 0, s, t->mat, G, t->dim, threshold, ws.chunk_rows, nqg, nwork,
                         degree_out, ws.core, ws.parent, ws.partial);
    else
      hipLaunchKernelGGL((cluster_link_kernel<GAL_MAX_KG, false>), grid, dim3(256), 0, s, t->mat, G, t->dim, threshold, ws.chunk_rows, nqg, nwork,
                         degree_out, ws.core, ws.parent, ws.partial);
    VNF_HIP(hipGetLastError());
    VNF_HIP(gallery_launch_merge(ws.partial, ws.nchunks, (int)G, 1, t->labels, ws.border_idx, ws.label_tmp, ws.border_score, s));

    // C: flatten, number, write
    hipLaunchKernelGGL(cluster_flatten_kernel, rows_grid, dim3(256), 0, s, ws.parent, ws.core, ws.border_idx, G, ws.padded, ws.root, ws.flag);
    VNF_HIP(hipGetLastError());
    hipLaunchKernelGGL(cluster_number_kernel, dim3(1), dim3(kScanLanes), 0, s, ws.flag, (uint32_t)G, n_clusters_out);
    VNF_HIP(hipGetLastError());
    hipLaunchKernelGGL(cluster_write_kernel, rows_grid, dim3(256), 0, s, ws.root, ws.flag, G, cluster_out);
    VNF_HIP(hipGetLastError());
    return VNF_OK;
  } catch (const std::exception& ex) {
    return fail(VNF_E_INVALID, std::string("exception: ") + ex.what());
  }
}
