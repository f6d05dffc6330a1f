// Gallery clustering: DBSCAN over the gallery's own stored rows, by an all-pairs cosine self-join.
//
//   s(i,j)     the fp32 dot of stored rows i and j: the stream of gallery_core.h with row i among a wave's B fragments
//              (gallery_load_rows: the stored row as it is) and row j streaming past as an A fragment.  The products
//              commute and the k order is one, so s(i,j) and s(j,i) have the same bits.  NOT vnf_gallery_search's bits
//              for the pair: the search normalises its query once more.
//   N(i)       { j != i : s(i,j) >= t }, a NaN never; degree(i) = |N(i)|; core: degree(i) + 1 >= min_samples
//   clusters   connected components of the core rows, numbered by their smallest row
//   border     a non-core row with a core neighbour joins its best core neighbour's cluster (gallery_key order)
//
// Stage A (cluster_degree_kernel): a lane keeps one key (its best other row) and one count; the key goes to the workspace
// as a (chunk, G, 1) partial for the search's merge and the count to degree[] by one integer atomic add per (row, chunk)
// -- integer sums do not depend on their order.
// Stage B (cluster_link_kernel): the same pairs through the same adjacency test (cluster_adjacent), so an edge exists in
// B exactly where A counted it.  A core row i unites with each core neighbour j < i in parent[] by a lock-free
// union-find: find both roots, compare-and-swap the larger root's parent from itself to the smaller root, start over if
// another lane got there first.  parent[x] <= x always and only ever decreases, so a find terminates, and the root a
// component ends with is its smallest row whatever the order of arrival.  No lane waits for another: a failed
// compare-and-swap means somebody else made progress.  A non-core row keeps the best key among its core neighbours in a
// register (gallery_mated_kernel's pattern with core[j] for the label predicate).  Rows without a neighbour have nothing
// to do in this stage and waves of only such rows leave at once; a wave of only core rows stops at its own last row,
// since its edges to later rows belong to those rows' waves.
// Stage C: roots flattened (cluster_flatten_kernel), then gallery_launch_number, defined here and shared with the tracks:
// the roots numbered by one workgroup's exclusive scan (block_scan.h), every row written its root's number.
// parent[] is initialised by a launch of its own, then written by atomics and read by relaxed agent-scope loads only.
#include <string>

#include "block_scan.h"
#include "gallery_core.h"

namespace vnf {

// Row j (in: inside its chunk) is a neighbour of row i at score s.  NaN >= t is false.
static __device__ __forceinline__ bool cluster_adjacent(float s, float t, int64_t j, int64_t i, int64_t r_end) {
  return j < r_end && j != i && s >= t;
}

// The root of x's tree.  On the way a row whose parent is not a root is moved up to its grandparent (atomicMin: the
// entry only decreases, and only to an ancestor), which keeps later finds short.  parent[x] < x off the root: bounded.
static __device__ __forceinline__ int32_t cluster_find(int32_t* parent, int32_t x) {
  int32_t p = gallery_load_relaxed(parent + x);
  while (p != x) {
    const int32_t gp = gallery_load_relaxed(parent + p);
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
  GalleryLane<int64_t> L;
  const int64_t w = gallery_wave();
  if (w >= nwork) return;
  gallery_lane_chunked<KG, EXACT>(L, w, nqg, G, dim);

  f32x4_t qf[KG];   // the wave's 16 rows, as stored, as B fragments
  gallery_load_rows<KG, EXACT>(gal, L.qrow, L.qok, dim, L.g, L.kgs, qf);

  uint64_t best = 0;   // the lane's best other row so far; 0: none
  int32_t count = 0;   // its neighbours so far
  gallery_lane_rows(L, chunk_rows, G);
  for (int64_t r0 = L.r_begin; r0 < L.r_end; r0 += 32) {
    f32x4_t acc0, acc1;
    gallery_tile<KG, EXACT>(gal, r0, L.r_begin, L.r_end, dim, L.c, L.g, L.kgs, qf, acc0, acc1);
    // gallery_for_each's walk, written out (see there)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t i0 = r0 + 4 * L.g + r, i1 = i0 + 16;
      const uint64_t k0 = (i0 < L.r_end && i0 != L.qrow) ? gallery_key(acc0[r], (uint32_t)i0) : 0;
      const uint64_t k1 = (i1 < L.r_end && i1 != L.qrow) ? gallery_key(acc1[r], (uint32_t)i1) : 0;
      best = k0 > best ? k0 : best;
      best = k1 > best ? k1 : best;
      count += (int32_t)cluster_adjacent(acc0[r], t, i0, L.qrow, L.r_end) + (int32_t)cluster_adjacent(acc1[r], t, i1, L.qrow, L.r_end);
    }
  }

  best = gallery_max4(best);
  count += __shfl_xor(count, 16);
  count += __shfl_xor(count, 32);
  if (L.g == 0 && L.qok) {
    partial[(size_t)L.chunk * G + L.qrow] = best;
    if (count) atomicAdd(degree + L.qrow, count);
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
  GalleryLane<int64_t> L;
  const int64_t w = gallery_wave();
  if (w >= nwork) return;
  gallery_lane_chunked<KG, EXACT>(L, w, nqg, G, dim);
  const bool linked = L.qok && degree[L.qok ? L.qrow : 0] > 0;   // a row without a neighbour has no edge and no cluster to join
  const bool qcore = linked && core[L.qok ? L.qrow : 0] != 0;

  uint64_t best = 0;   // a non-core row's best core neighbour so far; 0: none
  gallery_lane_rows(L, chunk_rows, G);
  if (__any(linked)) {
    // core rows take their edges to earlier rows only: a wave without a non-core row stops behind its own last row
    if (!__any(linked && !qcore) && L.qrow - L.c + 16 < L.r_end) L.r_end = L.qrow - L.c + 16;
    f32x4_t qf[KG];
    gallery_load_rows<KG, EXACT>(gal, L.qrow, L.qok, dim, L.g, L.kgs, qf);
    const bool vec = (L.r_begin & 3) == 0;   // r0 + 4 g (+ 16) is then a multiple of 4 at every step
    for (int64_t r0 = L.r_begin; r0 < L.r_end; r0 += 32) {
      int32_t c0[4], c1[4];
      gallery_int4(core, r0 + 4 * L.g, L.r_begin, L.r_end, vec, c0);
      gallery_int4(core, r0 + 16 + 4 * L.g, L.r_begin, L.r_end, vec, c1);
      f32x4_t acc0, acc1;
      gallery_tile<KG, EXACT>(gal, r0, L.r_begin, L.r_end, dim, L.c, L.g, L.kgs, qf, acc0, acc1);
      // gallery_for_each's walk, written out (see there)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t i0 = r0 + 4 * L.g + r, i1 = i0 + 16;
        const bool e0 = linked && c0[r] != 0 && cluster_adjacent(acc0[r], t, i0, L.qrow, L.r_end);
        const bool e1 = linked && c1[r] != 0 && cluster_adjacent(acc1[r], t, i1, L.qrow, L.r_end);
        if (qcore) {
          if (e0 && i0 < L.qrow) cluster_unite(parent, (int32_t)L.qrow, (int32_t)i0);
          if (e1 && i1 < L.qrow) cluster_unite(parent, (int32_t)L.qrow, (int32_t)i1);
        } else {
          const uint64_t k0 = e0 ? gallery_key(acc0[r], (uint32_t)i0) : 0;
          const uint64_t k1 = e1 ? gallery_key(acc1[r], (uint32_t)i1) : 0;
          best = k0 > best ? k0 : best;
          best = k1 > best ? k1 : best;
        }
      }
    }
  }
  best = gallery_max4(best);
  if (L.g == 0 && L.qok) partial[(size_t)L.chunk * G + L.qrow] = best;
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

// flag -> its exclusive scan: at a root, the number of its cluster (or track).  One workgroup.
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

hipError_t gallery_launch_number(const int32_t* root, uint32_t* flag, int64_t G, int32_t* n_out, int32_t* out, hipStream_t stream) {
  hipLaunchKernelGGL(cluster_number_kernel, dim3(1), dim3(kScanLanes), 0, stream, flag, (uint32_t)G, n_out);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(cluster_write_kernel, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, stream, root, flag, G, out);
  return hipGetLastError();
}

// The workspace: (nchunks, G) keys, then seven (G) 32-bit arrays padded to a multiple of 4 entries.
struct ClusterWorkspace {
  int64_t padded, bytes;
  uint64_t* partial;
  int32_t *label_tmp, *border_idx, *parent, *core, *root;
  float* border_score;
  uint32_t* flag;
  ClusterWorkspace(const GalleryPlan& plan, int64_t G, void* base) {
    padded = (G + 3) / 4 * 4;
    GalleryCarver w{(char*)base};
    partial = w.take<uint64_t>(plan.nchunks * G * 8);
    label_tmp = w.take<int32_t>(padded * 4);
    border_idx = w.take<int32_t>(padded * 4);
    border_score = w.take<float>(padded * 4);
    parent = w.take<int32_t>(padded * 4);
    core = w.take<int32_t>(padded * 4);
    root = w.take<int32_t>(padded * 4);
    flag = w.take<uint32_t>(padded * 4);
    bytes = w.bytes;
  }
};

}  // namespace vnf
using namespace vnf;

extern "C" int64_t vnf_gallery_cluster_workspace_bytes(int64_t G, int64_t chunk_rows) {
  if (G < 0 || G > GAL_MAX_ROWS || chunk_rows < 0) return VNF_E_INVALID;
  const GalleryPlan plan(G, G, chunk_rows);
  if (G > 0 && plan.nchunks > ((int64_t)1 << 58) / G) return VNF_E_INVALID;   // the keys alone would not fit in 2^61 bytes
  const int64_t bytes = ClusterWorkspace(plan, G, nullptr).bytes;
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
    const GalleryPlan plan(G, G, chunk_rows);
    if (!plan.ok) return fail(VNF_E_INVALID, "vnf_gallery_cluster: chunk_rows too small for this gallery");
    const ClusterWorkspace ws(plan, G, workspace);
    const dim3 grid((unsigned)plan.blocks), rows_grid((unsigned)((ws.padded + 255) / 256));

    // A: degrees and nearest neighbours
    VNF_HIP(hipMemsetAsync(degree_out, 0, (size_t)G * 4, s));
    gallery_dispatch(t->dim, [&](auto exact) {
      hipLaunchKernelGGL((cluster_degree_kernel<GAL_MAX_KG, decltype(exact)::value>), grid, dim3(256), 0, s, t->mat, G, t->dim, threshold,
                         plan.chunk_rows, plan.nqg, plan.nwork, ws.partial, degree_out);
    });
    VNF_HIP(hipGetLastError());
    VNF_HIP(gallery_launch_merge(ws.partial, plan.nchunks, (int)G, 1, t->labels, nn_idx_out, ws.label_tmp, nn_score_out, s));
    hipLaunchKernelGGL(cluster_init_kernel, rows_grid, dim3(256), 0, s, degree_out, G, min_samples, ws.parent, ws.core);
    VNF_HIP(hipGetLastError());

    // B: links between core rows, best core neighbour of the others
    gallery_dispatch(t->dim, [&](auto exact) {
      hipLaunchKernelGGL((cluster_link_kernel<GAL_MAX_KG, decltype(exact)::value>), grid, dim3(256), 0, s, t->mat, G, t->dim, threshold,
                         plan.chunk_rows, plan.nqg, plan.nwork, degree_out, ws.core, ws.parent, ws.partial);
    });
    VNF_HIP(hipGetLastError());
    VNF_HIP(gallery_launch_merge(ws.partial, plan.nchunks, (int)G, 1, t->labels, ws.border_idx, ws.label_tmp, ws.border_score, s));

    // C: flatten, number, write
    hipLaunchKernelGGL(cluster_flatten_kernel, rows_grid, dim3(256), 0, s, ws.parent, ws.core, ws.border_idx, G, ws.padded, ws.root, ws.flag);
    VNF_HIP(hipGetLastError());
    VNF_HIP(gallery_launch_number(ws.root, ws.flag, G, n_clusters_out, cluster_out, s));
    return VNF_OK;
  } catch (const std::exception& ex) {
    return fail(VNF_E_INVALID, std::string("exception: ") + ex.what());
  }
}
