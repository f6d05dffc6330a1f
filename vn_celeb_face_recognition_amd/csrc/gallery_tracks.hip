// Face tracks: the faces of a video, stored as a gallery in frame order, linked across frames.
//
//   s(i,j)      the fp32 dot of stored rows i and j: gallery_cluster.hip's score, the same bits from either side (the same
//               gallery_load_rows and gallery_tile of gallery_core.h produce it)
//   candidate   j is a forward candidate of i where 0 < f(j) - f(i) <= max_gap, j > i (which the order of the rows implies),
//               s(i,j) >= t (a NaN never) and, with min_iou > 0, the boxes overlap by inter >= min_iou * union.  Every term
//               is symmetric or antisymmetric in (i, j), so i is a backward candidate of j exactly then
//   next / pred the best forward / backward candidate under (frame distance ascending, gallery_key descending)
//   link        i -> j where next(i) == j and pred(j) == i: chains through strictly increasing rows
//   track       a chain, numbered by its first row
//
// Stage A (tracks_best_kernel): a wave owns 16 rows.  The rows are sorted by frame, so everything within max_gap frames
// of them is ONE contiguous row range, read from frame_first: the core's stream over a window in place of a chunk.  A lane
// keeps its best forward and its best backward candidate (frame distance and key) in registers; the four lanes of a
// row combine by shuffle and write the two candidates to the workspace.  The work follows the window, not G^2.
// Stage B (tracks_mutual_kernel): a row keeps a candidate that names it back.
// Stage C: clustering's (gallery_launch_number) with another way to the roots: parent[i] = prev[i] (< i) or i,
// ceil(log2(n_frames)) rounds of pointer jumping bring every row to its head, tracks_flatten_kernel flags the heads.
// vnf_gallery_track_sums: the heads enter counts[] by track, then a wave per track walks next[] and adds the stored rows
// in row order.
//
// No float atomics, nothing allocated, no synchronisation.  frame_first, the labels and the link tables live in device
// memory and are not trusted for addressing: every row index taken from them is clamped or tested against [0, G) before
// it is used; the pointer jumping runs a number of rounds fixed by n_frames, the walk of the sums moves to a strictly
// larger row or stops.
#include <string>

#include "gallery_core.h"

namespace vnf {

// A lane's best candidate in one direction is two registers: near = 256 - frame distance (0: none yet), then the
// score-and-row key.  (near, key) replaces (b_near, b_key) where it is a candidate (near != 0) and the better of the two.
static __device__ __forceinline__ void track_take(uint32_t& b_near, uint64_t& b_key, uint32_t near, uint64_t key) {
  const bool better = near != 0 && (near > b_near || (near == b_near && key > b_key));
  b_near = better ? near : b_near;
  b_key = better ? key : b_key;
}

static __device__ __forceinline__ void track_combine(uint32_t& b_near, uint64_t& b_key, int mask) {
  const uint32_t near = __shfl_xor(b_near, mask);
  const uint64_t key = shfl_xor_u64(b_key, mask);
  track_take(b_near, b_key, near, key);
}

// inter >= min_iou * union of two x1,y1,x2,y2 boxes, every operation in fp32 as written (the build does not contract).
// The same bits whichever box comes first.  A NaN anywhere: false, or an intersection of 0.
static __device__ __forceinline__ bool track_overlap(const f32x4_t a, const f32x4_t b, float min_iou) {
  const float iw = fmaxf(0.f, fminf(a[2], b[2]) - fmaxf(a[0], b[0]));
  const float ih = fmaxf(0.f, fminf(a[3], b[3]) - fmaxf(a[1], b[1]));
  const float inter = iw * ih;
  const float area_a = (a[2] - a[0]) * (a[3] - a[1]), area_b = (b[2] - b[0]) * (b[3] - b[1]);
  const float uni = area_a + area_b - inter;
  return inter >= min_iou * uni;
}

// Row j (in: inside the window; score s against the lane's row) offered to the lane's row qrow (frame fq).
static __device__ __forceinline__ void track_offer(uint32_t& f_near, uint64_t& f_key, uint32_t& b_near, uint64_t& b_key, float s, int64_t j,
                                                   bool in, int64_t qrow, bool qok,
                                                   int32_t fq, const int32_t* __restrict__ labels, float t, int max_gap, float min_iou,
                                                   const f32x4_t qbox, const f32x4_t* __restrict__ boxes) {
  if (!qok || !in || !(s >= t)) return;
  const int64_t d = (int64_t)labels[j] - (int64_t)fq;
  const bool f = d > 0 && d <= max_gap && j > qrow, b = d < 0 && -d <= max_gap && j < qrow;
  if (!f && !b) return;
  if (min_iou > 0.f && !track_overlap(qbox, boxes[j], min_iou)) return;
  const uint64_t key = gallery_key(s, (uint32_t)j);
  // both directions are offered, one of them nothing: a branch on f would make the compiler index the two bests in scratch
  track_take(f_near, f_key, f ? (uint32_t)(256 - d) : 0u, key);
  track_take(b_near, b_key, b ? (uint32_t)(256 + d) : 0u, key);
}

static __device__ __forceinline__ int64_t track_clamp(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <int KG, bool EXACT>
__global__ void __launch_bounds__(256) tracks_best_kernel(const float* __restrict__ gal, const int32_t* __restrict__ labels, int64_t G, int dim,
                                                          const int32_t* __restrict__ frame_first, int n_frames,
                                                          const f32x4_t* __restrict__ boxes, float t, float min_iou, int max_gap, int64_t nqg,
                                                          int32_t* __restrict__ next_cand, int32_t* __restrict__ pred_cand,
                                                          float* __restrict__ pred_score) {
  const int64_t qg = gallery_wave();
  if (qg >= nqg) return;
  GalleryLane<int64_t> L;
  gallery_lane<KG, EXACT>(L, qg, G, dim);
  const int64_t q0 = qg * 16, qrow = L.qrow;
  const bool qok = L.qok;

  // the window: the rows of the frames within max_gap of the wave's first and last row, as frame_first has them
  int64_t w_begin = 0, w_end = 0;
  if (n_frames > 0) {
    const int64_t q_last = q0 + 15 < G ? q0 + 15 : G - 1;
    const int64_t f_lo = track_clamp(labels[q0], 0, n_frames - 1), f_hi = track_clamp(labels[q_last], 0, n_frames - 1);
    w_begin = track_clamp(frame_first[track_clamp(f_lo - max_gap, 0, n_frames)], 0, G);
    w_end = track_clamp(frame_first[track_clamp(f_hi + max_gap + 1, 0, n_frames)], 0, G);
  }

  uint32_t f_near = 0, b_near = 0;   // the lane's best forward and backward candidate so far; near 0: none
  uint64_t f_key = 0, b_key = 0;
  if (w_begin < w_end) {
    f32x4_t qf[KG];   // the wave's 16 rows, as stored, as B fragments
    gallery_load_rows<KG, EXACT>(gal, qrow, qok, dim, L.g, L.kgs, qf);
    const int32_t fq = labels[qok ? qrow : 0];
    f32x4_t qbox = {0.f, 0.f, 0.f, 0.f};
    if (min_iou > 0.f && qok) qbox = boxes[qrow];
    for (int64_t r0 = w_begin; r0 < w_end; r0 += 32) {
      f32x4_t acc0, acc1;
      gallery_tile<KG, EXACT>(gal, r0, w_begin, w_end, dim, L.c, L.g, L.kgs, qf, acc0, acc1);
      gallery_for_each(r0, L.g, w_end, acc0, acc1, [&](int, int64_t i, float s, bool in) {
        track_offer(f_near, f_key, b_near, b_key, s, i, in, qrow, qok, fq, labels, t, max_gap, min_iou, qbox, boxes);
      });
    }
  }

  // the four lanes of a row hold disjoint rows of the window
  track_combine(f_near, f_key, 16);
  track_combine(f_near, f_key, 32);
  track_combine(b_near, b_key, 16);
  track_combine(b_near, b_key, 32);
  if (L.g == 0 && qok) {
    next_cand[qrow] = f_near ? (int32_t)gallery_key_row(f_key) : -1;
    pred_cand[qrow] = b_near ? (int32_t)gallery_key_row(b_key) : -1;
    pred_score[qrow] = b_near ? gallery_key_score(b_key) : __uint_as_float(0xFF800000u);
  }
}

// The candidates are rows of [0, G) on the right side of i by construction (track_offer): parent[i] <= i.
__global__ void __launch_bounds__(256) tracks_mutual_kernel(const int32_t* __restrict__ next_cand, const int32_t* __restrict__ pred_cand,
                                                            const float* __restrict__ pred_score, int64_t G, int32_t* __restrict__ prev_out,
                                                            int32_t* __restrict__ next_out, float* __restrict__ link_score_out,
                                                            int32_t* __restrict__ parent) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= G) return;
  const int32_t n = next_cand[i], p = pred_cand[i];
  const bool has_next = n >= 0 && pred_cand[n] == (int32_t)i, has_prev = p >= 0 && next_cand[p] == (int32_t)i;
  next_out[i] = has_next ? n : -1;
  prev_out[i] = has_prev ? p : -1;
  link_score_out[i] = has_prev ? pred_score[i] : __uint_as_float(0xFF800000u);
  parent[i] = has_prev ? p : (int32_t)i;
}

// One round of pointer jumping, in place: every row moves up to its grandparent.  Whatever mix of old and new entries
// a lane reads, an entry only ever moves to an ancestor and at least as far as a round on a snapshot would take it, so
// ceil(log2(n)) rounds bring every row of a chain of n rows to its head -- a chain of a track has n_frames rows at most.
// A chain of a hundred thousand frames is seventeen launches, where a walk per row would be its length.
__global__ void __launch_bounds__(256) tracks_jump_kernel(int32_t* parent, int64_t G) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= G) return;
  const int32_t p = gallery_load_relaxed(parent + i);
  const int32_t gp = gallery_load_relaxed(parent + p);
  if (gp != p) __hip_atomic_store(parent + i, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// flag[i] = 1 where row i is a head (its own parent), 0 elsewhere, up to the next multiple of 4 entries.
__global__ void __launch_bounds__(256) tracks_flatten_kernel(const int32_t* __restrict__ parent, int64_t G, int64_t padded,
                                                             uint32_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= padded) return;
  flag[i] = i < G && parent[i] == (int32_t)i;
}

// counts[track of a head] = the head's row.  counts was filled with -1.
__global__ void __launch_bounds__(256) tracks_heads_kernel(const int32_t* __restrict__ prev, const int32_t* __restrict__ track, int64_t G,
                                                           int n_tracks, int32_t* __restrict__ counts) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= G || prev[i] >= 0) return;
  const int32_t k = track[i];
  if (k >= 0 && k < n_tracks) counts[k] = (int32_t)i;
}

// A wave per track: from the head counts[] names, along next[] while it leads to a later row of [0, G), s = s + x from 0
// per element.  Lane l holds elements 4 l .. 4 l + 3 and 256 + 4 l .. 256 + 4 l + 3.  A track without a head: zeros, 0.
__global__ void __launch_bounds__(64) tracks_sums_kernel(const float* __restrict__ gal, const int32_t* __restrict__ next, int64_t G, int dim,
                                                         float* __restrict__ sums, int32_t* __restrict__ counts) {
  const int lane = threadIdx.x, k = blockIdx.x;
  f32x4_t s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
  const int e0 = 4 * lane, e1 = 256 + 4 * lane;
  int64_t cur = counts[k];
  int32_t cnt = 0;
  while (cur >= 0 && cur < G) {
    const int64_t nx = next[cur];   // ahead of the row: the walk waits for this load alone
    const float* xr = gal + (size_t)cur * dim;
    if (e0 < dim) {
      const f32x4_t v = *reinterpret_cast<const f32x4_t*>(xr + e0);
#pragma unroll
      for (int j = 0; j < 4; ++j) s0[j] = s0[j] + v[j];
    }
    if (e1 < dim) {
      const f32x4_t v = *reinterpret_cast<const f32x4_t*>(xr + e1);
#pragma unroll
      for (int j = 0; j < 4; ++j) s1[j] = s1[j] + v[j];
    }
    ++cnt;
    cur = nx > cur ? nx : -1;
  }
  float* srow = sums + (size_t)k * dim;
  if (e0 < dim) *reinterpret_cast<f32x4_t*>(srow + e0) = s0;
  if (e1 < dim) *reinterpret_cast<f32x4_t*>(srow + e1) = s1;
  if (lane == 0) counts[k] = cnt;
}

// The workspace: five (G) 32-bit arrays, each padded to a multiple of 4 entries.
struct TracksWorkspace {
  int64_t padded, bytes;
  int32_t *next_cand, *pred_cand, *parent;
  float* pred_score;
  uint32_t* flag;
  TracksWorkspace(int64_t G, void* base) {
    padded = (G + 3) / 4 * 4;
    GalleryCarver w{(char*)base};
    next_cand = w.take<int32_t>(padded * 4);
    pred_cand = w.take<int32_t>(padded * 4);
    pred_score = w.take<float>(padded * 4);
    parent = w.take<int32_t>(padded * 4);
    flag = w.take<uint32_t>(padded * 4);
    bytes = w.bytes;
  }
};

}  // namespace vnf
using namespace vnf;

extern "C" int64_t vnf_gallery_tracks_workspace_bytes(int64_t G) {
  if (G < 0 || G > GAL_MAX_ROWS) return VNF_E_INVALID;
  const int64_t bytes = TracksWorkspace(G, nullptr).bytes;
  return bytes > 0 ? bytes : 16;
}

extern "C" int vnf_gallery_tracks(vnf_handle h, const int32_t* frame_first_dev, int n_frames, const float* boxes_dev, float threshold,
                                  float min_iou, int max_gap, int32_t* prev_out, int32_t* next_out, float* link_score_out,
                                  int32_t* track_out, int32_t* n_tracks_out, void* workspace, int64_t workspace_bytes, void* stream) {
  try {
    Gallery* t = handle_cast<Gallery>(h);
    if (!t) return fail(VNF_E_INVALID, "not a gallery handle");
    if (threshold != threshold || min_iou != min_iou || max_gap < 1 || max_gap > 255 || n_frames < 0 || !n_tracks_out)
      return fail(VNF_E_INVALID, "vnf_gallery_tracks: bad argument (a NaN threshold or min_iou, max_gap outside 1..255, n_frames < 0, "
                                 "no n_tracks_out)");
    hipStream_t s = (hipStream_t)stream;
    const int64_t G = t->rows;
    if (G == 0) {
      VNF_HIP(hipMemsetAsync(n_tracks_out, 0, 4, s));
      return VNF_OK;
    }
    if (!frame_first_dev || !prev_out || !next_out || !link_score_out || !track_out || !workspace || ((uintptr_t)workspace & 15) ||
        (min_iou > 0.f && (!boxes_dev || ((uintptr_t)boxes_dev & 15))))
      return fail(VNF_E_INVALID, "vnf_gallery_tracks: null or misaligned pointer");
    if (workspace_bytes < vnf_gallery_tracks_workspace_bytes(G))
      return fail(VNF_E_CAPACITY, "vnf_gallery_tracks: workspace smaller than vnf_gallery_tracks_workspace_bytes");
    const TracksWorkspace ws(G, workspace);
    const int64_t nqg = (G + 15) / 16;
    const dim3 grid((unsigned)((nqg + 3) / 4)), rows_grid((unsigned)((ws.padded + 255) / 256));
    const f32x4_t* boxes = reinterpret_cast<const f32x4_t*>(boxes_dev);

    // A: every row's best forward and backward candidate
    gallery_dispatch(t->dim, [&](auto exact) {
      hipLaunchKernelGGL((tracks_best_kernel<GAL_MAX_KG, decltype(exact)::value>), grid, dim3(256), 0, s, t->mat, t->labels, G, t->dim,
                         frame_first_dev, n_frames, boxes, threshold, min_iou, max_gap, nqg, ws.next_cand, ws.pred_cand, ws.pred_score);
    });
    VNF_HIP(hipGetLastError());
    // B: mutual bests
    hipLaunchKernelGGL(tracks_mutual_kernel, rows_grid, dim3(256), 0, s, ws.next_cand, ws.pred_cand, ws.pred_score, G, prev_out, next_out,
                       link_score_out, ws.parent);
    VNF_HIP(hipGetLastError());
    // C: jump, number, write.  A chain passes through strictly increasing frames: n_frames rows at most
    for (int64_t reach = 1; reach < n_frames; reach *= 2) {
      hipLaunchKernelGGL(tracks_jump_kernel, rows_grid, dim3(256), 0, s, ws.parent, G);
      VNF_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(tracks_flatten_kernel, rows_grid, dim3(256), 0, s, ws.parent, G, ws.padded, ws.flag);
    VNF_HIP(hipGetLastError());
    VNF_HIP(gallery_launch_number(ws.parent, ws.flag, G, n_tracks_out, track_out, s));
    return VNF_OK;
  } catch (const std::exception& ex) {
    return fail(VNF_E_INVALID, std::string("exception: ") + ex.what());
  }
}

extern "C" int vnf_gallery_track_sums(vnf_handle h, const int32_t* prev_dev, const int32_t* next_dev, const int32_t* track_dev, int n_tracks,
                                      float* sums_out, int32_t* counts_out, void* stream) {
  try {
    Gallery* t = handle_cast<Gallery>(h);
    if (!t) return fail(VNF_E_INVALID, "not a gallery handle");
    if (n_tracks < 0) return fail(VNF_E_INVALID, "vnf_gallery_track_sums: n_tracks < 0");
    if (n_tracks == 0) return VNF_OK;
    if (!prev_dev || !next_dev || !track_dev || !sums_out || !counts_out || ((uintptr_t)sums_out & 15))
      return fail(VNF_E_INVALID, "vnf_gallery_track_sums: null or misaligned pointer");
    hipStream_t s = (hipStream_t)stream;
    const int64_t G = t->rows;
    VNF_HIP(hipMemsetAsync(counts_out, 0xFF, (size_t)n_tracks * 4, s));
    if (G > 0) {
      hipLaunchKernelGGL(tracks_heads_kernel, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, s, prev_dev, track_dev, G, n_tracks, counts_out);
      VNF_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(tracks_sums_kernel, dim3((unsigned)n_tracks), dim3(64), 0, s, t->mat, next_dev, G, t->dim, sums_out, counts_out);
    VNF_HIP(hipGetLastError());
    return VNF_OK;
  } catch (const std::exception& ex) {
    return fail(VNF_E_INVALID, std::string("exception: ") + ex.what());
  }
}
