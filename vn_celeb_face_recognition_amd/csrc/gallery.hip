// Gallery identification: a device matrix of unit-norm fp32 embeddings with one int32 label per row,
// and an exact cosine top-k search over it.  fp32 end to end on the exact-f32 MFMA (v_mfma_f32_16x16x4_f32 == an fp32 fma
// chain), as head_train.hip and mlp_train.hip use it.
//
//   add     x -> x / max(||x||_2, 1e-12) appended to the matrix (F.normalize's rule), labels copied behind it
//   search  score[f][g] = <q_f / max(||q_f||, 1e-12), gallery_g>; per query the k best rows under the TOTAL order
//           (score descending, row index ascending), a NaN score below every number, an absent row below that
//
// The order is total, so it is one unsigned 64-bit comparison (gallery_key): a larger key is a better candidate, every
// real candidate has a key of its own, and a merge of sorted lists is exact.
//
// Stage one (gallery_search_kernel) is the stream of gallery_core.h with a top-k list per lane on top: a wave owns 16
// queries and a chunk of gallery rows, and a lane keeps the top-k of ITS rows in LDS (an unordered list per lane, touched
// by no other lane, so nothing is synchronised), entered only by candidates that beat the lane's k-th key, which take that
// key's slot; at the end of the chunk the four lanes of a query merge their lists by k rounds of gallery_max4.  The sum
// of squares of a vector is formed in the same lane layout (sum_of_squares) by the search and by add.
// Stage two (gallery_merge_kernel, which the other users of the core launch too): a workgroup per query takes, k times,
// the largest key below the one it took last.
// No atomics; every loop is bounded by k, dim / 16 or the number of chunks.
#include <memory>
#include <string>

#include "gallery_core.h"

namespace vnf {

// rows [0, n) of x (n, dim) -> out, each divided by max(its norm, eps).  A wave per 16 rows.
__global__ void __launch_bounds__(256) gallery_normalize_kernel(const float* __restrict__ x, int64_t n, int dim, float* __restrict__ out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t row = ((int64_t)blockIdx.x * 4 + wave) * 16 + (lane & 15);
  const bool ok = row < n;
  const int kgs = dim >> 4;
  const size_t off = (size_t)(ok ? row : 0) * dim + 4 * (lane >> 4);
  float ss = 0.f;
  for (int kg = 0; kg < kgs; ++kg) {
    const f32x4_t v = *reinterpret_cast<const f32x4_t*>(x + off + kg * 16);
#pragma unroll
    for (int j = 0; j < 4; ++j) ss = ss + v[j] * v[j];
  }
  const float d = fmaxf(sqrtf(sum_of_squares(ss)), GAL_EPS);
  if (!ok) return;
  for (int kg = 0; kg < kgs; ++kg) {
    f32x4_t v = *reinterpret_cast<const f32x4_t*>(x + off + kg * 16);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = v[j] / d;
    *reinterpret_cast<f32x4_t*>(out + off + kg * 16) = v;
  }
}

// sums[c] += x_i / max(||x_i||, eps) and counts[c] += 1 for the rows i with labels[i] == c, in row order.  A wave per
// class walks all n labels: enrolment only.  A label outside [0, C) matches no class.
__global__ void __launch_bounds__(64) gallery_class_sums_kernel(const float* __restrict__ x, const int32_t* __restrict__ labels, int64_t n,
                                                                int dim, float* __restrict__ sums, int32_t* __restrict__ counts) {
  const int lane = threadIdx.x, cls = blockIdx.x;
  const int kgs = dim >> 4;
  float* srow = sums + (size_t)cls * dim;
  int cnt = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (labels[i] != cls) continue;
    const float* xr = x + (size_t)i * dim;
    float ss = 0.f;
    for (int kg = 0; kg < kgs; ++kg) {
      const f32x4_t v = *reinterpret_cast<const f32x4_t*>(xr + kg * 16 + 4 * (lane >> 4));
#pragma unroll
      for (int j = 0; j < 4; ++j) ss = ss + v[j] * v[j];
    }
    const float d = fmaxf(sqrtf(sum_of_squares(ss)), GAL_EPS);
    for (int e = lane; e < dim; e += 64) srow[e] = srow[e] + xr[e] / d;
    ++cnt;
  }
  if (lane == 0) counts[cls] += cnt;
}

// The lane's list L[0..k) is unordered; thr is its smallest key and minpos where that lies.  v (> thr) takes that slot,
// then the k reads that find the new smallest are independent of each other (a sorted insert would chain them).
#define GAL_L(j) lists[((wave * GAL_MAX_K) + (j)) * 64 + lane]
#define GAL_INSERT(v)                                  \
  do {                                                 \
    GAL_L(minpos) = (v);                               \
    thr = ~0ull;                                       \
    _Pragma("unroll") for (int _j = 0; _j < GAL_MAX_K; ++_j)  \
      if (_j < k) {                                    \
        const uint64_t _u = GAL_L(_j);                 \
        if (_u < thr) { thr = _u; minpos = _j; }       \
      }                                                \
  } while (0)

template <int KG, bool EXACT>
__global__ void __launch_bounds__(256) gallery_search_kernel(const float* __restrict__ gal, int64_t G, int dim, const float* __restrict__ q,
                                                             int F, int k, int64_t chunk_rows, int nqg, int64_t nwork,
                                                             uint64_t* __restrict__ partial) {
  __shared__ uint64_t lists[4 * GAL_MAX_K * 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;   // GAL_L's
  GalleryLane<int> L;
  const int64_t w = gallery_wave();
  if (w >= nwork) return;
  gallery_lane_chunked<KG, EXACT>(L, w, nqg, F, dim);

  f32x4_t qf[KG];   // the wave's 16 queries, normalised, as B fragments
  gallery_load_queries<KG, EXACT>(q, L.qrow, L.qok, dim, L.g, L.kgs, qf);

  for (int j = 0; j < k; ++j) GAL_L(j) = 0;
  uint64_t thr = 0;   // the lane's k-th best key so far
  int minpos = 0;

  gallery_lane_rows(L, chunk_rows, G);
  for (int64_t r0 = L.r_begin; r0 < L.r_end; r0 += 32) {
    f32x4_t acc0, acc1;
    gallery_tile<KG, EXACT>(gal, r0, L.r_begin, L.r_end, dim, L.c, L.g, L.kgs, qf, acc0, acc1);
    uint64_t cand[8];
    bool any = false;
    // gallery_for_each's walk, written out (see there)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t i0 = r0 + 4 * L.g + r, i1 = i0 + 16;
      cand[r] = i0 < L.r_end ? gallery_key(acc0[r], (uint32_t)i0) : 0;
      cand[4 + r] = i1 < L.r_end ? gallery_key(acc1[r], (uint32_t)i1) : 0;
      any = any || cand[r] > thr || cand[4 + r] > thr;
    }
    if (any) {
#pragma unroll
      for (int t = 0; t < 8; ++t)
        if (cand[t] > thr) GAL_INSERT(cand[t]);
    }
  }

  // the four lanes of a query merge their lists: k times the largest key below the one taken last (real keys differ
  // pairwise; once only empty slots are left the maximum is 0 and stays 0)
  uint64_t e[GAL_MAX_K];
#pragma unroll
  for (int j = 0; j < GAL_MAX_K; ++j) e[j] = j < k ? GAL_L(j) : 0;
  uint64_t prev = ~0ull;
  for (int r = 0; r < k; ++r) {
    uint64_t m = 0;
#pragma unroll
    for (int j = 0; j < GAL_MAX_K; ++j) m = (e[j] < prev && e[j] > m) ? e[j] : m;
    prev = m = gallery_max4(m);
    if (L.g == 0 && L.qok) partial[((size_t)L.chunk * F + L.qrow) * k + r] = m;
  }
}

// partial (nchunks, F, k) descending lists -> the k best of query blockIdx.x, decoded.
__global__ void __launch_bounds__(256) gallery_merge_kernel(const uint64_t* __restrict__ partial, int64_t nchunks, int F, int k,
                                                            const int32_t* __restrict__ labels, int32_t* __restrict__ idx_out,
                                                            int32_t* __restrict__ label_out, float* __restrict__ score_out) {
  __shared__ uint64_t red[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int f = blockIdx.x;
  uint64_t prev = ~0ull;
  for (int r = 0; r < k; ++r) {
    uint64_t best = 0;
    for (int64_t ch = threadIdx.x; ch < nchunks; ch += 256) {
      const uint64_t* lp = partial + ((size_t)ch * F + f) * k;
      for (int j = 0; j < k; ++j) {   // descending: the first key below prev is this list's best that is left
        const uint64_t v = lp[j];
        if (v < prev) {
          best = v > best ? v : best;
          break;
        }
      }
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
      const uint64_t o = shfl_xor_u64(best, m);
      best = o > best ? o : best;
    }
    __syncthreads();
    if (lane == 0) red[wave] = best;
    __syncthreads();
    best = red[0];
#pragma unroll
    for (int i = 1; i < 4; ++i) best = red[i] > best ? red[i] : best;
    prev = best;
    if (threadIdx.x == 0) {
      const size_t o = (size_t)f * k + r;
      if (best == 0) {
        idx_out[o] = -1;
        label_out[o] = -1;
        score_out[o] = __uint_as_float(0xFF800000u);
      } else {
        const uint32_t row = gallery_key_row(best);
        idx_out[o] = (int32_t)row;
        label_out[o] = labels[row];
        score_out[o] = gallery_key_score(best);
      }
    }
  }
}

static bool gallery_dim_ok(int dim) { return dim >= 16 && dim <= 16 * GAL_MAX_KG && dim % 16 == 0; }

hipError_t gallery_launch_merge(const uint64_t* partial, int64_t nchunks, int F, int k, const int32_t* labels, int32_t* idx_out,
                                int32_t* label_out, float* score_out, hipStream_t stream) {
  hipLaunchKernelGGL(gallery_merge_kernel, dim3(F), dim3(256), 0, stream, partial, nchunks, F, k, labels, idx_out, label_out, score_out);
  return hipGetLastError();
}

}  // namespace vnf
using namespace vnf;

extern "C" int vnf_gallery_create(int dim, int64_t capacity_rows, vnf_handle* out) {
  try {
    if (!out) return fail(VNF_E_INVALID, "vnf_gallery_create: bad argument");
    *out = nullptr;
    if (!gallery_dim_ok(dim)) return fail(VNF_E_INVALID, "vnf_gallery_create: dim must be a multiple of 16 in 16..512");
    if (capacity_rows < 0 || capacity_rows > GAL_MAX_ROWS) return fail(VNF_E_INVALID, "vnf_gallery_create: bad capacity");
    std::unique_ptr<Gallery> t(new Gallery());
    (void)hipGetDevice(&t->device);
    t->dim = dim;
    t->cap = capacity_rows > 0 ? capacity_rows : 1;
    VNF_HIP(hipMalloc((void**)&t->mat, (size_t)t->cap * dim * 4));
    VNF_HIP(hipMalloc((void**)&t->labels, (size_t)t->cap * 4));
    *out = reinterpret_cast<vnf_handle>(static_cast<HandleBase*>(t.release()));
    return VNF_OK;
  } catch (const std::exception& ex) {
    return fail(VNF_E_INVALID, std::string("exception: ") + ex.what());
  }
}

extern "C" int vnf_gallery_size(vnf_handle h, int64_t* rows) {
  Gallery* t = handle_cast<Gallery>(h);
  if (!t || !rows) return fail(VNF_E_INVALID, "vnf_gallery_size: not a gallery handle");
  *rows = t->rows;
  return VNF_OK;
}

// Appends n rows, normalised or as they are.
static int gallery_append(vnf_handle h, const float* rows_dev, const int32_t* labels_dev, int64_t n, bool normalise, void* stream) {
  try {
    Gallery* t = handle_cast<Gallery>(h);
    if (!t) return fail(VNF_E_INVALID, "not a gallery handle");
    if (n < 0 || (n > 0 && (!rows_dev || !labels_dev)) || ((uintptr_t)rows_dev & 15))
      return fail(VNF_E_INVALID, "vnf_gallery_add: bad argument");
    if (n == 0) return VNF_OK;
    if (n > GAL_MAX_ROWS - t->rows) return fail(VNF_E_CAPACITY, "vnf_gallery_add: more than 2^31 - 1 rows");
    hipStream_t s = (hipStream_t)stream;
    const size_t row_bytes = (size_t)t->dim * 4;
    if (t->rows + n > t->cap) {   // amortised doubling; the old matrix is released once its copy has run
      int64_t cap = t->cap * 2 > t->rows + n ? t->cap * 2 : t->rows + n;
      if (cap > GAL_MAX_ROWS) cap = GAL_MAX_ROWS;
      float* mat = nullptr;
      int32_t* labels = nullptr;
      VNF_HIP(hipMalloc((void**)&mat, (size_t)cap * row_bytes));
      hipError_t e = hipMalloc((void**)&labels, (size_t)cap * 4);
      if (e == hipSuccess && t->rows) e = hipMemcpyAsync(mat, t->mat, (size_t)t->rows * row_bytes, hipMemcpyDeviceToDevice, s);
      if (e == hipSuccess && t->rows) e = hipMemcpyAsync(labels, t->labels, (size_t)t->rows * 4, hipMemcpyDeviceToDevice, s);
      if (e == hipSuccess) e = hipStreamSynchronize(s);
      if (e != hipSuccess) {
        (void)hipFree(mat);
        (void)hipFree(labels);
        return fail(VNF_E_HIP, std::string("vnf_gallery_add: grow: ") + hipGetErrorString(e));
      }
      (void)hipFree(t->mat);
      (void)hipFree(t->labels);
      t->mat = mat; t->labels = labels; t->cap = cap;
    }
    float* dst = t->mat + (size_t)t->rows * t->dim;
    if (normalise) {
      hipLaunchKernelGGL(gallery_normalize_kernel, dim3((unsigned)((n + 63) / 64)), dim3(256), 0, s, rows_dev, n, t->dim, dst);
      VNF_HIP(hipGetLastError());
    } else {
      VNF_HIP(hipMemcpyAsync(dst, rows_dev, (size_t)n * row_bytes, hipMemcpyDeviceToDevice, s));
    }
    VNF_HIP(hipMemcpyAsync(t->labels + t->rows, labels_dev, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
    t->rows += n;
    return VNF_OK;
  } catch (const std::exception& ex) {
    return fail(VNF_E_INVALID, std::string("exception: ") + ex.what());
  }
}

extern "C" int vnf_gallery_add(vnf_handle h, const float* rows_dev, const int32_t* labels_dev, int64_t n, void* stream) {
  return gallery_append(h, rows_dev, labels_dev, n, true, stream);
}

extern "C" int vnf_gallery_add_unit(vnf_handle h, const float* rows_dev, const int32_t* labels_dev, int64_t n, void* stream) {
  return gallery_append(h, rows_dev, labels_dev, n, false, stream);
}

extern "C" int vnf_gallery_rows(vnf_handle h, float* rows_out_dev, int64_t first, int64_t n, void* stream) {
  Gallery* t = handle_cast<Gallery>(h);
  if (!t) return fail(VNF_E_INVALID, "not a gallery handle");
  if (first < 0 || n < 0 || first > t->rows || n > t->rows - first || (n > 0 && !rows_out_dev))
    return fail(VNF_E_INVALID, "vnf_gallery_rows: rows outside the gallery");
  if (n == 0) return VNF_OK;
  VNF_HIP(hipMemcpyAsync(rows_out_dev, t->mat + (size_t)first * t->dim, (size_t)n * t->dim * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return VNF_OK;
}

extern "C" int vnf_gallery_class_sums(const float* rows_dev, const int32_t* labels_dev, int64_t n, int dim, float* sums_inout_dev,
                                      int32_t* counts_inout_dev, int num_classes, void* stream) {
  if (!gallery_dim_ok(dim) || n < 0 || n > GAL_MAX_ROWS || num_classes < 0 || ((uintptr_t)rows_dev & 15))
    return fail(VNF_E_INVALID, "vnf_gallery_class_sums: bad argument");
  if (n == 0 || num_classes == 0) return VNF_OK;
  if (!rows_dev || !labels_dev || !sums_inout_dev || !counts_inout_dev) return fail(VNF_E_INVALID, "vnf_gallery_class_sums: null pointer");
  hipLaunchKernelGGL(gallery_class_sums_kernel, dim3(num_classes), dim3(64), 0, (hipStream_t)stream, rows_dev, labels_dev, n, dim,
                     sums_inout_dev, counts_inout_dev);
  VNF_HIP(hipGetLastError());
  return VNF_OK;
}

extern "C" int64_t vnf_gallery_search_workspace_bytes(int F, int k, int64_t G, int64_t chunk_rows) {
  if (F < 0 || k < 1 || k > GAL_MAX_K || G < 0 || G > GAL_MAX_ROWS || chunk_rows < 0) return VNF_E_INVALID;
  const int64_t bytes = GalleryPlan(F, G, chunk_rows).nchunks * F * k * 8;
  return bytes > 0 ? bytes : 8;
}

extern "C" int vnf_gallery_search(vnf_handle h, const float* q_dev, int F, int k, int32_t* idx_out, int32_t* label_out, float* score_out,
                                  int64_t chunk_rows, void* workspace, int64_t workspace_bytes, void* stream) {
  try {
    Gallery* t = handle_cast<Gallery>(h);
    if (!t) return fail(VNF_E_INVALID, "not a gallery handle");
    if (F < 0 || k < 1 || k > GAL_MAX_K || chunk_rows < 0) return fail(VNF_E_INVALID, "vnf_gallery_search: bad argument (1 <= k <= 16)");
    if (F == 0) return VNF_OK;
    if (!q_dev || !idx_out || !label_out || !score_out || !workspace || ((uintptr_t)q_dev & 15) || ((uintptr_t)workspace & 7))
      return fail(VNF_E_INVALID, "vnf_gallery_search: null or misaligned pointer");
    const int64_t G = t->rows;
    const GalleryPlan plan(F, G, chunk_rows);
    if (workspace_bytes < vnf_gallery_search_workspace_bytes(F, k, G, chunk_rows))
      return fail(VNF_E_CAPACITY, "vnf_gallery_search: workspace smaller than vnf_gallery_search_workspace_bytes");
    if (!plan.ok) return fail(VNF_E_INVALID, "vnf_gallery_search: chunk_rows too small for this gallery");
    hipStream_t s = (hipStream_t)stream;
    uint64_t* partial = (uint64_t*)workspace;
    if (plan.blocks > 0) {
      gallery_dispatch(t->dim, [&](auto exact) {
        hipLaunchKernelGGL((gallery_search_kernel<GAL_MAX_KG, decltype(exact)::value>), dim3((unsigned)plan.blocks), dim3(256), 0, s, t->mat,
                           G, t->dim, q_dev, F, k, plan.chunk_rows, plan.nqg, plan.nwork, partial);
      });
      VNF_HIP(hipGetLastError());
    }
    VNF_HIP(gallery_launch_merge(partial, plan.nchunks, F, k, t->labels, idx_out, label_out, score_out, s));
    return VNF_OK;
  } catch (const std::exception& ex) {
    return fail(VNF_E_INVALID, std::string("exception: ") + ex.what());
  }
}
