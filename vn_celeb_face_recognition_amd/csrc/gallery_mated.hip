// Gallery calibration: the label-aware search.  Per probe f of known label, over a gallery handle,
//
//   column 0 (mate)      the best row g with labels[g] == qlabels[f] and g != exclude[f]
//   column 1 (non-mate)  the best row g with labels[g] != qlabels[f]
//
// under the search's own total order (gallery_key), an absent candidate being (-1, -1, -inf).  The non-mate score is what
// the same face would score if its owner were not enrolled; a threshold for a target false-accept rate is read off these
// 2 F numbers on the host (calibration.py).
//
// Stage one (gallery_mated_kernel) is the stream of gallery_core.h -- gallery_load_queries and gallery_tile, the very code
// the search runs, so a (probe, row) score has the search's bits -- with two keyed maxima in place of the top-k list: a
// lane keeps two 64-bit keys in registers, no LDS, no atomics.  The per-step extra is the labels of the lane's 8 rows.
// The partials go to the workspace as (chunk, 2 F, 1): pseudo-query 2 f + col.
// Stage two is gallery_merge_kernel with F' = 2 F, k = 1, which writes (F, 2) outputs.
#include <string>

#include "gallery_core.h"

namespace vnf {

template <int KG, bool EXACT>
__global__ void __launch_bounds__(256) gallery_mated_kernel(const float* __restrict__ gal, const int32_t* __restrict__ labels, int64_t G, int dim,
                                                            const float* __restrict__ q, const int32_t* __restrict__ qlabels,
                                                            const int32_t* __restrict__ exclude, int F, int64_t chunk_rows, int nqg,
                                                            int64_t nwork, uint64_t* __restrict__ partial) {
  GalleryLane<int> L;
  const int64_t w = gallery_wave();
  if (w >= nwork) return;
  gallery_lane_chunked<KG, EXACT>(L, w, nqg, F, dim);

  f32x4_t qf[KG];   // the wave's 16 probes, normalised, as B fragments
  gallery_load_queries<KG, EXACT>(q, L.qrow, L.qok, dim, L.g, L.kgs, qf);
  const int32_t ql = qlabels[L.qok ? L.qrow : 0];
  const int64_t excl = exclude ? (int64_t)exclude[L.qok ? L.qrow : 0] : -1;

  uint64_t best_m = 0, best_n = 0;   // the lane's best mate and non-mate keys so far; 0: none
  gallery_lane_rows(L, chunk_rows, G);
  const bool vec = (L.r_begin & 3) == 0;   // r0 + 4 g (+ 16) is then a multiple of 4 at every step
  for (int64_t r0 = L.r_begin; r0 < L.r_end; r0 += 32) {
    int32_t l0[4], l1[4];
    gallery_int4(labels, r0 + 4 * L.g, L.r_begin, L.r_end, vec, l0);
    gallery_int4(labels, r0 + 16 + 4 * L.g, L.r_begin, L.r_end, vec, l1);
    f32x4_t acc0, acc1;
    gallery_tile<KG, EXACT>(gal, r0, L.r_begin, L.r_end, dim, L.c, L.g, L.kgs, qf, acc0, acc1);
    // gallery_for_each's walk, written out (see there)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t i0 = r0 + 4 * L.g + r, i1 = i0 + 16;
      const uint64_t k0 = i0 < L.r_end ? gallery_key(acc0[r], (uint32_t)i0) : 0;
      const uint64_t k1 = i1 < L.r_end ? gallery_key(acc1[r], (uint32_t)i1) : 0;
      const uint64_t m0 = (l0[r] == ql && i0 != excl) ? k0 : 0, n0 = (l0[r] != ql) ? k0 : 0;
      const uint64_t m1 = (l1[r] == ql && i1 != excl) ? k1 : 0, n1 = (l1[r] != ql) ? k1 : 0;
      best_m = m0 > best_m ? m0 : best_m;
      best_m = m1 > best_m ? m1 : best_m;
      best_n = n0 > best_n ? n0 : best_n;
      best_n = n1 > best_n ? n1 : best_n;
    }
  }

  best_m = gallery_max4(best_m);
  best_n = gallery_max4(best_n);
  if (L.g == 0 && L.qok) {
    uint64_t* p = partial + ((size_t)L.chunk * F + L.qrow) * 2;
    p[0] = best_m;
    p[1] = best_n;
  }
}

}  // namespace vnf
using namespace vnf;

extern "C" int64_t vnf_gallery_mated_search_workspace_bytes(int F, int64_t G, int64_t chunk_rows) {
  if (F < 0 || G < 0 || G > GAL_MAX_ROWS || chunk_rows < 0) return VNF_E_INVALID;
  const int64_t bytes = GalleryPlan(F, G, chunk_rows).nchunks * F * 2 * 8;
  return bytes > 0 ? bytes : 8;
}

extern "C" int vnf_gallery_mated_search(vnf_handle h, const float* q_dev, const int32_t* qlabels_dev, const int32_t* exclude_dev, int F,
                                        int32_t* idx_out, int32_t* label_out, float* score_out, int64_t chunk_rows, void* workspace,
                                        int64_t workspace_bytes, void* stream) {
  try {
    Gallery* t = handle_cast<Gallery>(h);
    if (!t) return fail(VNF_E_INVALID, "not a gallery handle");
    if (F < 0 || F > 0x3FFFFFFF || chunk_rows < 0) return fail(VNF_E_INVALID, "vnf_gallery_mated_search: bad argument");
    if (F == 0) return VNF_OK;
    if (!q_dev || !qlabels_dev || !idx_out || !label_out || !score_out || !workspace || ((uintptr_t)q_dev & 15) || ((uintptr_t)workspace & 7))
      return fail(VNF_E_INVALID, "vnf_gallery_mated_search: null or misaligned pointer");
    const int64_t G = t->rows;
    const GalleryPlan plan(F, G, chunk_rows);
    if (workspace_bytes < vnf_gallery_mated_search_workspace_bytes(F, G, chunk_rows))
      return fail(VNF_E_CAPACITY, "vnf_gallery_mated_search: workspace smaller than vnf_gallery_mated_search_workspace_bytes");
    if (!plan.ok) return fail(VNF_E_INVALID, "vnf_gallery_mated_search: chunk_rows too small for this gallery");
    hipStream_t s = (hipStream_t)stream;
    uint64_t* partial = (uint64_t*)workspace;
    if (plan.blocks > 0) {
      gallery_dispatch(t->dim, [&](auto exact) {
        hipLaunchKernelGGL((gallery_mated_kernel<GAL_MAX_KG, decltype(exact)::value>), dim3((unsigned)plan.blocks), dim3(256), 0, s, t->mat,
                           t->labels, G, t->dim, q_dev, qlabels_dev, exclude_dev, F, plan.chunk_rows, plan.nqg, plan.nwork, partial);
      });
      VNF_HIP(hipGetLastError());
    }
    // pseudo-query 2 f + col, one key each: the (F, 2) outputs are the merge's (2 F, 1)
    VNF_HIP(gallery_launch_merge(partial, plan.nchunks, 2 * F, 1, t->labels, idx_out, label_out, score_out, s));
    return VNF_OK;
  } catch (const std::exception& ex) {
    return fail(VNF_E_INVALID, std::string("exception: ") + ex.what());
  }
}
