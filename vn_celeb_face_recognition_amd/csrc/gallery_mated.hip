// Gallery calibration: the label-aware search.  Per probe f of known label, over a gallery handle,
//
//   column 0 (mate)      the best row g with labels[g] == qlabels[f] and g != exclude[f]
//   column 1 (non-mate)  the best row g with labels[g] != qlabels[f]
//
// under the search's own total order (score descending, row index ascending, NaN below every number; gallery_key), an
// absent candidate being (-1, -1, -inf).  The non-mate score is what the same face would score if its owner were not
// enrolled; a threshold for a target false-accept rate is read off these 2 F numbers on the host (calibration.py).
//
// Stage one (gallery_mated_kernel) is gallery_search_kernel's stream with two keyed maxima in place of the top-k list:
// a wave owns 16 probes and a chunk of rows, the normalised probes are MFMA B fragments in registers, the chunk streams
// 32 rows a step through v_mfma_f32_16x16x4_f32 -- gallery_load_queries and gallery_tile of gallery_core.h, the very
// code the search runs, so a (probe, row) score has the search's bits.  A lane keeps two 64-bit keys in registers: no
// LDS, no atomics.  The per-step extra is the labels of the lane's 8 rows.  At the end of the chunk the four lanes of
// a probe combine by a shuffled maximum and the partials go to the workspace as (chunk, 2 F, 1): pseudo-query 2 f + col.
// Stage two is gallery_merge_kernel with F' = 2 F, k = 1, which writes (F, 2) outputs.
#include <string>

#include "gallery_core.h"

namespace vnf {

// labels of rows i0 .. i0 + 3; a row at or past r_end reads the chunk's first row instead (its key is 0 anyway).
// vec: i0 is a multiple of 4 (wave-uniform), so that 16 bytes can be read at once.
static __device__ __forceinline__ void gallery_labels4(const int32_t* __restrict__ labels, int64_t i0, int64_t r_begin, int64_t r_end,
                                                       bool vec, int32_t (&out)[4]) {
  if (vec && i0 + 3 < r_end) {
    const int4 v = *reinterpret_cast<const int4*>(labels + i0);
    out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = v.w;
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r) out[r] = labels[i0 + r < r_end ? i0 + r : r_begin];
  }
}

template <int KG, bool EXACT>
__global__ void __launch_bounds__(256) gallery_mated_kernel(const float* __restrict__ gal, const int32_t* __restrict__ labels, int64_t G, int dim,
                                                            const float* __restrict__ q, const int32_t* __restrict__ qlabels,
                                                            const int32_t* __restrict__ exclude, int F, int64_t chunk_rows, int nqg,
                                                            int64_t nwork, uint64_t* __restrict__ partial) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t w = (int64_t)blockIdx.x * 4 + wave;
  if (w >= nwork) return;
  const int64_t chunk = w / nqg;
  const int qg = (int)(w % nqg);
  const int c = lane & 15, g = lane >> 4;
  const int kgs = EXACT ? KG : (dim >> 4);
  const int qrow = qg * 16 + c;
  const bool qok = qrow < F;

  f32x4_t qf[KG];   // the wave's 16 probes, normalised, as B fragments
  gallery_load_queries<KG, EXACT>(q, qrow, qok, dim, g, kgs, qf);
  const int32_t ql = qlabels[qok ? qrow : 0];
  const int64_t excl = exclude ? (int64_t)exclude[qok ? qrow : 0] : -1;

  uint64_t best_m = 0, best_n = 0;   // the lane's best mate and non-mate keys so far; 0: none
  const int64_t r_begin = chunk * chunk_rows;
  const int64_t r_end = (r_begin + chunk_rows < G) ? r_begin + chunk_rows : G;
  const bool vec = (r_begin & 3) == 0;   // r0 + 4 g (+ 16) is then a multiple of 4 at every step
  for (int64_t r0 = r_begin; r0 < r_end; r0 += 32) {
    int32_t l0[4], l1[4];
    gallery_labels4(labels, r0 + 4 * g, r_begin, r_end, vec, l0);
    gallery_labels4(labels, r0 + 16 + 4 * g, r_begin, r_end, vec, l1);
    f32x4_t acc0, acc1;
    gallery_tile<KG, EXACT>(gal, r0, r_begin, r_end, dim, c, g, kgs, qf, acc0, acc1);
    // D[row = 4 g + r][col = c]: this lane's probe against rows r0 + 4 g + r and r0 + 16 + 4 g + r
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t i0 = r0 + 4 * g + r, i1 = i0 + 16;
      const uint64_t k0 = i0 < r_end ? gallery_key(acc0[r], (uint32_t)i0) : 0;
      const uint64_t k1 = i1 < r_end ? gallery_key(acc1[r], (uint32_t)i1) : 0;
      const uint64_t m0 = (l0[r] == ql && i0 != excl) ? k0 : 0, n0 = (l0[r] != ql) ? k0 : 0;
      const uint64_t m1 = (l1[r] == ql && i1 != excl) ? k1 : 0, n1 = (l1[r] != ql) ? k1 : 0;
      best_m = m0 > best_m ? m0 : best_m;
      best_m = m1 > best_m ? m1 : best_m;
      best_n = n0 > best_n ? n0 : best_n;
      best_n = n1 > best_n ? n1 : best_n;
    }
  }

  // the four lanes of a probe hold disjoint rows: the maximum of their keys (real keys differ pairwise)
  uint64_t o = shfl_xor_u64(best_m, 16);
  best_m = o > best_m ? o : best_m;
  o = shfl_xor_u64(best_m, 32);
  best_m = o > best_m ? o : best_m;
  o = shfl_xor_u64(best_n, 16);
  best_n = o > best_n ? o : best_n;
  o = shfl_xor_u64(best_n, 32);
  best_n = o > best_n ? o : best_n;
  if (g == 0 && qok) {
    uint64_t* p = partial + ((size_t)chunk * F + qrow) * 2;
    p[0] = best_m;
    p[1] = best_n;
  }
}

}  // namespace vnf
using namespace vnf;

extern "C" int64_t vnf_gallery_mated_search_workspace_bytes(int F, int64_t G, int64_t chunk_rows) {
  if (F < 0 || G < 0 || G > GAL_MAX_ROWS || chunk_rows < 0) return VNF_E_INVALID;
  const int64_t cr = gallery_chunk_rows(F, G, chunk_rows);
  const int64_t nchunks = (G + cr - 1) / cr;
  const int64_t bytes = nchunks * F * 2 * 8;
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
    const int64_t cr = gallery_chunk_rows(F, G, chunk_rows);
    const int64_t nchunks = (G + cr - 1) / cr;
    if (workspace_bytes < vnf_gallery_mated_search_workspace_bytes(F, G, chunk_rows))
      return fail(VNF_E_CAPACITY, "vnf_gallery_mated_search: workspace smaller than vnf_gallery_mated_search_workspace_bytes");
    hipStream_t s = (hipStream_t)stream;
    const int nqg = (F + 15) / 16;
    const int64_t nwork = nchunks * nqg, blocks = (nwork + 3) / 4;
    if (blocks > 0x7FFFFFFF) return fail(VNF_E_INVALID, "vnf_gallery_mated_search: chunk_rows too small for this gallery");
    uint64_t* partial = (uint64_t*)workspace;
    if (blocks > 0) {
      if (t->dim == 16 * GAL_MAX_KG)
        hipLaunchKernelGGL((gallery_mated_kernel<GAL_MAX_KG, true>), dim3((unsigned)blocks), dim3(256), 0, s, t->mat, t->labels, G, t->dim, q_dev,
                           qlabels_dev, exclude_dev, F, cr, nqg, nwork, partial);
      else
        hipLaunchKernelGGL((gallery_mated_kernel<GAL_MAX_KG, false>), dim3((unsigned)blocks), dim3(256), 0, s, t->mat, t->labels, G, t->dim, q_dev,
                           qlabels_dev, exclude_dev, F, cr, nqg, nwork, partial);
      VNF_HIP(hipGetLastError());
    }
    // pseudo-query 2 f + col, one key each: the (F, 2) outputs are the merge's (2 F, 1)
    VNF_HIP(gallery_launch_merge(partial, nchunks, 2 * F, 1, t->labels, idx_out, label_out, score_out, s));
    return VNF_OK;
  } catch (const std::exception& ex) {
    return fail(VNF_E_INVALID, std::string("exception: ") + ex.what());
  }
}
