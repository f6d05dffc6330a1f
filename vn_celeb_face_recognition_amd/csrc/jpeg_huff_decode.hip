// Device Huffman decoder of the JPEG frame decoder: frames prepared by vnf_jpeg_huff_prepare (jpeg_entropy.cpp: the scan
// unstuffed and cut at its restart markers, the decode tables, a segment table -- no symbol decoded) -> the quantised
// coefficients vnf_jpeg_entropy_decode writes, in HBM, where vnf_jpeg_decode_frames (jpeg_decode.hip) reads them.  A
// compressed frame crosses the bus as it is (603 KB at 1080p, quality 92) instead of as 6.27 MB of int16.
//
// The algorithm is the self-synchronising parallel decode of Weissenberger and Schmidt adapted to JPEG's interleaved
// scan; jpeg_huff_decode.h describes the passes and holds their per-lane bodies.  This file holds the kernels that call
// them, the fixed-point loops of the synchronise pass and the entry points.
//
// Synchronisation between workgroups is the kernel boundary and nothing else: the convergence loops run inside one
// workgroup between __syncthreads(), a load's entry state comes from a launch that has finished.  Every kernel clamps
// by the blob sizes the host passed (they travel as kernel arguments); what a blob says about itself is checked
// against them by the plan pass before any lane follows it.  Two memsets and nine launches plus one per kLoad * kLoad
// lanes per group of kGroup frames, nothing allocated, no host synchronisation.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "block_scan.h"
#include "engine.h"
#include "jpeg_huff_decode.h"

namespace vnf {
namespace hdec {

constexpr int kGroup = 32;   // frames per launch: their blob offsets and sizes are kernel arguments

struct Batch {
  Geom g;
  int ncomp, subseq_bits;
  uint32_t mcus;
  const uint8_t* blobs;
  long long off[kGroup];
  uint32_t bytes[kGroup];
  int16_t* coefs;
  long long coef_count;
  Meta* meta;
  uint32_t* dctmp;
  long long dc_stride;
  uint32_t* seg_lane0;
  long long seg_stride;
  uint32_t* state;
  uint32_t* cnt;
  long long lane_cap, seg_cap;
  int32_t* status;
};

__device__ __forceinline__ Frame frame_of(const Batch& b, int f) {
  Frame r;
  r.blob = b.blobs + b.off[f];
  r.blob_bytes = b.bytes[f];
  r.meta = b.meta + f;
  r.seg_lane0 = b.seg_lane0 + (long long)f * b.seg_stride;
  r.state = b.state + (long long)f * b.lane_cap;
  r.cnt = b.cnt + (long long)f * b.lane_cap;
  r.dctmp = b.dctmp + (long long)f * b.dc_stride;
  r.coefs = b.coefs + (long long)f * b.coef_count;
  r.coef_count = b.coef_count;
  r.lane_cap = (uint32_t)b.lane_cap;
  r.seg_cap = (uint32_t)b.seg_cap;
  return r;
}

constexpr int kTableWords = kMaxTables * (int)sizeof(DTable) / 4;

// the frame's decode tables into LDS, once per workgroup: every symbol is a lookup, every lane at another entry.
// All lanes of the workgroup call this (it holds a barrier); the frame has passed the plan pass.
__device__ __forceinline__ const DTable* stage_tables(const Frame& f, uint32_t* lds) {
  const uint32_t* src = reinterpret_cast<const uint32_t*>(tables_of(f));
  const unsigned words = f.meta->ntables * (unsigned)(sizeof(DTable) / 4);
  for (unsigned i = threadIdx.x; i < words; i += blockDim.x) lds[i] = src[i];
  __syncthreads();
  return reinterpret_cast<const DTable*>(lds);
}

__global__ __launch_bounds__(kScanLanes) void hdec_plan_kernel(Batch b) {
  const Frame f = frame_of(b, blockIdx.x);
  __shared__ int ok;
  if (threadIdx.x == 0) {
    ok = plan_header(f, b.ncomp, b.mcus);
    if (!ok) f.meta->invalid = 1;
  }
  __syncthreads();
  if (!ok) return;
  const uint32_t nseg = f.meta->nseg;
  for (uint32_t s = threadIdx.x; s < nseg; s += kScanLanes) plan_seg(f, s, b.subseq_bits);
  __syncthreads();
  const uint32_t total = block_scan(f.seg_lane0, nseg);
  if (threadIdx.x == 0) plan_finish(f, total);
}

__global__ __launch_bounds__(kLoad) void hdec_speculate_kernel(Batch b) {
  __shared__ uint32_t lds[kTableWords];
  const Frame f = frame_of(b, blockIdx.y);
  if (blockIdx.x * kLoad >= f.meta->nlanes) return;
  const DTable* t = stage_tables(f, lds);
  const uint32_t lane = blockIdx.x * kLoad + threadIdx.x;
  if (lane < f.meta->nlanes) speculate_lane(f, t, make_sel(b.g, *f.meta), lane, b.subseq_bits);
}

// level 1 of the synchronise pass: the fixed point of one load.  A round reads the exit states of the round before
// from one LDS array and writes its own into the other; at most kLoad rounds.
__global__ __launch_bounds__(kLoad) void hdec_sync_lanes_kernel(Batch b) {
  __shared__ uint32_t lds[kTableWords];
  __shared__ uint32_t exits[2][kLoad];
  const Frame f = frame_of(b, blockIdx.y);
  const uint32_t nlanes = f.meta->nlanes;
  if (blockIdx.x * kLoad >= nlanes) return;
  const DTable* t = stage_tables(f, lds);
  const Sel sel = make_sel(b.g, *f.meta);
  const uint32_t lane = blockIdx.x * kLoad + threadIdx.x;
  const bool live = lane < nlanes;
  Lane l{};
  uint32_t st = 0, used = kNoEntry;
  bool head = true;
  if (live) {
    l = lane_at(f, lane, b.subseq_bits);
    head = lane == l.lane0;
    st = f.state[lane];
  }
  exits[0][threadIdx.x] = st;
  __syncthreads();
  for (int round = 0; round < kLoad; ++round) {
    const int cur = round & 1;
    bool changed = false;
    if (live && !head) changed = resync_lane(l, t, sel, threadIdx.x ? exits[cur][threadIdx.x - 1] : 0u, &used, &st);
    exits[cur ^ 1][threadIdx.x] = st;
    if (!__syncthreads_or(changed)) break;
  }
  if (live && !head) f.state[lane] = st;
}

// level 2: the fixed point of the loads [group * kLoad, + kLoad), one lane per load.  The entry of the group's first
// load is the exit state of the lane before it, final since the launch before this one.
__global__ __launch_bounds__(kLoad) void hdec_sync_loads_kernel(Batch b, uint32_t group) {
  __shared__ uint32_t lds[kTableWords];
  __shared__ uint32_t exits[2][kLoad];
  const Frame f = frame_of(b, blockIdx.x);
  const uint32_t nlanes = f.meta->nlanes;
  const uint32_t load = group * kLoad + threadIdx.x;
  if ((unsigned long long)group * kLoad * kLoad >= nlanes) return;
  const DTable* t = stage_tables(f, lds);
  const Sel sel = make_sel(b.g, *f.meta);
  const unsigned long long first64 = (unsigned long long)load * kLoad;
  const bool live = first64 < nlanes;
  const uint32_t first = (uint32_t)first64;
  uint32_t used = kNoEntry, exit_state = 0;
  if (live) exit_state = f.state[(nlanes - first < (uint32_t)kLoad ? nlanes : first + kLoad) - 1];
  const uint32_t before = threadIdx.x == 0 && live && first > 0 ? f.state[first - 1] : 0u;
  exits[0][threadIdx.x] = exit_state;
  __syncthreads();
  for (int round = 0; round < kLoad; ++round) {
    const int cur = round & 1;
    bool changed = false;
    if (live && first > 0) {
      const uint32_t n = resync_load(f, t, sel, first, b.subseq_bits, threadIdx.x ? exits[cur][threadIdx.x - 1] : before, &used);
      changed = n != exit_state;
      exit_state = n;
    }
    exits[cur ^ 1][threadIdx.x] = exit_state;
    if (!__syncthreads_or(changed)) break;
  }
}

__global__ __launch_bounds__(kLoad) void hdec_count_kernel(Batch b) {
  __shared__ uint32_t lds[kTableWords];
  const Frame f = frame_of(b, blockIdx.y);
  if (blockIdx.x * kLoad >= f.meta->nlanes) return;
  const DTable* t = stage_tables(f, lds);
  const uint32_t lane = blockIdx.x * kLoad + threadIdx.x;
  if (lane < f.meta->nlanes) count_lane(f, t, make_sel(b.g, *f.meta), lane, b.subseq_bits);
}

__global__ __launch_bounds__(kScanLanes) void hdec_scan_units_kernel(Batch b) {
  const Frame f = frame_of(b, blockIdx.x);
  block_scan(f.cnt, f.meta->nlanes);
}

__global__ __launch_bounds__(kLoad) void hdec_write_kernel(Batch b) {
  __shared__ uint32_t lds[kTableWords];
  const Frame f = frame_of(b, blockIdx.y);
  if (blockIdx.x * kLoad >= f.meta->nlanes) return;
  const DTable* t = stage_tables(f, lds);
  const uint32_t lane = blockIdx.x * kLoad + threadIdx.x;
  if (lane < f.meta->nlanes) write_lane(b.g, f, t, make_sel(b.g, *f.meta), b.mcus, lane, b.subseq_bits);
}

__global__ __launch_bounds__(kScanLanes) void hdec_scan_dc_kernel(Batch b) {
  const Frame f = frame_of(b, blockIdx.x);
  if (f.meta->nlanes) block_scan(f.dctmp, b.g.units);
}

__global__ __launch_bounds__(kLoad) void hdec_dc_kernel(Batch b) {
  const Frame f = frame_of(b, blockIdx.y);
  const uint32_t u = blockIdx.x * kLoad + threadIdx.x;
  if (f.meta->nlanes && u < b.g.units) dc_unit(b.g, f, b.mcus, u);
}

__global__ void hdec_status_kernel(Batch b, int n) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f < n) b.status[f] = b.meta[f].invalid ? kInvalid : kOk;
}

// info as vnf_jpeg_probe fills it -> the geometry of its units
int checked_geom(const char* who, const vnf_jpeg_info* info, JpegGeom* jg, Geom* g) {
  if (!info || info->components < 1 || info->components > 3 || !jpeg_geom(info->width, info->height, info->sampling, jg) ||
      info->width < 1 || info->height < 1 || info->width > 65535 || info->height > 65535 || jg->ncomp != info->components ||
      jg->plane_frame != info->coef_count)
    return fail(VNF_E_INVALID, std::string(who) + ": info is not one vnf_jpeg_probe fills");
  *g = make_geom(*info, *jg);
  return VNF_OK;
}

}  // namespace hdec
}  // namespace vnf

using namespace vnf;
using namespace vnf::hdec;

extern "C" int64_t vnf_jpeg_huff_decode_workspace_bytes(int n, const vnf_jpeg_info* info, int64_t max_blob_bytes, int subseq_bits) {
  JpegGeom jg;
  Geom g;
  if (subseq_bits == 0) subseq_bits = kDefaultSubseqBits;
  if (n < 0 || n > 65535 || !subseq_ok(subseq_bits))
    return fail(VNF_E_INVALID, "vnf_jpeg_huff_decode_workspace_bytes: n outside 0..65535 or subseq_bits not 0 or a multiple of 32 in 32..8192");
  const int rc = checked_geom("vnf_jpeg_huff_decode_workspace_bytes", info, &jg, &g);
  if (rc != VNF_OK) return rc;
  Layout l;
  if (!layout(n, jg, g, max_blob_bytes, subseq_bits, &l))
    return fail(VNF_E_INVALID, "vnf_jpeg_huff_decode_workspace_bytes: max_blob_bytes outside 0..2^28 or a frame of 2^28 blocks or more");
  return l.bytes;
}

extern "C" int vnf_jpeg_huff_decode_frames(const uint8_t* blobs_dev, const int64_t* blob_offsets, const int64_t* blob_bytes,
                                           int n, const vnf_jpeg_info* info, int subseq_bits, int16_t* coefs_dev,
                                           int32_t* status_dev, void* workspace, int64_t workspace_bytes, void* stream) {
  if (n == 0) return VNF_OK;
  if (subseq_bits == 0) subseq_bits = kDefaultSubseqBits;
  if (n < 0 || n > 65535 || !blobs_dev || !blob_offsets || !blob_bytes || !coefs_dev || !status_dev || !workspace)
    return fail(VNF_E_INVALID, "vnf_jpeg_huff_decode_frames: bad argument");
  if (!subseq_ok(subseq_bits))
    return fail(VNF_E_INVALID, "vnf_jpeg_huff_decode_frames: subseq_bits must be 0 or a multiple of 32 in 32..8192");
  JpegGeom jg;
  Geom g;
  const int rc = checked_geom("vnf_jpeg_huff_decode_frames", info, &jg, &g);
  if (rc != VNF_OK) return rc;
  if (((uintptr_t)blobs_dev & 15) || ((uintptr_t)workspace & 15) || ((uintptr_t)coefs_dev & 1) || ((uintptr_t)status_dev & 3))
    return fail(VNF_E_INVALID, "vnf_jpeg_huff_decode_frames: blobs_dev and workspace must be 16-byte aligned");
  long long max_blob = 0;
  for (int i = 0; i < n; ++i) {
    if (blob_offsets[i] < 0 || (blob_offsets[i] & 15) || blob_bytes[i] < 0 || blob_bytes[i] > kMaxBlobBytes)
      return fail(VNF_E_INVALID, "vnf_jpeg_huff_decode_frames: a blob offset that is negative or not a multiple of 16, or a size outside 0..2^28");
    if (blob_bytes[i] > max_blob) max_blob = blob_bytes[i];
  }
  Layout l;
  if (!layout(n, jg, g, max_blob, subseq_bits, &l))
    return fail(VNF_E_INVALID, "vnf_jpeg_huff_decode_frames: a frame of 2^28 blocks or more");
  if (workspace_bytes < l.bytes)
    return fail(VNF_E_CAPACITY, "vnf_jpeg_huff_decode_frames: workspace_bytes is below vnf_jpeg_huff_decode_workspace_bytes");
  const long long lane_blocks = l.lane_cap / kLoad, unit_blocks = (jg.blocks + kLoad - 1) / kLoad;
  const long long load_groups = (lane_blocks + kLoad - 1) / kLoad;
  if (lane_blocks > 0x7fffffffLL) return fail(VNF_E_CAPACITY, "vnf_jpeg_huff_decode_frames: frame too large for one grid");

  uint8_t* ws = (uint8_t*)workspace;
  hipStream_t st = (hipStream_t)stream;
  VNF_HIP(hipMemsetAsync(ws, 0, (size_t)l.seg_lane_at, st));   // the invalid marks and the DC differences
  VNF_HIP(hipMemsetAsync(coefs_dev, 0, (size_t)n * (size_t)info->coef_count * sizeof(int16_t), st));
  for (int f0 = 0; f0 < n; f0 += kGroup) {
    const int m = n - f0 < kGroup ? n - f0 : kGroup;
    Batch b;
    b.g = g;
    b.ncomp = info->components;
    b.subseq_bits = subseq_bits;
    b.mcus = (uint32_t)(jg.blocks / g.upm);
    b.blobs = blobs_dev;
    for (int i = 0; i < kGroup; ++i) {
      b.off[i] = i < m ? blob_offsets[f0 + i] : 0;
      b.bytes[i] = i < m ? (uint32_t)blob_bytes[f0 + i] : 0u;
    }
    b.coefs = coefs_dev + (long long)f0 * info->coef_count;
    b.coef_count = info->coef_count;
    b.meta = (Meta*)ws + f0;
    b.dctmp = (uint32_t*)(ws + l.dc_at) + (long long)f0 * l.dc_stride;
    b.dc_stride = l.dc_stride;
    b.seg_lane0 = (uint32_t*)(ws + l.seg_lane_at) + (long long)f0 * l.seg_stride;
    b.seg_stride = l.seg_stride;
    b.state = (uint32_t*)(ws + l.state_at) + (long long)f0 * l.lane_cap;
    b.cnt = (uint32_t*)(ws + l.cnt_at) + (long long)f0 * l.lane_cap;
    b.lane_cap = l.lane_cap;
    b.seg_cap = l.seg_cap;
    b.status = status_dev + f0;
    const dim3 per_frame((unsigned)m), per_lane((unsigned)lane_blocks, (unsigned)m), per_unit((unsigned)unit_blocks, (unsigned)m);
    hipLaunchKernelGGL(hdec_plan_kernel, per_frame, dim3(kScanLanes), 0, st, b);
    VNF_HIP(hipGetLastError());
    hipLaunchKernelGGL(hdec_speculate_kernel, per_lane, dim3(kLoad), 0, st, b);
    VNF_HIP(hipGetLastError());
    hipLaunchKernelGGL(hdec_sync_lanes_kernel, per_lane, dim3(kLoad), 0, st, b);
    VNF_HIP(hipGetLastError());
    for (long long grp = 0; grp < load_groups; ++grp) {
      hipLaunchKernelGGL(hdec_sync_loads_kernel, per_frame, dim3(kLoad), 0, st, b, (uint32_t)grp);
      VNF_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(hdec_count_kernel, per_lane, dim3(kLoad), 0, st, b);
    VNF_HIP(hipGetLastError());
    hipLaunchKernelGGL(hdec_scan_units_kernel, per_frame, dim3(kScanLanes), 0, st, b);
    VNF_HIP(hipGetLastError());
    hipLaunchKernelGGL(hdec_write_kernel, per_lane, dim3(kLoad), 0, st, b);
    VNF_HIP(hipGetLastError());
    hipLaunchKernelGGL(hdec_scan_dc_kernel, per_frame, dim3(kScanLanes), 0, st, b);
    VNF_HIP(hipGetLastError());
    hipLaunchKernelGGL(hdec_dc_kernel, per_unit, dim3(kLoad), 0, st, b);
    VNF_HIP(hipGetLastError());
    hipLaunchKernelGGL(hdec_status_kernel, dim3(1), dim3(kGroup), 0, st, b, m);
    VNF_HIP(hipGetLastError());
  }
  return VNF_OK;
}
