// Device Huffman coder of the JPEG frame encoder: the quantised coefficients vnf_jpeg_encode_frames leaves in HBM ->
// complete baseline JFIF files in HBM, byte for byte those vnf_jpeg_entropy_encode (jpeg_huff_encode.cpp) writes, so
// that a frame's coefficients (6.27 MB at 1080p 4:2:0) never cross to the host -- only its file does.
//
// Baseline JPEG with the fixed annex K tables is parallel over 8x8 blocks: a block's code depends on its own
// coefficients and on one neighbour's DC, its place in the stream is a prefix sum of the code lengths, and byte stuffing
// is a second prefix sum over the FF bytes.  The per-lane bodies are plain functions in jpeg_huff_device.h (its header
// comment lists the passes); this file holds the kernels that call them, the two scans and the entry points.
//
// Synchronisation between workgroups is the kernel boundary and nothing else.  Bit offsets are 32-bit (a geometry with
// 1658 * units >= 2^32 is refused).  The bit stream is assembled in a zeroed workspace area with plain stores and, for
// the first and last word of a unit, atomicOr -- order-independent, so the bytes repeat from run to run.  Six launches
// and one memset per call, nothing allocated, no host synchronisation.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "block_scan.h"
#include "engine.h"
#include "jpeg_huff_device.h"

namespace vnf {
namespace huff {

constexpr int kLanes = 256;         // per workgroup of the per-unit and per-chunk kernels

// a batch's buffers; frame f's slices are `frame_of(b, f)`
struct Batch {
  Geom g;
  const int16_t* coefs;
  long long coef_count;
  uint32_t* bits;
  long long bits_stride;   // entries per frame, a multiple of 4
  uint32_t* cnt;
  long long cnt_stride;    // a multiple of 4
  uint8_t* area;
  long long area_bytes;
  int32_t* invalid;
  uint32_t* total_bits;
  uint32_t* ff_total;
  const uint8_t* header;
  long long header_len;
  uint8_t* out;
  long long capacity;
  int64_t* lengths;
  int32_t* status;
};

__device__ __forceinline__ Frame frame_of(const Batch& b, int f) {
  Frame r;
  r.coefs = b.coefs + (long long)f * b.coef_count;
  r.bits = b.bits + (long long)f * b.bits_stride;
  r.cnt = b.cnt + (long long)f * b.cnt_stride;
  r.area = reinterpret_cast<uint32_t*>(b.area + (long long)f * b.area_bytes);
  r.area_bytes = b.area_bytes;
  r.invalid = b.invalid + f;
  r.total_bits = b.total_bits + f;
  r.ff_total = b.ff_total + f;
  r.header = b.header;
  r.header_len = b.header_len;
  r.out = b.out + (long long)f * b.capacity;
  r.capacity = b.capacity;
  r.length = b.lengths + f;
  r.status = b.status + f;
  return r;
}

// the code tables into LDS: the walk looks a symbol up per coefficient, every lane another one
__device__ __forceinline__ const Tables& stage_tables(uint32_t* lds) {
  static_assert(sizeof(Tables) % 4 == 0, "Tables is copied by words");
  const uint32_t* src = reinterpret_cast<const uint32_t*>(&kTables);
  for (unsigned i = threadIdx.x; i < sizeof(Tables) / 4; i += blockDim.x) lds[i] = src[i];
  __syncthreads();
  return *reinterpret_cast<const Tables*>(lds);
}

__global__ __launch_bounds__(kLanes) void huff_size_kernel(Batch b) {
  __shared__ uint32_t lds[sizeof(Tables) / 4];
  const Tables& t = stage_tables(lds);
  const unsigned u = blockIdx.x * kLanes + threadIdx.x;
  if (u < b.g.units) size_unit(b.g, frame_of(b, blockIdx.y), t, u);
}

__global__ __launch_bounds__(kLanes) void huff_pack_kernel(Batch b) {
  __shared__ uint32_t lds[sizeof(Tables) / 4];
  const Tables& t = stage_tables(lds);
  const unsigned u = blockIdx.x * kLanes + threadIdx.x;
  if (u < b.g.units) pack_unit(b.g, frame_of(b, blockIdx.y), t, u);
}

__global__ __launch_bounds__(kLanes) void huff_count_kernel(Batch b) {
  __shared__ uint32_t lds[sizeof(Tables) / 4];
  const Tables& t = stage_tables(lds);   // for the chunks past the stream area
  const long long c = (long long)blockIdx.x * kLanes + threadIdx.x;
  if (c < b.cnt_stride) count_chunk(b.g, frame_of(b, blockIdx.y), t, c);   // returns at once behind the stream's end
}

__global__ __launch_bounds__(kLanes) void huff_emit_kernel(Batch b) {
  const Frame f = frame_of(b, blockIdx.y);
  const long long i = (long long)blockIdx.x * kLanes + threadIdx.x;
  emit_header_byte(f, i);
  if (i == 0) emit_tail(f);
  if (i < b.cnt_stride) emit_chunk(f, i);
}

__global__ __launch_bounds__(kScanLanes) void huff_scan_bits_kernel(Batch b) {
  const Frame f = frame_of(b, blockIdx.x);
  const uint32_t total = block_scan(f.bits, b.g.units);
  if (threadIdx.x == 0) *f.total_bits = total;
}

__global__ __launch_bounds__(kScanLanes) void huff_scan_ff_kernel(Batch b) {
  const Frame f = frame_of(b, blockIdx.x);
  const uint32_t chunks = (uint32_t)((stream_bytes(f) + kChunk - 1) / kChunk);
  const uint32_t total = block_scan(f.cnt, chunks);
  if (threadIdx.x == 0) *f.ff_total = total;
}

// info as vnf_jpeg_entropy_encode accepts it (vnf_jpeg_huff_header holds that check) -> its geometry
int checked_geom(const char* who, const vnf_jpeg_info* info, JpegGeom* jg) {
  uint8_t head[kHeaderLen];
  int64_t len = 0;
  if (!info || vnf_jpeg_huff_header(info, head, kHeaderLen, &len) != VNF_OK || len != kHeaderLen ||
      !jpeg_geom(info->width, info->height, info->sampling, jg))
    return fail(VNF_E_INVALID, std::string(who) + ": info is not one vnf_jpeg_entropy_encode accepts");
  return VNF_OK;
}

}  // namespace huff
}  // namespace vnf

using namespace vnf;
using namespace vnf::huff;

extern "C" int64_t vnf_jpeg_huff_workspace_bytes(int n, const vnf_jpeg_info* info, int64_t capacity_per_frame) {
  JpegGeom jg;
  if (n < 0 || n > 65535 || capacity_per_frame < 0)
    return fail(VNF_E_INVALID, "vnf_jpeg_huff_workspace_bytes: n outside 0..65535 or a negative capacity");
  const int rc = checked_geom("vnf_jpeg_huff_workspace_bytes", info, &jg);
  if (rc != VNF_OK) return rc;
  Layout l;
  if (!layout(n, jg, capacity_per_frame, &l))
    return fail(VNF_E_INVALID, "vnf_jpeg_huff_workspace_bytes: the frame is too large for 32-bit bit offsets");
  return l.bytes;
}

extern "C" int vnf_jpeg_huff_encode_frames(const int16_t* coefs_dev, int n, const vnf_jpeg_info* info,
                                           const uint8_t* header_dev, int64_t header_len, uint8_t* out_dev,
                                           int64_t capacity_per_frame, int64_t* lengths_dev, int32_t* status_dev,
                                           void* workspace, int64_t workspace_bytes, void* stream) {
  if (n == 0) return VNF_OK;
  if (n < 0 || n > 65535 || capacity_per_frame < 0 || !coefs_dev || !header_dev || !lengths_dev || !status_dev || !workspace ||
      (!out_dev && capacity_per_frame > 0))
    return fail(VNF_E_INVALID, "vnf_jpeg_huff_encode_frames: bad argument");
  JpegGeom jg;
  const int rc = checked_geom("vnf_jpeg_huff_encode_frames", info, &jg);
  if (rc != VNF_OK) return rc;
  if (header_len != kHeaderLen)
    return fail(VNF_E_INVALID, "vnf_jpeg_huff_encode_frames: header_len is not the length vnf_jpeg_huff_header reports");
  // 16-byte loads of the coefficients (a frame is a multiple of 64 of them) and of the stream area, uint4 in the scans
  if (((uintptr_t)coefs_dev & 15) || ((uintptr_t)workspace & 15) || ((uintptr_t)lengths_dev & 7) || ((uintptr_t)status_dev & 3))
    return fail(VNF_E_INVALID, "vnf_jpeg_huff_encode_frames: coefs_dev and workspace must be 16-byte aligned");
  Layout l;
  if (!layout(n, jg, capacity_per_frame, &l))
    return fail(VNF_E_INVALID, "vnf_jpeg_huff_encode_frames: the frame is too large for 32-bit bit offsets");
  if (workspace_bytes < l.bytes)
    return fail(VNF_E_CAPACITY, "vnf_jpeg_huff_encode_frames: workspace_bytes is below vnf_jpeg_huff_workspace_bytes");
  const long long unit_blocks = (jg.blocks + kLanes - 1) / kLanes;
  const long long lanes = l.cnt_stride > kHeaderLen ? l.cnt_stride : kHeaderLen;
  const long long chunk_blocks = (lanes + kLanes - 1) / kLanes;
  if (unit_blocks > 0x7fffffffLL || chunk_blocks > 0x7fffffffLL)
    return fail(VNF_E_CAPACITY, "vnf_jpeg_huff_encode_frames: frame too large for one grid");

  uint8_t* ws = (uint8_t*)workspace;
  Batch b;
  b.g = make_geom(*info, jg);
  b.coefs = coefs_dev;
  b.coef_count = info->coef_count;
  b.bits = (uint32_t*)(ws + l.bits_at);
  b.bits_stride = l.bits_stride;
  b.cnt = (uint32_t*)(ws + l.cnt_at);
  b.cnt_stride = l.cnt_stride;
  b.area = ws;
  b.area_bytes = l.area_bytes;
  b.invalid = (int32_t*)(ws + l.invalid_at);
  b.total_bits = (uint32_t*)(ws + l.total_at);
  b.ff_total = (uint32_t*)(ws + l.ff_at);
  b.header = header_dev;
  b.header_len = header_len;
  b.out = out_dev;
  b.capacity = capacity_per_frame;
  b.lengths = lengths_dev;
  b.status = status_dev;

  hipStream_t st = (hipStream_t)stream;
  VNF_HIP(hipMemsetAsync(ws, 0, (size_t)l.total_at, st));   // the stream areas and the invalid marks
  const dim3 per_unit((unsigned)unit_blocks, (unsigned)n), per_chunk((unsigned)chunk_blocks, (unsigned)n);
  hipLaunchKernelGGL(huff_size_kernel, per_unit, dim3(kLanes), 0, st, b);
  VNF_HIP(hipGetLastError());
  hipLaunchKernelGGL(huff_scan_bits_kernel, dim3((unsigned)n), dim3(kScanLanes), 0, st, b);
  VNF_HIP(hipGetLastError());
  hipLaunchKernelGGL(huff_pack_kernel, per_unit, dim3(kLanes), 0, st, b);
  VNF_HIP(hipGetLastError());
  hipLaunchKernelGGL(huff_count_kernel, per_chunk, dim3(kLanes), 0, st, b);
  VNF_HIP(hipGetLastError());
  hipLaunchKernelGGL(huff_scan_ff_kernel, dim3((unsigned)n), dim3(kScanLanes), 0, st, b);
  VNF_HIP(hipGetLastError());
  hipLaunchKernelGGL(huff_emit_kernel, per_chunk, dim3(kLanes), 0, st, b);
  VNF_HIP(hipGetLastError());
  return VNF_OK;
}
