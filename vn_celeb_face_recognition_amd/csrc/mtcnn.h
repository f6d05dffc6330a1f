// Interface between the MTCNN host layer (mtcnn_host.cpp) and its kernels (mtcnn.hip): the types both sides share and one
// launcher per decision the host takes.  A launcher owns its grid arithmetic, its dynamic LDS and the choice between the
// forms of a kernel; it returns the launch status.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

namespace vnf {

constexpr int MAX_LEVELS = 24;
// Candidate tables.  Stage 1 is sized by the pyramid itself: every (level, frame) list has room for all cells of the
// level, so it cannot overflow.  The stage-2 / stage-3 tables hold `keep` rows per frame, a RUN-TIME capacity
// (vnf_mtcnn_cfg.max_candidates, default KEEP).  The NMS kernels keep their sort keys and kept boxes in LDS while a
// list fits the constants below and switch to global-memory scratch beyond them -- the reference has no cap at all
// (detect_face.py:79-93,203-218) and neither has the arithmetic here; only the row tables of stages 2 / 3 are bounded,
// by a capacity the caller can raise (the host layer grows it and retries on VNF_E_CAPACITY).
constexpr int CAP_LDS_KEYS = 8192;   // sort keys held in LDS by the stage-1 NMS kernels
constexpr int KEEP = 2048;           // kept boxes / post-kernel keys held in LDS; default rows per frame of the stage tables
constexpr int FIN_FAST = 32;  // faces per frame covered by the one-copy read-back (VNF_FIN_FAST lowers it: test hook)

struct LevelDesc {
  int Hs, Ws, Hp, Wp, H2, W2, oh, ow;
  float scale;
  int off_px, off_p1, off_c2, off_out;  // prefix offsets (in pixels of that stage) over levels
};

struct LevelTable {
  int n;
  int tot_px, tot_p1, tot_c2, tot_out;
  LevelDesc l[MAX_LEVELS];
};

struct PNetW {  // transposed to [cin][3][3][cout] so one tap's output-channel weights are contiguous
  const float *w1, *b1, *a1, *w2, *b2, *a2, *w3, *b3, *a3, *w41, *b41, *w42, *b42;
};

struct Cand { float score, r0, r1, r2, r3; int cell; };
struct Row { float x1, y1, x2, y2, score; int y, ey, x, ex; };  // stage-2 / stage-3 table row

// global-memory fallback of the NMS kernels (per frame `stride` entries; a level's region starts at its off_out)
struct NmsScratch {
  unsigned long long* keys;
  float4* kbox;
  int* keep;
  float4* reg;
  int stride;
};

struct FrontW { const float* w; const float* b; const float* a; };   // [32][9 taps][4 channels (3 + zero)], [32], [32]
struct MidW { const uint4* w; const float* b; const float* a; };   // [CO/16][18][64 lanes] fragments, [CO], [CO]

// dynamic LDS (bytes) of the launches that take some: the NMS kernels of stage 1, the post kernels of stages 2 / 3, the
// fronts ((crop rows of a band * S + conv rows of a band * C * 8) float4) and the mids (input map + conv map)
constexpr int LDS_NMS = CAP_LDS_KEYS * 8 + KEEP * 20 + 256 * 20, LDS_POST = KEEP * 44 + 256 * 20;
constexpr int LDS_RFRONT = (25 * 24 + 22 * 22 * 8) * 16, LDS_OFRONT = (11 * 48 + 9 * 46 * 8) * 16;
constexpr int LDS_RMID = 11 * 11 * 128 + 9 * 9 * 12 * 16, LDS_OMID = 23 * 23 * 128 + 21 * 21 * 8 * 16;
// the most any launcher below asks for: a device with less per workgroup cannot run the detector
constexpr int MTCNN_LDS_MAX = std::max({LDS_NMS, LDS_POST, LDS_RFRONT, LDS_OFRONT, LDS_RMID, LDS_OMID});

// frames whose rows and base address are 16-byte aligned take the row form of the pyramid and the strips of the crop kernel
inline bool frames_aligned(const uint8_t* frames, int W) { return (W * 3) % 16 == 0 && (reinterpret_cast<uintptr_t>(frames) & 15) == 0; }
// ... the pyramid only while a frame row fits 64 KiB of LDS as fp32
inline bool pyramid_by_rows(const uint8_t* frames, int W) { return frames_aligned(frames, W) && (size_t)W * 12 <= 64 * 1024; }

// K1: u8 frames (B,H,W,3) -> all pyramid levels.  row_order: the dispatch order of the row form, which the caller builds
// where pyramid_by_rows() holds; nullptr takes the gather form
hipError_t launch_pyramid(const uint8_t* frames, int B, int H, int W, const LevelTable& t, float* lvl, const int* row_order,
                          hipStream_t s);
// K2 / K3: the three P-Net launches over all levels and frames; conv3 + heads also thresholds and compacts
hipError_t launch_pnet_conv1_pool(const float* lvl, int B, const LevelTable& t, const PNetW& w, float* p1, hipStream_t s);
hipError_t launch_pnet_conv2(const float* p1, int B, const LevelTable& t, const PNetW& w, float* c2, hipStream_t s);
hipError_t launch_pnet_conv3_heads(const float* c2, int B, const LevelTable& t, const PNetW& w, float thr, int cap_out, Cand* cand,
                                   int* cells, int* cand_cnt, float* prob_dbg, float* reg_dbg, hipStream_t s);
// K4: NMS per (level, frame) at IoU 0.5, then per frame at IoU 0.7 + regress, rerec, pad -> rows / row_cnt
hipError_t launch_nms_stage1(const Cand* cand, const int* cells, const int* cand_cnt, const LevelTable& t, int B, int cap_out, int H,
                             int W, int KR, int* keep1c, int* keep1_cnt, Row* rows, int* row_cnt, int* status, const NmsScratch& g,
                             hipStream_t s);
// K5: candidates [c0, c0 + cap) of the dense batch -> cap x S x S x 4 crops (S = 24 | 48)
hipError_t launch_crop_resize(const uint8_t* frames, int B, int H, int W, const Row* rows, const int* row_cnt, int maxc, int S,
                              float* out, int* status, const int* offs, int c0, int cap, int KR, hipStream_t s);
// K6: conv1 + PReLU + pool1 and conv2 + PReLU + pool2 of R-Net (S = 24) / O-Net (S = 48) over n candidates
hipError_t launch_net_front(int S, bool split, const float* crops, const FrontW& fw, float* p1, int n, hipStream_t s);
hipError_t launch_net_mid(int S, const float* p1, const MidW& mw, float* p2, int n, hipStream_t s);
// compact-batch offsets of the frames' candidates, and the nets' head outputs scattered back to per-frame rows
hipError_t launch_prefix_offsets(const int* cnt, int B, int* offs, hipStream_t s);
hipError_t launch_heads_scatter(const float* heads, int hw, const int* offs, const int* cnt, int maxc, int B, int c0, int cap,
                                float* dst, int nf, bool split, int KR, hipStream_t s);
// K4 / K7: the post kernels of stages 2 and 3, one workgroup per frame
hipError_t launch_stage2_post(const Row* rows, const int* row_cnt, const float* rout, float thr_score, int B, int H, int W, int KR,
                              Row* rows3, int* row3_cnt, int* status, const NmsScratch& g, hipStream_t s);
hipError_t launch_stage3_post(const Row* rows3, const int* row3_cnt, const float* oout, float thr_score, int select_largest, int B,
                              int KR, float* fin, int* fin_cnt, int* status, const NmsScratch& g, hipStream_t s);
// counts block (row_cnt .. status) followed by [B][FIN_FAST][15] result rows
hipError_t launch_pack_results(const int* cnt_block, int ncnt, const float* fin, const int* fin_cnt, int B, int KR, float* stage,
                               hipStream_t s);
// the kernels' status word (nms_device.h ST_*): did a stage-1 list outgrow the candidate tables?
bool stage_tables_overflowed(int status);

}  // namespace vnf
