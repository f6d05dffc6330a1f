// Internal launch interface between the engine (engine.cpp) and the HIP kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vnface.h"

namespace vnf {

// F16X2: split-f16 (hi, lo) pairs, split_f16.h -- fp32-class accuracy on the 16-bit MFMA (ids follow include/vnface.h)
// F16P: planar split-f16 (8-channel units [8 hi][8 lo], three MFMAs per product): what the ENCODERS run when the caller
// asks for VNF_F16X2; F16X2 itself (interleaved pairs) stays the storage of the R-Net / O-Net / RetinaFace plans
enum DType { F32 = 0, BF16 = 1, F16 = 2, F16X2 = 5, F16P = 6 };
inline int dtype_size(int dt) { return (dt == F32 || dt == F16X2 || dt == F16P) ? 4 : 2; }
inline int dtype_chan_align(int dt) { return dt == F16P ? 8 : 16 / dtype_size(dt); }   // channel granularity of slices / gathers

enum Act { ACT_NONE = 0, ACT_RELU = 1, ACT_PRELU = 2 };

struct ConvSeg {   // output columns [c0,c1) of the GEMM go to ptr (already channel-offset), pixel stride ld
  int c0, c1;
  void* ptr;
  int ld;
};

// One implicit-GEMM convolution over NHWC activations.
//   out[m][co] = act( sum_k x[pix(m) + tap(k)] * w[co][k] + bias[cls(m)][co] + res[m][co] )
// m = (n*Ho + ho)*Wo + wo; k = (kh*KW + kw)*Cin + c.
struct ConvArgs {
  int dtype;            // compute/storage dtype of x, w, res, out (unless out_f32)
  const void* x;        // channel-offset base of the input slice
  int ldx;              // pixel stride of x in elements
  int H, W, Cin;        // Cin = channels consumed (multiple of the 16-byte chunk)
  int Ho, Wo;
  int KH, KW, sh, sw, ph, pw;
  const void* w;        // packed [Cout_pad][Kpad], k-order (kh,kw,c)
  int K, Kpad;
  const float* bias;    // [ncls][Cout_pad]
  int ncls;             // 1, or 9 for the border-class bias of a folded pre-conv BatchNorm
  int cout_pad;         // row stride of bias / slope tables
  const int4* ktab;     // per 16-byte k-chunk: {element offset, dh, dw, valid}
  int M, Cout;
  int nseg;
  ConvSeg seg[4];
  const void* res;      // optional residual [M][ldres] (channel-offset base)
  int ldres;
  int act;
  const float* slope;   // PReLU slopes [Cout_pad]
  int out_f32;          // store fp32 instead of dtype
  int cfg;              // tile configuration id (conv_cfg_ok), -1 = heuristic
  int ws_persist;       // wave-specialised kernel: the persistent form where the layer allows it (VNF_WS_PERSIST; host side only)
};

hipError_t launch_conv(const ConvArgs& a, hipStream_t s);
int conv_num_cfgs();
bool conv_cfg_ok(const ConvArgs& a, int cfg);  // is tile configuration `cfg` usable for this convolution
// the ids are three families one after another: ring tiles (conv_igemm.hip), patch tiles (conv_patch.hip),
// wave-specialised tiles (conv_ws.hip); their sizes add up to conv_num_cfgs()
void conv_family_sizes(int sizes[3]);
// the tile of configuration `cfg`: family (0 ring, 1 patch, 2 wave-specialised), BM x BN, waves along M and N (the
// wave-specialised family: consumer waves), ring stages; false: no such id
struct ConvTile { int family, bm, bn, wm, wn, stages; };
bool conv_cfg_tile(int cfg, ConvTile& t);

// NCHW (n,3,S,S) of x_dtype -> NHWC8 of dtype (channels 3..7 zero)
hipError_t launch_pack_input(const void* x, int x_dtype, void* out, int dtype, int n, int hw, hipStream_t s);

// IRv1 stem: NCHW (n,3,160,160) of x_dtype -> conv2d_1a (3x3 s2, folded BN, ReLU) NHWC (n,79,79,32) of dtype;
// wt = fp32 [27][32] folded weights (k = (c*3+kh)*3+kw) followed by 32 biases; mode (VNF_STEM1A_MFMA): the 16-bit / planar
// outputs on the f32 MFMA, 2 (default) fed from LDS-staged input rows (x 16-byte aligned; else as 1), 1 with per-lane
// gathers, 0 the VALU kernel -- bitwise the same result in all three
hipError_t launch_stem_conv1a(const void* x, int x_dtype, void* y, int ldy, int dtype, int n, const float* wt, int mode,
                              hipStream_t s);

// K x K stride-2 max pool, NHWC slice -> NHWC slice; padding and the overhang of a ceil-mode window compare as -inf.
// The windows and storage layouts the plans use (any other combination: hipErrorInvalidValue):
//   3x3 floor  F32 BF16 F16 F16P         nn.MaxPool2d(3, 2)                  IRv1
//   3x3 ceil   F32 F16X2                 nn.MaxPool2d(3, 2, ceil_mode=True)  R-Net, O-Net
//   2x2 ceil   F32 F16X2                 nn.MaxPool2d(2, 2, ceil_mode=True)  O-Net
//   3x3 pad 1  F32 BF16 F16 F16X2 F16P   nn.MaxPool2d(3, 2, 1)               ResNet-50, vnf_maxpool3s2p1
//   2x2 floor  F32 BF16 F16 F16P         nn.MaxPool2d(2, 2)                  SE-IR ResNet-101 stem
// ldx, ldy and C are multiples of the layout's storage unit (dtype_chan_align); a floor-mode window fits the image
struct PoolWindow { int k, pad; bool ceil; };
inline int pool_out_size(int in, PoolWindow w) {   // < 1: the image is smaller than a floor-mode window
  const int span = in + 2 * w.pad - w.k;
  return span < 0 && !w.ceil ? 0 : (span + (w.ceil ? 1 : 0)) / 2 + 1;
}
hipError_t launch_maxpool(const void* x, int ldx, void* y, int ldy, int dtype, int n, int H, int W, int C, PoolWindow w,
                          hipStream_t s);

// trans_emotion_inf on the device: u8 faces (n,S,S,3), S <= 224 -> Pillow-exact bilinear 224x224 -> x/255 -> (x-mean)/std,
// written as NCHW (n,3,224,224) of F32/BF16/F16, or (packed) as the NHWC8 plan input of F32/BF16/F16/F16P
hipError_t launch_emotion_prep(const uint8_t* faces, int n, int S, void* out, int out_dtype, bool packed, hipStream_t s);

// transforms_facenet_aug on the device (augment.hip): row r of the output is face index[r] (NULL: r) of the u8 data set
// (n_faces,S,S,3), rotated / padded / cropped / mirrored as params[r] says -> NCHW (n,3,T,T) of F32/BF16/F16 (x_out) and /
// or the augmented bytes (n,T,T,3) (u8_out); n <= 65535
hipError_t launch_augment_faces(const uint8_t* faces, int n_faces, int S, const int32_t* index, const vnf_aug_param* params, int n,
                                int T, void* x_out, int out_dtype, uint8_t* u8_out, hipStream_t s);

// rows of fp32 logits (n,C): indices of the k (1..16, <= C) largest in descending order (exact ties: lower index first)
// and their softmax values
hipError_t launch_softmax_topk(const float* logits, int n, int C, int k, int32_t* idx, float* prob, hipStream_t s);

// fp32 rows (n,C): pitched copy src (row stride lds) -> dst (row stride ldd)
hipError_t launch_copy_rows_f32(const float* src, int lds, float* dst, int ldd, int n, int C, hipStream_t s);

// global average pool NHWC (n,HW,C) -> (n,C); C and ldx are multiples of the layout's storage unit (dtype_chan_align)
hipError_t launch_avgpool(const void* x, int ldx, void* y, int dtype, int n, int HW, int C, hipStream_t s);

// Squeeze-and-excitation tail of an IRBlock (se_block.hip), dense NHWC tensors (n,HW,C) of F32 / BF16 / F16 / F16P:
//   y = prelu(t * gate + res, slope_out),  gate = sigmoid(w2 . prelu(w1 . mean_hw(t) + b1, slope_se) + b2)
// w1 [C/16][C], b1 [C/16], w2 [C][C/16], b2 [C]: device fp32; C % 16 == 0, 16 <= C <= 1024.  Two launches; `part` is their
// scratch: se_slices(dtype, HW, C) * C channel sums per image (0 slices: the shape is not supported), images part_stride
// floats apart.  Bitwise repeatable, and an image's result does not depend on the batch around it.  y may be t or res.
struct SeWeights { const float *w1, *b1, *w2, *b2; float slope_se, slope_out; };
int se_slices(int dtype, int HW, int C);
hipError_t launch_se_block(const void* t, const void* res, void* y, int dtype, int n, int HW, int C, const SeWeights& w, float* part,
                           size_t part_stride, hipStream_t s);

// rows of fp32 (n,C): y = x / max(||x||_2, 1e-12)
hipError_t launch_l2norm(const float* x, float* y, int n, int C, hipStream_t s);

// rows of fp32 logits (n, ld >= C) (head_eval.hip): log_softmax over the first C columns, argmax (first occurrence) and
// exp(logp[argmax]); with targets, nll[r] = -logp[r][target[r]], hit[r] = argmax == target, sums = {sum nll, sum hit}
// added in index order.  Every output may be NULL; target may be NULL when nll, hit and sums are.
// A target outside [0, C) is never an index: nll = +inf, hit = 0.
hipError_t launch_head_eval(const float* logits, int ld, int C, int n, const int64_t* target, float* logp, int32_t* amax,
                            float* prob, float* nll, int32_t* hit, float* sums, hipStream_t s);

// depthwise 3x3 convolution, padding 1, stride 1 or 2, fp32 NHWC (C % 4 == 0): y = leaky(sum_t x[tap t] * w[t][c] + bias[c])
// (retina_face_utils/components.py:30-40 conv_dw, first half; BatchNorm folded into w / bias)
// (split: the tensors hold split-f16 pairs in their 32-bit elements -- F16X2 plans -- instead of fp32; same for the
// three launchers below)
hipError_t launch_dwconv3x3(const float* x, float* y, int n, int H, int W, int C, int stride, const float* w9c,
                            const float* bias, float slope, bool split, hipStream_t s);

// RetinaFace stem: u8 RGB frames (n,H,W,3) -> (x - (104,117,123)) -> 3x3 stride-2 pad-1 conv 3->8 + folded BN + LeakyReLU,
// NHWC8 fp32 out (retina_face.py:158-164 + components.py:103 conv_bn(3, 8, 2)); wa = [7][64] MFMA lane table
hipError_t launch_retina_stem(const uint8_t* frames, int n, int H, int W, const float* wa, const float* bias, float slope, float* y,
                              bool split, hipStream_t s);
// conv_dw in one pass (components.py:30-40): depthwise 3x3 pad 1 (stride 1|2) + BN + LeakyReLU + pointwise 1x1 + BN +
// LeakyReLU, fp32 NHWC; (cin, cout) in {(8,16), (16,32), (32,32), (32,64)}
bool dwpw_supported(int cin, int cout);
hipError_t launch_dwpw(const float* x, float* y, int n, int H, int W, int cin, int cout, int stride, const float* dw, const float* dbias,
                       float dslope, const float* pw, const float* pbias, float pslope, bool split, hipStream_t s);

// y[n][h][w][c] += x[n][floor(h * Hs/H)][floor(w * Ws/W)][c]: F.interpolate(mode="nearest") + add
// (retina_face_utils/components.py:88-94), fp32 NHWC
hipError_t launch_upsample_add(const float* x, int Hs, int Ws, float* y, int H, int W, int C, int n, bool split, hipStream_t s);

// NHWC slice (dtype) -> NCHW fp32 (for taps / debugging); the slice starts and ends on a storage-unit boundary: C and ldx
// are multiples of dtype_chan_align(dtype)
hipError_t launch_nhwc_to_nchw_f32(const void* x, int ldx, int dtype, float* y, int n, int HW, int C, hipStream_t s);

}  // namespace vnf
