// Fused stacks: runs of plan ops that one kernel replaces when the compute dtype allows it (engine.h FusedStack).
#include "engine.h"
#include "block35.h"
#include "block8.h"
#include "mixed6a.h"
#include "stem_mid.h"
#include "trunk17.h"

#include <cstring>

namespace vnf {

using Kind = FusedStack::Kind;

namespace {

// One convolution's biases into a stack's concatenated bias array, device to device.
hipError_t copy_bias(float* dst, const ConvLayer& L) { return hipMemcpy(dst, L.bias, (size_t)L.cout * 4, hipMemcpyDeviceToDevice); }

// One function per kind: check the layer shapes the kernel is written for, gather the weight stream on the device from
// the packed per-convolution weights the plan already uploaded (same folding, same k order), concatenate the biases.
// Each leaves f.active set, or clear when the switch or the dtype leaves the stack to the plan.
int prepare_stem_mid(Encoder& e, FusedStack& f) {
  if (!(e.env.fuse & 4)) return VNF_OK;
  const ConvLayer& c2a = e.convs[f.conv0];
  const ConvLayer& c2b = e.convs[f.conv0 + 1];
  if (c2a.cout != 32 || c2a.K != 288 || c2b.cout != 64 || c2b.K != 288 || c2a.ncls != 1 || c2b.ncls != 1)
    return fail(VNF_E_INVALID, "fused stem: unexpected layer shapes");
  bool ext_ok = false;
  if ((e.env.fuse & 8) && f.ext_conv >= 0) {
    const ConvLayer& c3b = e.convs[f.ext_conv];
    ext_ok = c3b.cout == 80 && c3b.K == 64 && c3b.KH == 1 && c3b.ncls == 1 && c3b.nseg == 1 && c3b.res_buf < 0 && c3b.act == ACT_RELU &&
             e.bufs[f.ext_out_buf].C == 80;
  }
  if (e.dtype == F16P && !ext_ok) return VNF_OK;   // the planar split-f16 stem kernel (stem_mids.hip) always carries conv2d_3b
  StemMidPack pk;
  pk.w[0] = c2a.w; pk.kpad[0] = c2a.Kpad;
  pk.w[1] = c2b.w; pk.kpad[1] = c2b.Kpad;
  f.wstream = e.dalloc(stem_mid_wfrag_bytes(e.dtype));
  f.bias = (float*)e.dalloc(SM_BIAS * 4);
  if (!f.wstream || !f.bias) return VNF_E_HIP;
  VNF_HIP(copy_bias(f.bias, c2a));
  VNF_HIP(copy_bias(f.bias + 32, c2b));
  VNF_HIP(stem_mid_repack(pk, e.dtype, f.wstream, 0));
  VNF_HIP(hipDeviceSynchronize());
  f.macs_alg = c2a.macs_alg + c2b.macs_alg;
  f.active = true;
  f.ext = ext_ok;
  if (ext_ok) f.macs_alg += e.convs[f.ext_conv].macs_alg;
  return VNF_OK;
}

int prepare_block35(Encoder& e, FusedStack& f) {
  if (!(e.env.fuse & 2)) return VNF_OK;
  static const int rows[5] = {96, 32, 32, 32, 256}, ks[5] = {256, 288, 288, 288, 96}, boff[5] = {0, 96, 128, 160, 192};
  const size_t wimg_bytes = block35_wimg_bytes(e.dtype);
  f.wstream = e.dalloc((size_t)f.nblocks * wimg_bytes);
  f.bias = (float*)e.dalloc((size_t)f.nblocks * B35_BIAS * 4);
  if (!f.wstream || !f.bias) return VNF_E_HIP;
  for (int b = 0; b < f.nblocks; ++b) {
    Block35Pack pk;
    float* bias = f.bias + (size_t)b * B35_BIAS;
    pk.bias = bias;
    for (int c = 0; c < 5; ++c) {
      const ConvLayer& L = e.convs[f.conv0 + 5 * b + c];
      if (L.cout != rows[c] || L.K != ks[c] || L.ncls != 1) return fail(VNF_E_INVALID, "fused Block35: unexpected layer shapes");
      pk.w[c] = L.w;
      pk.kpad[c] = L.Kpad;
      VNF_HIP(copy_bias(bias + boff[c], L));
      f.macs_alg += L.macs_alg;
    }
    VNF_HIP(block35_repack(pk, e.dtype, (char*)f.wstream + (size_t)b * wimg_bytes, 0));
  }
  VNF_HIP(hipDeviceSynchronize());
  f.active = true;
  f.stack = (e.env.fuse & 16) && e.dtype != F16P;
  f.ext = false;
  if (f.stack && (e.env.fuse & 32) && f.ext_conv >= 0) {
    const ConvLayer& t = e.convs[f.ext_conv];
    const ConvLayer& last_up = e.convs[f.conv0 + 5 * (f.nblocks - 1) + 4];
    const bool ok = t.KH == 1 && t.KW == 1 && t.K == 256 && t.cout == 192 && t.ncls == 1 && t.nseg == 1 && t.res_buf < 0 &&
                    t.act == ACT_RELU && !t.out_f32 && t.x_buf == last_up.seg[0].buf && t.x_coff == 0 &&
                    t.seg[0].buf == f.ext_out_buf && t.seg[0].coff == 0 && e.bufs[f.ext_out_buf].C == 192;
    if (ok) {
      f.wtail = e.dalloc(B35_TAIL_BYTES);
      if (!f.wtail) return VNF_E_HIP;
      VNF_HIP(block35_tail_repack(t.w, t.Kpad, t.bias, f.wtail, 0));
      VNF_HIP(hipDeviceSynchronize());
      f.ext = true;
      f.macs_alg += t.macs_alg;
    }
  }
  return VNF_OK;
}

int prepare_block8(Encoder& e, FusedStack& f) {
  if (!(e.env.fuse & 64) || e.dtype == F16P) return VNF_OK;   // the planar split-f16 dtype keeps the three plan convolutions
  const ConvLayer& red = e.convs[f.conv0];
  const ConvLayer& c13 = e.convs[f.conv0 + 1];
  const ConvLayer& c31 = e.convs[f.conv0 + 2];
  const std::vector<Buf>& bufs = e.bufs;
  auto plain = [](const ConvLayer& L, int cout, int K) {
    return L.cout == cout && L.K == K && L.Kpad == K && L.ncls == 1 && L.res_buf < 0 && L.act == ACT_RELU && !L.out_f32 &&
           L.sh == 1 && L.sw == 1 && L.H == 3 && L.W == 3 && L.Ho == 3 && L.Wo == 3;
  };
  const bool ok =
      plain(red, 384, 1792) && plain(c13, 192, 576) && plain(c31, 192, 576) && f.last - f.first == 3 &&
      red.KH == 1 && red.KW == 1 && red.x_buf == f.in_buf && red.x_coff == 0 && bufs[f.in_buf].C == 1792 && red.nseg == 2 &&
      red.seg[0].c0 == 0 && red.seg[0].c1 == 192 && red.seg[0].buf == f.out_buf && red.seg[0].coff == 0 &&
      red.seg[1].c0 == 192 && red.seg[1].c1 == 384 && red.seg[1].coff == 0 &&
      c13.KH == 1 && c13.KW == 3 && c13.ph == 0 && c13.pw == 1 && c13.x_buf == red.seg[1].buf && c13.x_coff == 0 &&
      c13.nseg == 1 && c13.seg[0].coff == 0 &&
      c31.KH == 3 && c31.KW == 1 && c31.ph == 1 && c31.pw == 0 && c31.x_buf == c13.seg[0].buf && c31.x_coff == 0 &&
      c31.nseg == 1 && c31.seg[0].buf == f.out_buf && c31.seg[0].coff == 192 && bufs[f.out_buf].C == 384;
  if (!ok) return fail(VNF_E_INVALID, "fused Block8 chain: unexpected layer shapes");
  Block8Pack pk;
  pk.w[0] = red.w; pk.kpad[0] = red.Kpad;
  pk.w[1] = c13.w; pk.kpad[1] = c13.Kpad;
  pk.w[2] = c31.w; pk.kpad[2] = c31.Kpad;
  f.wstream = e.dalloc(block8_stream_bytes());
  f.bias = (float*)e.dalloc(B8_BIAS * 4);
  if (!f.wstream || !f.bias) return VNF_E_HIP;
  VNF_HIP(copy_bias(f.bias, red));
  VNF_HIP(copy_bias(f.bias + 384, c13));
  VNF_HIP(copy_bias(f.bias + 576, c31));
  VNF_HIP(block8_repack(pk, f.wstream, 0));
  VNF_HIP(hipDeviceSynchronize());
  f.macs_alg = red.macs_alg + c13.macs_alg + c31.macs_alg;
  f.active = true;
  return VNF_OK;
}

int prepare_mixed6a(Encoder& e, FusedStack& f) {
  if (!(e.env.fuse & 128) || e.dtype == F16P) return VNF_OK;   // the planar split-f16 dtype keeps the three plan convolutions
  for (const FusedStack& g : e.fused)   // the Block35 stack kernel has taken branch1.0 (prepared before this stack)
    if (g.kind == Kind::Block35 && g.active && g.ext && g.ext_conv == f.conv0) return VNF_OK;
  const ConvLayer& c0 = e.convs[f.conv0];
  const ConvLayer& c1 = e.convs[f.conv0 + 1];
  const ConvLayer& c2 = e.convs[f.conv0 + 2];
  const std::vector<Buf>& bufs = e.bufs;
  auto plain = [](const ConvLayer& L, int cout, int K, int kh, int st, int pad, int H, int Ho) {
    return L.cout == cout && L.K == K && L.Kpad == K && L.ncls == 1 && L.nseg == 1 && L.res_buf < 0 && L.act == ACT_RELU &&
           !L.out_f32 && L.KH == kh && L.KW == kh && L.sh == st && L.sw == st && L.ph == pad && L.pw == pad && L.H == H &&
           L.W == H && L.Ho == Ho && L.Wo == Ho && L.x_coff == 0 && L.seg[0].c0 == 0 && L.seg[0].c1 == cout;
  };
  bool ok = f.last - f.first == 3 && plain(c0, 192, 256, 1, 1, 0, 17, 17) && plain(c1, 192, 1728, 3, 1, 1, 17, 17) &&
            plain(c2, 256, 1728, 3, 2, 0, 17, 8);
  for (int i = 0; ok && i < 3; ++i) ok = e.ops[f.first + i].kind == Op::CONV && e.ops[f.first + i].layer == f.conv0 + i;
  ok = ok && c0.x_buf == f.in_buf && bufs[f.in_buf].H == 17 && bufs[f.in_buf].W == 17 && bufs[f.in_buf].C == 256 &&
       c0.seg[0].coff == 0 && bufs[c0.seg[0].buf].C == 192 && c1.x_buf == c0.seg[0].buf && c1.cin == 192 &&
       c1.seg[0].coff == 0 && bufs[c1.seg[0].buf].C == 192 && c2.x_buf == c1.seg[0].buf && c2.cin == 192 &&
       c2.seg[0].buf == f.out_buf && bufs[f.out_buf].H == 8 && bufs[f.out_buf].W == 8 && c2.seg[0].coff % 8 == 0 &&
       bufs[f.out_buf].C % 8 == 0 && c2.seg[0].coff + 256 <= bufs[f.out_buf].C;
  if (!ok) return fail(VNF_E_INVALID, "fused mixed_6a chain: unexpected layer shapes");
  Mixed6aPack pk;
  pk.w[0] = c0.w; pk.kpad[0] = c0.Kpad;
  pk.w[1] = c1.w; pk.kpad[1] = c1.Kpad;
  pk.w[2] = c2.w; pk.kpad[2] = c2.Kpad;
  f.wstream = e.dalloc(mixed6a_stream_bytes());
  f.bias = (float*)e.dalloc(M6_BIAS * 4);
  if (!f.wstream || !f.bias) return VNF_E_HIP;
  VNF_HIP(copy_bias(f.bias, c0));
  VNF_HIP(copy_bias(f.bias + 192, c1));
  VNF_HIP(copy_bias(f.bias + 384, c2));
  VNF_HIP(mixed6a_repack(pk, f.wstream, 0));
  VNF_HIP(hipDeviceSynchronize());
  f.macs_alg = c0.macs_alg + c1.macs_alg + c2.macs_alg;
  f.active = true;
  return VNF_OK;
}

int prepare_block17(Encoder& e, FusedStack& f) {
  if (!(e.env.fuse & 1)) return VNF_OK;
  Trunk17Pack pk;
  memset(&pk, 0, sizeof pk);
  pk.nblocks = f.nblocks;
  static const int rows[4] = {256, 128, 128, 896}, ks[4] = {896, 896, 896, 256}, boff[4] = {0, 256, 384, 512};
  for (int b = 0; b < f.nblocks; ++b)
    for (int c = 0; c < 4; ++c) {
      const ConvLayer& L = e.convs[f.conv0 + 4 * b + c];
      if (L.cout != rows[c] || L.K != ks[c] || L.Kpad != ks[c] || L.ncls != 1)
        return fail(VNF_E_INVALID, "fused Block17 stack: unexpected layer shapes");
      pk.w[b][c] = L.w;
      pk.kpad[c] = L.Kpad;
      f.macs_alg += L.macs_alg;
    }
  f.wstream = e.dalloc(trunk17_stream_bytes(f.nblocks, e.dtype));
  f.bias = (float*)e.dalloc((size_t)f.nblocks * T17_BIAS * 4);
  if (!f.wstream || !f.bias) return VNF_E_HIP;
  for (int b = 0; b < f.nblocks; ++b)
    for (int c = 0; c < 4; ++c) VNF_HIP(copy_bias(f.bias + (size_t)b * T17_BIAS + boff[c], e.convs[f.conv0 + 4 * b + c]));
  VNF_HIP(trunk17_repack(pk, e.dtype, f.wstream, 0));
  VNF_HIP(hipDeviceSynchronize());
  f.active = true;
  return VNF_OK;
}

}  // namespace

// env.fuse: bit 0: Block17 stack, bit 1: Block35, bit 2: stem 2a+2b+pool, bit 3: conv2d_3b inside the stem kernel, bit 4:
// the five Block35 in one launch (with bit 1), bit 5 (off by default: measured at parity with the separate launch):
// mixed_6a.branch1.0 inside that launch, bit 6: reduce + 1x3 + 3x1 of every Block8 in one launch (bf16 / f16), bit 7:
// mixed_6a.branch1.0 + 1.1 + 1.2 in one launch (bf16 / f16; bit 5, where it applies, takes branch1.0 and leaves the plan)
int Encoder::prepare_fused() {
  for (FusedStack& f : fused) {
    f.active = false;
    if (!env.fuse || (dtype != BF16 && dtype != F16 && dtype != F16P) || f.nblocks < 1 || f.nblocks > T17_MAX_BLOCKS) continue;
    int rc = VNF_OK;
    switch (f.kind) {
      case Kind::StemMid: rc = prepare_stem_mid(*this, f); break;
      case Kind::Block35: rc = prepare_block35(*this, f); break;
      case Kind::Block17: rc = prepare_block17(*this, f); break;
      case Kind::Block8: rc = prepare_block8(*this, f); break;
      case Kind::Mixed6a: rc = prepare_mixed6a(*this, f); break;
    }
    if (rc != VNF_OK) return rc;
  }
  return VNF_OK;
}

// A tap's buffer exists in memory unless every op that writes it sits inside an active fused stack and the stack's own
// kernel does not produce it (conv2d_2a / conv2d_2b / maxpool_3a with the fused stem: those tensors only ever live in LDS).
bool Encoder::buf_materialised(int buf) const {
  for (const FusedStack& f : fused) {
    if (!f.active) continue;
    bool written = false;
    for (int oi = f.first; oi < f.end(); ++oi) {
      const Op& op = ops[oi];
      if (op.kind == Op::CONV) {
        const ConvLayer& L = convs[op.layer];
        for (int i = 0; i < L.nseg; ++i) written |= L.seg[i].buf == buf;
      } else if (op.kind == Op::MAXPOOL) {
        written |= op.dst == buf;
      }
    }
    if (!written) continue;
    bool produced = false;
    switch (f.kind) {
      case Kind::StemMid: produced = buf == (f.ext ? f.ext_out_buf : f.out_buf); break;
      case Kind::Block35:
        for (int b = 0; b < f.nblocks; ++b) produced |= convs[f.conv0 + 5 * b + 4].seg[0].buf == buf;
        produced |= f.ext && buf == f.ext_out_buf;
        break;
      case Kind::Block17: produced = buf == f.out_buf; break;
      case Kind::Block8: produced = buf == f.out_buf; break;   // the concat; branch1.0 / 1x3 outputs only ever live in LDS
      case Kind::Mixed6a: produced = buf == f.out_buf; break;  // the mixed_6a output; the two 17 x 17 tensors only live in LDS
    }
    if (!produced) return false;
  }
  return true;
}

// One launch of the stack's kernel (one per block for Block35 without `stack`) on images [n0, n0 + nn): what run_range
// does in place of ops [first, end()).
int Encoder::launch_fused(const FusedStack& f, int n0, int nn, hipStream_t s) {
  hipError_t err = hipSuccess;
  const char* what = "";
  switch (f.kind) {
    case Kind::StemMid: {
      const int out = f.ext ? f.ext_out_buf : f.out_buf;
      StemMidArgs sa;
      sa.x = at(f.in_buf, n0); sa.ldx = bufs[f.in_buf].C;
      sa.y = at(out, n0); sa.ldy = bufs[out].C;
      sa.n = nn;
      sa.wfrag = f.wstream; sa.bias = f.bias;
      sa.w3b = nullptr; sa.b3b = nullptr; sa.k3b_pad = 0;
      if (f.ext) {
        const ConvLayer& c3b = convs[f.ext_conv];
        sa.w3b = c3b.w; sa.b3b = c3b.bias; sa.k3b_pad = c3b.Kpad;
      }
      what = "fused stem";
      err = launch_stem_mid(sa, dtype, s);
      break;
    }
    case Kind::Block35:
      if (f.stack) {
        const int in = convs[f.conv0 + 4].res_buf;                                // first block's input
        const int out = convs[f.conv0 + 5 * (f.nblocks - 1) + 4].seg[0].buf;      // last block's output
        Block35StackArgs ba;
        ba.x = at(in, n0); ba.ldx = bufs[in].C;
        ba.y = at(out, n0); ba.ldy = bufs[out].C;
        ba.n = nn; ba.nblocks = f.nblocks;
        ba.wimg = f.wstream;
        if (f.ext) {
          ba.wtail = f.wtail;
          ba.ytail = at(f.ext_out_buf, n0);
          ba.ldyt = bufs[f.ext_out_buf].C;
        }
        what = "fused Block35 stack";
        err = launch_block35_stack(ba, dtype, s);
        break;
      }
      what = "fused Block35";
      for (int b = 0; b < f.nblocks && err == hipSuccess; ++b) {
        const ConvLayer& up = convs[f.conv0 + 5 * b + 4];   // residual source = block input, segment 0 = block output
        Block35Args ba;
        ba.x = at(up.res_buf, n0); ba.ldx = bufs[up.res_buf].C;
        ba.y = at(up.seg[0].buf, n0); ba.ldy = bufs[up.seg[0].buf].C;
        ba.n = nn;
        ba.wimg = (const char*)f.wstream + (size_t)b * block35_wimg_bytes(dtype);
        ba.zero = conv_zero_page();
        err = launch_block35(ba, dtype, s);
      }
      break;
    case Kind::Block17: {
      Trunk17Args ta;
      ta.x = at(f.in_buf, n0); ta.ldx = bufs[f.in_buf].C;
      ta.y = at(f.out_buf, n0); ta.ldy = bufs[f.out_buf].C;
      ta.n = nn; ta.nblocks = f.nblocks;
      ta.wstream = f.wstream; ta.bias = f.bias;
      what = "fused Block17 stack";
      err = launch_trunk17(ta, dtype, s);
      break;
    }
    case Kind::Block8: {
      Block8Args ba;
      ba.x = at(f.in_buf, n0); ba.ldx = bufs[f.in_buf].C;
      ba.y = at(f.out_buf, n0); ba.ldy = bufs[f.out_buf].C;
      ba.n = nn;
      ba.wstream = f.wstream; ba.bias = f.bias;
      what = "fused Block8 chain";
      err = launch_block8(ba, dtype, s);
      break;
    }
    case Kind::Mixed6a: {
      Mixed6aArgs ma;
      ma.x = at(f.in_buf, n0); ma.ldx = bufs[f.in_buf].C;
      ma.y = at(f.out_buf, n0); ma.ldy = bufs[f.out_buf].C;
      ma.coff = convs[f.conv0 + 2].seg[0].coff;
      ma.n = nn;
      ma.wstream = f.wstream; ma.bias = f.bias;
      what = "fused mixed_6a chain";
      err = launch_mixed6a(ma, dtype, s);
      break;
    }
  }
  return err == hipSuccess ? VNF_OK : fail(VNF_E_HIP, std::string(what) + ": " + hipGetErrorString(err));
}

const char* fused_label(const FusedStack& f) {
  if (f.kind == Kind::StemMid) return f.ext ? "conv2d_2a+2b+maxpool_3a+3b" : "conv2d_2a+2b+maxpool_3a";
  if (f.kind == Kind::Block8 || f.kind == Kind::Mixed6a) return f.label.c_str();
  return f.kind == Kind::Block35 ? "repeat_1 (fused blocks)" : "repeat_2 (persistent trunk)";
}

const char* fused_detail(const FusedStack& f) {
  if (f.kind == Kind::StemMid) return "rolling rows, one launch, one workgroup per image";
  if (f.kind == Kind::Block17) return "10 x Block17 in one launch, one workgroup per image";
  if (f.kind == Kind::Block8) return "one launch, G = 3 images per workgroup, weights streamed to registers";
  if (f.kind == Kind::Mixed6a) return "1x1 + 3x3 + 3x3 s2 in one launch, image in LDS, one workgroup per image";
  if (!f.stack) return "5 x Block35, one launch per block, one workgroup per image";
  return f.ext ? "5 x Block35 + mixed_6a.branch1.0 in one launch, x in registers"
               : "5 x Block35 in one launch, x in registers, one workgroup per image";
}

}  // namespace vnf
