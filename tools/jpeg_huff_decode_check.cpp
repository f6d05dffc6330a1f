// Stand-alone checker of the device Huffman decoder's host step and per-lane bodies for a sanitizer build (it loads
// nothing into Python and uses no GPU):
//
//   c++ -std=c++17 -g -O2 -fsanitize=address,undefined -fno-sanitize-recover=undefined
//       tools/jpeg_huff_decode_check.cpp vn_celeb_face_recognition_amd/csrc/jpeg_entropy.cpp -o jpeg_huff_decode_check
//   ./jpeg_huff_decode_check tests/golden/images/*.jpg
//
// The kernels of csrc/jpeg_huff_decode.hip call plain functions of (lane index, buffers, subseq_bits) from
// csrc/jpeg_huff_decode.h.  Here vnf_jpeg_huff_prepare and those same functions run over every file: all lanes of a
// pass serially in a seeded shuffled order, the rounds of the two synchronise levels with the double-buffered exit
// states of the kernels, the scans between the passes (workgroup code on the device) as plain loops.  The coefficients
// are compared with vnf_jpeg_entropy_decode's:
//   * subseq_bits 32, 64, 128 and the default on the intact file;
//   * once with the speculate pass skipped and every exit state but the heads' pre-filled with seeded garbage: the
//     synchronise pass alone has to reach the same coefficients, within its bound of rounds;
//   * the damaged inputs of jpeg_entropy_check.cpp: the file cut at 16 lengths, 32 copies with one seeded bit flipped.
// Required: lanes OK => host OK and identical coefficients, always; every intact file the host decodes, the lanes
// decode.  How many damaged streams the host accepts but the lanes refuse is printed.  Every input, blob, workspace and
// coefficient buffer is a heap block of exactly the size handed over, so a stray access is a sanitizer report.  Exit
// status 0 and one summary line.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../include/vnface.h"
#include "../vn_celeb_face_recognition_amd/csrc/jpeg_huff_decode.h"

using namespace vnf;
using namespace vnf::hdec;

static uint64_t g_seed = 0x9E3779B97F4A7C15ull;  // xorshift64*, fixed seed
static uint64_t rnd() {
  g_seed ^= g_seed >> 12;
  g_seed ^= g_seed << 25;
  g_seed ^= g_seed >> 27;
  return g_seed * 0x2545F4914F6CDD1Dull;
}

static std::vector<uint32_t> shuffled(uint32_t n) {
  std::vector<uint32_t> p(n);
  for (uint32_t i = 0; i < n; ++i) p[i] = i;
  for (uint32_t i = n; i > 1; --i) std::swap(p[i - 1], p[(uint32_t)(rnd() % i)]);
  return p;
}

static void exclusive_scan(uint32_t* a, uint32_t n, uint32_t* total) {
  uint32_t sum = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t v = a[i];
    a[i] = sum;
    sum += v;
  }
  if (total) *total = sum;
}

static int g_bad = 0, g_max_rounds = 0;
static void fault(const char* what) {
  printf("FAULT: %s\n", what);
  ++g_bad;
}

// the passes of vnf_jpeg_huff_decode_frames for one prepared frame -> status; coefs: exactly coef_count
static int lane_passes(const uint8_t* blob, int64_t blob_bytes, const vnf_jpeg_info& info, int sb, bool garbage, int16_t* coefs) {
  JpegGeom jg;
  Layout l;
  if (!jpeg_geom(info.width, info.height, info.sampling, &jg)) { fault("geometry"); return kInvalid; }
  const Geom g = make_geom(info, jg);
  if (!layout(1, jg, g, blob_bytes, sb, &l)) { fault("layout"); return kInvalid; }
  uint8_t* ws = new uint8_t[l.bytes];   // 16-byte aligned like the device workspace: operator new gives that
  memset(ws, 0xA5, l.bytes);
  memset(ws, 0, l.seg_lane_at);         // the entry point's memsets
  memset(coefs, 0, sizeof(int16_t) * info.coef_count);
  Frame f;
  f.blob = blob;
  f.blob_bytes = (uint32_t)blob_bytes;
  f.meta = reinterpret_cast<Meta*>(ws);
  f.dctmp = reinterpret_cast<uint32_t*>(ws + l.dc_at);
  f.seg_lane0 = reinterpret_cast<uint32_t*>(ws + l.seg_lane_at);
  f.state = reinterpret_cast<uint32_t*>(ws + l.state_at);
  f.cnt = reinterpret_cast<uint32_t*>(ws + l.cnt_at);
  f.coefs = coefs;
  f.coef_count = info.coef_count;
  f.lane_cap = (uint32_t)l.lane_cap;
  f.seg_cap = (uint32_t)l.seg_cap;
  const uint32_t mcus = (uint32_t)(jg.blocks / g.upm);

  // plan
  if (!plan_header(f, info.components, mcus)) f.meta->invalid = 1;
  if (!f.meta->invalid) {
    for (uint32_t s : shuffled(f.meta->nseg)) plan_seg(f, s, sb);
    uint32_t total = 0;
    exclusive_scan(f.seg_lane0, f.meta->nseg, &total);
    plan_finish(f, total);
  }
  const uint32_t nlanes = f.meta->nlanes;
  if (nlanes) {
    const DTable* t = tables_of(f);
    const Sel sel = make_sel(g, *f.meta);
    // speculate
    for (uint32_t lane : shuffled(nlanes)) {
      if (!garbage || lane == lane_at(f, lane, sb).lane0) speculate_lane(f, t, sel, lane, sb);
      else f.state[lane] = (uint32_t)rnd();
    }
    // synchronise, level 1: hdec_sync_lanes_kernel, one load after another
    const uint32_t loads = (nlanes + kLoad - 1) / kLoad;
    for (uint32_t load : shuffled(loads)) {
      const uint32_t first = load * kLoad, m = nlanes - first < (uint32_t)kLoad ? nlanes - first : (uint32_t)kLoad;
      uint32_t exits[2][kLoad], used[kLoad], st[kLoad];
      for (uint32_t i = 0; i < m; ++i) {
        used[i] = kNoEntry;
        exits[0][i] = st[i] = f.state[first + i];
      }
      int round = 0;
      for (;; ++round) {   // the kernel stops after kLoad rounds; here one more shows that nothing moves any longer
        const int cur = round & 1;
        bool changed = false;
        for (uint32_t i : shuffled(m)) {
          const Lane ln = lane_at(f, first + i, sb);
          if (first + i != ln.lane0) changed |= resync_lane(ln, t, sel, i ? exits[cur][i - 1] : 0u, &used[i], &st[i]);
          exits[cur ^ 1][i] = st[i];
        }
        if (changed && round >= kLoad) fault("level 1 went past its bound of rounds");
        if (!changed || round >= kLoad) break;
      }
      if (round > g_max_rounds) g_max_rounds = round;
      for (uint32_t i = 0; i < m; ++i)
        if (first + i != lane_at(f, first + i, sb).lane0) f.state[first + i] = st[i];
    }
    // level 2: hdec_sync_loads_kernel, one launch per group of kLoad loads, in order
    for (uint32_t group = 0; group * kLoad < loads; ++group) {
      const uint32_t m = loads - group * kLoad < (uint32_t)kLoad ? loads - group * kLoad : (uint32_t)kLoad;
      uint32_t exits[2][kLoad], used[kLoad], ex[kLoad];
      for (uint32_t i = 0; i < m; ++i) {
        const uint32_t first = (group * kLoad + i) * kLoad;
        used[i] = kNoEntry;
        exits[0][i] = ex[i] = f.state[(nlanes - first < (uint32_t)kLoad ? nlanes : first + kLoad) - 1];
      }
      const uint32_t before = group ? f.state[group * kLoad * kLoad - 1] : 0u;
      int round = 0;
      for (;; ++round) {   // the kernel stops after kLoad rounds; here one more shows that nothing moves any longer
        const int cur = round & 1;
        bool changed = false;
        for (uint32_t i : shuffled(m)) {
          const uint32_t first = (group * kLoad + i) * kLoad;
          if (first > 0) {
            const uint32_t n = resync_load(f, t, sel, first, sb, i ? exits[cur][i - 1] : before, &used[i]);
            changed |= n != ex[i];
            ex[i] = n;
          }
          exits[cur ^ 1][i] = ex[i];
        }
        if (changed && round >= kLoad) fault("level 2 went past its bound of rounds");
        if (!changed || round >= kLoad) break;
      }
      if (round > g_max_rounds) g_max_rounds = round;
    }
    // count, scan, write, scan, dc
    for (uint32_t lane : shuffled(nlanes)) count_lane(f, t, sel, lane, sb);
    exclusive_scan(f.cnt, nlanes, nullptr);
    for (uint32_t lane : shuffled(nlanes)) write_lane(g, f, t, sel, mcus, lane, sb);
    exclusive_scan(f.dctmp, g.units, nullptr);
    for (uint32_t u : shuffled(g.units)) dc_unit(g, f, mcus, u);
  }
  const int status = f.meta->invalid ? kInvalid : kOk;
  delete[] ws;
  return status;
}

struct Result {
  int host, prepare, lanes;   // statuses; lanes is VNF_E_INVALID when prepare refused
  bool equal;                 // the coefficients, when both decoded
};

// bytes[0, len) through the host decoder and through prepare + the lane passes, every buffer of exactly its size
static Result both(const std::vector<uint8_t>& bytes, size_t len, const vnf_jpeg_info& info, int sb, bool garbage) {
  Result r{VNF_E_INVALID, VNF_E_INVALID, VNF_E_INVALID, false};
  uint8_t* in = new uint8_t[len ? len : 1];
  memcpy(in, bytes.data(), len);
  int16_t* want = new int16_t[info.coef_count];
  int16_t* got = new int16_t[info.coef_count];
  r.host = vnf_jpeg_entropy_decode(in, (int64_t)len, &info, want, info.coef_count);
  const int64_t bound = vnf_jpeg_huff_prepared_bound((int64_t)len, &info);
  if (bound < 0) fault("prepared_bound");
  uint8_t* scratch = new uint8_t[bound > 0 ? bound : 1];
  int64_t blen = -1;
  r.prepare = vnf_jpeg_huff_prepare(in, (int64_t)len, &info, scratch, bound, &blen);
  if (r.prepare == VNF_E_CAPACITY) fault("the bound was too small");
  if (r.prepare == VNF_OK) {
    if (blen < 64 || blen > bound || (blen & 15)) fault("blob length");
    uint8_t* blob = new uint8_t[blen];   // exactly the blob
    memcpy(blob, scratch, blen);
    // one byte less has to be refused, and without a byte behind out + blen - 1 being written
    uint8_t* tight = new uint8_t[blen - 1];
    int64_t tl = -7;
    if (vnf_jpeg_huff_prepare(in, (int64_t)len, &info, tight, blen - 1, &tl) != VNF_E_CAPACITY || tl != -7) fault("a short capacity was not refused");
    delete[] tight;
    r.lanes = lane_passes(blob, blen, info, sb, garbage, got);
    delete[] blob;
  }
  if (r.lanes == VNF_OK && r.host == VNF_OK) r.equal = memcmp(want, got, sizeof(int16_t) * info.coef_count) == 0;
  delete[] scratch;
  delete[] got;
  delete[] want;
  delete[] in;
  return r;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s file.jpg ...\n", argv[0]);
    return 2;
  }
  int files = 0, damaged = 0, host_only = 0, both_ok = 0;
  for (int a = 1; a < argc; ++a) {
    FILE* fp = fopen(argv[a], "rb");
    if (!fp) {
      fprintf(stderr, "%s: cannot open\n", argv[a]);
      return 2;
    }
    std::vector<uint8_t> bytes;
    uint8_t chunk[65536];
    size_t n;
    while ((n = fread(chunk, 1, sizeof(chunk), fp)) > 0) bytes.insert(bytes.end(), chunk, chunk + n);
    fclose(fp);
    vnf_jpeg_info info;
    const int prc = vnf_jpeg_probe(bytes.data(), (int64_t)bytes.size(), &info);
    if (prc != VNF_OK) {
      printf("%s: probe %d (%s), nothing to decode\n", argv[a], prc, prc > 0 ? "not taken" : "invalid");
      continue;
    }
    ++files;
    const int before = g_bad;
    const int sbs[4] = {32, 64, 128, kDefaultSubseqBits};
    for (int i = 0; i < 5; ++i) {   // the fifth run: no speculation, garbage states, at 64 bits
      const Result r = both(bytes, bytes.size(), info, i < 4 ? sbs[i] : 64, i == 4);
      if (r.lanes == VNF_OK && !(r.host == VNF_OK && r.equal)) fault("the lanes decoded what the host refuses, or other coefficients");
      if (r.host == VNF_OK && r.lanes != VNF_OK) fault("an intact file the host decodes was refused");
    }
    size_t scan = 2;   // the first entropy-coded byte: behind the SOS segment
    while (scan + 4 <= bytes.size() && !(bytes[scan] == 0xFF && bytes[scan + 1] == 0xDA)) scan += 2 + ((bytes[scan + 2] << 8) | bytes[scan + 3]);
    scan += 2 + ((bytes[scan + 2] << 8) | bytes[scan + 3]);
    int cut_ok = 0, flip_ok = 0;
    uint64_t s = 0x9E3779B97F4A7C15ull;
    for (int k = 0; k < 48; ++k) {
      std::vector<uint8_t> b = bytes;
      size_t len = bytes.size();
      if (k < 16) {
        len = bytes.size() * (k + 1) / 17;
      } else {
        s ^= s >> 12; s ^= s << 25; s ^= s >> 27;
        const uint64_t r = s * 0x2545F4914F6CDD1Dull;
        b[scan + (size_t)((r >> 16) % (bytes.size() - 2 - scan))] ^= (uint8_t)(1u << (r & 7));
      }
      const Result r = both(b, len, info, k & 1 ? kDefaultSubseqBits : 32, false);
      ++damaged;
      if (r.lanes == VNF_OK && !(r.host == VNF_OK && r.equal)) fault("a damaged stream: the lanes decoded what the host refuses, or other coefficients");
      if (r.host == VNF_OK && r.lanes != VNF_OK) {
        ++host_only;
        printf("%s: damaged input %d: host ok, prepare %d, lanes %d\n", argv[a], k, r.prepare, r.lanes);
      }
      if (r.lanes == VNF_OK) {
        ++both_ok;
        ++(k < 16 ? cut_ok : flip_ok);
      }
    }
    if (cut_ok) fault("a cut stream decoded without an error");
    printf("%s: %dx%d sampling %d, restart interval %d: intact equal at 32, 64, 128, %d bits and from garbage states; 32 flips -> %d decoded%s\n",
           argv[a], info.width, info.height, info.sampling, info.restart_interval, kDefaultSubseqBits, flip_ok, g_bad == before ? "" : "  ** FAULTS **");
  }
  if (g_bad) {
    printf("FAILED (%d)\n", g_bad);
    return 1;
  }
  printf("every file equal: %d files, %d damaged inputs (%d decoded by both, identical), host-accepted but lane-refused: %d, most rounds of a synchronise level: %d\n",
         files, damaged, both_ok, host_only, g_max_rounds);
  return 0;
}
