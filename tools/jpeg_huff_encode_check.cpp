// Stand-alone checker of the host JPEG entropy encoder for a sanitizer build (it loads nothing into Python and uses no
// GPU):
//
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       tools/jpeg_huff_encode_check.cpp vn_celeb_face_recognition_amd/csrc/jpeg_huff_encode.cpp \
//       vn_celeb_face_recognition_amd/csrc/jpeg_entropy.cpp -o jpeg_huff_encode_check
//   ./jpeg_huff_encode_check tests/golden/images/*.jpg
//
// For every baseline file: its coefficients (vnf_jpeg_entropy_decode) are encoded again into a heap block of exactly
// the needed size, of one byte less, of every size up to 700 bytes (the headers) and of 16 evenly spaced sizes, so a
// write past `capacity` is a sanitizer report; the full-size output must decode to the same coefficients.  Then seeded
// random coefficients, in and out of the baseline range, go through every sampling at a few odd sizes.  Exit status 0
// and a summary line per file otherwise.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../include/vnface.h"

static int encode_exact(const int16_t* coefs, const vnf_jpeg_info* info, int64_t cap, std::vector<uint8_t>* keep, int64_t* len) {
  uint8_t* out = new uint8_t[cap ? cap : 1];  // exactly cap bytes: the sanitizer sees one byte too many
  const int rc = vnf_jpeg_entropy_encode(coefs, info, cap ? out : nullptr, cap, len);
  if (keep && rc == VNF_OK) keep->assign(out, out + *len);
  delete[] out;
  return rc;
}

static int check(const char* what, const std::vector<int16_t>& coefs, const vnf_jpeg_info& info, bool expect_ok) {
  int64_t need = -1, len = -1;
  int rc = encode_exact(coefs.data(), &info, 0, nullptr, &need);
  if (!expect_ok) {
    if (rc != VNF_E_INVALID) { printf("%s: out-of-range coefficients gave %d\n", what, rc); return 1; }
    return 0;
  }
  if (rc != VNF_E_CAPACITY || need < 600) { printf("%s: sizing call gave %d, %lld\n", what, rc, (long long)need); return 1; }
  std::vector<uint8_t> file;
  if (encode_exact(coefs.data(), &info, need, &file, &len) != VNF_OK || len != need) { printf("%s: exact capacity failed\n", what); return 1; }
  int bad = 0;
  if (encode_exact(coefs.data(), &info, need - 1, nullptr, &len) != VNF_E_CAPACITY || len != need) ++bad;
  for (int64_t cap = 0; cap < 700 && cap < need; ++cap)
    if (encode_exact(coefs.data(), &info, cap, nullptr, &len) != VNF_E_CAPACITY) ++bad;
  for (int k = 1; k <= 16; ++k)
    if (encode_exact(coefs.data(), &info, need * k / 17, nullptr, &len) != VNF_E_CAPACITY) ++bad;
  vnf_jpeg_info back;
  std::vector<int16_t> again(coefs.size());
  if (vnf_jpeg_probe(file.data(), (int64_t)file.size(), &back) != VNF_OK || back.coef_count != info.coef_count ||
      vnf_jpeg_entropy_decode(file.data(), (int64_t)file.size(), &back, again.data(), (int64_t)again.size()) != VNF_OK ||
      memcmp(again.data(), coefs.data(), coefs.size() * sizeof(int16_t)) != 0)
    ++bad;
  if (bad) printf("%s: %d checks failed\n", what, bad);
  return bad ? 1 : 0;
}

int main(int argc, char** argv) {
  int bad = 0;
  for (int a = 1; a < argc; ++a) {
    FILE* f = fopen(argv[a], "rb");
    if (!f) { fprintf(stderr, "%s: cannot open\n", argv[a]); return 2; }
    std::vector<uint8_t> bytes;
    uint8_t chunk[65536];
    size_t got;
    while ((got = fread(chunk, 1, sizeof(chunk), f)) > 0) bytes.insert(bytes.end(), chunk, chunk + got);
    fclose(f);
    vnf_jpeg_info info;
    const int prc = vnf_jpeg_probe(bytes.data(), (int64_t)bytes.size(), &info);
    if (prc != VNF_OK || info.components != 3 || info.restart_interval != 0) {
      printf("%s: probe %d, not a frame the encoder writes: skipped\n", argv[a], prc);
      continue;
    }
    std::vector<int16_t> coefs(info.coef_count);
    if (vnf_jpeg_entropy_decode(bytes.data(), (int64_t)bytes.size(), &info, coefs.data(), info.coef_count) != VNF_OK) {
      printf("%s: does not decode\n", argv[a]);
      ++bad;
      continue;
    }
    const int b = check(argv[a], coefs, info, true);
    bad += b;
    if (!b) printf("%s: %dx%d sampling %d, %lld coefficients: every capacity inside its buffer, round trip equal\n", argv[a],
                   info.width, info.height, info.sampling, (long long)info.coef_count);
  }
  // seeded random coefficients: sparse blocks (long zero runs, ZRL), dense blocks, the edges of the baseline range
  uint64_t s = 0x9E3779B97F4A7C15ull;  // xorshift64*, fixed seed
  auto rnd = [&s]() { s ^= s >> 12; s ^= s << 25; s ^= s >> 27; return s * 0x2545F4914F6CDD1Dull; };
  const int sizes[][2] = {{1, 1}, {8, 8}, {17, 9}, {8, 24}, {33, 47}};
  int synthetic = 0;
  for (int sampling = VNF_JPEG_444; sampling <= VNF_JPEG_420; ++sampling) {
    for (const auto& wh : sizes) {
      for (int mode = 0; mode < 4; ++mode) {
        vnf_jpeg_info info;
        if (vnf_jpeg_encode_info(wh[0], wh[1], sampling, 75, &info) != VNF_OK) { ++bad; continue; }
        std::vector<int16_t> coefs(info.coef_count, 0);
        for (auto& c : coefs) {
          const uint64_t r = rnd();
          if (mode == 0) c = (r & 31) ? 0 : (int16_t)((int)((r >> 8) % 2047) - 1023);       // sparse
          else if (mode == 1) c = (int16_t)((int)((r >> 8) % 2047) - 1023);                  // dense, full AC range
          else if (mode == 2) c = (int16_t)((r & 1) ? 1023 : -1023);                         // longest codes everywhere
          else c = (int16_t)(r >> 8);                                                        // anything: must be refused
        }
        char what[64];
        snprintf(what, sizeof(what), "synthetic %dx%d sampling %d mode %d", wh[0], wh[1], sampling, mode);
        bad += check(what, coefs, info, mode != 3);
        ++synthetic;
      }
    }
  }
  printf("%d synthetic frames\n", synthetic);
  printf(bad ? "FAILED (%d)\n" : "all inside their buffers\n", bad);
  return bad ? 1 : 0;
}
