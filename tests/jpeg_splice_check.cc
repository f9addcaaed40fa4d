// Stand-alone check (no GPU, built with ASan + UBSan by tests/test_jpeg_batch.py) of the host half of batch JPEG reconstruction:
// jpeg_recon.cc WriteJpegMarkers + SpliceJpegScan assemble a JPEG from segment records as the device writer leaves them.
//   1. a real file: the jbrd box of <file.jxl> and the entropy-coded segments cut out of <file.jpg> itself (split at the RSTn markers) must give
//      <file.jpg> back byte for byte;
//   2. synthetic records: padding of the last byte with ones and with recorded padding bits, stuffing of a padded 0xFF, the RSTn counter
//      wrapping past D7, exhausted padding bits.
// usage: jpeg_splice_check file.jxl file.jpg
#include "jpeg_recon.h"
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>

using namespace jxlhip;

static std::vector<uint8_t> ReadFile(const char* path) {
  std::ifstream f(path, std::ios::binary);
  return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
static int Fail(const char* what) { printf("FAIL: %s\n", what); return 1; }

static const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

static int CheckRealFile(const std::vector<uint8_t>& jxl, const std::vector<uint8_t>& jpg) {
  // the jbrd box of the container
  size_t pos = 0, jbrd_off = 0, jbrd_size = 0;
  while (pos + 8 <= jxl.size()) {
    uint64_t size = ((uint64_t)jxl[pos] << 24) | (jxl[pos + 1] << 16) | (jxl[pos + 2] << 8) | jxl[pos + 3];
    size_t hdr = 8;
    if (size == 1) { if (pos + 16 > jxl.size()) break; size = 0; for (int i = 0; i < 8; i++) size = (size << 8) | jxl[pos + 8 + i]; hdr = 16; }
    if (size == 0) size = jxl.size() - pos;
    if (size < hdr || pos + size > jxl.size()) break;
    if (!memcmp(&jxl[pos + 4], "jbrd", 4)) { jbrd_off = pos + hdr; jbrd_size = size - hdr; }
    pos += size;
  }
  if (!jbrd_size) return Fail("no jbrd box");
  JpegData jd;
  std::string err;
  if (!ParseJbrd(&jxl[jbrd_off], jbrd_size, &jd, &err)) { printf("%s\n", err.c_str()); return Fail("ParseJbrd"); }
  // the JPEG: quantisation tables, size and sampling factors, and every scan's segments
  std::vector<std::vector<std::pair<size_t, size_t>>> scans;   // per scan: (offset, size) of each restart segment
  uint32_t width = 0, height = 0;
  size_t qi = 0;
  pos = 2;
  while (pos + 4 <= jpg.size()) {
    if (jpg[pos] != 0xFF) return Fail("marker expected");
    const uint8_t m = jpg[pos + 1];
    if (m == 0xD9) break;
    const size_t len = ((size_t)jpg[pos + 2] << 8) | jpg[pos + 3];
    const uint8_t* seg = &jpg[pos + 4];
    if (m == 0xDB) {
      for (size_t p = 0; p + 65 <= len - 2 && qi < jd.quant.size();) {
        const int prec = seg[p] >> 4;
        for (int k = 0; k < 64; k++) jd.quant[qi].values[kZigzag[k]] = prec ? (seg[p + 1 + 2 * k] << 8) | seg[p + 2 + 2 * k] : seg[p + 1 + k];
        qi++; p += 1 + (prec ? 128 : 64);
      }
    } else if (m == 0xC0 || m == 0xC1 || m == 0xC2) {
      height = (seg[1] << 8) | seg[2]; width = (seg[3] << 8) | seg[4];
      for (size_t c = 0; c < jd.components.size() && c < seg[5]; c++) { jd.components[c].h_samp = seg[7 + 3 * c] >> 4; jd.components[c].v_samp = seg[7 + 3 * c] & 15; }
    }
    pos += 2 + len;
    if (m != 0xDA) continue;
    scans.emplace_back();
    size_t start = pos;
    for (;; pos++) {
      if (pos + 1 >= jpg.size()) return Fail("scan runs off the file");
      if (jpg[pos] != 0xFF || jpg[pos + 1] == 0) continue;
      scans.back().push_back({start, pos - start});
      if (jpg[pos + 1] >= 0xD0 && jpg[pos + 1] <= 0xD7) { pos++; start = pos + 1; continue; }
      break;
    }
  }
  size_t scan_k = 0, num_segs = 0;
  vec<uint8_t> out;
  const bool ok = WriteJpegMarkers(jd, width, height, [&](const JpegScanContext& cx, vec<uint8_t>* o, std::string* e) {
    if (scan_k >= scans.size()) return false;
    vec<JpegSegmentRecord> recs;
    for (auto& s : scans[scan_k]) { JpegSegmentRecord r; r.bytes = jpg.data() + s.first; r.size = s.second; recs.push_back(r); }   // complete bytes only: nothing left to pad
    scan_k++; num_segs += recs.size();
    return SpliceJpegScan(cx, recs.data(), recs.size(), o, e);
  }, &out, &err);
  if (!ok) { printf("%s\n", err.c_str()); return Fail("WriteJpegMarkers"); }
  if (out.size() != jpg.size() || memcmp(out.data(), jpg.data(), jpg.size())) return Fail("assembled file differs from the JPEG");
  printf("real file: %zu bytes, %zu scans, %zu segments: identical\n", jpg.size(), scans.size(), num_segs);
  return 0;
}

static int CheckSynthetic() {
  JpegData jd;
  jd.components.resize(1);
  JpegScanInfo scan;
  size_t pad_pos = 0;
  JpegScanContext cx;
  cx.jd = &jd; cx.scan = &scan; cx.pad_pos = &pad_pos;
  std::string err;
  // ones: 3 data bits 111 + 5 ones = FF -> stuffed; 0 trailing bits: nothing added; ten segments: RST0..RST7, RST0
  const uint8_t a[2] = {0x12, 0x34};
  vec<JpegSegmentRecord> recs(10);
  for (auto& r : recs) { r.bytes = a; r.size = 2; }
  recs[0].trail_bits = 0xE0; recs[0].trail_count = 3;
  recs[1].trail_bits = 0x40; recs[1].trail_count = 2;     // 01 + 111111 = 7F
  vec<uint8_t> out;
  if (!SpliceJpegScan(cx, recs.data(), recs.size(), &out, &err)) return Fail("splice with ones");
  vec<uint8_t> want = {0x12, 0x34, 0xFF, 0x00, 0xFF, 0xD0, 0x12, 0x34, 0x7F};
  for (int k = 2; k < 10; k++) { want.push_back(0xFF); want.push_back((uint8_t)(0xD0 + ((k - 1) & 7))); want.push_back(0x12); want.push_back(0x34); }
  if (out != want) return Fail("ones padding / restart counter");
  if (out[out.size() - 4] != 0xFF || out[out.size() - 3] != 0xD0) return Fail("RST counter does not wrap past D7");
  // recorded padding bits: the cursor runs on across segments
  jd.has_zero_padding_bit = true;
  jd.padding_bits = {1, 0, 1, 1, 0, 0, 1};
  recs.resize(2);
  recs[0].trail_bits = 0xE0; recs[0].trail_count = 3;      // 111 + 10110 = F6
  recs[1].trail_bits = 0x80; recs[1].trail_count = 6;      // 100000 + 01 = 81
  out.clear();
  if (!SpliceJpegScan(cx, recs.data(), recs.size(), &out, &err)) return Fail("splice with recorded bits");
  const vec<uint8_t> want2 = {0x12, 0x34, 0xF6, 0xFF, 0xD0, 0x12, 0x34, 0x81};
  if (out != want2 || pad_pos != 7) return Fail("recorded padding bits");
  out.clear();
  if (SpliceJpegScan(cx, recs.data(), 1, &out, &err) || err.find("padding bits exhausted") == std::string::npos) return Fail("exhausted padding bits not reported");
  printf("synthetic records: ok\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 3) { printf("usage: %s file.jxl file.jpg\n", argv[0]); return 2; }
  const std::vector<uint8_t> jxl = ReadFile(argv[1]), jpg = ReadFile(argv[2]);
  if (jxl.empty() || jpg.size() < 4) return Fail("input files");
  if (int rc = CheckRealFile(jxl, jpg)) return rc;
  if (int rc = CheckSynthetic()) return rc;
  printf("0 failures\n");
  return 0;
}
