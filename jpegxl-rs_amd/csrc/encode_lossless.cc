// jxl-hip: lossless batch encoder, host half (include/jxl_hip.h JxlHipEncoder*; encode_lossless.hip holds the kernels).
//
// Stream shape — one Modular frame per image, a bare codestream: group dimension 256, one pass, no Squeeze / palette / LZ77; RCT type 6 over three colour channels as a
// global transform; one fixed MA tree (a split on the channel, then cut-offs on property 9 with clamped-gradient leaves: encode_lossless.h); prefix codes from the image's
// own histograms, one histogram per leaf, clustered; hybrid-uint (4, 2, 0).  An image that fits one group lies entirely in GlobalModular (single-section TOC form);
// otherwise every group's samples lie in its PassGroup section, GlobalModular carries no samples and the LfGroup / HfGlobal slots of the TOC are empty.
//
// A call: upload (host inputs) -> tokenise + histogram (device) -> read the histograms back, build the codes and the LfGlobal prefix of every image (host) -> bits per row,
// scans (device) -> read the section sizes back, allocate the compact buffer -> pack (device) -> one copy back -> splice headers, TOC and sections (host).
// Everything is a function of one image's samples only, so an image's bytes do not depend on what else is in the call.
#include "encode_lossless.h"
#include "../../include/jxl_hip.h"
#include <hip/hip_runtime_api.h>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

namespace jxlhip {
void SetLastErrorText(const std::string& s);

namespace {

// ---- bit writer and field writers (LSB-first, as the format reads) -------------------------------------------------------------------------
struct EncBits {
  std::vector<uint8_t> bytes;
  uint64_t acc = 0;
  int nacc = 0;
  void put(uint64_t v, int n) {      // n <= 32
    if (n == 0) return;
    acc |= (v & ((1ull << n) - 1)) << nacc;
    nacc += n;
    while (nacc >= 8) { bytes.push_back((uint8_t)acc); acc >>= 8; nacc -= 8; }
  }
  void align() { if (nacc) { bytes.push_back((uint8_t)acc); acc = 0; nacc = 0; } }
  size_t bits() const { return bytes.size() * 8 + nacc; }
};
int CeilLog2(uint32_t x) { int r = 0; while ((1ull << r) < x) r++; return r; }
int FloorLog2(uint32_t x) { int r = 0; while (x >>= 1) r++; return r; }
uint32_t PackSigned(int32_t v) { return v >= 0 ? (uint32_t)v * 2 : (uint32_t)(-(int64_t)v) * 2 - 1; }
struct Dist { int bits; uint32_t off; };
void WriteU32(EncBits& w, uint32_t v, Dist d0, Dist d1, Dist d2, Dist d3) {      // the first distribution that can represent v
  const Dist d[4] = {d0, d1, d2, d3};
  for (int i = 0; i < 4; i++)
    if (v >= d[i].off && (uint64_t)(v - d[i].off) < (1ull << d[i].bits)) { w.put(i, 2); w.put(v - d[i].off, d[i].bits); return; }
  throw std::runtime_error("U32 value not representable");
}
void WriteEnum(EncBits& w, uint32_t v) { WriteU32(w, v, {0, 0}, {0, 1}, {4, 2}, {6, 18}); }
void WriteBitDepth(EncBits& w, uint32_t bits) { w.put(0, 1); WriteU32(w, bits, {0, 8}, {0, 10}, {0, 12}, {6, 1}); }      // integer samples
void WriteVarLenUint16(EncBits& w, uint32_t n) {
  if (n == 0) { w.put(0, 1); return; }
  w.put(1, 1);
  const int nb = FloorLog2(n);
  w.put(nb, 4);
  w.put(n - (1u << nb), nb);
}

// ---- hybrid-uint (4, 2, 0), the one configuration of every code written here -------------------------------------------------------------------
void EncodeHybrid(uint32_t v, uint32_t* tok, uint32_t* nbits, uint32_t* bits) {
  if (v < 16) { *tok = v; *nbits = 0; *bits = 0; return; }
  const uint32_t n = FloorLog2(v), m = v - (1u << n);
  *tok = 16 + ((n - 4) << 2) + (m >> (n - 2));
  *nbits = n - 2;
  *bits = m & ((1u << *nbits) - 1);
}
void WriteUintConfig420(EncBits& w) { w.put(4, 4); w.put(2, 3); w.put(0, 2); }      // log_alpha_size 15: split_exponent in 4 bits, msb in 3, lsb in 2

// ---- prefix codes --------------------------------------------------------------------------------------------------------------------------
// Huffman code lengths (<= max_len) for counts (0 = unused symbol): plain Huffman, flattened (counts halved towards 1) until it fits
std::vector<uint8_t> HuffmanLengths(std::vector<uint64_t> counts, int max_len) {
  const size_t n = counts.size();
  std::vector<uint8_t> len(n, 0);
  size_t used = 0;
  for (uint64_t c : counts) used += c != 0;
  if (used == 0) return len;
  if (used == 1) { for (size_t i = 0; i < n; i++) if (counts[i]) len[i] = 1; return len; }
  for (;;) {
    struct Node { uint64_t w; int l, r; };
    std::vector<Node> nodes;
    std::vector<int> live;
    for (size_t i = 0; i < n; i++) if (counts[i]) { nodes.push_back({counts[i], -1, (int)i}); live.push_back((int)nodes.size() - 1); }
    while (live.size() > 1) {
      std::sort(live.begin(), live.end(), [&](int a, int b) { return nodes[a].w > nodes[b].w || (nodes[a].w == nodes[b].w && a < b); });
      const int a = live.back(); live.pop_back();
      const int b = live.back(); live.pop_back();
      nodes.push_back({nodes[a].w + nodes[b].w, a, b});
      live.push_back((int)nodes.size() - 1);
    }
    std::fill(len.begin(), len.end(), 0);
    int deepest = 0;
    std::vector<std::pair<int, int>> stack{{live[0], 0}};
    while (!stack.empty()) {
      const auto [id, d] = stack.back(); stack.pop_back();
      if (nodes[id].l < 0) { len[nodes[id].r] = (uint8_t)d; deepest = std::max(deepest, d); }
      else { stack.push_back({nodes[id].l, d + 1}); stack.push_back({nodes[id].r, d + 1}); }
    }
    if (deepest <= max_len) return len;
    for (auto& c : counts) if (c) c = c / 2 + 1;
  }
}
std::vector<uint16_t> CanonicalCodes(const std::vector<uint8_t>& len) {      // by (length, symbol)
  std::vector<uint16_t> code(len.size(), 0);
  uint32_t next = 0;
  for (int l = 1; l <= 15; l++) {
    for (size_t s = 0; s < len.size(); s++) if (len[s] == l) code[s] = (uint16_t)next++;
    next <<= 1;
  }
  return code;
}
uint32_t ReverseBits(uint32_t code, int len) { uint32_t r = 0; for (int b = 0; b < len; b++) if (code >> b & 1) r |= 1u << (len - 1 - b); return r; }
// Brotli-style description of a prefix code over `alphabet` symbols: the simple form for one or two used symbols, else the complex form — a code-length code over the
// lengths that occur (no repeat symbols), then one length per symbol up to the last used one.
void WritePrefixCodeDescription(EncBits& w, const std::vector<uint8_t>& len, int alphabet) {
  if (alphabet == 1) return;
  std::vector<int> used;
  for (int i = 0; i < alphabet; i++) if (len[i]) used.push_back(i);
  int max_bits = 0;
  for (int v = alphabet - 1; v; v >>= 1) max_bits++;
  if (used.size() <= 2) {
    w.put(1, 2);
    w.put((uint32_t)std::max<size_t>(used.size(), 1) - 1, 2);
    if (used.empty()) w.put(0, max_bits);
    for (int sym : used) w.put((uint32_t)sym, max_bits);
    return;
  }
  w.put(0, 2);
  std::vector<uint64_t> freq(18, 0);
  for (int i = 0; i <= used.back(); i++) freq[len[i]]++;
  const std::vector<uint8_t> cl = HuffmanLengths(freq, 5);
  int distinct = 0;
  for (int i = 0; i < 18; i++) distinct += cl[i] != 0;
  static const uint8_t kOrder[18] = {1, 2, 3, 4, 0, 5, 17, 6, 16, 7, 8, 9, 10, 11, 12, 13, 14, 15};
  auto put_cl = [&](int v) {      // the fixed code of the code-length-code lengths
    switch (v) { case 0: w.put(0, 2); break; case 4: w.put(1, 2); break; case 3: w.put(2, 2); break; case 2: w.put(3, 3); break; case 1: w.put(7, 4); break; default: w.put(15, 4); break; }
  };
  int space = 32;
  for (int i = 0; i < 18 && space > 0; i++) {
    const int v = cl[kOrder[i]];
    put_cl(v);
    if (v) space -= 32 >> v;
  }
  if (distinct != 1 && space != 0) throw std::runtime_error("prefix writer: incomplete code-length code");
  if (distinct == 1) return;
  const std::vector<uint16_t> clcode = CanonicalCodes(cl);
  int sp = 32768;
  for (int i = 0; i <= used.back() && sp > 0; i++) {
    w.put(ReverseBits(clcode[len[i]], cl[len[i]]), cl[len[i]]);
    if (len[i]) sp -= 32768 >> len[i];
  }
  if (sp != 0) throw std::runtime_error("prefix writer: incomplete code");
}

using Histo = std::vector<uint64_t>;
// What a prefix code spends on a histogram, roughly: the entropy, but at least one bit per symbol once two symbols are in use (a lone symbol costs nothing).
double PrefixCost(const Histo& h) {
  uint64_t total = 0; int used = 0;
  for (uint64_t v : h) { total += v; used += v != 0; }
  if (used <= 1) return 0;
  double c = 0;
  for (uint64_t v : h) if (v) c += (double)v * std::max(1.0, std::log2((double)total / (double)v));
  return c;
}
// An entropy code of the stream: context map + one length-limited prefix code per cluster.
struct PrefixCoder {
  std::vector<uint8_t> ctx_map;
  struct Cluster { std::vector<uint8_t> len; std::vector<uint16_t> rev; bool single = false; };      // rev: the code, first bit in bit 0
  std::vector<Cluster> clusters;

  // Clustering, one pass over the contexts from the largest down: a context joins the cluster whose cost grows least by taking it in, unless even that growth outweighs
  // the cost of describing one more code (about 5 bits per symbol of its alphabet) — then it founds a cluster.  Empty contexts go to cluster 0.
  void Build(const std::vector<Histo>& h) {
    const int num_ctx = (int)h.size();
    std::vector<uint64_t> tot(num_ctx, 0);
    std::vector<int> order, assign(num_ctx, -1);
    for (int i = 0; i < num_ctx; i++) { for (uint64_t v : h[i]) tot[i] += v; if (tot[i]) order.push_back(i); }
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return tot[a] > tot[b]; });
    std::vector<Histo> ch;
    std::vector<double> ccost;
    for (int i : order) {
      const double own = PrefixCost(h[i]);
      size_t alphabet = h[i].size();
      while (alphabet && !h[i][alphabet - 1]) alphabet--;
      int best = -1; double best_growth = 20.0 + 5.0 * (double)alphabet;
      Histo merged;
      for (int cl = 0; cl < (int)ch.size(); cl++) {
        merged = ch[cl];
        if (merged.size() < h[i].size()) merged.resize(h[i].size(), 0);
        for (size_t s = 0; s < h[i].size(); s++) merged[s] += h[i][s];
        const double growth = PrefixCost(merged) - ccost[cl] - own;
        if (growth < best_growth || (best < 0 && ch.size() >= 256)) { best_growth = growth; best = cl; }
      }
      if (best < 0) { ch.push_back(h[i]); ccost.push_back(own); assign[i] = (int)ch.size() - 1; continue; }
      if (ch[best].size() < h[i].size()) ch[best].resize(h[i].size(), 0);
      for (size_t s = 0; s < h[i].size(); s++) ch[best][s] += h[i][s];
      ccost[best] = PrefixCost(ch[best]);
      assign[i] = best;
    }
    if (ch.empty()) ch.push_back({});
    ctx_map.assign(num_ctx, 0);
    for (int i = 0; i < num_ctx; i++) ctx_map[i] = (uint8_t)(assign[i] < 0 ? 0 : assign[i]);
    clusters.assign(ch.size(), Cluster());
    for (size_t c = 0; c < ch.size(); c++) {
      Histo counts = ch[c];
      while (!counts.empty() && counts.back() == 0) counts.pop_back();
      if (counts.empty()) counts.push_back(1);
      Cluster& k = clusters[c];
      k.len = HuffmanLengths(counts, (int)kEncMaxCodeBits);
      size_t used = 0;
      for (uint8_t l : k.len) used += l != 0;
      k.single = used <= 1;                                         // a single symbol costs no bits
      const std::vector<uint16_t> code = CanonicalCodes(k.len);
      k.rev.resize(code.size());
      for (size_t s = 0; s < code.size(); s++) k.rev[s] = (uint16_t)ReverseBits(code[s], k.len[s]);
    }
  }
  void Put(EncBits& w, uint32_t ctx, uint32_t value) const {
    uint32_t tok, nb, bits;
    EncodeHybrid(value, &tok, &nb, &bits);
    const Cluster& k = clusters[ctx_map[ctx]];
    if (tok >= k.len.size() || (!k.single && !k.len[tok])) throw std::runtime_error("prefix: symbol without a code");
    if (!k.single) w.put(k.rev[tok], k.len[tok]);
    w.put(bits, (int)nb);
  }
  void Write(EncBits& w) const {
    w.put(0, 1);                                                     // no LZ77
    if (ctx_map.size() > 1) WriteContextMap(w);
    w.put(1, 1);                                                     // prefix codes: log_alpha_size is 15
    for (size_t c = 0; c < clusters.size(); c++) WriteUintConfig420(w);
    for (const Cluster& k : clusters) WriteVarLenUint16(w, (uint32_t)k.len.size() - 1);
    for (const Cluster& k : clusters) WritePrefixCodeDescription(w, k.len, (int)k.len.size());
  }
  void WriteContextMap(EncBits& w) const {
    const int nc = (int)clusters.size(), bits = nc <= 1 ? 0 : CeilLog2(nc);
    if (bits <= 3 && ctx_map.size() * bits <= 2048) {
      w.put(1, 1); w.put(bits, 2);
      for (uint8_t m : ctx_map) w.put(m, bits);
      return;
    }
    w.put(0, 1); w.put(0, 1);                                        // not simple, no move-to-front: the cluster numbers themselves under a one-context prefix code
    std::vector<Histo> h(1);
    for (uint8_t m : ctx_map) { uint32_t tok, nb, b; EncodeHybrid(m, &tok, &nb, &b); if (h[0].size() <= tok) h[0].resize(tok + 1, 0); h[0][tok]++; }
    PrefixCoder nested;
    nested.Build(h);
    nested.Write(w);
    for (uint8_t m : ctx_map) nested.Put(w, 0, m);
  }
};

// ---- the fixed tree --------------------------------------------------------------------------------------------------------------------------
struct TreeNode { int prop, split, l, r, ctx; };
struct FixedTree {
  std::vector<TreeNode> nodes;
  std::vector<int> bfs;
  int root = 0, num_leaves = 0;
  int Leaf() { nodes.push_back({-1, 0, -1, -1, 0}); return (int)nodes.size() - 1; }
  int Inner(int prop, int split, int l, int r) { nodes.push_back({prop, split, l, r, 0}); return (int)nodes.size() - 1; }      // property > split ? l : r
  int Cutoffs(const int32_t* cut, int lo, int hi) {
    if (lo >= hi) return Leaf();
    const int mid = (lo + hi) / 2, l = Cutoffs(cut, mid + 1, hi), r = Cutoffs(cut, lo, mid);
    return Inner(9, cut[mid], l, r);
  }
  explicit FixedTree(int ntot) {
    static const int32_t cuts[kEncNumCuts] = JXL_ENC_CUTS;
    std::vector<int> sub(ntot);
    for (int c = 0; c < ntot; c++) sub[c] = Cutoffs(cuts, 0, kEncNumCuts);
    root = sub[ntot - 1];
    for (int c = ntot - 2; c >= 0; c--) root = Inner(0, c, root, sub[c]);
    bfs.push_back(root);
    for (size_t i = 0; i < bfs.size(); i++) { const TreeNode& n = nodes[bfs[i]]; if (n.prop >= 0) { bfs.push_back(n.l); bfs.push_back(n.r); } }
    for (int id : bfs) if (nodes[id].prop < 0) nodes[id].ctx = num_leaves++;      // a leaf's context: its number in BFS order
  }
  int Context(int channel, int32_t prop9) const {
    int pos = root;
    while (nodes[pos].prop >= 0) pos = (nodes[pos].prop == 0 ? channel : prop9) > nodes[pos].split ? nodes[pos].l : nodes[pos].r;
    return nodes[pos].ctx;
  }
  void Write(EncBits& w) const {      // tree tokens under their own six-context code
    std::vector<std::pair<uint32_t, uint32_t>> tok;
    for (int id : bfs) {
      const TreeNode& n = nodes[id];
      if (n.prop < 0) { tok.push_back({1, 0}); tok.push_back({2, 5}); tok.push_back({3, 0}); tok.push_back({4, 0}); tok.push_back({5, 0}); }      // leaf: predictor 5, offset 0, multiplier 1
      else { tok.push_back({1, (uint32_t)n.prop + 1}); tok.push_back({0, PackSigned(n.split)}); }
    }
    std::vector<Histo> h(6);
    for (auto& t : tok) { uint32_t s, nb, b; EncodeHybrid(t.second, &s, &nb, &b); if (h[t.first].size() <= s) h[t.first].resize(s + 1, 0); h[t.first][s]++; }
    PrefixCoder code;
    code.Build(h);
    code.Write(w);
    for (auto& t : tok) code.Put(w, t.first, t.second);
  }
};
// bucket b of property 9 (the number of cut-offs below the value) -> context, for the device: [channel count - 1][channel][bucket]
std::vector<uint8_t> LeafContextTable() {
  static const int32_t cuts[kEncNumCuts] = JXL_ENC_CUTS;
  std::vector<uint8_t> t(4 * kEncNumCtx, 0);
  for (int ntot = 1; ntot <= 4; ntot++) {
    const FixedTree tree(ntot);
    for (int c = 0; c < ntot; c++)
      for (int b = 0; b < (int)kEncLeaves; b++) t[(ntot - 1) * kEncNumCtx + c * kEncLeaves + b] = (uint8_t)tree.Context(c, b == 0 ? cuts[0] : cuts[b - 1] + 1);
  }
  return t;
}

// ---- geometry, bound, headers ---------------------------------------------------------------------------------------------------------------
constexpr uint32_t kEncMaxSide = 16384;
struct Geometry {
  uint32_t xg, yg, ngroups, nlf;
  bool single;
  uint32_t toc_entries() const { return single ? 1 : 2 + nlf + ngroups; }
};
Geometry MakeGeometry(uint32_t xs, uint32_t ys) {
  Geometry g;
  g.xg = (xs + kEncGroupDim - 1) / kEncGroupDim; g.yg = (ys + kEncGroupDim - 1) / kEncGroupDim; g.ngroups = g.xg * g.yg;
  g.nlf = ((xs + 2047) / 2048) * ((ys + 2047) / 2048);
  g.single = g.ngroups == 1;
  return g;
}
bool HasRct(uint32_t nch) { return nch >= 3; }
// the largest number of extra bits of a token: residuals are below 2^(bits + 1) in magnitude after the RCT (2^bits without), PackSigned doubles them, and a
// hybrid-uint (4, 2, 0) value of n + 1 bits (n >= 4) has n - 2 extra bits
uint32_t MaxExtraBits(uint32_t bits, bool rct) { const uint32_t n = bits + (rct ? 1 : 0); return n >= 4 ? n - 2 : 0; }
constexpr size_t kBoundHeaders = 48;        // image header (signature, size, bit depth, alpha, colour encoding: < 32 bytes) + frame header (< 8 bytes)
// LfGlobal prefix: tree tokens (at most 95 nodes, 334 tokens of at most 15 + 9 bits: 1002 bytes) + tree code (6 clusters) + context map (48 x 15 bits) + at most 48 codes of
// at most 72 symbols (5 bits each + 18 x 4 bits of code-length code + 32 bits of configuration and alphabet size: 58 bytes) + group header: below 5 KiB
constexpr size_t kBoundGlobal = 8192;
size_t BoundOf(uint32_t xs, uint32_t ys, uint32_t nch, uint32_t bits) {
  const Geometry g = MakeGeometry(xs, ys);
  const uint64_t samples = (uint64_t)xs * ys * nch;
  return kBoundHeaders + kBoundGlobal + 2 + 6 * (size_t)g.toc_entries() + (size_t)((samples * (kEncMaxCodeBits + MaxExtraBits(bits, HasRct(nch))) + 7) / 8);
}

std::string Validate(const JxlHipEncodeImage& im, bool host_only) {
  if (im.xsize == 0 || im.ysize == 0 || im.xsize > kEncMaxSide || im.ysize > kEncMaxSide) return "xsize and ysize must be 1.." + std::to_string(kEncMaxSide);
  if (im.num_channels < 1 || im.num_channels > 4) return "num_channels must be 1..4 (grey, grey + alpha, RGB, RGBA)";
  if (im.bits_per_sample < 1 || im.bits_per_sample > 16) return "bits_per_sample must be 1..16";
  if (im.data_type != JXL_TYPE_UINT8 && im.data_type != JXL_TYPE_UINT16) return "data_type must be JXL_TYPE_UINT8 or JXL_TYPE_UINT16";
  if (im.data_type == JXL_TYPE_UINT8 && im.bits_per_sample > 8) return "data_type does not fit the depth: JXL_TYPE_UINT8 holds at most 8 bits";
  const size_t row = (size_t)im.xsize * im.num_channels * (im.data_type == JXL_TYPE_UINT8 ? 1 : 2);
  if (im.row_pitch != 0 && im.row_pitch < row) return "row_pitch is below one row (" + std::to_string(row) + " bytes)";
  if (!im.pixels) return "pixels is NULL";
  if (host_only && im.on_device) return "a device pointer on a host-only encoder";
  return "";
}

void WriteHeaders(EncBits& w, const JxlHipEncodeImage& im) {
  const uint32_t bits = im.bits_per_sample;
  const bool grey = im.num_channels <= 2, alpha = im.num_channels == 2 || im.num_channels == 4;
  // image header
  w.put(0xFF, 8); w.put(0x0A, 8);
  w.put(0, 1);                                                       // SizeHeader: not small, ratio 0
  WriteU32(w, im.ysize, {9, 1}, {13, 1}, {18, 1}, {30, 1});
  w.put(0, 3);
  WriteU32(w, im.xsize, {9, 1}, {13, 1}, {18, 1}, {30, 1});
  w.put(0, 1);                                                       // ImageMetadata: not all_default
  w.put(0, 1);                                                       // no extra_fields (orientation 1)
  WriteBitDepth(w, bits);
  w.put(bits <= 12 ? 1 : 0, 1);                                      // modular_16bit_buffers: the RCT of deeper samples leaves int16
  WriteU32(w, alpha ? 1 : 0, {0, 0}, {0, 1}, {4, 2}, {12, 1});       // extra channels
  if (alpha) {
    if (bits == 8 && !im.alpha_premultiplied) w.put(1, 1);           // the default alpha channel
    else {
      w.put(0, 1);
      WriteEnum(w, 0);                                               // kAlpha
      WriteBitDepth(w, bits);
      WriteU32(w, 0, {0, 0}, {0, 3}, {0, 4}, {3, 1});                // dim_shift
      WriteU32(w, 0, {0, 0}, {4, 0}, {5, 16}, {10, 48});             // no name
      w.put(im.alpha_premultiplied ? 1 : 0, 1);
    }
  }
  w.put(0, 1);                                                       // not XYB
  w.put(grey ? 0 : 1, 1);                                            // ColourEncoding all_default = sRGB
  if (grey) {
    w.put(0, 1);                                                     // no ICC
    WriteEnum(w, 1);                                                 // grey
    WriteEnum(w, 1);                                                 // D65
    w.put(0, 1);                                                     // no gamma
    WriteEnum(w, 13);                                                // sRGB transfer function
    WriteEnum(w, 1);                                                 // relative
  }
  w.put(0, 2);                                                       // no extensions
  w.put(1, 1);                                                       // default transform data
  w.align();
  // frame header
  w.put(0, 1);                                                       // not all_default
  w.put(0, 2);                                                       // regular frame
  w.put(1, 1);                                                       // Modular
  w.put(0, 2);                                                       // flags 0
  w.put(0, 1);                                                       // no YCbCr
  w.put(0, 2);                                                       // upsampling 1
  if (alpha) w.put(0, 2);
  w.put(1, 2);                                                       // group_size_shift 1
  w.put(0, 2);                                                       // one pass
  w.put(0, 1);                                                       // no crop
  for (int i = 0; i < 1 + (alpha ? 1 : 0); i++) w.put(0, 2);         // blending: replace
  w.put(1, 1);                                                       // is_last
  w.put(0, 2);                                                       // no name
  w.put(0, 1); w.put(0, 1); w.put(0, 2); w.put(0, 2);                // restoration filter: no gaborish, no EPF, no extensions
  w.put(0, 2);                                                       // no extensions
}
void WriteToc(EncBits& w, const std::vector<uint32_t>& sizes) {
  w.put(0, 1);                                                       // not permuted
  w.align();
  for (uint32_t s : sizes) WriteU32(w, s, {10, 0}, {14, 1024}, {22, 17408}, {30, 4211712});
  w.align();
}
// the LfGlobal section up to the first token of GlobalModular
void WriteGlobalPrefix(EncBits& w, const JxlHipEncodeImage& im, const PrefixCoder& code) {
  w.put(1, 1);                                                       // LfChannelDequantization: default
  w.put(1, 1);                                                       // a global tree follows
  FixedTree(im.num_channels).Write(w);
  code.Write(w);
  w.put(1, 1); w.put(1, 1);                                          // GroupHeader: global tree, default weighted-predictor parameters
  const bool rct = HasRct(im.num_channels);
  WriteU32(w, rct ? 1 : 0, {0, 0}, {0, 1}, {4, 2}, {8, 18});
  if (rct) { w.put(0, 2); WriteU32(w, 0, {3, 0}, {6, 8}, {10, 72}, {13, 1096}); WriteU32(w, 6, {0, 6}, {2, 0}, {4, 2}, {6, 10}); }      // RCT from channel 0, type 6
}

// A device buffer the encoder keeps from call to call: it grows on demand (by half again, so that a series of slightly larger calls does not reallocate each time).
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  void Free() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
  void Reserve(size_t n) {
    if (n <= cap && p) return;
    Free();
    const size_t want = std::max<size_t>(n + n / 2, 256);
    if (hipMalloc(&p, want) != hipSuccess) {
      (void)hipGetLastError();
      if (hipMalloc(&p, std::max<size_t>(n, 256)) != hipSuccess) { p = nullptr; (void)hipGetLastError(); throw std::runtime_error("out of device memory (" + std::to_string(n) + " bytes)"); }
      cap = std::max<size_t>(n, 256);
    } else cap = want;
  }
  template <class T> T* as() const { return (T*)p; }
};
// makes `device` current and puts the caller's device back on exit
struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int device) {
    if (hipGetDevice(&prev) != hipSuccess) { (void)hipGetLastError(); prev = -1; }
    if (prev != device) { if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); prev = -1; throw std::runtime_error("hipSetDevice failed"); } } else prev = -1;
  }
  ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};
void Check(hipError_t e, const char* what) { if (e != hipSuccess) { (void)hipGetLastError(); throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e)); } }
double NowMs() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

}  // namespace
}  // namespace jxlhip

using namespace jxlhip;

struct JxlHipEncoderStruct {
  int device = -1;
  struct Result { int status = 1; std::string error = "not encoded"; std::vector<uint8_t> bytes; uint32_t max_token = 0; };
  std::vector<Result> results;
  float phase_ms[JXL_HIP_ENCODE_PHASES] = {0};
  // device buffers, kept between calls
  DevBuf b_stage, b_img, b_sec, b_leaf, b_hist, b_flags, b_codes, b_rows, b_secbytes, b_secoff, b_out;
  bool leaf_uploaded = false;
  hipEvent_t ev_pack0 = nullptr, ev_pack1 = nullptr;

  ~JxlHipEncoderStruct() {
    if (device < 0) return;
    try {
      DeviceGuard guard(device);
      for (DevBuf* b : {&b_stage, &b_img, &b_sec, &b_leaf, &b_hist, &b_flags, &b_codes, &b_rows, &b_secbytes, &b_secoff, &b_out}) b->Free();
      if (ev_pack0) (void)hipEventDestroy(ev_pack0);
      if (ev_pack1) (void)hipEventDestroy(ev_pack1);
    } catch (const std::exception&) {}
  }
  void Encode(const JxlHipEncodeImage* images, size_t n, hipStream_t stream);
};

void JxlHipEncoderStruct::Encode(const JxlHipEncodeImage* images, size_t n, hipStream_t stream) {
  results.assign(n, Result());
  for (float& v : phase_ms) v = 0;
  std::vector<uint32_t> live;                                        // indices of the images that go to the device
  for (size_t i = 0; i < n; i++) {
    const std::string why = Validate(images[i], device < 0);
    if (!why.empty()) results[i].error = "image " + std::to_string(i) + ": " + why;
    else if (device < 0) results[i].error = "image " + std::to_string(i) + ": a host-only encoder cannot encode (it answers bounds and refusals)";
    else live.push_back((uint32_t)i);
  }
  if (live.empty()) return;
  auto fail_live = [&](const std::string& why) { for (uint32_t i : live) { results[i].status = 1; results[i].error = why; results[i].bytes.clear(); } };
  try {
    DeviceGuard guard(device);
    if (!ev_pack0) { Check(hipEventCreate(&ev_pack0), "hipEventCreate"); Check(hipEventCreate(&ev_pack1), "hipEventCreate"); }
    double t0 = NowMs();
    // ---- tables: images, sections, staging of host inputs
    const uint32_t nimg = (uint32_t)live.size();
    std::vector<EncImageDev> dimg(nimg);
    std::vector<EncSectionDev> dsec;
    std::vector<uint32_t> first_sec(nimg + 1, 0);
    std::vector<size_t> stage_off(nimg, 0);
    size_t stage_bytes = 0;
    uint64_t rows = 0;
    for (uint32_t k = 0; k < nimg; k++) {
      const JxlHipEncodeImage& im = images[live[k]];
      EncImageDev& d = dimg[k];
      d.bytes_per_sample = im.data_type == JXL_TYPE_UINT8 ? 1 : 2;
      const size_t row = (size_t)im.xsize * im.num_channels * d.bytes_per_sample;
      d.pitch = im.row_pitch ? im.row_pitch : row;
      d.xsize = im.xsize; d.ysize = im.ysize; d.nch = im.num_channels; d.max_value = (1u << im.bits_per_sample) - 1; d.rct = HasRct(im.num_channels) ? 1 : 0;
      d.src = (const uint8_t*)im.pixels;
      if (!im.on_device) { stage_off[k] = stage_bytes; stage_bytes += (d.pitch * (im.ysize - 1) + row + 255) & ~(size_t)255; }
      const Geometry g = MakeGeometry(im.xsize, im.ysize);
      first_sec[k] = (uint32_t)dsec.size();
      for (uint32_t gi = 0; gi < g.ngroups; gi++) {
        EncSectionDev s;
        s.image = k; s.x0 = (gi % g.xg) * kEncGroupDim; s.y0 = (gi / g.xg) * kEncGroupDim;
        s.w = std::min(kEncGroupDim, im.xsize - s.x0); s.h = std::min(kEncGroupDim, im.ysize - s.y0);
        s.lead_bits = g.single ? 0 : 4; s.lead_value = g.single ? 0 : 3;      // a PassGroup's GroupHeader: global tree, default predictor parameters, no transforms
        s.row_base = (uint32_t)rows;
        rows += (uint64_t)im.num_channels * s.h;
        dsec.push_back(s);
      }
    }
    first_sec[nimg] = (uint32_t)dsec.size();
    if (rows >= (1ull << 32)) throw std::runtime_error("too many rows in one call");
    const uint32_t nsec = (uint32_t)dsec.size();
    if (stage_bytes) {
      b_stage.Reserve(stage_bytes);
      for (uint32_t k = 0; k < nimg; k++) {
        const JxlHipEncodeImage& im = images[live[k]];
        if (im.on_device) continue;
        const size_t row = (size_t)im.xsize * im.num_channels * dimg[k].bytes_per_sample;
        Check(hipMemcpyAsync(b_stage.as<uint8_t>() + stage_off[k], im.pixels, dimg[k].pitch * (im.ysize - 1) + row, hipMemcpyHostToDevice, stream), "upload of the samples");
        dimg[k].src = b_stage.as<uint8_t>() + stage_off[k];
      }
    }
    static const std::vector<uint8_t> leaf_table = LeafContextTable();
    b_img.Reserve(nimg * sizeof(EncImageDev)); b_sec.Reserve(nsec * sizeof(EncSectionDev));
    b_hist.Reserve((size_t)nimg * kEncHistSize * 4); b_flags.Reserve(nimg * 4); b_codes.Reserve((size_t)nimg * kEncHistSize * 4);
    b_rows.Reserve((size_t)rows * 4); b_secbytes.Reserve(nsec * 4); b_secoff.Reserve(((size_t)nsec + 1) * 8);
    if (!leaf_uploaded) {
      b_leaf.Reserve(leaf_table.size());
      Check(hipMemcpyAsync(b_leaf.p, leaf_table.data(), leaf_table.size(), hipMemcpyHostToDevice, stream), "upload");
      leaf_uploaded = true;
    }
    Check(hipMemcpyAsync(b_img.p, dimg.data(), nimg * sizeof(EncImageDev), hipMemcpyHostToDevice, stream), "upload");
    Check(hipMemcpyAsync(b_sec.p, dsec.data(), nsec * sizeof(EncSectionDev), hipMemcpyHostToDevice, stream), "upload");
    Check(hipMemsetAsync(b_hist.p, 0, (size_t)nimg * kEncHistSize * 4, stream), "memset");
    Check(hipMemsetAsync(b_flags.p, 0, nimg * 4, stream), "memset");
    EncPlan plan = {};
    plan.images = b_img.as<EncImageDev>(); plan.sections = b_sec.as<EncSectionDev>(); plan.num_images = nimg; plan.num_sections = nsec;
    plan.leaf_ctx = b_leaf.as<uint8_t>(); plan.hist = b_hist.as<uint32_t>(); plan.flags = b_flags.as<uint32_t>(); plan.codes = b_codes.as<uint32_t>();
    plan.row_off = b_rows.as<uint32_t>(); plan.sec_bytes = b_secbytes.as<uint32_t>(); plan.sec_off = b_secoff.as<uint64_t>();
    Check(hipStreamSynchronize(stream), "upload");
    double t1 = NowMs();
    phase_ms[0] = (float)(t1 - t0);
    // ---- pass 1
    EncLaunchTokenise(plan, stream);
    std::vector<uint32_t> hist((size_t)nimg * kEncHistSize), flags(nimg);
    Check(hipMemcpyAsync(hist.data(), b_hist.p, hist.size() * 4, hipMemcpyDeviceToHost, stream), "histogram readback");
    Check(hipMemcpyAsync(flags.data(), b_flags.p, nimg * 4, hipMemcpyDeviceToHost, stream), "flag readback");
    Check(hipStreamSynchronize(stream), "tokenise");
    t0 = NowMs();
    phase_ms[1] = (float)(t0 - t1);
    // ---- codes and LfGlobal prefixes
    std::vector<EncBits> prefix(nimg);
    std::vector<uint32_t> codes((size_t)nimg * kEncHistSize, 0);
    std::vector<std::string> host_error(nimg);                       // an image whose code build or splice throws fails alone (its code table stays empty: it packs no bits)
    for (uint32_t k = 0; k < nimg; k++) try {
      const JxlHipEncodeImage& im = images[live[k]];
      const uint32_t num_ctx = im.num_channels * kEncLeaves;
      std::vector<Histo> h(num_ctx, Histo(kEncAlphabet, 0));
      const uint32_t* src = &hist[(size_t)k * kEncHistSize];
      for (uint32_t c = 0; c < num_ctx; c++) for (uint32_t s = 0; s < kEncAlphabet; s++) { h[c][s] = src[c * kEncAlphabet + s]; if (src[c * kEncAlphabet + s]) results[live[k]].max_token = std::max(results[live[k]].max_token, s); }
      PrefixCoder code;
      code.Build(h);
      uint32_t* dst = &codes[(size_t)k * kEncHistSize];
      for (uint32_t c = 0; c < num_ctx; c++) {
        const PrefixCoder::Cluster& cl = code.clusters[code.ctx_map[c]];
        for (uint32_t s = 0; s < kEncAlphabet && s < cl.len.size(); s++) if (!cl.single) dst[c * kEncAlphabet + s] = (uint32_t)cl.rev[s] | ((uint32_t)cl.len[s] << 16);
      }
      WriteGlobalPrefix(prefix[k], im, code);
      if (first_sec[k + 1] - first_sec[k] == 1) dsec[first_sec[k]].lead_bits = (uint32_t)(prefix[k].bits() & 7);      // single section: the tokens follow the prefix bit for bit
    } catch (const std::exception& e) {
      host_error[k] = e.what();
      std::fill(codes.begin() + (size_t)k * kEncHistSize, codes.begin() + (size_t)(k + 1) * kEncHistSize, 0u);
    }
    Check(hipMemcpyAsync(b_codes.p, codes.data(), codes.size() * 4, hipMemcpyHostToDevice, stream), "upload of the codes");
    Check(hipMemcpyAsync(b_sec.p, dsec.data(), nsec * sizeof(EncSectionDev), hipMemcpyHostToDevice, stream), "upload");
    t1 = NowMs();
    phase_ms[2] = (float)(t1 - t0);
    // ---- pass 2
    EncLaunchCount(plan, stream);
    std::vector<uint32_t> sec_bytes(nsec);
    std::vector<uint64_t> sec_off((size_t)nsec + 1);
    Check(hipMemcpyAsync(sec_bytes.data(), b_secbytes.p, nsec * 4, hipMemcpyDeviceToHost, stream), "size readback");
    Check(hipMemcpyAsync(sec_off.data(), b_secoff.p, ((size_t)nsec + 1) * 8, hipMemcpyDeviceToHost, stream), "size readback");
    Check(hipStreamSynchronize(stream), "count");
    t0 = NowMs();
    phase_ms[3] = (float)(t0 - t1);
    // ---- pass 3
    const uint64_t total = sec_off[nsec];
    uint64_t check = 0;
    for (uint32_t s = 0; s < nsec; s++) { if (sec_off[s] != check) throw std::runtime_error("section offsets do not add up"); check += sec_bytes[s]; }
    if (check != total) throw std::runtime_error("section offsets do not add up");
    plan.out_words = (total + 3) / 4 + 1;
    b_out.Reserve(plan.out_words * 4);
    plan.out = b_out.as<uint32_t>();
    Check(hipEventRecord(ev_pack0, stream), "hipEventRecord");
    Check(hipMemsetAsync(b_out.p, 0, plan.out_words * 4, stream), "memset");
    EncLaunchPack(plan, stream);
    Check(hipEventRecord(ev_pack1, stream), "hipEventRecord");      // (pack and the copy back are one stretch of the stream: events split their times, not a synchronisation)
    std::vector<uint8_t> packed(total);
    if (total) Check(hipMemcpyAsync(packed.data(), b_out.p, total, hipMemcpyDeviceToHost, stream), "readback of the sections");
    Check(hipMemcpyAsync(flags.data(), b_flags.p, nimg * 4, hipMemcpyDeviceToHost, stream), "flag readback");
    Check(hipStreamSynchronize(stream), "pack and readback");
    t1 = NowMs();
    Check(hipEventElapsedTime(&phase_ms[4], ev_pack0, ev_pack1), "hipEventElapsedTime");
    phase_ms[5] = std::max(0.0f, (float)(t1 - t0) - phase_ms[4]);
    t0 = t1;
    // ---- splice
    for (uint32_t k = 0; k < nimg; k++) try {
      const JxlHipEncodeImage& im = images[live[k]];
      Result& r = results[live[k]];
      if (!host_error[k].empty()) { r.error = "image " + std::to_string(live[k]) + ": internal error: " + host_error[k]; continue; }
      if (flags[k] & kEncFlagRange) { r.error = "image " + std::to_string(live[k]) + ": a sample is above 2^bits_per_sample - 1"; continue; }
      if (flags[k] & kEncFlagPack) { r.error = "image " + std::to_string(live[k]) + ": internal error: the pack pass left its section"; continue; }
      const Geometry g = MakeGeometry(im.xsize, im.ysize);
      EncBits w;
      WriteHeaders(w, im);
      EncBits& pre = prefix[k];
      const uint32_t s0 = first_sec[k];
      if (g.single) {
        const size_t whole = pre.bits() / 8;
        const uint8_t partial = (uint8_t)pre.acc;                   // the prefix's last, incomplete byte (0 if none)
        const uint32_t nb = sec_bytes[s0];
        WriteToc(w, {(uint32_t)(whole + std::max<uint32_t>(nb, pre.nacc ? 1 : 0))});
        w.bytes.insert(w.bytes.end(), pre.bytes.begin(), pre.bytes.begin() + whole);
        if (nb) { const size_t at = w.bytes.size(); w.bytes.insert(w.bytes.end(), packed.begin() + sec_off[s0], packed.begin() + sec_off[s0] + nb); w.bytes[at] |= partial; }
        else if (pre.nacc) w.bytes.push_back(partial);
      } else {
        pre.align();
        std::vector<uint32_t> sizes;
        sizes.push_back((uint32_t)pre.bytes.size());
        for (uint32_t i = 0; i < g.nlf + 1; i++) sizes.push_back(0);  // LfGroups, HfGlobal: empty
        for (uint32_t gi = 0; gi < g.ngroups; gi++) sizes.push_back(sec_bytes[s0 + gi]);
        WriteToc(w, sizes);
        w.bytes.insert(w.bytes.end(), pre.bytes.begin(), pre.bytes.end());
        w.bytes.insert(w.bytes.end(), packed.begin() + sec_off[s0], packed.begin() + sec_off[s0 + g.ngroups]);
      }
      r.bytes.swap(w.bytes);
      r.status = 0; r.error.clear();
    } catch (const std::exception& e) {
      results[live[k]].status = 1; results[live[k]].error = "image " + std::to_string(live[k]) + ": internal error: " + e.what(); results[live[k]].bytes.clear();
    }
    phase_ms[6] = (float)(NowMs() - t0);
  } catch (const std::exception& e) {
    (void)hipStreamSynchronize(stream);
    fail_live(std::string("lossless encode: ") + e.what());
  }
}

extern "C" {

JxlHipEncoder* JxlHipEncoderCreate(int device) {
  if (device >= 0) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device >= count) { (void)hipGetLastError(); SetLastErrorText("JxlHipEncoderCreate: no such HIP device"); return nullptr; }
  }
  JxlHipEncoder* e = new JxlHipEncoderStruct();
  e->device = device < 0 ? -1 : device;
  return e;
}
void JxlHipEncoderDestroy(JxlHipEncoder* enc) { delete enc; }

int JxlHipEncodeLosslessBound(const JxlHipEncodeImage* image, size_t* bytes) {
  if (!image || !bytes) { SetLastErrorText("JxlHipEncodeLosslessBound: NULL argument"); return 1; }
  JxlHipEncodeImage probe = *image;
  static const uint8_t dummy = 0;
  probe.pixels = &dummy; probe.on_device = 0;                        // (the bound does not look at the samples)
  const std::string why = Validate(probe, false);
  if (!why.empty()) { SetLastErrorText("JxlHipEncodeLosslessBound: " + why); return 1; }
  *bytes = BoundOf(image->xsize, image->ysize, image->num_channels, image->bits_per_sample);
  return 0;
}

int JxlHipEncoderEncodeLossless(JxlHipEncoder* enc, const JxlHipEncodeImage* images, size_t num_images, void* hip_stream) {
  if (!enc || (!images && num_images)) { SetLastErrorText("JxlHipEncoderEncodeLossless: NULL argument"); return 1; }
  try { enc->Encode(images, num_images, (hipStream_t)hip_stream); }
  catch (const std::exception& e) { SetLastErrorText(std::string("JxlHipEncoderEncodeLossless: ") + e.what()); return 1; }
  for (const auto& r : enc->results) if (r.status) { SetLastErrorText(r.error); return 1; }
  return 0;
}

int JxlHipEncoderStatus(JxlHipEncoder* enc, size_t index) {
  if (!enc || index >= enc->results.size()) { SetLastErrorText("JxlHipEncoderStatus: no such image"); return 1; }
  if (enc->results[index].status) SetLastErrorText(enc->results[index].error);
  return enc->results[index].status;
}
size_t JxlHipEncoderSize(JxlHipEncoder* enc, size_t index) {
  if (!enc || index >= enc->results.size() || enc->results[index].status) return 0;
  return enc->results[index].bytes.size();
}
int JxlHipEncoderCopy(JxlHipEncoder* enc, size_t index, uint8_t* dst, size_t capacity) {
  if (!enc || index >= enc->results.size()) { SetLastErrorText("JxlHipEncoderCopy: no such image"); return 1; }
  const auto& r = enc->results[index];
  if (r.status) { SetLastErrorText(r.error); return 1; }
  if (!dst || capacity < r.bytes.size()) { SetLastErrorText("JxlHipEncoderCopy: the buffer is too small (" + std::to_string(r.bytes.size()) + " bytes needed)"); return 1; }
  memcpy(dst, r.bytes.data(), r.bytes.size());
  return 0;
}
uint32_t JxlHipEncoderMaxToken(JxlHipEncoder* enc, size_t index) {
  if (!enc || index >= enc->results.size()) return 0;
  return enc->results[index].max_token;
}
void JxlHipEncoderPhaseTimes(JxlHipEncoder* enc, float* ms) {
  if (!enc || !ms) return;
  for (int i = 0; i < JXL_HIP_ENCODE_PHASES; i++) ms[i] = enc->phase_ms[i];
}

}  // extern "C"
