// jxlsynth — "scripted" VarDCT coefficient streams (fixture generator; NOT on the product decode path, independent of oracle/).
// The counterpart of synth_script.h for the step between the PassGroup tokens and the quantised coefficient planes.  The writer simulates
// nothing and computes NO context, NO coefficient order and NO non-zero count: the caller gives the block grid (varblocks, quantiser field,
// quantised LF), the block context map, the passes with their shifts, the coefficient orders as permutations, the histogram set of every
// (pass, group), the (context, value) pairs of every PassGroup section, the context map of the AC code and pseudo-counts per cluster.  A test
// that restates the format's context model can therefore say which pairs a given set of coefficients must be coded as — and every decoder has
// to read the coefficients back from exactly those pairs.
// The frame: one XYB VarDCT frame, no gaborish, no EPF, no patches / splines / noise, upsampling 1, chroma-from-luma maps zero, sharpness zero,
// default quantisation tables.  Everything outside the script (frame header, LfGlobal, LfGroups, HfGlobal, TOC) is WriteVarDCTFrame's.
#pragma once

namespace synth {

struct HfScript {
  int w = 0, h = 0;
  struct Vb { int by, bx, strategy, hf_mul; };
  std::vector<Vb> varblocks;
  const int32_t* lfq[3] = {nullptr, nullptr, nullptr};   // X, Y, B: quantised LF per block, row-major over the block grid
  int nctx = 0;                                          // 0: the default block context map; else the number of block contexts of the map below
  std::vector<int32_t> lf_thr[3]; std::vector<uint32_t> qf_thr; std::vector<uint8_t> bcm_map;
  int num_passes = 1, shift[2] = {0, 0};
  std::vector<HfOrders> orders;                          // per pass (used mask + a permutation per set bucket and channel X, Y, B)
  int num_presets = 1; std::vector<int> preset;          // per pass * groups + group
  std::vector<std::vector<Token>> tokens;                // per pass * groups + group; contexts final, in [0, 495 * nctx * num_presets)
  ScriptedAcCode code;
};

static std::vector<uint8_t> EncodeVarDCTScripted(HfScript& sc) {
  auto fail = [](const std::string& m) { throw std::runtime_error("scripted VarDCT stream: " + m); };
  const int w = sc.w, h = sc.h;
  if (w < 1 || h < 1) fail("empty image");
  const int bw = (w + 7) / 8, bh = (h + 7) / 8, ngroups = ((w + 255) / 256) * ((h + 255) / 256);
  if (sc.num_passes < 1 || sc.num_passes > 3) fail("1 to 3 passes");
  for (int i = 0; i + 1 < sc.num_passes; i++) if (sc.shift[i] < 0 || sc.shift[i] > 3) fail("a pass's shift must be 0..3");
  VarDctBody b;
  b.w = b.img_w = w; b.h = b.img_h = h;
  b.strat.assign((size_t)bw * bh, -1); b.first.assign((size_t)bw * bh, 0);
  b.hf_mul.assign((size_t)bw * bh, 1); b.sharp.assign((size_t)bw * bh, 0);
  for (const HfScript::Vb& v : sc.varblocks) {
    if (v.strategy < 0 || v.strategy > 26) fail("strategy out of range");
    if (v.hf_mul < 1 || v.hf_mul > 256) fail("hf_mul must be 1..256");
    const int cx = kCovX[v.strategy], cy = kCovY[v.strategy];
    if (v.bx < 0 || v.by < 0 || v.bx + cx > bw || v.by + cy > bh) fail("a varblock leaves the block grid");
    if ((v.bx % 32) + cx > 32 || (v.by % 32) + cy > 32) fail("a varblock crosses a 256x256 group");
    for (int iy = 0; iy < cy; iy++) for (int ix = 0; ix < cx; ix++) {
      const size_t o = (size_t)(v.by + iy) * bw + v.bx + ix;
      if (b.strat[o] >= 0) fail("varblocks overlap");
      b.strat[o] = (int8_t)v.strategy; b.hf_mul[o] = v.hf_mul;
    }
    b.first[(size_t)v.by * bw + v.bx] = 1;
  }
  for (int8_t s : b.strat) if (s < 0) fail("the varblocks do not tile the block grid");
  for (int c = 0; c < 3; c++) { if (!sc.lfq[c]) fail("no quantised LF plane"); b.lfq[c].assign(sc.lfq[c], sc.lfq[c] + (size_t)bw * bh); }
  const int cw = (bw + 7) / 8, chh = (bh + 7) / 8;
  b.ytox.assign((size_t)cw * chh, 0); b.ytob.assign((size_t)cw * chh, 0);
  bool used_kind[17] = {false};
  for (int8_t s : b.strat) used_kind[kKind[s]] = true;
  for (int k = 0; k < 17; k++) { if (used_kind[k]) b.specs[k] = DefaultSpec(k); else b.specs[k].mode = 0; }
  b.global_scale = 4587;
  b.custom_bcm = sc.nctx != 0;
  b.nctx = sc.nctx ? sc.nctx : 15;
  if (b.custom_bcm) {
    if (sc.nctx < 1 || sc.nctx > 16) fail("1 to 16 block contexts");
    size_t num_lf = 1;
    for (int c = 0; c < 3; c++) { if (sc.lf_thr[c].size() > 15) fail("at most 15 LF thresholds a channel"); num_lf *= sc.lf_thr[c].size() + 1; b.lf_thr[c] = sc.lf_thr[c]; }
    if (sc.qf_thr.size() > 15) fail("at most 15 quantiser thresholds");
    for (uint32_t t : sc.qf_thr) if (t < 1 || t > 299) fail("quantiser threshold out of range");
    const size_t n = 39 * num_lf * (sc.qf_thr.size() + 1);
    if (n > 39 * 64) fail("block context map too large");
    if (sc.bcm_map.size() != n) fail("the block context map must have " + std::to_string(n) + " entries");
    int top = 0;
    for (uint8_t m : sc.bcm_map) top = std::max<int>(top, m);
    if (top + 1 != sc.nctx) fail("the block context map must use block contexts 0 .. nctx - 1");
    b.qf_thr = sc.qf_thr; b.bcm_map = sc.bcm_map;
  }
  const size_t nsec = (size_t)sc.num_passes * ngroups;
  if (sc.num_presets < 1 || sc.num_presets > ngroups) fail("1 .. number of groups histogram sets");
  if (sc.preset.size() != nsec || sc.tokens.size() != nsec) fail("a preset and a token list for every (pass, group)");
  for (int v : sc.preset) if (v < 0 || v >= sc.num_presets) fail("preset out of range");
  if ((int)sc.orders.size() != sc.num_passes) fail("coefficient orders for every pass");
  static const int bucket_size[13] = {64, 64, 256, 1024, 128, 256, 512, 4096, 2048, 16384, 8192, 65536, 32768};
  for (const HfOrders& ho : sc.orders) {
    if (ho.used >> 13) fail("used_orders has 13 bits");
    size_t k = 0;
    for (int bk = 0; bk < 13; bk++) if (ho.used & (1u << bk)) for (int c = 0; c < 3; c++, k++)
      if (k >= ho.perm.size() || ho.perm[k].size() != (size_t)bucket_size[bk]) fail("a permutation of the bucket's size for every set bucket and channel");
    if (k != ho.perm.size()) fail("more permutations than set buckets");
  }
  b.orders = sc.orders;
  b.npresets = sc.num_presets; b.preset = sc.preset;
  b.ac_tok_all = sc.tokens;
  b.code = &sc.code;
  Params p;
  p.gab = 0; p.epf_iters = 0; p.noise = 0; p.upsampling = 1; p.out_bits = 8; p.skip_lf_smoothing = 0;
  p.num_passes = sc.num_passes; p.pass_shift[0] = sc.shift[0]; p.pass_shift[1] = sc.shift[1];
  return WriteVarDCTFrame(b, p, nullptr);
}

}  // namespace synth
