// jxlsynth — "scripted" Modular streams (fixture generator; NOT on the product decode path, independent of oracle/).
// Like the free-running writer (synth_free.h) this one simulates nothing: every context of a stream maps to ONE histogram, so any token
// sequence is a valid stream.  Unlike it, nothing is random: the caller gives the geometry, the global and the local transform list, the MA
// tree node by node and, per channel of the CODED channel list, the value every token carries (the residual the decoder multiplies, offsets
// and adds to its prediction).  A test that restates the decoder's integer arithmetic can therefore say what the image must be.
//
// The coded channel list (what the planes are given for, in this order):
//   1. the image's channels (nchan colour + alpha) after the global transforms, meta channels (palettes, nb_colors x num_c) first — the
//      leading channels that the GlobalModular section carries: every meta channel and every following channel that fits one group;
//   2. the others ride in the PassGroup sections.  Without local transforms: one plane of the image's size each, cut into the group
//      rectangles here.  With local transforms the list of a section stream is what they make of those channels: first the local meta
//      channels (a local palette, nb_colors x num_c — ONE plane, written into every section stream alike), then the remaining channels as
//      planes of the image's size, cut into rectangles.
// Weighted-predictor headers: one for the GlobalModular stream (gwp) and one that every section stream carries (swp); the two may differ.
// Squeeze (transform id 2) in the global list only, as explicit steps or as the default chain, and only for images of at most one group: every
// channel the Squeeze leaves then rides in GlobalModular, residual channels of width or height 0 included (they carry no token; their plane is
// empty).  A Squeeze transform is written as a run of entries: the first {2, begin_c, num_c, horizontal, in_place, 0}, every further step of the
// same transform with d = 1; {2, 0, 0, 0, 0, 0} is the default chain (zero explicit steps: the decoder derives it from the channel list).
// Out of scope: local Squeeze, Squeeze of images larger than a group (section routing by shift), Squeeze over meta channels, LZ77, several frames.
#pragma once

namespace synth {

struct ScriptTransform { int id, begin_c, a, b, c, d; };   // id 0 RCT: a = rct_type;  id 1 palette: a = num_c, b = nb_colors, c = nb_deltas, d = predictor
                                                           // id 2 Squeeze step: a = num_c (0: default chain), b = horizontal, c = in_place, d = 1: continues the transform before
struct ScriptWp { int custom = 0, p1 = 16, p2 = 10, p3[5] = {7, 7, 7, 0, 0}, w[4] = {13, 12, 12, 12}; };   // custom = 0: the header says "all default"
struct ScriptChan { int w, h; bool meta; };
struct ScriptParams {
  int w = 0, h = 0, bits = 8, nchan = 3, has_alpha = 0, group_shift = 1;
  int local_tree = 0;                        // 1: no global tree; every stream (the global one too) carries the tree and a code of its own
  ScriptWp gwp, swp;                         // weighted-predictor header of the GlobalModular stream / of every section stream
  std::vector<ScriptTransform> global_t, local_t;
  GTree tree;                                // node 0 is the root; an inner node goes to `l` when property > split
  std::vector<const int32_t*> planes;        // the coded channel list (above)
  std::vector<std::pair<int, int>> dims;     // (w, h) of every plane, as the caller believes them to be
};

namespace script_detail {

inline void Fail(const std::string& m) { throw std::runtime_error("scripted stream: " + m); }

// transform.cc MetaApply on a list of channel sizes; `where` names the list in messages
inline void MetaApply(std::vector<ScriptChan>& ch, int& nmeta, const ScriptTransform& t, const char* where, bool local) {
  const int n = (int)ch.size();
  if (t.id == 0) {
    if (t.a < 0 || t.a >= 42) Fail(std::string(where) + " RCT type out of range");
    if (t.begin_c < nmeta || t.begin_c + 3 > n) Fail(std::string(where) + " RCT does not cover three non-meta channels");
    for (int k = 1; k < 3; k++) if (ch[t.begin_c + k].w != ch[t.begin_c].w || ch[t.begin_c + k].h != ch[t.begin_c].h) Fail(std::string(where) + " RCT over channels of different size");
    return;
  }
  if (t.id == 2) {
    if (local) Fail("Squeeze in a section stream: the GPU decoder's section parser takes none (test_squeeze_over_passes covers squeezed sections)");
    if (nmeta) Fail("Squeeze after a palette is out of scope");
    std::vector<SqStep> steps;
    if (t.a == 0) {
      std::vector<SChan> dims;
      for (const ScriptChan& c : ch) dims.push_back(SChan{{}, c.w, c.h, 0, 0});
      steps = DefaultSqueezeSteps(dims);
    } else steps.push_back(SqStep{t.b != 0, t.c != 0, t.begin_c, t.a});
    for (const SqStep& q : steps) {
      const int endc = q.begin_c + q.num_c - 1;
      if (q.begin_c < 0 || q.num_c < 1 || endc >= (int)ch.size()) Fail("Squeeze step out of range");
      const int offset = q.in_place ? endc + 1 : (int)ch.size();
      for (int c = q.begin_c; c <= endc; c++) {
        if (ch[c].w == 0 || ch[c].h == 0) Fail("Squeeze of an empty channel");
        ScriptChan res = ch[c];
        if (q.horizontal) { res.w = ch[c].w / 2; ch[c].w = (ch[c].w + 1) / 2; }
        else { res.h = ch[c].h / 2; ch[c].h = (ch[c].h + 1) / 2; }
        ch.insert(ch.begin() + offset + (c - q.begin_c), res);
      }
    }
    return;
  }
  if (t.id != 1) Fail(std::string(where) + " transform id must be 0 (RCT), 1 (palette) or 2 (Squeeze)");
  const int num_c = t.a, endc = t.begin_c + num_c - 1;
  if (num_c != 1 && num_c != 3 && num_c != 4) Fail(std::string(where) + " palette num_c must be 1, 3 or 4");
  if (t.b < 1 || t.b > 65536 || t.c < 0 || t.d < 0 || t.d >= 14) Fail(std::string(where) + " palette parameters out of range");
  if (t.begin_c < nmeta) Fail(std::string(where) + " palette over meta channels (no decoder here takes one)");
  if (endc >= n) Fail(std::string(where) + " palette channels out of range");
  for (int k = 1; k < num_c; k++) if (ch[t.begin_c + k].w != ch[t.begin_c].w || ch[t.begin_c + k].h != ch[t.begin_c].h) Fail(std::string(where) + " palette over channels of different size");
  if (local && (t.c != 0 || t.d != 0)) Fail("a local palette must be plain (nb_deltas = 0, predictor 0): the GPU decoder takes no other in a section stream");
  ch.erase(ch.begin() + t.begin_c + 1, ch.begin() + endc + 1);
  ch.insert(ch.begin(), ScriptChan{t.b, num_c, true});
  nmeta++;
}

inline void WriteWpHeader(BitWriter& s, const ScriptWp& q) {
  if (!q.custom) { s.put(1, 1); return; }
  if (q.p1 < 0 || q.p1 > 31 || q.p2 < 0 || q.p2 > 31) Fail("weighted-predictor header: p1, p2 must be 0..31");
  for (int i = 0; i < 5; i++) if (q.p3[i] < 0 || q.p3[i] > 31) Fail("weighted-predictor header: p3 must be 0..31");
  for (int i = 0; i < 4; i++) if (q.w[i] < 0 || q.w[i] > 15) Fail("weighted-predictor header: weights must be 0..15");
  s.put(0, 1); s.put((uint32_t)q.p1, 5); s.put((uint32_t)q.p2, 5);
  for (int i = 0; i < 5; i++) s.put((uint32_t)q.p3[i], 5);
  for (int i = 0; i < 4; i++) s.put((uint32_t)q.w[i], 4);
}

inline void WriteTransforms(BitWriter& s, const std::vector<ScriptTransform>& ts) {
  size_t count = 0;
  for (const ScriptTransform& t : ts) count += !(t.id == 2 && t.d == 1);
  WriteU32(s, (uint32_t)count, {0, 0}, {0, 1}, {4, 2}, {8, 18});
  for (size_t i = 0; i < ts.size(); i++) {
    const ScriptTransform& t = ts[i];
    s.put((uint32_t)t.id, 2);
    if (t.id == 2) {                      // the header encoding of EncodeModular: number of steps, then per step horizontal, in_place, begin_c, num_c
      size_t n = t.a == 0 ? 0 : 1;
      while (t.a != 0 && i + n < ts.size() && ts[i + n].id == 2 && ts[i + n].d == 1) n++;
      WriteU32(s, (uint32_t)n, {0, 0}, {4, 1}, {6, 9}, {8, 41});
      for (size_t k = 0; k < n; k++) {
        const ScriptTransform& q = ts[i + k];
        s.put(q.b != 0, 1); s.put(q.c != 0, 1);
        WriteU32(s, (uint32_t)q.begin_c, {3, 0}, {6, 8}, {10, 72}, {13, 1096});
        WriteU32(s, (uint32_t)q.a, {0, 1}, {0, 2}, {0, 3}, {4, 4});
      }
      if (n) i += n - 1;
      continue;
    }
    WriteU32(s, (uint32_t)t.begin_c, {3, 0}, {6, 8}, {10, 72}, {13, 1096});
    if (t.id == 0) WriteU32(s, (uint32_t)t.a, {0, 6}, {2, 0}, {4, 2}, {6, 10});
    else {
      WriteU32(s, (uint32_t)t.a, {0, 1}, {0, 3}, {0, 4}, {13, 1});
      WriteU32(s, (uint32_t)t.b, {8, 0}, {10, 256}, {12, 1280}, {16, 5376});
      WriteU32(s, (uint32_t)t.c, {0, 0}, {8, 1}, {10, 257}, {16, 1281});
      s.put((uint32_t)t.d, 4);
    }
  }
}

}  // namespace script_detail

static std::vector<uint8_t> EncodeModularScripted(const ScriptParams& sp) {
  using namespace script_detail;
  if (sp.w < 1 || sp.h < 1) Fail("empty image");
  if (sp.nchan != 1 && sp.nchan != 3) Fail("nchan must be 1 or 3");
  if (sp.bits != 2 && sp.bits != 8 && sp.bits != 12 && sp.bits != 16) Fail("bit depth must be 2, 8, 12 or 16");
  if (sp.group_shift < 0 || sp.group_shift > 3) Fail("group shift must be 0..3");
  if (sp.global_t.size() > 16 || sp.local_t.size() > 4) Fail("at most 16 global entries (Squeeze steps count) and 4 local transforms");
  for (size_t i = 0; i < sp.global_t.size(); i++) {
    const ScriptTransform& t = sp.global_t[i];
    if (t.id == 2 && t.d == 1 && (i == 0 || sp.global_t[i - 1].id != 2 || sp.global_t[i - 1].a == 0 || t.a == 0)) Fail("a Squeeze step continues nothing");
  }
  const int gd = 128 << sp.group_shift, lfd = gd * 8, w = sp.w, h = sp.h;
  const int xg = (w + gd - 1) / gd, yg = (h + gd - 1) / gd, ngroups = xg * yg;
  const int nlf = ((w + lfd - 1) / lfd) * ((h + lfd - 1) / lfd);
  const int ntot = sp.nchan + (sp.has_alpha ? 1 : 0);
  // ---- the channel lists the decoder will derive
  std::vector<ScriptChan> glist(ntot, ScriptChan{w, h, false});
  int nmeta = 0;
  bool squeezed = false;
  for (const ScriptTransform& t : sp.global_t) { MetaApply(glist, nmeta, t, "global", false); squeezed |= t.id == 2; }
  if (squeezed && (w > gd || h > gd)) Fail("Squeeze needs an image of at most one group: every channel must ride in GlobalModular");
  int nglobal = 0;
  while (nglobal < (int)glist.size() && (nglobal < nmeta || (glist[nglobal].w <= gd && glist[nglobal].h <= gd))) nglobal++;
  std::vector<ScriptChan> llist(glist.begin() + nglobal, glist.end());       // the section streams' channels, at the image's size
  int lmeta = 0;
  if (!sp.local_t.empty() && llist.empty()) Fail("local transforms need channels in the section streams (an image larger than one group)");
  for (const ScriptTransform& t : sp.local_t) MetaApply(llist, lmeta, t, "local", true);
  if (llist.size() > 8) Fail("more than 8 channels in a section stream with local transforms");
  std::vector<ScriptChan> want(glist.begin(), glist.begin() + nglobal);
  want.insert(want.end(), llist.begin(), llist.end());
  if (sp.planes.size() != want.size()) Fail("the coded channel list has " + std::to_string(want.size()) + " channels, " + std::to_string(sp.planes.size()) + " planes given");
  for (size_t i = 0; i < want.size(); i++)
    if (sp.dims[i].first != want[i].w || sp.dims[i].second != want[i].h)
      Fail("plane " + std::to_string(i) + " is " + std::to_string(sp.dims[i].first) + "x" + std::to_string(sp.dims[i].second) + ", the coded channel is " + std::to_string(want[i].w) + "x" + std::to_string(want[i].h));
  // ---- the tree: node 0 is the root, written breadth first
  GTree tree = sp.tree;
  const int nn = (int)tree.nodes.size();
  if (nn < 1) Fail("empty tree");
  for (const TNode& n : tree.nodes) {
    if (n.prop >= 0) { if (n.l <= 0 || n.l >= nn || n.r <= 0 || n.r >= nn || n.prop > 255) Fail("tree: child index or property out of range"); }
    else if (n.pred < 0 || n.pred >= 14 || n.mul_log < 0 || n.mul_log > 30 || n.mul_bits < 0) Fail("tree: leaf out of range");
  }
  std::vector<int> bfs(1, 0);
  for (size_t i = 0; i < bfs.size(); i++) {
    const TNode& n = tree.nodes[bfs[i]];
    if (n.prop >= 0) { bfs.push_back(n.l); bfs.push_back(n.r); }
    if ((int)bfs.size() > nn) Fail("tree: a node is reached twice");
  }
  if ((int)bfs.size() != nn) Fail("tree: unreachable nodes");
  int leaf = 0;
  for (int id : bfs) if (tree.nodes[id].prop < 0) tree.nodes[id].ctx = leaf++;
  tree.num_leaves = leaf;
  // ---- token streams: every token in context 0 (all contexts share one histogram)
  auto push = [](std::vector<Token>& out, const int32_t* p, int pw, int x0, int y0, int rw, int rh) {
    for (int y = 0; y < rh; y++) for (int x = 0; x < rw; x++) out.push_back(Token{0, PackSigned(p[(size_t)(y0 + y) * pw + x0 + x])});
  };
  std::vector<Token> gtok;
  for (int c = 0; c < nglobal; c++) push(gtok, sp.planes[c], want[c].w, 0, 0, want[c].w, want[c].h);
  std::vector<std::vector<Token>> stok(llist.empty() ? 0 : ngroups);
  for (size_t g = 0; g < stok.size(); g++) {
    const int x0 = ((int)g % xg) * gd, y0 = ((int)g / xg) * gd;
    const int rw = std::min(gd, w - x0), rh = std::min(gd, h - y0);
    for (size_t c = 0; c < llist.size(); c++) {
      const int32_t* p = sp.planes[nglobal + c];
      if (llist[c].meta) push(stok[g], p, llist[c].w, 0, 0, llist[c].w, llist[c].h);
      else push(stok[g], p, w, x0, y0, rw, rh);
    }
  }
  auto make_code = [&](const std::vector<const std::vector<Token>*>& ss, EntropyCoder& ec) { BuildEntropyCoder(ss, tree.num_leaves, UintConfig{4, 1, 0}, 1, ec, &LfCodeShape()); };
  auto write_tree_and_code = [&](BitWriter& s, const EntropyCoder& code) {
    std::vector<Token> tt;
    TreeTokens(tree, bfs, tt);
    EntropyCoder tc;
    { std::vector<const std::vector<Token>*> ss{&tt}; BuildEntropyCoder(ss, 6, UintConfig{4, 2, 0}, 6, tc); }
    WriteEntropyCode(s, tc);
    EncodeTokens(s, tc, tt);
    WriteEntropyCode(s, code);
  };
  EntropyCoder gcode;
  if (!sp.local_tree) {
    std::vector<const std::vector<Token>*> ss{&gtok};
    for (auto& t : stok) ss.push_back(&t);
    make_code(ss, gcode);
  }
  auto write_stream = [&](BitWriter& s, const std::vector<ScriptTransform>& ts, const std::vector<Token>& tok, const ScriptWp& wp) {
    s.put(sp.local_tree ? 0 : 1, 1);     // use_global_tree
    WriteWpHeader(s, wp);
    WriteTransforms(s, ts);
    if (sp.local_tree) {
      EntropyCoder lc;
      std::vector<const std::vector<Token>*> ss{&tok};
      make_code(ss, lc);
      write_tree_and_code(s, lc);
      EncodeTokens(s, lc, tok);
    } else EncodeTokens(s, gcode, tok);
  };
  std::vector<BitWriter> sections;
  {
    BitWriter s;
    s.put(1, 1);                         // LfChannelDequantization default
    s.put(sp.local_tree ? 0 : 1, 1);     // a global tree follows
    if (!sp.local_tree) write_tree_and_code(s, gcode);
    write_stream(s, sp.global_t, gtok, sp.gwp);
    sections.push_back(s);
  }
  for (int g = 0; g < nlf; g++) sections.push_back(BitWriter());   // no squeezed channels: ModularLfGroup is empty
  sections.push_back(BitWriter());                                  // HfGlobal slot
  for (int g = 0; g < ngroups; g++) {
    BitWriter s;
    if (!stok.empty()) write_stream(s, sp.local_t, stok[g], sp.swp);
    sections.push_back(s);
  }
  BitWriter out;
  Params p;
  p.out_bits = sp.bits; p.gab = 0; p.epf_iters = 0; p.noise = 0; p.upsampling = 1; p.num_passes = 1; p.skip_lf_smoothing = 0;
  WriteImageHeader(out, w, h, p, false, sp.bits, sp.has_alpha != 0, sp.nchan == 1);
  WriteFrameHeader(out, p, true, false, sp.has_alpha ? 1 : 0, sp.group_shift, false, w, h);
  WriteTOCAndSections(out, sections, ngroups == 1);
  out.align();
  return out.bytes;
}

}  // namespace synth
