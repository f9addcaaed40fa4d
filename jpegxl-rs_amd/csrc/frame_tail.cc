// jxl-hip: what the host plans and enqueues behind the entropy stages — the Modular tail (sub-streams, inverse transforms, write) and the frame tail of complex images.
#include "decoder.h"
#include "decoder_impl.h"
#include <deque>

namespace jxlhip {

// ---- rules shared by the planners ---------------------------------------------------------------------------------------------------------
// integer samples -> [0, 1]: the factor, or — float samples — the bit counts IntToFloatSample goes by
struct SampleScale { float factor; uint32_t float_bits, float_exp_bits; };
static SampleScale ScaleOf(const BitDepthInfo& d) { return {d.is_float ? 1.0f : 1.0f / (float)((1u << d.bits) - 1), d.is_float ? d.bits : 0, d.exp_bits}; }
// the extra channel the caller's layout takes as alpha: the picked one (OutputSpec::alpha_from_extra), else the first of type alpha; -1: none
static int AlphaExtra(const ImageHeader& ih, int pick) {
  for (size_t k = 0; k < ih.extra.size(); k++) if (pick >= 0 ? (int)k == pick : ih.extra[k].type == 0) return (int)k;
  return -1;
}
// blend mode, alpha channel and clamp as the kernels take them (BlendInfoH, PatchBlendH)
template <class B> static uint32_t PackBlend(const B& b) { return b.mode | (b.alpha_channel << 8) | ((uint32_t)b.clamp << 16); }

// ---- Modular tail --------------------------------------------------------------------------------------------------------------------------
static void CheckModLaunch(const char* what, int kind) {
  static const bool dbg = getenv("JXL_HIP_DEBUG_SYNC") != nullptr;
  if (!dbg) return;
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) fprintf(stderr, "[jxl-hip] launch of %s (%d) rejected: %s\n", what, kind, hipGetErrorString(e));
}

void Batch::RunModOp(int i, const ModOp& op, void* st) {
  auto P = [&](size_t off) { return (int32_t*)(dwork_ + off); };
  CheckModLaunch("Modular tail op before", (int)op.kind);
  switch (op.kind) {
    case ModOp::kRct: LaunchModRct(P(op.in[0]), P(op.in[1]), P(op.in[2]), op.n, op.param, st); break;
    case ModOp::kPalette: {
      int32_t* outs[4] = {nullptr, nullptr, nullptr, nullptr};
      for (uint32_t c = 0; c < op.num_c; c++) outs[c] = P(op.out[c]);
      if (op.nb_deltas == 0 && op.predictor == 0) LaunchModPalette(P(op.in[0]), outs, op.param, op.num_c, op.bits, op.n, st);
      else LaunchModPaletteDelta(P(op.in[0]), outs, op.param, op.num_c, op.bits, op.nb_deltas, op.predictor, op.aw, op.ah, images_[i]->plan.gwp,
                                 op.predictor == 6 ? P(op.wp_scratch) : nullptr, op.wp_stride, st);
      break;
    }
    case ModOp::kSqueeze: LaunchModInvSqueeze(P(op.in[0]), P(op.in[1]), P(op.out[0]), op.param, op.aw, op.ah, op.rw, op.rh, st); break;
    case ModOp::kOutput: {
      ModOutputArgs a;
      memset(&a, 0, sizeof(a));
      a.ncolor = op.num_c;
      for (uint32_t c = 0; c < a.ncolor; c++) a.color[c] = P(op.in[c]);
      a.color_factor = op.color_factor; a.float_bits = op.float_bits; a.float_exp_bits = op.float_exp_bits;
      a.alpha = op.has_alpha ? P(op.in[3]) : nullptr; a.alpha_factor = op.alpha_factor;
      LaunchModOutput(dframes_, i, a, images_[i]->plan.width, images_[i]->plan.height, st);
      break;
    }
  }
}

// Everything Modular after the entropy decode of the global stream: the LfGroup / PassGroup sub-streams, then the
// host-planned inverse transforms (and, for Modular frames, the write stage).
void Batch::EnqueueModularTail(void* stream_v) {
  const int n = (int)images_.size();
  int max_units = 1;
  for (auto& im : images_) max_units = std::max<int>(max_units, (int)im->plan.NumModUnits());
  CheckModLaunch("(before the Modular tail)", -1);
  LaunchModularGroups(dframes_, n, max_units, cfg, stream_v);
  CheckModLaunch("ModularGroupFastKernel", max_units);
  // The inverse transforms of different images are independent chains of latency-bound kernels (an inverse Squeeze step is one thread per row / column walking a recurrence:
  // 32 workgroups for the last step of an 8192 x 8192 channel, ~40 launches per channel).  Images whose chains have the same shape — the frames of a job usually do — go through
  // them together: step k of up to kSqueezeBatch images is ONE launch (blockIdx.y = image).  Side streams per image gave the same overlap and made every later latency-bound
  // decode of the process 1.3-1.6x slower (profiles/r06_notes.md section 12): everything stays on the caller's stream.
  auto P = [&](size_t off) { return (int32_t*)(dwork_ + off); };
  static const bool no_batch = getenv("JXL_HIP_NO_SQUEEZE_BATCH") != nullptr;      // A/B: every image's chain on its own
  vec<int> with_ops;
  for (int i = 0; i < n; i++) if (!mod_ops_[i].empty()) with_ops.push_back(i);
  // groups of images whose chains have the same shape (kind and geometry of every step)
  auto same_shape = [&](int a, int b) {
    const vec<ModOp>& x = mod_ops_[a]; const vec<ModOp>& y = mod_ops_[b];
    if (x.size() != y.size()) return false;
    for (size_t k = 0; k < x.size(); k++)
      if (x[k].kind != y[k].kind || x[k].param != y[k].param || x[k].aw != y[k].aw || x[k].ah != y[k].ah || x[k].rw != y[k].rw || x[k].rh != y[k].rh) return false;
    return true;
  };
  vec<char> done((size_t)n, 0);
  for (int lead : with_ops) {
    if (done[(size_t)lead]) continue;
    vec<int> grp;
    for (int i : with_ops) if (!done[(size_t)i] && (int)grp.size() < kSqueezeBatch && (i == lead || (!no_batch && same_shape(lead, i)))) { grp.push_back(i); done[(size_t)i] = 1; }
    const vec<ModOp>& ops = mod_ops_[lead];
    for (size_t k = 0; k < ops.size(); k++) {
      if (ops[k].kind == ModOp::kSqueeze && grp.size() > 1) {
        CheckModLaunch("Modular tail op before", (int)ops[k].kind);
        SqueezeBatch b;
        memset(&b, 0, sizeof(b));
        for (size_t g = 0; g < grp.size(); g++) { const ModOp& o = mod_ops_[grp[g]][k]; b.avg[g] = P(o.in[0]); b.res[g] = P(o.in[1]); b.out[g] = P(o.out[0]); }
        LaunchModInvSqueezeBatch(b, (int)grp.size(), ops[k].param, ops[k].aw, ops[k].ah, ops[k].rw, ops[k].rh, stream_v);
      } else {
        for (int i : grp) RunModOp(i, mod_ops_[i][k], stream_v);
      }
    }
  }
}

struct Batch::ModChan { size_t off; uint32_t w, h; };      // a channel of the list PlanModularUndo tracks: its plane in the work arena, its size

// Builds the list of kernels that undo the global transforms of Modular image i (transform.cc, reverse order) and feed
// the write stage, tracking the channel list on the host exactly as MetaApply built it; `take` reserves work-arena bytes.
void Batch::PlanModularUndo(int i, const std::function<size_t(size_t)>& take) {
  const ImageEntry& e = *images_[i]; const FramePlan& p = e.plan;
  vec<ModChan> list;
  for (size_t k = 0; k < p.gchannels.size(); k++) list.push_back({mod_plane_offsets_[i][k], p.gchannels[k].w, p.gchannels[k].h});
  vec<ModOp>& ops = mod_ops_[i];
  ops.clear();
  for (int t = (int)p.gtransforms.size() - 1; t >= 0; t--) {
    const TransformDesc& td = p.gtransforms[t];
    if (td.id == 0) {
      if (td.begin_c + 3 > list.size()) throw ParseError("rct range", false);
      const ModChan &a = list[td.begin_c], &b = list[td.begin_c + 1], &c = list[td.begin_c + 2];
      if (a.w != b.w || a.w != c.w || a.h != b.h || a.h != c.h) throw ParseError("rct over channels of different size", false);
      ModOp op; op.kind = ModOp::kRct; op.in[0] = a.off; op.in[1] = b.off; op.in[2] = c.off; op.n = (size_t)a.w * a.h; op.param = td.rct_type;
      ops.push_back(op);
    } else if (td.id == 1) {
      // list[0] = palette, list[begin_c + 1] = index channel -> num_c channels in its place
      if (td.begin_c + 1 >= list.size()) throw ParseError("palette range", false);
      const ModChan idx = list[td.begin_c + 1];
      ModOp op; op.kind = ModOp::kPalette; op.in[0] = list[0].off; op.num_c = td.num_c; op.param = td.nb_colors;
      op.bits = std::min<uint32_t>(e.ih.depth.bits, 24); op.n = (size_t)idx.w * idx.h;
      if (td.num_c > 4) throw ParseError("unsupported: palette with more than 4 channels", true);
      op.out[0] = idx.off;
      for (uint32_t c = 1; c < td.num_c; c++) op.out[c] = take(op.n * 4 + 64);
      op.nb_deltas = td.nb_deltas; op.predictor = td.predictor; op.aw = idx.w; op.ah = idx.h;
      if (td.predictor == 6) { op.wp_stride = 10 * (idx.w + 2); op.wp_scratch = take((size_t)op.wp_stride * 4 * td.num_c); }   // weighted-predictor state per output channel
      ops.push_back(op);
      vec<ModChan> nl;
      for (size_t k = 1; k < list.size(); k++) {
        if (k - 1 == td.begin_c) { for (uint32_t c = 0; c < td.num_c; c++) nl.push_back({op.out[c], idx.w, idx.h}); }
        else nl.push_back(list[k]);
      }
      list.swap(nl);
    } else {
      for (int q = (int)td.squeeze.size() - 1; q >= 0; q--) {
        const SqueezeStep& sq = td.squeeze[q];
        const uint32_t endc = sq.begin_c + sq.num_c - 1;
        const uint32_t offset = sq.in_place ? endc + 1 : (uint32_t)(list.size() + sq.begin_c - endc - 1);
        if (offset + sq.num_c > list.size() || endc >= offset) throw ParseError("squeeze range", false);
        for (uint32_t c = sq.begin_c; c <= endc; c++) {
          const ModChan avg = list[c], res = list[offset + c - sq.begin_c];
          ModOp op; op.kind = ModOp::kSqueeze; op.param = sq.horizontal; op.in[0] = avg.off; op.in[1] = res.off;
          op.aw = avg.w; op.ah = avg.h; op.rw = res.w; op.rh = res.h;
          ModChan out;
          if (sq.horizontal) { if (avg.h != res.h) throw ParseError("squeeze dims", false); out = {0, avg.w + res.w, avg.h}; }
          else { if (avg.w != res.w) throw ParseError("squeeze dims", false); out = {0, avg.w, avg.h + res.h}; }
          out.off = take((size_t)out.w * out.h * 4 + 64);
          op.out[0] = out.off;
          ops.push_back(op);
          list[c] = out;
        }
        list.erase(list.begin() + offset, list.begin() + offset + sq.num_c);
      }
    }
  }
  PlanModularOutput(i, list);
}

// ... and what becomes of the channels once the transforms are undone: the write stage of a Modular frame, the alpha plane of a VarDCT frame's write stage, or —
// frames of complex images — the integer planes the frame tail converts itself (PlanPostOps)
void Batch::PlanModularOutput(int i, const vec<ModChan>& list) {
  const ImageEntry& e = *images_[i]; const FramePlan& p = e.plan;
  ModOp op; op.kind = ModOp::kOutput; op.num_c = p.nb_color_channels;   // (0 for VarDCT frames: only extra channels are Modular)
  if (list.size() < op.num_c + e.ih.extra.size()) throw ParseError("modular channel list", false);
  for (size_t k = 0; k < op.num_c + e.ih.extra.size(); k++)
    if (list[k].w != p.width || list[k].h != p.height) throw ParseError("unsupported: channel of a different size than the image (dim_shift)", true);
  for (uint32_t c = 0; c < op.num_c; c++) op.in[c] = list[c].off;
  const SampleScale cs = ScaleOf(e.ih.depth);
  op.color_factor = cs.factor; op.float_bits = cs.float_bits; op.float_exp_bits = cs.float_exp_bits;
  const int alpha = AlphaExtra(e.ih, images_[pub_[e.pub_index].first_unit]->out.alpha_from_extra);
  if (alpha >= 0) {
    op.has_alpha = true; op.in[3] = list[op.num_c + alpha].off;
    op.alpha_factor = ScaleOf(e.ih.extra[alpha].depth).factor;   // (float alpha: converted in the frame tail)
  }
  if (e.complex) {
    ComplexBufs& cb = cbufs_[i];
    cb.nb_color_int = op.num_c;
    for (uint32_t c = 0; c < op.num_c; c++) cb.color_int[c] = list[c].off;
    cb.ec_int.clear();
    for (size_t k = 0; k < e.ih.extra.size(); k++) cb.ec_int.push_back(list[op.num_c + k].off);
    return;
  }
  if (p.modular) mod_ops_[i].push_back(op);
  else vardct_alpha_[i] = VarDctAlpha{op.has_alpha, op.in[3], op.alpha_factor};   // the VarDCT write stage reads the plane itself
}

// ---- frame tail of complex images -------------------------------------------------------------------------------------------------
// Walks the frames of every complex image in codestream order and records, as closures over device addresses, the kernels
// that turn each frame's planes into the image: dec_cache.cc PreparePipeline's stage order (patches, splines, upsampling,
// noise | save as reference before the colour transform | XYB / YCbCr -> output colour space | blending onto the canvas |
// save as reference | write).  Reference slots are tracked here (frame_header.cc save_as_reference / CanBeReferenced).
// Every recorded op carries the name of its stage (Batch::PostOp); one function per stage, over the two structs below.
namespace {
struct Slot { bool valid = false, before_ct = false; size_t p[3] = {0, 0, 0}; uint32_t stride = 0; vec<size_t> ec; uint32_t ec_stride = 0; uint32_t w = 0, h = 0; };
void FillSlot(Slot& sl, bool before_ct, const size_t p[3], uint32_t stride, const vec<size_t>& ec, uint32_t ec_stride, uint32_t w, uint32_t h) {
  sl.valid = true; sl.before_ct = before_ct; sl.stride = stride; sl.ec_stride = ec_stride; sl.w = w; sl.h = h;
  for (int c = 0; c < 3; c++) sl.p[c] = p[c];
  sl.ec = ec;
}
// channel tables of the frames with extra channels (kernels.h EcChanDev): a frame's table takes its place in the constant arena when the frame's
// plan starts and is filled step by step; the finished tables are copied into the arena once every frame is planned (the end of PlanPostOps)
struct PendingTable { size_t off; vec<EcChanDev> entries; };
}  // namespace

// one complex image: what its frames share
struct Batch::TailImage {
  Arena& arena; std::deque<PendingTable>& tables; const vec<size_t>& up_weights_off;
  const PubImage& pi; const ImageEntry& first; const ImageHeader& ih;
  uint32_t ne;              // extra channels
  bool render_spots;
  Slot slots[4];            // the reference slots
};
// one frame of it on its way through the stages
struct Batch::TailUnit {
  int u; const ImageEntry& e; const FramePlan& p; const ComplexBufs& cb;
  uint32_t cw, ch, fw, fh;                                      // coded size, frame size (after upsampling)
  bool needs_blending;
  size_t cur[3]; uint32_t cur_stride;                          // current planes of the frame: after the restoration filters (VarDCT) / the int -> float conversion (Modular)
  vec<size_t> cur_ec; uint32_t cur_ec_stride;
  vec<EcChanDev>* tbl; size_t o_tab;                            // the frame's channel table (empty without extra channels: the extra-channel steps are skipped) and its place in the constant arena
  EcFrameArgs efa;
  size_t canvas[3]; vec<size_t> canvas_ec; uint32_t canvas_stride, canvas_ec_stride;   // behind the blending stage
  ColorArgs deferred_tf; bool have_deferred_tf;                 // the transfer function, put off behind a spot-colour stage
};

// the write stage's arguments: colour planes, the alpha the caller's layout takes, w x h samples
WriteArgs Batch::TailWriteArgs(const TailImage& im, const size_t p[3], uint32_t stride, const vec<size_t>& ec, uint32_t ec_stride, uint32_t w, uint32_t h) {
  WriteArgs wa;
  memset(&wa, 0, sizeof(wa));
  for (int c = 0; c < 3; c++) wa.p[c] = BigPlane(p[c]);
  wa.stride = stride;
  const int k = AlphaExtra(im.ih, im.first.out.alpha_from_extra);
  if (k >= 0) {
    wa.alpha = BigPlane(ec[k]); wa.alpha_stride = ec_stride;
    wa.unpremul = im.first.out.unpremul_alpha && im.ih.extra[k].alpha_associated && (im.first.out.num_channels == 2 || im.first.out.num_channels == 4);
  }
  wa.img_w = w; wa.img_h = h;
  wa.od = FillOutput(im.first, dwork_, dbig_);
  return wa;
}

// the transfer function that was put off (TailColour), over the planes it ends up on
void Batch::TailDeferredTf(const TailUnit& t, const char* stage, const size_t p[3], uint32_t stride, uint32_t w, uint32_t h) {
  if (!t.have_deferred_tf) return;
  ColorArgs ta = t.deferred_tf;
  for (int c = 0; c < 3; c++) { ta.src[c] = BigPlane(p[c]); ta.dst[c] = BigPlane(p[c]); }
  ta.src_stride = ta.dst_stride = stride; ta.w = w; ta.h = h;
  PostOp(stage, [=](void* st) { LaunchColor(ta, st); });
}

// ---- extra-channel planes beside the colour output (OutputSpec::planes): one more op behind the write stage, over the extra channels of what was just written — the
// canvas planes (TailDeliver) or the frame's own (TailOwnFrame), w x h samples each.  One table entry per request in the constant arena; a resized output takes the plane
// as oriented f32 into its resize source among the pixel planes, from where the plane's one-slot entry of the resample table stores it (Batch::BuildResizeTable).
void Batch::TailPlanes(TailImage& im, const char* stage, const vec<size_t>& ec, uint32_t ec_stride, uint32_t w, uint32_t h) {
  const ImageEntry& first = im.first;
  const OutputPlanes& pl = first.out.planes;
  if (!pl.any()) return;
  vec<EcPlaneOutDev> table(pl.req.size());
  for (size_t k = 0; k < pl.req.size(); k++) {
    if (pl.req[k].index >= ec.size()) throw ParseError("unsupported: extra planes of extra channel " + std::to_string(pl.req[k].index) + ": the image has " + std::to_string(ec.size()) + " extra channels", true);
    EcPlaneOutDev& e = table[k];
    memset(&e, 0, sizeof(e));
    e.src = BigPlane(ec[pl.req[k].index]); e.src_stride = ec_stride;
    if (first.out.resized()) {
      if (k >= first.off_plane_src.size()) throw ParseError("resize source of an extra plane", false);
      e.od.out = dbig_ + first.off_plane_src[k];
      e.od.out_stride = (uint64_t)first.src_w * 4; e.od.out_channels = 1; e.od.out_type = 2; e.od.out_int_mul = 1.0f; e.od.planar = 1;
      e.od.out_orient = first.out.keep_orientation ? 1 : im.ih.orientation; e.od.is_gray = 1;
    } else {
      e.od = FillPlaneOutput(first, k, dwork_);
    }
  }
  EcPlanesOutArgs a;
  memset(&a, 0, sizeof(a));
  a.num_planes = (uint32_t)table.size(); a.w = w; a.h = h;
  const size_t o_tab = im.arena.Put(table.data(), table.size() * sizeof(EcPlaneOutDev));
  plane_outputs_planned_ += (int64_t)table.size();
  PostOp(stage, [=](void* st) { EcPlanesOutArgs b = a; b.table = (const EcPlaneOutDev*)(dconst_ + o_tab); LaunchEcPlanesOut(b, st); });
}

// ---- chroma upsampling, int -> float, the channel table
void Batch::TailToFloat(TailImage& im, TailUnit& t) {
  const FramePlan& p = t.p; const ComplexBufs& cb = t.cb; const ImageHeader& ih = im.ih;
  const uint32_t cw = t.cw, ch = t.ch, cur_stride = t.cur_stride;
  if (p.subsampled) {
    // the subsampled channels sit in the top-left corner of their planes: bring them to full resolution (plane b)
    for (int c = 0; c < 3; c++) {
      if (!p.hs[c] && !p.vs[c]) continue;
      if (cb.pb[c] == (size_t)-1) throw ParseError("chroma upsampling needs the second plane set", false);
      const size_t src = t.cur[c], dst = cb.pb[c];
      const uint32_t chs = p.hs[c], cvs = p.vs[c];
      PostOp("chroma upsampling", [=](void* st) { LaunchChromaUpsample(BigPlane(src), cur_stride, BigPlane(dst), cur_stride, chs, cvs, cw, ch, st); });
      t.cur[c] = dst;
    }
  }
  if (p.modular && ih.xyb_encoded) {
    if (cb.nb_color_int != 3) throw ParseError("XYB Modular frame without three colour channels", false);
    const size_t cy = cb.color_int[0], cx = cb.color_int[1], cbb = cb.color_int[2], d0 = t.cur[0], d1 = t.cur[1], d2 = t.cur[2];
    const float f0 = p.m_lf[0], f1 = p.m_lf[1], f2 = p.m_lf[2];
    PostOp("int to float", [=](void* st) {
      float* dst[3] = {BigPlane(d0), BigPlane(d1), BigPlane(d2)};
      const float fac[3] = {f0, f1, f2};
      LaunchXybModToFloat((const int32_t*)(dwork_ + cy), (const int32_t*)(dwork_ + cx), (const int32_t*)(dwork_ + cbb), cw, dst, cur_stride, cw, ch, fac, st);
    });
  } else if (p.modular) {
    const SampleScale s = ScaleOf(ih.depth);
    for (int c = 0; c < 3; c++) {
      const size_t src = cb.color_int[cb.nb_color_int == 1 ? 0 : c], dst = t.cur[c];
      PostOp("int to float", [=](void* st) { LaunchIntToFloat((const int32_t*)(dwork_ + src), cw, BigPlane(dst), cur_stride, cw, ch, s.factor, st, s.float_bits, s.float_exp_bits); });
    }
  }
  for (uint32_t k = 0; k < im.ne; k++) {
    if (k >= cb.ec_int.size()) throw ParseError("missing extra channel", false);
    const SampleScale s = ScaleOf(ih.extra[k].depth);
    EcChanDev& e = (*t.tbl)[k];
    e.src_int = (const int32_t*)(dwork_ + cb.ec_int[k]); e.plane = BigPlane(cb.ecf[k]); e.factor = s.factor; e.float_bits = s.float_bits; e.float_exp_bits = s.float_exp_bits;
    e.premul = ih.extra[k].alpha_associated ? 1 : 0; e.type = ih.extra[k].type;
    for (int c = 0; c < 4; c++) e.spot[c] = ih.extra[k].spot[c];
    e.fg = e.plane; e.fg_stride = cw;
    t.cur_ec[k] = cb.ecf[k];
  }
  memset(&t.efa, 0, sizeof(t.efa));
  t.efa.num_extra = im.ne; t.efa.w = cw; t.efa.h = ch; t.efa.ow = t.fw; t.efa.oh = t.fh; t.efa.up = p.upsampling;
  const EcFrameArgs efa = t.efa; const size_t o_tab = t.o_tab;
  PostOp("int to float", [=](void* st) { EcFrameArgs a = efa; a.table = EcTable(o_tab); LaunchEcIntToFloat(a, st); });
}

// per 32x32 tile: the placements touching it, in dictionary order
static void PatchTileLists(const vec<PatchEntryDev>& entries, uint32_t cw, uint32_t ch, vec<uint32_t>* start, vec<uint32_t>* flat) {
  const uint32_t tx = (cw + 31) / 32, ty = (ch + 31) / 32;
  vec<vec<uint32_t>> lists((size_t)tx * ty);
  for (uint32_t k = 0; k < entries.size(); k++) {
    const PatchEntryDev& en = entries[k];
    // (sizes are >= 1 and the placement lies inside the frame — checked by the caller; clamped all the same: the lists must not be overrun)
    const uint32_t y1 = std::min(ty - 1, ((uint32_t)en.y + std::max(en.ys, 1u) - 1) / 32), x1 = std::min(tx - 1, ((uint32_t)en.x + std::max(en.xs, 1u) - 1) / 32);
    for (uint32_t yy = (uint32_t)en.y / 32; yy <= y1; yy++)
      for (uint32_t xx = (uint32_t)en.x / 32; xx <= x1; xx++) lists[(size_t)yy * tx + xx].push_back(k);
  }
  start->assign(lists.size() + 1, 0);
  for (size_t t = 0; t < lists.size(); t++) { (*start)[t + 1] = (*start)[t] + (uint32_t)lists[t].size(); flat->insert(flat->end(), lists[t].begin(), lists[t].end()); }
  if (flat->empty()) flat->push_back(0);
}

// ---- patches
void Batch::TailPatches(TailImage& im, TailUnit& t) {
  const FramePlan& p = t.p; const uint32_t ne = im.ne, cw = t.cw, ch = t.ch;
  if (!(p.flags & 2)) return;
  vec<PatchEntryDev> entries;
  vec<PatchEcDev> pec;        // [placement * ne + channel]
  for (const PatchRefH& pr : p.feat.patches) {
    const Slot& sl = im.slots[pr.ref];
    if (!sl.valid) throw ParseError("patch refers to an empty reference slot", false);
    if (!sl.before_ct) throw ParseError("patch refers to a frame saved after the colour transform", false);
    if (pr.xsize == 0 || pr.ysize == 0) throw ParseError("empty patch", false);
    if ((uint64_t)pr.x0 + pr.xsize > sl.w || (uint64_t)pr.y0 + pr.ysize > sl.h) throw ParseError("patch exceeds its reference frame", false);
    for (const PatchPosH& pp : pr.pos) {
      if (pp.x + pr.xsize > cw || pp.y + pr.ysize > ch) throw ParseError("patch exceeds the frame", false);
      PatchEntryDev en;
      memset(&en, 0, sizeof(en));
      for (int c = 0; c < 3; c++) en.src[c] = BigPlane(sl.p[c]) + (size_t)pr.y0 * sl.stride + pr.x0;
      if (sl.ec.size() < ne) throw ParseError("patch source without the extra channels", false);
      if (pp.blend.size() < 1 + ne) throw ParseError("patch blending list", false);
      for (uint32_t k = 0; k < ne; k++) {
        const float* esrc = BigPlane(sl.ec[k]) + (size_t)pr.y0 * sl.ec_stride + pr.x0;
        if (pp.blend[1 + k].alpha_channel >= ne) throw ParseError("patch alpha channel", false);
        pec.push_back(PatchEcDev{esrc, PackBlend(pp.blend[1 + k]), 0});
      }
      if (ne && pp.blend[0].alpha_channel >= ne) throw ParseError("patch alpha channel", false);
      en.src_stride = sl.stride; en.esrc_stride = sl.ec_stride;
      en.x = (int32_t)pp.x; en.y = (int32_t)pp.y; en.xs = pr.xsize; en.ys = pr.ysize;
      en.mode = PackBlend(pp.blend[0]);
      entries.push_back(en);
    }
  }
  if (entries.empty()) return;
  vec<uint32_t> start, flat;
  PatchTileLists(entries, cw, ch, &start, &flat);
  const size_t o_e = im.arena.Put(entries.data(), entries.size() * sizeof(PatchEntryDev)), o_s = im.arena.Put(start.data(), start.size() * 4), o_l = im.arena.Put(flat.data(), flat.size() * 4);
  PatchFrameArgs pa;
  memset(&pa, 0, sizeof(pa));
  for (int c = 0; c < 3; c++) pa.p[c] = BigPlane(t.cur[c]);
  pa.stride = t.cur_stride; pa.ec_stride = t.cur_ec_stride; pa.w = cw; pa.h = ch; pa.num_extra = ne;
  if (t.cb.ec_tmp.size() < ne) throw ParseError("patch planes of the extra channels", false);
  for (uint32_t k = 0; k < ne; k++) (*t.tbl)[k].tmp = BigPlane(t.cb.ec_tmp[k]);
  const size_t o_p = im.arena.Put(pec.data(), pec.size() * sizeof(PatchEcDev)), o_tab = t.o_tab;
  PostOp("patches", [=](void* st) {
    LaunchPatches(pa, EcTable(o_tab), (const PatchEntryDev*)(dconst_ + o_e), (const PatchEcDev*)(dconst_ + o_p), (const uint32_t*)(dconst_ + o_s), (const uint32_t*)(dconst_ + o_l), st);
  });
}

// ---- splines (segments from the host, host_features.cc)
void Batch::TailSplines(TailImage& im, TailUnit& t) {
  if (!(t.p.flags & 16)) return;
  SplineDrawList dl;
  BuildSplineDrawList(t.p.feat, t.p.base_x, t.p.base_b, t.ch, &dl);
  if (dl.segments.empty() || dl.indices.empty()) return;
  const size_t o_g = im.arena.Put(dl.segments.data(), dl.segments.size() * sizeof(SplineSegmentDev)), o_r = im.arena.Put(dl.row_start.data(), dl.row_start.size() * 4),
               o_i = im.arena.Put(dl.indices.data(), dl.indices.size() * 4);
  const size_t c0 = t.cur[0], c1 = t.cur[1], c2 = t.cur[2];
  const uint32_t cw = t.cw, ch = t.ch, cur_stride = t.cur_stride;
  PostOp("splines", [=](void* st) {
    float* pl[3] = {BigPlane(c0), BigPlane(c1), BigPlane(c2)};
    LaunchSplines(pl, cur_stride, cw, ch, (const SplineSegmentDev*)(dconst_ + o_g), (const uint32_t*)(dconst_ + o_r), (const uint32_t*)(dconst_ + o_i), st);
  });
}

// ---- upsampling to the frame size
void Batch::TailUpsample(TailImage& im, TailUnit& t) {
  if (t.p.upsampling <= 1) return;
  const size_t o_w = im.up_weights_off[t.u], o_tab = t.o_tab;
  const uint32_t up = t.p.upsampling, cw = t.cw, ch = t.ch, fw = t.fw, fh = t.fh;
  for (int c = 0; c < 3; c++) {
    const size_t src = t.cur[c], dst = t.cb.up[c]; const uint32_t ss = t.cur_stride;
    PostOp("upsampling", [=](void* st) { LaunchUpsamplePlane(BigPlane(src), ss, cw, ch, BigPlane(dst), fw, fw, fh, up, (const float*)(dconst_ + o_w), st); });
    t.cur[c] = dst;
  }
  for (uint32_t k = 0; k < im.ne; k++) {
    EcChanDev& e = (*t.tbl)[k];
    e.up = BigPlane(t.cb.up_ec[k]); e.fg = e.up; e.fg_stride = fw;
    t.cur_ec[k] = t.cb.up_ec[k];
  }
  const EcFrameArgs efa = t.efa;
  PostOp("upsampling", [=](void* st) { EcFrameArgs a = efa; a.table = EcTable(o_tab); a.up_weights = (const float*)(dconst_ + o_w); LaunchEcUpsample(a, st); });
  t.cur_stride = fw; t.cur_ec_stride = fw;
}

// ---- noise
void Batch::TailNoise(TailUnit& t) {
  const FramePlan& p = t.p;
  if (!p.feat.has_noise) return;
  NoiseArgs na;
  memset(&na, 0, sizeof(na));
  for (int c = 0; c < 3; c++) { na.p[c] = BigPlane(t.cur[c]); na.noise[c] = BigPlane(t.cb.noise[c]); }
  na.stride = t.cur_stride; na.w = t.fw; na.h = t.fh; na.noise_stride = t.fw; na.group_dim = p.group_dim;
  na.visible_frame_index = t.e.visible_frame_index; na.nonvisible_frame_index = t.e.nonvisible_frame_index;
  for (int k = 0; k < 8; k++) na.lut[k] = p.feat.noise_lut[k];
  na.ytox = p.base_x; na.ytob = p.base_b;
  PostOp("noise", [=](void* st) { LaunchNoise(na, st); });
}

// ---- an LF frame (this batch is another batch's lf_batch_): its planes, before any colour transform, are the LF image of the frame that refers to it
void Batch::TailLfHandOver(TailUnit& t) {
  const int pub = t.e.pub_index;
  const size_t s0 = t.cur[0], s1 = t.cur[1], s2 = t.cur[2];
  const uint32_t cur_stride = t.cur_stride;
  PostOp("LF-frame hand-over", [=](void* st) {
    if ((size_t)pub >= lf_targets_.size() || !lf_targets_[pub].dst[0]) return;
    const LfTarget& tg = lf_targets_[pub];
    const size_t src[3] = {s0, s1, s2};
    for (int c = 0; c < 3; c++)
      HIP_CHECK(hipMemcpy2DAsync(tg.dst[c], (size_t)tg.pitch * 4, BigPlane(src[c]), (size_t)cur_stride * 4, (size_t)tg.w * 4, tg.h, hipMemcpyDeviceToDevice, (hipStream_t)st));
  });
}

// ---- colour transform into the output space
void Batch::TailColour(TailImage& im, TailUnit& t) {
  const FramePlan& p = t.p;
  const bool spot_after_linear = im.render_spots && p.is_last && !t.needs_blending;
  ColorArgs ca;
  memset(&ca, 0, sizeof(ca));
  ca.w = t.fw; ca.h = t.fh; ca.src_stride = t.cur_stride;
  ca.mode = im.ih.xyb_encoded ? 0 : p.do_ycbcr ? 1 : 2;
  const bool separate = t.cb.rgb[0] != (size_t)-1;
  // An image that is not XYB on its way to a requested encoding (OutputSpec::color_non_xyb): the conversion applies to the finished picture — blending and spot colours
  // work on the image's own samples —, so it rides behind them like the transfer function put off for a spot-colour stage; a last frame that is the picture by itself
  // takes it in this launch
  const bool converts = ca.mode != 0 && ConvertsNonXyb(im.ih, im.first.out);
  const bool convert_here = converts && p.is_last && !t.needs_blending && !im.render_spots;
  if (converts && !convert_here) {
    t.deferred_tf = ca; t.deferred_tf.mode = 2;
    FillColourConversion(im.ih, im.first.out, &t.deferred_tf);
    t.have_deferred_tf = true;
  }
  if (ca.mode == 2 && !separate && !convert_here) return;
  for (int c = 0; c < 3; c++) { ca.src[c] = BigPlane(t.cur[c]); ca.dst[c] = separate ? BigPlane(t.cb.rgb[c]) : BigPlane(t.cur[c]); }
  ca.dst_stride = separate ? t.fw : t.cur_stride;
  FrameDev fd;
  ImageHeader colour_store;
  FillColor(ColourHeader(im.ih, im.first.out, &colour_store), p.do_ycbcr, fd);
  for (int k = 0; k < 9; k++) ca.opsin_inv[k] = fd.opsin_inv[k];
  for (int k = 0; k < 3; k++) { ca.neg_bias[k] = fd.neg_bias[k]; ca.neg_bias_cbrt[k] = fd.neg_bias_cbrt[k]; }
  ca.tf_kind = fd.color_mode;
  for (int k = 0; k < 5; k++) ca.hdr_par[k] = fd.hdr_par[k];
  ca.inverse_gamma = fd.inverse_gamma;
  if (convert_here) FillColourConversion(im.ih, im.first.out, &ca);
  // spot colours are mixed in linear light when the frame goes straight to the output (dec_cache.cc PreparePipeline: XYB stage,
  // [from-linear + blending], spot stage, from-linear): the transfer function then follows the spot stage
  if (spot_after_linear && ca.mode == 0) { t.deferred_tf = ca; t.deferred_tf.mode = 3; ca.tf_kind = 1; t.have_deferred_tf = true; }
  PostOp("colour transform", [=](void* st) { LaunchColor(ca, st); });
  if (separate) { for (int c = 0; c < 3; c++) t.cur[c] = t.cb.rgb[c]; t.cur_stride = t.fw; }
}

// ---- non-coalesced output (JxlDecoderSetCoalescing(false)): this frame's own pixels after the colour transform, frame-sized, not
// blended; the frames before it have been composed as usual (it may draw patches from them), the ones after it are not needed
void Batch::TailOwnFrame(TailImage& im, TailUnit& t) {
  const WriteArgs wa = TailWriteArgs(im, t.cur, t.cur_stride, t.cur_ec, t.cur_ec_stride, t.fw, t.fh);
  TailDeferredTf(t, "own-frame output", t.cur, t.cur_stride, t.fw, t.fh);          // (the transfer function had been put off for a spot-colour stage this output does not run)
  PostOp("own-frame output", [=](void* st) { LaunchWrite(wa, st); });
  TailPlanes(im, "own-frame output", t.cur_ec, t.cur_ec_stride, t.fw, t.fh);
}

static const Slot* BlendSource(const Slot* slots, const ImageHeader& ih, uint32_t idx) {
  const Slot& sl = slots[idx];
  if (!sl.valid) return nullptr;
  if (sl.before_ct) throw ParseError("blending source was saved before the colour transform", false);
  if (sl.w != ih.xsize || sl.h != ih.ysize) throw ParseError("blending source has the wrong size", false);
  return &sl;
}

// ---- blending onto the canvas
void Batch::TailBlend(TailImage& im, TailUnit& t) {
  const FramePlan& p = t.p; const ImageHeader& ih = im.ih; const uint32_t ne = im.ne;
  if (!t.needs_blending) {
    if (t.fw != ih.xsize || t.fh != ih.ysize) throw ParseError("frame size differs from the image size without a crop", false);
    for (int c = 0; c < 3; c++) t.canvas[c] = t.cur[c];
    t.canvas_ec = t.cur_ec;
    t.canvas_stride = t.cur_stride; t.canvas_ec_stride = t.cur_ec_stride;
    return;
  }
  BlendArgs ba;
  memset(&ba, 0, sizeof(ba));
  for (int c = 0; c < 3; c++) { ba.fg[c] = BigPlane(t.cur[c]); ba.canvas[c] = BigPlane(t.cb.canvas[c]); }
  ba.fg_stride = t.cur_stride; ba.fw = t.fw; ba.fh = t.fh; ba.x0 = p.x0; ba.y0 = p.y0;
  ba.canvas_stride = ih.xsize; ba.img_w = ih.xsize; ba.img_h = ih.ysize; ba.num_extra = ne;
  const Slot* bg = BlendSource(im.slots, ih, p.blend.source);
  if (bg) { for (int c = 0; c < 3; c++) ba.bg[c] = BigPlane(bg->p[c]); ba.bg_stride = bg->stride; }
  ba.mode = PackBlend(p.blend);
  if (p.blend.mode == 2 || p.blend.mode == 3) {
    if (ne == 0) throw ParseError("alpha blending without extra channels", false);
    if (p.blend.alpha_channel >= ne) throw ParseError("blend alpha channel", false);
    if (bg) { ba.bg_alpha = BigPlane(bg->ec.at(p.blend.alpha_channel)); ba.bg_alpha_stride = bg->ec_stride; }
  }
  for (uint32_t k = 0; k < ne; k++) {
    const BlendInfoH& bi = p.ec_blend[k];
    if (bi.alpha_channel >= ne) throw ParseError("blend alpha channel", false);
    const Slot* eb = BlendSource(im.slots, ih, bi.source);
    if (eb && eb->ec.size() < ne) throw ParseError("blending source without the extra channels", false);
    EcChanDev& e = (*t.tbl)[k];
    e.mode = PackBlend(bi); e.canvas = BigPlane(t.cb.canvas_ec[k]); e.canvas_stride = ih.xsize;
    if (eb) { e.bg = BigPlane(eb->ec[k]); e.bg_alpha = BigPlane(eb->ec[bi.alpha_channel]); e.bg_stride = eb->ec_stride; }
  }
  const size_t o_tab = t.o_tab;
  PostOp("blending", [=](void* st) { LaunchBlend(ba, EcTable(o_tab), st); });
  for (int c = 0; c < 3; c++) t.canvas[c] = t.cb.canvas[c];
  t.canvas_ec = t.cb.canvas_ec;
  t.canvas_stride = ih.xsize; t.canvas_ec_stride = ih.xsize;
}

// ---- delivery: spot colours, the deferred transfer function, the write stage (slot: which of the kept canvases of an animation decoded once, else -1)
void Batch::TailDeliver(TailImage& im, TailUnit& t, int slot) {
  const ImageHeader& ih = im.ih;
  const bool all_frames = !im.first.deliver_frames.empty();
  // (delivery must leave the canvas as it is: the frames behind blend onto it)
  if (all_frames && (im.render_spots || t.have_deferred_tf)) throw ParseError("unsupported: all frames of an animation in one decode with spot colours to render", true);
  // spot colours (stage_spot.cc): colour = mix * spot + (1 - mix) * colour with mix = solidity * channel, channel by channel
  if (im.render_spots) {
    const size_t c0 = t.canvas[0], c1 = t.canvas[1], c2 = t.canvas[2], o_tab = t.o_tab;
    const uint32_t use_canvas = t.needs_blending ? 1 : 0, iw = ih.xsize, ihh = ih.ysize, ne = im.ne, canvas_stride = t.canvas_stride;
    PostOp("delivery", [=](void* st) { float* pl[3] = {BigPlane(c0), BigPlane(c1), BigPlane(c2)}; LaunchSpot(pl, canvas_stride, EcTable(o_tab), ne, use_canvas, iw, ihh, st); });
  }
  TailDeferredTf(t, "delivery", t.canvas, t.canvas_stride, ih.xsize, ih.ysize);
  WriteArgs wa = TailWriteArgs(im, t.canvas, t.canvas_stride, t.canvas_ec, t.canvas_ec_stride, ih.xsize, ih.ysize);
  if (all_frames) wa.od.out += (size_t)slot * (im.first.out_size + 64);
  PostOp("delivery", [=](void* st) { LaunchWrite(wa, st); });
  TailPlanes(im, "delivery", t.canvas_ec, t.canvas_ec_stride, ih.xsize, ih.ysize);      // (never with kept canvases: SetOutputAllFrames refuses planes)
}

void Batch::PlanPostOps(HostStage& hconst, const vec<size_t>& up_weights_off) {
  Arena arena(hconst);
  std::deque<PendingTable> tables;
  plane_outputs_planned_ = 0;
  for (const PubImage& pi : pub_) {
    if (!pi.complex) continue;
    const ImageEntry& first = *images_[pi.first_unit];
    const ImageHeader& ih = first.ih;
    bool has_spot = false;
    for (const ExtraChannel& ec : ih.extra) has_spot |= ec.type == 2;
    TailImage im{arena, tables, up_weights_off, pi, first, ih, (uint32_t)ih.extra.size(), has_spot && first.out.render_spotcolors, {}};
    for (int u = pi.first_unit; u < pi.first_unit + pi.num_units; u++) {
      const FramePlan& p = images_[u]->plan;
      bool blends = p.have_crop || p.blend.mode != 0;
      for (auto& b : p.ec_blend) if (b.mode != 0) blends = true;
      TailUnit t{u, *images_[u], p, cbufs_[u], p.width, p.height, p.frame_w, p.frame_h, blends};
      const uint32_t nstages = p.modular ? 0 : (p.lf.gab ? 1 : 0) + (p.lf.epf_iters >= 3 ? 3 : p.lf.epf_iters);
      for (int c = 0; c < 3; c++) t.cur[c] = (nstages & 1) ? t.cb.pb[c] : t.cb.pa[c];
      t.cur_stride = p.bw * 8; t.cur_ec.assign(im.ne, 0); t.cur_ec_stride = t.cw;
      tables.emplace_back();
      t.tbl = &tables.back().entries;
      t.tbl->assign(im.ne, EcChanDev{});
      t.o_tab = tables.back().off = arena.Put(t.tbl->data(), im.ne * sizeof(EcChanDev));
      memset(&t.deferred_tf, 0, sizeof(t.deferred_tf)); t.have_deferred_tf = false;
      TailToFloat(im, t); TailPatches(im, t); TailSplines(im, t); TailUpsample(im, t); TailNoise(t);
      if (p.frame_type == 1) { TailLfHandOver(t); continue; }
      const bool can_ref = !p.is_last && p.frame_type != 1 && (p.duration == 0 || p.save_as_reference != 0);
      if (can_ref && p.save_before_ct) FillSlot(im.slots[p.save_as_reference], true, t.cur, t.cur_stride, t.cur_ec, t.cur_ec_stride, t.fw, t.fh);
      if (p.frame_type == 2) continue;    // reference-only frames are not displayed
      TailColour(im, t);
      if (first.out.only_frame >= 0 && u == pi.first_unit + first.out.only_frame) { TailOwnFrame(im, t); break; }
      TailBlend(im, t);
      if (can_ref && !p.save_before_ct) FillSlot(im.slots[p.save_as_reference], false, t.canvas, t.canvas_stride, t.canvas_ec, t.canvas_ec_stride, ih.xsize, ih.ysize);
      // coalescing: the composite of the last frame is what the caller receives — or, for a frame of an animation, the canvas after that frame
      // ... or, decoded once for all of them (SetOutputAllFrames), after every frame of the list, each canvas to its own slot of the output area
      int slot = -1;
      for (size_t k = 0; k < first.deliver_frames.size(); k++) if (first.deliver_frames[k] == u - pi.first_unit) slot = (int)k;
      const bool all_frames = !first.deliver_frames.empty();
      const bool deliver = all_frames ? slot >= 0 : (first.out.upto_frame >= 0 ? u == pi.first_unit + first.out.upto_frame : p.is_last);
      if (!deliver) continue;
      TailDeliver(im, t, slot);
      if (all_frames && slot + 1 < (int)first.deliver_frames.size()) continue;
      break;                      // (frames behind the delivered one: nothing of theirs is needed)
    }
  }
  for (const PendingTable& t : tables) if (!t.entries.empty()) memcpy(hconst.data() + t.off, t.entries.data(), t.entries.size() * sizeof(EcChanDev));
}

// Under JXL_HIP_DEBUG_SYNC every op is named and waited for (DebugSync), so that a fault in the tail is reported with its stage.
void Batch::EnqueuePostOps(void* stream) {
  for (auto& op : post_ops_) { op.second(stream); DebugSync(op.first, stream); }
  plane_outputs_ = plane_outputs_planned_;
}

}  // namespace jxlhip
