// jxl-hip: batch decoder (see decoder.h).
#include "decoder.h"
#include "decoder_impl.h"
#include <atomic>
#include <exception>
#include <deque>
#include <mutex>
#include <thread>
#include <chrono>
#include <map>
#include <queue>
#include <algorithm>
#include <cmath>
#include <cstring>

namespace jxlhip {

// Growable byte buffer in pinned host memory — what Prepare assembles the constant arena in and uploads from.  Pinned: the upload is a
// DMA at link speed (57 GB/s) instead of a staged copy, and can overlap the GPU's work.  The capacity survives clear(): a batch object that is
// refilled step after step (JxlHipBatchReset) allocates once.  Falls back to pageable memory when pinning fails (no GPU: host-only describe).
HostStage::~HostStage() {
  Release();
  for (auto& r : retired_) { if (r.second) (void)hipHostFree(r.first); else std::free(r.first); }
}
void HostStage::Release() {
  if (!p_) return;
  if (pinned_) (void)hipHostFree(p_); else std::free(p_);
  p_ = nullptr; n_ = cap_ = 0;
}
void HostStage::Reserve(size_t n) {
  if (n <= cap_) return;
  const size_t keep = n_;
  Resize(n);
  n_ = keep;
}
void HostStage::Resize(size_t n) {
  if (n > cap_) {
    // (pinned allocations cost milliseconds each and serialise with the rest of the runtime: capacities double, so that an arena assembled piece by piece
    // — or a batch object refilled with jobs of changing size — settles after a few)
    size_t cap = std::max<size_t>(cap_ * 2, 1 << 20);
    while (cap < n) cap *= 2;
    uint8_t* q = nullptr;
    bool pinned = hipHostMalloc((void**)&q, cap, hipHostMallocDefault) == hipSuccess && q;
    if (!pinned) { (void)hipGetLastError(); q = (uint8_t*)std::malloc(cap); if (!q) throw std::bad_alloc(); }
    const size_t keep = n_;
    if (keep) memcpy(q, p_, keep);
    // (hipHostFree waits for the whole device — hundreds of milliseconds under a busy pipeline: the outgrown block is kept until the object dies; capacities
    // double, so all of them together are smaller than the live one)
    if (p_) retired_.push_back({p_, pinned_});
    p_ = q; cap_ = cap; pinned_ = pinned; n_ = keep;
  }
  if (n > n_) {   // zero what Put does not overwrite: alignment gaps (< 256 B) — the payload is copied over right after
    const size_t gap_end = std::min(n, n_ + 512);
    memset(p_ + n_, 0, gap_end - n_);
  }
  n_ = n;
}

namespace {

// library-default kernels (image_metadata.cc kWeights2 / 4 / 8): each sub-pixel kernel sums to 1
static const float kUp2[15] = {-0.01716200f, -0.03452303f, -0.04022174f, -0.02921014f, -0.00624645f, 0.14111091f, 0.28896755f, 0.00278718f,
                               -0.01610267f, 0.56661550f,  0.03777607f,  -0.01986694f, -0.03144731f, -0.01185068f, -0.00213539f};
static const float kUp4[55] = {
    -0.02419067f, -0.03491987f, -0.03693351f, -0.03094285f, -0.00529785f, -0.01663432f, -0.03556863f, -0.03888905f, -0.03516850f, -0.00989469f, 0.23651958f,
    0.33392945f,  -0.01073543f, -0.01313181f, -0.03556694f, 0.13048175f,  0.40103025f,  0.03951150f,  -0.02077584f, 0.46914198f,  -0.00209270f, -0.01484589f,
    -0.04064806f, 0.18942530f,  0.56279892f,  0.06674400f,  -0.02335494f, -0.03551682f, -0.00754830f, -0.02267919f, -0.02363578f, 0.00315804f,  -0.03399098f,
    -0.01359519f, -0.00091653f, -0.00335467f, -0.01163294f, -0.01610294f, -0.00974088f, -0.00191622f, -0.01095446f, -0.03198464f, -0.04455121f, -0.02799790f,
    -0.00645912f, 0.06390599f,  0.22963888f,  0.00630981f,  -0.01897349f, 0.67537268f,  0.08483369f,  -0.02534994f, -0.02205197f, -0.01667999f, -0.00384443f};
static const float kUp8[210] = {
    -0.02928613f, -0.03706353f, -0.03783812f, -0.03324558f, -0.00447632f, -0.02519406f, -0.03752601f, -0.03901508f, -0.03663285f, -0.00646649f,
    -0.02066407f, -0.03838633f, -0.04002101f, -0.03900035f, -0.00901973f, -0.01626393f, -0.03954148f, -0.04046620f, -0.03979621f, -0.01224485f,
    0.29895328f, 0.35757708f, -0.02447552f, -0.01081748f, -0.04314594f, 0.23903219f, 0.41119301f, -0.00573046f, -0.01450239f, -0.04246845f,
    0.17567618f, 0.45220643f, 0.02287757f, -0.01936783f, -0.03583255f, 0.11572472f, 0.47416733f, 0.06284440f, -0.02685066f, 0.42720050f,
    -0.02248939f, -0.01155273f, -0.04562755f, 0.28689496f, 0.49093869f, -0.00007891f, -0.01545926f, -0.04562659f, 0.21238920f, 0.53980934f,
    0.03369474f, -0.02070211f, -0.03866988f, 0.14229550f, 0.56593398f, 0.08045181f, -0.02888298f, -0.03680918f, -0.00542229f, -0.02920477f,
    -0.02788574f, -0.02118180f, -0.03942402f, -0.00775547f, -0.02433614f, -0.03193943f, -0.02030828f, -0.04044014f, -0.01074016f, -0.01930822f,
    -0.03620399f, -0.01974125f, -0.03919545f, -0.01456093f, -0.00045072f, -0.00360110f, -0.01020207f, -0.01231907f, -0.00638988f, -0.00071592f,
    -0.00279122f, -0.00957115f, -0.01288327f, -0.00730937f, -0.00107783f, -0.00210156f, -0.00890705f, -0.01317668f, -0.00813895f, -0.00153491f,
    -0.02128481f, -0.04173044f, -0.04831487f, -0.03293190f, -0.00525260f, -0.01720322f, -0.04052736f, -0.05045706f, -0.03607317f, -0.00738030f,
    -0.01341764f, -0.03965629f, -0.05151616f, -0.03814886f, -0.01005819f, 0.18968273f, 0.33063684f, -0.01300105f, -0.01372950f, -0.04017465f,
    0.13727832f, 0.36402234f, 0.01027890f, -0.01832107f, -0.03365072f, 0.08734506f, 0.38194295f, 0.04338228f, -0.02525993f, 0.56408126f,
    0.00458352f, -0.01648227f, -0.04887868f, 0.24585519f, 0.62026135f, 0.04314807f, -0.02213737f, -0.04158014f, 0.16637289f, 0.65027023f,
    0.09621636f, -0.03101388f, -0.04082742f, -0.00904519f, -0.02790922f, -0.02117818f, 0.00798662f, -0.03995711f, -0.01243427f, -0.02231705f,
    -0.02946266f, 0.00992055f, -0.03600283f, -0.01684920f, -0.00111684f, -0.00411204f, -0.01297130f, -0.01723725f, -0.01022545f, -0.00165306f,
    -0.00313110f, -0.01218016f, -0.01763266f, -0.01125620f, -0.00231663f, -0.01374149f, -0.03797620f, -0.05142937f, -0.03117307f, -0.00581914f,
    -0.01064003f, -0.03608089f, -0.05272168f, -0.03375670f, -0.00795586f, 0.09628104f, 0.27129991f, -0.00353779f, -0.01734151f, -0.03153981f,
    0.05686230f, 0.28500998f, 0.02230594f, -0.02374955f, 0.68214326f, 0.05018048f, -0.02320852f, -0.04383616f, 0.18459474f, 0.71517975f,
    0.10805613f, -0.03263677f, -0.03637639f, -0.01394373f, -0.02511203f, -0.01728636f, 0.05407331f, -0.02867568f, -0.01893131f, -0.00240854f,
    -0.00446511f, -0.01636187f, -0.02377053f, -0.01522848f, -0.00333334f, -0.00819975f, -0.02964169f, -0.04499287f, -0.02745350f, -0.00612408f,
    0.02727416f, 0.19446600f, 0.00159832f, -0.02232473f, 0.74982506f, 0.11452620f, -0.03348048f, -0.01605681f, -0.02070339f, -0.00458223f,
};


struct ConstOffsets {
  size_t cs = 0, sec_off = 0, sec_size = 0, tree = 0, bcm = 0;
  size_t hf_list = (size_t)-1; uint32_t hf_count = 0;      // a frame decoded by region (Batch::JpegRegionUnit): the indices of the groups to decode, raster order
  size_t mod_ctx = 0, mod_cfg = 0, mod_alias = 0, mod_pc = 0, mod_po = 0, mod_ps = 0, mod_chan = 0, up_weights = 0;
  struct Pass { size_t ac_ctx = 0, ac_cfg = 0, ac_alias = 0, ac_pc = 0, ac_po = 0, ac_ps = 0; size_t orders[39] = {0}; };
  vec<Pass> pass;
  struct Local { uint32_t unit = 0; size_t tree = 0, ctx = 0, cfg = 0, alias = 0, pc = 0, po = 0, ps = 0; };   // sub-streams with their own tree / code
  vec<Local> local;
  vec<Local> lf_local;   // LfGroup sub-streams with their own tree / code (FramePlan::lf_local; unit = 3 g + k)
  size_t qtable[17 * 3] = {0};
  bool has_qtable[17] = {false};
};

void PutCode(Arena& a, const HostCode& c, size_t* ctx, size_t* cfg, size_t* alias, size_t* pc, size_t* po, size_t* ps) {
  *ctx = a.Put(c.ctx_map.data(), c.ctx_map.size());
  *cfg = a.Put(c.cfg.data(), c.cfg.size() * 4);
  *alias = a.Put(c.alias.data(), c.alias.size() * 8);
  *pc = a.Put(c.pfx_count.data(), c.pfx_count.size() * 2);
  *po = a.Put(c.pfx_sym_off.data(), c.pfx_sym_off.size() * 4);
  *ps = a.Put(c.pfx_syms.data(), c.pfx_syms.size() * 2);
}
// ---- SIMT LF decode: channel classes (kernels.h LfSimtPlan) -----------------------------------------------------------------------------
// Classifies the part of the MA tree channel `chan` of sub-stream `stream_id` can reach (static splits on the channel index / stream id are
// followed wherever they occur; splits on the row — property 2 — partition the channel's rows into classes).  Within a row class the
// subtree may test at most two of {W + N - NW (9), W (7), N (6), the weighted predictor's largest error (15)}: one property through a
// 1024-entry value -> cluster table (splits inside [-512, 510]), two through a 32 x 32 table (splits inside [-16, 14]); its leaves share one
// predictor out of zero / W / N / clamped gradient / weighted / (W + N) / 2 / select / NE, with offset 0 and multiplier 1.  That covers the
// fixed trees libjxl's encoder writes for LF-group streams at its default and faster efforts (enc_modular.cc: "WP fixed DC", "gradient
// fixed DC", "AC meta" and its variants); learned trees (slower efforts) usually test more properties and keep LfDecodeKernel.
struct LfRowClass { uint32_t kind = 0, pred = 0, sel_a = 0, sel_b = 0, cluster = 0; vec<uint8_t> lut; };
struct LfChanClass { bool uses_wp = false; vec<LfRowClass> rows; uint8_t row_to_class[512]; };
namespace {
struct LfClassifier {
  const vec<TreeNode>& nd;
  const HostCode& code;
  int chan; int32_t stream_id;
  LfClassifier(const HostTree& t, const HostCode& c, int ch, uint32_t sid) : nd(t.nodes), code(c), chan(ch), stream_id((int32_t)sid) {}
  static int SelOf(int prop) { return prop == 9 ? 0 : prop == 7 ? 1 : prop == 6 ? 2 : prop == 15 ? 3 : -1; }
  static int PredCode(int p) { static const int k[8] = {0, 1, 2, 5, 6, 3, 4, 7}; for (int i = 0; i < 8; i++) if (k[i] == p) return i; return -1; }
  // child taken at a static node, or -1 for a dynamic one; y < 0: the row is not fixed (its splits count as dynamic)
  int Static(const TreeNode& n, int y) const {
    if (n.prop == 0) return chan > n.val ? (int)n.a : (int)n.b;
    if (n.prop == 1) return stream_id > n.val ? (int)n.a : (int)n.b;
    if (n.prop == 2 && y >= 0) return y > n.val ? (int)n.a : (int)n.b;
    return -1;
  }
  // row thresholds and weighted-predictor use of the whole reachable subtree
  bool Survey(vec<int32_t>* ysplits, bool* uses_wp) const {
    vec<uint32_t> stack{0};
    size_t visited = 0;
    while (!stack.empty()) {
      const uint32_t pos = stack.back(); stack.pop_back();
      if (pos >= nd.size() || ++visited > 8192) return false;
      const TreeNode& n = nd[pos];
      if (n.prop < 0) { if ((n.a & 0xFF) == 6) *uses_wp = true; continue; }
      const int st = Static(n, -1);
      if (st >= 0) { stack.push_back((uint32_t)st); continue; }
      if (n.prop == 2) ysplits->push_back(n.val);
      if (n.prop == 15) *uses_wp = true;
      stack.push_back(n.a); stack.push_back(n.b);
    }
    return true;
  }
  bool ClassifyRow(int y, LfRowClass* out) const {
    int props[2] = {-1, -1}, np = 0, pred = -1;
    int32_t lo_split = 0, hi_split = 0;
    {
      vec<uint32_t> stack{0};
      size_t visited = 0;
      while (!stack.empty()) {
        const uint32_t pos = stack.back(); stack.pop_back();
        if (pos >= nd.size() || ++visited > 8192) return false;
        const TreeNode& n = nd[pos];
        if (n.prop < 0) {
          const int pc = PredCode((int)(n.a & 0xFF));
          if (pc < 0 || n.val != 0 || n.b != 1) return false;
          if (pred < 0) pred = pc; else if (pred != pc) return false;
          if ((n.a >> 8) >= code.ctx_map.size()) return false;
          continue;
        }
        const int st = Static(n, y);
        if (st >= 0) { stack.push_back((uint32_t)st); continue; }
        if (SelOf(n.prop) < 0) return false;
        int k = 0;
        while (k < np && props[k] != n.prop) k++;
        if (k == np) { if (np == 2) return false; props[np++] = n.prop; }
        lo_split = std::min(lo_split, n.val); hi_split = std::max(hi_split, n.val);
        stack.push_back(n.a); stack.push_back(n.b);
      }
    }
    if (pred < 0) return false;
    const int32_t lo = np == 2 ? -16 : -512, hi = np == 2 ? 15 : 511;
    if (np && (lo_split < lo || hi_split > hi - 1)) return false;
    out->kind = (uint32_t)np; out->pred = (uint32_t)pred;
    out->sel_a = np > 0 ? (uint32_t)SelOf(props[0]) : 0; out->sel_b = np > 1 ? (uint32_t)SelOf(props[1]) : 0;
    const int32_t span = hi - lo + 1;
    out->lut.assign(np == 0 ? 1 : np == 1 ? (size_t)span : (size_t)span * span, 0);
    // the table, by pushing the value box down the tree (a split at `val` sends (val, hi] to child a, [lo, val] to child b): every
    // reachable node once instead of a walk from the root per value — 7 tables per LF group of every frame add up in a streaming loop
    struct Box { uint32_t pos; int32_t lo[2], hi[2]; };
    vec<Box> stack{Box{0, {lo, lo}, {hi, hi}}};
    while (!stack.empty()) {
      const Box r = stack.back(); stack.pop_back();
      const TreeNode& n = nd[r.pos];
      if (n.prop < 0) {
        const uint8_t cl = code.ctx_map[n.a >> 8];
        if (np == 0) out->lut[0] = cl;
        else if (np == 1) memset(out->lut.data() + (r.lo[0] - lo), cl, (size_t)(r.hi[0] - r.lo[0] + 1));
        else for (int32_t a = r.lo[0]; a <= r.hi[0]; a++) memset(out->lut.data() + (size_t)(a - lo) * span + (r.lo[1] - lo), cl, (size_t)(r.hi[1] - r.lo[1] + 1));
        continue;
      }
      const int st = Static(n, y);
      if (st >= 0) { Box b = r; b.pos = (uint32_t)st; stack.push_back(b); continue; }
      const int k = n.prop == props[0] ? 0 : 1;
      if (r.hi[k] > n.val) { Box b = r; b.pos = n.a; b.lo[k] = std::max(r.lo[k], n.val + 1); stack.push_back(b); }
      if (r.lo[k] <= n.val) { Box b = r; b.pos = n.b; b.hi[k] = std::min(r.hi[k], n.val); stack.push_back(b); }
    }
    out->cluster = out->lut[0];
    return true;
  }
};
}  // namespace
// whether channel `chan` of sub-stream `stream_id` can reach a weighted-predictor leaf or a split on its error (a damaged tree counts as yes)
bool LfChannelUsesWp(const HostTree& tree, int chan, uint32_t stream_id) {
  static const HostCode no_code;
  vec<int32_t> ysplits;
  bool uses = false;
  return tree.nodes.empty() || !LfClassifier(tree, no_code, chan, stream_id).Survey(&ysplits, &uses) || uses;
}
bool ClassifyLfChannel(const HostTree& tree, const HostCode& code, int chan, uint32_t stream_id, LfChanClass* out) {
  if (tree.nodes.empty()) return false;
  LfClassifier cl(tree, code, chan, stream_id);
  vec<int32_t> ysplits;
  out->uses_wp = false;
  if (!cl.Survey(&ysplits, &out->uses_wp)) return false;
  // rows 0 ... 511 (the table's reach; LF-group channels have at most 256 rows): a class per interval between row thresholds
  vec<int32_t> starts{0};
  for (int32_t v : ysplits) if (v >= 0 && v < 511) starts.push_back(v + 1);
  std::sort(starts.begin(), starts.end());
  starts.erase(std::unique(starts.begin(), starts.end()), starts.end());
  if (starts.size() > 64) return false;
  out->rows.clear();
  for (size_t k = 0; k < starts.size(); k++) {
    LfRowClass rc;
    if (!cl.ClassifyRow(starts[k], &rc)) return false;
    size_t idx = 0;
    while (idx < out->rows.size() && !(out->rows[idx].kind == rc.kind && out->rows[idx].pred == rc.pred && out->rows[idx].sel_a == rc.sel_a && out->rows[idx].sel_b == rc.sel_b && out->rows[idx].lut == rc.lut)) idx++;
    if (idx == out->rows.size()) out->rows.push_back(std::move(rc));
    const int32_t end = k + 1 < starts.size() ? starts[k + 1] : 512;
    for (int32_t y = starts[k]; y < end; y++) out->row_to_class[y] = (uint8_t)idx;
  }
  return true;
}

DevCode ViewCode(const HostCode& c, const uint8_t* base, size_t ctx, size_t cfg, size_t alias, size_t pc, size_t po, size_t ps) {
  DevCode d;
  d.ctx_map = base + ctx; d.cfg = (const uint32_t*)(base + cfg); d.alias = (const uint64_t*)(base + alias);
  d.pfx_count = (const uint16_t*)(base + pc); d.pfx_sym_off = (const uint32_t*)(base + po); d.pfx_syms = (const uint16_t*)(base + ps);
  d.num_ctx = c.num_ctx; d.num_clusters = c.num_clusters; d.log_alpha = c.log_alpha; d.use_prefix = c.use_prefix;
  d.lz77 = c.lz77; d.lz_min_symbol = c.lz_min_symbol; d.lz_min_length = c.lz_min_length; d.lz_len_cfg = c.lz_len_cfg;
  return d;
}
}  // namespace

// Colour-transform parameters of an image (stage_xyb.cc OpsinParams, dec_xyb.cc OutputEncodingInfo::SetColorEncoding):
// inverse opsin matrix scaled to the intensity target — for grey-scale images its rows are replaced by their luminance-weighted
// sum (kSRGBLuminances; Mul3x3Matrix accumulates in double), so R = G = B — and the output transfer function.
// sRGB or linear output (colour modes 0 / 1): what the fused gaborish + EPF + output kernel computes; other transfer functions take the
// unfused filter kernels and OutputKernel
static bool SimpleTransfer(const ImageHeader& ih) { return ih.color_default || (!ih.have_gamma && (ih.tf == 13 || ih.tf == 8)); }

void FillColor(const ImageHeader& ih, bool do_ycbcr, FrameDev& f) {
  float inv[9];
  for (int k = 0; k < 9; k++) inv[k] = ih.opsin_inv[k];
  // images whose header names other primaries / another white point than sRGB / D65: XYB decodes to linear sRGB, the matrix takes it on
  // to the image's own primaries (icc_profile.cc SrgbToOriginalPrimaries)
  float luminances[3] = {0.2126f, 0.7152f, 0.0722f};
  double to_original[9];
  if (ih.xyb_encoded && SrgbToOriginalPrimaries(ih, to_original, luminances)) {   // (not for other images: their samples are in that space already)
    float adapted[9];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) {
      double e = 0;
      for (int k = 0; k < 3; k++) e += to_original[i * 3 + k] * (double)inv[k * 3 + j];
      adapted[i * 3 + j] = (float)e;
    }
    for (int k = 0; k < 9; k++) inv[k] = adapted[k];
  }
  if (ih.color_space == 1) {
    const float lum[3] = {0.2126f, 0.7152f, 0.0722f};
    float folded[9];
    for (int x = 0; x < 3; x++) for (int y = 0; y < 3; y++) {
      double e = 0;
      for (int z = 0; z < 3; z++) e += lum[z] * inv[z * 3 + x];
      folded[y * 3 + x] = (float)e;
    }
    for (int k = 0; k < 9; k++) inv[k] = folded[k];
  }
  const float s = 255.0f / ih.intensity_target;
  for (int k = 0; k < 9; k++) f.opsin_inv[k] = inv[k] * s;
  for (int k = 0; k < 3; k++) { f.neg_bias[k] = ih.opsin_bias[k]; f.neg_bias_cbrt[k] = std::cbrt(ih.opsin_bias[k]); }
  f.inverse_gamma = 1.0f;
  if (ih.xyb_encoded) {
    f.color_mode = 0;
    if (!ih.color_default) {
      if (ih.have_gamma) { f.color_mode = 4; f.inverse_gamma = (float)ih.gamma * 1e-7f; }
      else if (ih.tf == 8) f.color_mode = 1;
      else if (ih.tf == 17) { f.color_mode = 4; f.inverse_gamma = 1.0f / 2.6f; }
      else if (ih.tf == 1) f.color_mode = 5;
      else if (ih.tf == 16) { f.color_mode = 6; f.hdr_par[0] = ih.intensity_target * (1.0f / 10000.0f); }   // TF_PQ(intensity_target)
      else if (ih.tf == 18) {
        // stage_from_linear.cc OpHlg: HlgOOTF::ToSceneLight(display_luminance = intensity target, luminances of the output primaries)
        f.color_mode = 7;
        const float gamma = (1 / 1.2f) * std::pow(1.111f, -std::log2(ih.intensity_target / 1000.f));
        f.hdr_par[0] = gamma - 1;
        f.hdr_par[1] = (f.hdr_par[0] < -0.01f || 0.01f < f.hdr_par[0]) ? 1.0f : 0.0f;
        for (int k = 0; k < 3; k++) f.hdr_par[2 + k] = luminances[k];
      }
    }
  } else f.color_mode = do_ycbcr ? 2 : 3;
}

// ---- output colour (OutputSpec::color; include/jxl_hip.h has the rule)
// The header the colour stage and the kernel choice go by: an XYB image under a requested encoding is the same codestream under a header that names that encoding, at
// its own intensity target — everything FillColor and SimpleTransfer read is taken from there, so the pixels are those of that file bit for bit.  Every other image:
// its own header (`store` is only written when the two differ).
const ImageHeader& Batch::ColourHeader(const ImageHeader& ih, const OutputSpec& o, ImageHeader* store) {
  if (!o.color_set || !ih.xyb_encoded) return ih;
  ImageHeader& h = *store;
  h = ImageHeader();
  h.xyb_encoded = true; h.intensity_target = ih.intensity_target;
  for (int k = 0; k < 9; k++) h.opsin_inv[k] = ih.opsin_inv[k];
  for (int k = 0; k < 3; k++) h.opsin_bias[k] = ih.opsin_bias[k];
  ApplyColorTarget(o.color, &h);
  return h;
}
bool Batch::ConvertsNonXyb(const ImageHeader& ih, const OutputSpec& o) {
  return o.color_set && o.color_non_xyb && !ih.xyb_encoded && !ih.want_icc && !SameColorEncoding(ColorTargetOf(ih), o.color);
}
std::string Batch::ColourRefusal(const ImageHeader& ih, const OutputSpec& o) {
  if (!o.color_set) return std::string();
  if (o.color_non_xyb > 1) return "unsupported: output colour with non_xyb = " + std::to_string(o.color_non_xyb) + " (0 leave, 1 convert)";
  const std::string why = ColorTargetRefusal(o.color);
  if (!why.empty()) return why;
  if (o.jpeg_scale != 1 || o.resize_u8) return "unsupported: output colour of a libjpeg-exact output (jpeg_scale, the integer resample): those are libjpeg's samples";
  const bool grey = ih.color_space == 1 && !ih.color_default;
  if (o.color.color_space == 1 && !grey) return "unsupported: output colour: a grey encoding for a colour image";
  if (o.color.color_space == 0 && grey) return "unsupported: output colour: an RGB encoding for a grey image";
  if (o.color_non_xyb && !ih.xyb_encoded && ih.want_icc) return "unsupported: output colour of an image whose colour is an ICC profile needs a CMS";
  if (o.color_non_xyb && !ih.xyb_encoded) {
    // (the source side of the conversion: an encoding the decoder cannot take to linear light — an unknown transfer function or colour space, a bad chromaticity — is no
    // more convertible than an ICC profile; AddImage only checks the transfer function of XYB images, which are rendered through it)
    const std::string src = ColorTargetRefusal(ColorTargetOf(ih)), head = "unsupported: output colour ";
    if (!src.empty()) return "unsupported: output colour of an image whose own encoding cannot be converted: an encoding " + src.substr(head.size());
  }
  return std::string();
}
// The conversion of an image that is not XYB (ConvertsNonXyb), for ColorKernel: the source's inverse transfer function, the matrix between the two sets of primaries,
// and — in the fields TransferFromLinear reads — the target's transfer function.  Both parameter sets are the ones FillColor gives an XYB image of that encoding.
void FillColourConversion(const ImageHeader& ih, const OutputSpec& o, ColorArgs* ca) {
  const ColorTarget own = ColorTargetOf(ih);
  ImageHeader h;
  h.xyb_encoded = true; h.intensity_target = ih.intensity_target;
  for (int k = 0; k < 9; k++) h.opsin_inv[k] = ih.opsin_inv[k];
  for (int k = 0; k < 3; k++) h.opsin_bias[k] = ih.opsin_bias[k];
  FrameDev src, dst;
  memset(&src, 0, sizeof(src)); memset(&dst, 0, sizeof(dst));
  ApplyColorTarget(own, &h); FillColor(h, false, src);
  ApplyColorTarget(o.color, &h); FillColor(h, false, dst);
  double m[9];
  ColorConversionMatrix(own, o.color, m);
  ca->convert = 1;
  ca->src_tf = src.color_mode;
  for (int k = 0; k < 5; k++) ca->src_par[k] = 0.0f;
  if (src.color_mode == 4) ca->src_par[0] = 1.0f / src.inverse_gamma;                      // gamma: the reciprocal exponent
  else if (src.color_mode == 6) ca->src_par[0] = 10000.0f / ih.intensity_target;           // PQ: 1.0 = the intensity target
  else if (src.color_mode == 7) {                                                          // HLG: the OOTF's exponent gamma - 1 (FillColor's is 1 / gamma - 1), inside the same band
    ca->src_par[0] = 1.0f / (src.hdr_par[0] + 1.0f) - 1.0f; ca->src_par[1] = src.hdr_par[1];
    for (int k = 0; k < 3; k++) ca->src_par[2 + k] = src.hdr_par[2 + k];      // (luminances of the source's primaries)
  }
  for (int k = 0; k < 9; k++) ca->conv[k] = (float)m[k];
  ca->conv_identity = 1;
  for (int k = 0; k < 9; k++) if (m[k] != (k % 4 == 0 ? 1.0 : 0.0)) ca->conv_identity = 0;
  ca->tf_kind = dst.color_mode; ca->inverse_gamma = dst.inverse_gamma;
  for (int k = 0; k < 5; k++) ca->hdr_par[k] = dst.hdr_par[k];
}

// ---- device arena pool.  hipMalloc / hipFree of the multi-gigabyte arenas cost 0.5-3.5 s per batch object on the boxes measured (page tables of tens of GB set up and
// torn down), which is what a "fresh batch" paid each time (bench.py one_pass_128: 92 ms here, 3.6 s on the driver's box in round 3).  Arenas that a batch lets go of are kept
// in a process-wide free list (bounded: JXL_HIP_ARENA_POOL_MB, default 60 % of the device's memory; 0 turns the pool off) and handed to the next batch that asks for that much memory on that device.
namespace {
struct ArenaPool {
  struct Block { void* p; size_t cap; int dev; };
  std::mutex mu;
  std::vector<Block> blocks;
  size_t held = 0;
  static size_t Limit() {   // default: 60 % of the device's memory — what is handed back with hipFree is what the next hipMalloc (of any size) waits for: 2-3.5 s after a pipeline's 130 GB
    static const size_t v = [] {
      if (const char* e = getenv("JXL_HIP_ARENA_POOL_MB")) return (size_t)atoll(e) << 20;
      size_t free_b = 0, total_b = 0;
      if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); total_b = (size_t)64 << 30; }
      return total_b / 10 * 6;
    }();
    return v;
  }
  static constexpr size_t kMinBytes = (size_t)8 << 20;   // small allocations are cheap: not pooled
  void* Take(size_t want, size_t* cap, int dev) {
    if (want < kMinBytes || Limit() == 0) return nullptr;
    std::lock_guard<std::mutex> lock(mu);
    int best = -1;
    for (size_t i = 0; i < blocks.size(); i++)
      if (blocks[i].dev == dev && blocks[i].cap >= want && blocks[i].cap <= 4 * want + ((size_t)64 << 20) && (best < 0 || blocks[i].cap < blocks[(size_t)best].cap)) best = (int)i;
    if (best < 0) return nullptr;
    void* p = blocks[(size_t)best].p; *cap = blocks[(size_t)best].cap; held -= *cap;
    blocks.erase(blocks.begin() + best);
    return p;
  }
  // `dev`: the device the block was allocated on (the owner's, not the calling thread's current one).  The device-wide wait — what hipFree does implicitly: nothing in
  // flight may still touch the block when somebody else gets it — happens outside the pool's lock.
  // idle: the caller knows that nothing on the device refers to the block any more (a batch object is only refilled after its last decode has left the GPU) — no
  // device-wide wait, which under a busy pipeline takes as long as everything in flight (seen: 400 ms stalls of a prepare thread)
  void Give(void* p, size_t cap, int dev, bool idle = false) {
    if (!p) return;
    if (dev >= 0 && cap >= kMinBytes && Limit() != 0) {
      bool room;
      { std::lock_guard<std::mutex> lock(mu); room = held + cap <= Limit() && blocks.size() < 96; }
      if (room && idle) {
        std::lock_guard<std::mutex> lock(mu);
        if (held + cap <= Limit() && blocks.size() < 96) { blocks.push_back(Block{p, cap, dev}); held += cap; return; }
      } else if (room) {
        int cur = -1;
        if (hipGetDevice(&cur) != hipSuccess) { (void)hipGetLastError(); cur = -1; }
        if (cur != dev) (void)hipSetDevice(dev);
        (void)hipDeviceSynchronize();
        if (cur >= 0 && cur != dev) (void)hipSetDevice(cur);
        std::lock_guard<std::mutex> lock(mu);
        if (held + cap <= Limit() && blocks.size() < 96) { blocks.push_back(Block{p, cap, dev}); held += cap; return; }
      }
    }
    (void)hipFree(p);
  }
  size_t Trim() {   // gives everything back to the runtime (an allocation failed: the pool may be what is in the way; or the caller asked: JxlHipArenaPoolTrim)
    std::vector<Block> mine;
    size_t bytes;
    { std::lock_guard<std::mutex> lock(mu); mine.swap(blocks); bytes = held; held = 0; }
    for (auto& b : mine) (void)hipFree(b.p);
    return bytes;
  }
  size_t Held() { std::lock_guard<std::mutex> lock(mu); return held; }
};
ArenaPool& Pool() { static ArenaPool* pool = new ArenaPool(); return *pool; }     // (never destroyed: the runtime may be gone by then)
}  // namespace
size_t DeviceArenaPoolTrim() { return Pool().Trim(); }
size_t DeviceArenaPoolHeld() { return Pool().Held(); }
void* DeviceArenaTake(size_t want, size_t* cap, int device) { return Pool().Take(want, cap, device); }
void DeviceArenaGive(void* p, size_t cap, int device, bool idle) { Pool().Give(p, cap, device, idle); }

Batch::Batch(int device) : device_(device) {
  if (device_ >= 0) HIP_CHECK(hipSetDevice(device_));      // (-1: host-side parsing only, JxlHipDebugDescribe)
}
Batch::~Batch() {
  // (the calling thread's current device is left as it was found)
  int cur = -1;
  if (device_ >= 0 && hipGetDevice(&cur) != hipSuccess) { (void)hipGetLastError(); cur = -1; }
  if (device_ >= 0 && cur != device_) (void)hipSetDevice(device_);
  if (clear_stream_) { (void)hipStreamSynchronize((hipStream_t)clear_stream_); (void)hipStreamDestroy((hipStream_t)clear_stream_); }
  if (clear_event_) (void)hipEventDestroy((hipEvent_t)clear_event_);
  if (idct_event_) (void)hipEventDestroy((hipEvent_t)idct_event_);
  if (flags_event_) (void)hipEventDestroy((hipEvent_t)flags_event_);
  if (flags_pinned_) (void)hipHostFree(flags_pinned_);
  if (status_event_) (void)hipEventDestroy((hipEvent_t)status_event_);
  if (status_pinned_) (void)hipHostFree(status_pinned_);
  if (jpeg_pinned_) (void)hipHostFree(jpeg_pinned_);
  for (void* ev : jpeg_copy_event_) if (ev) (void)hipEventDestroy((hipEvent_t)ev);
  Pool().Give(dconst_, const_cap_, device_);
  Pool().Give(dwork_, work_cap_, device_);
  if (djpeg_) Pool().Give(djpeg_, jpeg_cap_, device_);
  if (djpeg_out_) Pool().Give(djpeg_out_, jpeg_out_cap_, device_);
  if (djpeg_table_) Pool().Give(djpeg_table_, jpeg_table_cap_, device_);
  if (dcoef_ && !coef_owner_ && !coef_is_ext_) Pool().Give(dcoef_, coef_cap_, device_);
  if (dbig_ && !big_owner_ && !big_is_ext_) Pool().Give(dbig_, big_cap_, device_);
  if (big_owner_) big_owner_->big_sharers_--;
  if (dframes_) (void)hipFree(dframes_);
  if (dpasses_) (void)hipFree(dpasses_);
  if (dlocal_) (void)hipFree(dlocal_);
  if (device_ >= 0 && cur >= 0 && cur != device_) (void)hipSetDevice(cur);
}

// The coefficient and pixel planes are only touched by the "rest" half of a decode (HF decode ... write), which a caller
// that pipelines two batches runs strictly one after the other on one stream: the second batch may therefore use the
// first one's buffers.  Must be called before Prepare(); `owner` must already be prepared and stay alive.
void Batch::ShareBigArena(Batch* owner) {
  if (prepared_) throw ParseError("ShareBigArena after Prepare", false);
  if (big_owner_ == owner) return;
  if (big_owner_) { big_owner_->big_sharers_--; dbig_ = nullptr; big_cap_ = 0; }       // (the pointer aliased the old owner's planes: not ours to free)
  if (dbig_ && !big_is_ext_) Pool().Give(dbig_, big_cap_, device_);
  dbig_ = nullptr; big_cap_ = 0; big_is_ext_ = false;
  big_owner_ = owner;
  if (owner) owner->big_sharers_++;
}
// Likewise for the quantised-coefficient planes (written by the HF stage, consumed — and zeroed again — by the IDCT of the same decode):
// batches whose [HF ... IDCT] intervals never overlap may use one set.  A deep pipeline alternates between two owners so that the HF
// stage of batch k + 1 can run beside the IDCT of batch k.
void Batch::ShareCoefArena(Batch* owner) {
  if (prepared_) throw ParseError("ShareCoefArena after Prepare", false);
  if (coef_owner_ == owner) return;
  if (coef_owner_) { dcoef_ = nullptr; coef_cap_ = 0; coef_laid_out_ = 0; }            // (aliased the old owner's planes: not ours to free)
  if (dcoef_ && !coef_is_ext_) Pool().Give(dcoef_, coef_cap_, device_);
  dcoef_ = nullptr; coef_cap_ = 0; coef_is_ext_ = false;
  coef_owner_ = owner;
}

void Batch::UseSharedPlanes(SharedPlanes* big, SharedPlanes* coef) {
  if (big_owner_ || coef_owner_) throw ParseError("UseSharedPlanes: the batch shares another batch's arenas already", false);
  ext_big_ = big; ext_coef_ = coef;
  prepared_ = false;
}

// ---- stream-ordered completion (pipelined callers): the status words travel to pinned memory behind the decode, an event says when
void Batch::EnqueueStatusReadback(void* stream_v) {
  hipStream_t stream = (hipStream_t)stream_v;
  const size_t n = images_.size();
  if (!status_pinned_ || status_pinned_n_ < 2 * n) {
    if (status_pinned_) (void)hipHostFree(status_pinned_);
    status_pinned_ = nullptr;
    const size_t cap = std::max<size_t>(8192, 4 * n);             // (hipHostFree waits for the device: generous, so that a refilled batch object rarely gets here)
    HIP_CHECK(hipHostMalloc((void**)&status_pinned_, cap * 4));
    status_pinned_n_ = cap;
  }
  if (!status_event_) { hipEvent_t ev; HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming)); status_event_ = ev; }
  if (n) {
    HIP_CHECK(hipMemcpyAsync(status_pinned_, dwork_ + status_off_, n * 4, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipMemcpyAsync(status_pinned_ + n, dwork_ + hfw_off_, n * 4, hipMemcpyDeviceToHost, stream));
  }
  HIP_CHECK(hipEventRecord((hipEvent_t)status_event_, stream));
  status_pending_ = true;
  if (lf_batch_) lf_batch_->EnqueueStatusReadback(stream_v);
}
void Batch::HarvestStatus(vec<uint32_t>* per_unit) {
  const size_t n = images_.size();
  per_unit->assign(n, 0);
  if (!status_pending_) throw ParseError("HarvestStatus without EnqueueStatusReadback", false);
  HIP_CHECK(hipEventSynchronize((hipEvent_t)status_event_));
  status_pending_ = false;
  bool any = false;
  for (size_t i = 0; i < n; i++) { (*per_unit)[i] = status_pinned_[i]; any |= status_pinned_[i] != 0; }
  if (any_vardct_ && decodes_since_finish_ > 0) {
    for (size_t i = 0; i < n; i++) hf_written_[i] = status_pinned_[n + i] / decodes_since_finish_;
    decodes_since_finish_ = 0;
  }
  if (lf_batch_) { vec<uint32_t> lf; if (lf_batch_->status_pending_) { lf_batch_->HarvestStatus(&lf); for (uint32_t v : lf) if (v) for (auto& s : *per_unit) s |= v; } }
  (void)any;    // (failed frames: ZeroFailedCoefficients has put zeros back on the device, the planes stay clean for the next user)
}

// Makes *ptr a device allocation of at least `bytes` (kept if it already is; grown with 1/8 of slack otherwise; taken from the arena pool when it has a block of
// that size).  Returns true if the memory is new (contents undefined).
bool Batch::DevReserve(void** ptr, size_t* cap, size_t bytes) {
  if (*ptr && *cap >= bytes) return false;
  // (no decode of this object is in flight when it is prepared again — the contract of Reset / Prepare —, so the outgrown block is idle unless other batches share it)
  if (*ptr) { Pool().Give(*ptr, *cap, device_, /*idle=*/!(ptr == (void**)&dbig_ && big_sharers_ > 0)); *ptr = nullptr; *cap = 0; }
  // below 4 GiB capacities are powers of two (a batch object refilled with jobs of changing size settles after a few allocations), above: 1/8 of slack
  size_t want = std::max<size_t>(bytes + bytes / 8, 256);
  if (bytes < ((size_t)4 << 30)) { want = 1 << 16; while (want < bytes) want *= 2; }
  if (void* p = Pool().Take(std::max<size_t>(bytes, 256), cap, device_)) { *ptr = p; return true; }
  if (hipMalloc(ptr, want) != hipSuccess) {
    (void)hipGetLastError();
    Pool().Trim();
    if (hipMalloc(ptr, want) == hipSuccess) { *cap = want; return true; }
    (void)hipGetLastError();
    HIP_CHECK(hipMalloc(ptr, std::max<size_t>(bytes, 256))); *cap = std::max<size_t>(bytes, 256);
  } else *cap = want;
  return true;
}

// Forgets the images (and everything derived from them) but keeps the device arenas, the pinned staging buffer and the sharing set up with
// ShareBigArena / ShareCoefArena: the batch object can be filled again.  The caller makes sure no decode of the old content is in flight.
void Batch::Reset() {
  images_.clear(); pub_.clear(); cbufs_.clear(); post_ops_.clear(); jpeg_data_.clear(); jw_.reset(); jpeg_pixel_results_.clear(); jpeg_pixel_table_.clear(); jpeg_pixel_table_image_.clear(); jpeg_pixel_groups_.clear(); resize_plans_.clear(); resize_groups_.clear();
  frames_host_.clear(); passes_host_.clear(); pass_first_.clear(); local_host_.clear(); local_first_.clear();
  mod_plane_offsets_.clear(); mod_ops_.clear(); vardct_alpha_.clear(); hf_written_.clear();
  // (stage timings recorded so far stay: CollectTimes sums over the object's life)
  any_complex_ = false; any_vardct_ = any_modchan_ = any_multipass_ = false;
  prepared_ = false; ran_once_ = false; flags_pending_ = false; decodes_since_finish_ = 0;
  cfg.idct_flags_known = 0; cfg.skip_hf = 0; cfg.max_passes = 0;
  lf_simt_ = LfSimtPlan();
  if (lf_batch_) lf_batch_->Reset();     // (kept for its arenas; Prepare drops it when no unit refers to an LF frame)
}

// Parses `n` images on `threads` host threads (the per-image work of AddImage — container, image and frame headers, TOC, the global
// sections' tables — is independent) and appends them in order.  Returns the index of the first one; throws what the first failing
// image threw.
int Batch::AddImages(const uint8_t* const* datas, const size_t* sizes, int n, int threads, bool allow_partial) {
  if (n <= 0) return (int)pub_.size();
  vec<int> index;
  std::vector<std::string> errors;
  return AddImagesImpl(datas, sizes, n, threads, /*tolerant=*/false, &index, &errors, allow_partial);
}

// The pipelined form: an image that does not parse (truncated, damaged headers, a feature the device path does not take) is left out instead of failing the call —
// (*index)[i] = its index in the batch or -1, (*errors)[i] = what it threw ("" if it parsed).
void Batch::AddImagesTolerant(const uint8_t* const* datas, const size_t* sizes, int n, int threads, vec<int>* index, std::vector<std::string>* errors, bool for_downscale, bool for_jpeg_dc) {
  AddImagesImpl(datas, sizes, n, threads, /*tolerant=*/true, index, errors, /*allow_partial=*/for_downscale || for_jpeg_dc, /*only_downscalable=*/for_downscale, /*partial_only_jpeg_dc=*/for_jpeg_dc);
}

static std::string DownscaleRefusalOf(int num_units, const ImageEntry& e);   // (below, with SetOutput)
static std::string JpegPixelsRefusalOf(int num_units, bool complex, const ImageEntry& e, const OutputSpec& out);   // (below, with DecodeJpegPixels)
static bool JpegDcEligibleOf(const FramePlan& p, const OutputSpec& out);
int Batch::AddImagesImpl(const uint8_t* const* datas, const size_t* sizes, int n, int threads, bool tolerant, vec<int>* index, std::vector<std::string>* errs, bool allow_partial, bool only_downscalable,
                         bool partial_only_jpeg_dc) {
  index->assign((size_t)std::max(n, 0), -1);
  errs->assign((size_t)std::max(n, 0), std::string());
  if (n <= 0) return (int)pub_.size();
  vec<ParsedImage> parsed((size_t)n);
  vec<std::exception_ptr> errors((size_t)n);
  const int nt = std::max(1, std::min(threads, n));
  std::atomic<int> next{0};
  const MmHooks* hooks = MmCurrent();
  auto work = [&]() {
    MmScope scope(hooks);                  // (worker threads allocate through the caller's memory manager, too)
    for (;;) {
      const int i = next.fetch_add(1);
      if (i >= n) break;
      try { ParseImage(datas[i], sizes[i], &parsed[i], allow_partial); } catch (...) { errors[i] = std::current_exception(); }
    }
  };
  if (nt == 1) work();
  else {
    std::vector<std::thread> pool;
    for (int t = 0; t < nt; t++) pool.emplace_back(work);
    for (auto& t : pool) t.join();
  }
  const int first = (int)pub_.size();
  if (!tolerant) for (int i = 0; i < n; i++) if (errors[i]) std::rethrow_exception(errors[i]);
  for (int i = 0; i < n; i++) {
    if (errors[i]) {
      try { std::rethrow_exception(errors[i]); } catch (const std::exception& e) { (*errs)[i] = e.what(); } catch (...) { (*errs)[i] = "unknown error"; }
      if ((*errs)[i].empty()) (*errs)[i] = "parse error";
      continue;
    }
    if (tolerant && only_downscalable && !parsed[i].units.empty()) {
      // a job decoded at 1:8: what that decode does not take is left out like an image that does not parse (nothing of it is uploaded or decoded)
      (*errs)[i] = DownscaleRefusalOf((int)parsed[i].units.size(), *parsed[i].units[0]);
      if (!(*errs)[i].empty()) continue;
    }
    if (tolerant && partial_only_jpeg_dc && !parsed[i].units.empty() && parsed[i].units[0]->plan.partial) {
      // a job decoded at libjpeg's scale 1/8: a stream that ends behind its LF part is enough for a DC-only image and for no other — that one is left out, "truncated"
      OutputSpec o8;
      o8.jpeg_scale = 8;
      const ImageEntry& e = *parsed[i].units[0];
      if (!jpeg_dc_only || !JpegPixelsRefusalOf((int)parsed[i].units.size(), parsed[i].complex, e, o8).empty() || !JpegDcEligibleOf(e.plan, o8)) { (*errs)[i] = "truncated"; continue; }
    }
    (*index)[i] = Append(std::move(parsed[i]));
  }
  return first;
}

int Batch::AddImage(const uint8_t* data, size_t size, bool allow_partial) {
  ParsedImage pi;
  ParseImage(data, size, &pi, allow_partial);
  return Append(std::move(pi));
}
bool Batch::is_partial(int i) const { return images_[pub_[i].first_unit]->plan.partial; }

int Batch::Append(ParsedImage&& im) {
  PubImage pi; pi.first_unit = (int)images_.size(); pi.num_units = (int)im.units.size(); pi.complex = pi.parsed_complex = im.complex;
  for (auto& u : im.units) { u->pub_index = (int)pub_.size(); images_.push_back(std::move(u)); }
  pub_.push_back(pi);
  prepared_ = false;
  return (int)pub_.size() - 1;
}

// what the device path cannot take of a frame that parsed (thrown as "unsupported: ...")
static void CheckFrameSupported(const FramePlan& p, const ImageHeader& ih) {
  if (!p.modular) {
    // (squeezed extra channels, what cjxl does to a progressive or lossy alpha of an RGBA picture, are taken: the sub-channels squeezed by >= 3 ride in the LfGroup
    // sections — the LF kernel decodes them between the LF coefficients and the HF metadata —, the others in the PassGroup sections of the passes whose brackets hold
    // them — ModularGroupFastKernel reads them behind that pass's coefficients, FramePlan::mod_pass / mod_passes)
    // (Modular sub-streams with MA trees and codes of their own are taken in the global stream and the LfGroup sections — FramePlan::lf_local, LfDecodeLocalKernel.
    // The extra-channel streams behind the AC coefficients of the PassGroup sections are not: their start is known only once the HF stage has run.  A frame with a
    // global tree whose PassGroup streams do not use it fails in ModularGroupFastKernel with kErrUnsupported; without a global tree it is refused here.)
    if (!p.has_global_tree) {
      bool tails = false;
      for (size_t c = p.global_decodable; c < p.gchannels.size(); c++) tails |= p.gchannels[c].w && p.gchannels[c].h && std::min(p.gchannels[c].hshift, p.gchannels[c].vshift) <= 2;
      if (tails) throw ParseError("unsupported: VarDCT frame without a global MA tree whose PassGroup sections carry extra channels (local trees behind the AC coefficients)", true);
    }
    if (p.subsampled && (p.base_x != 0.f || p.base_b != 0.f)) throw ParseError("unsupported: chroma from luma in a chroma-subsampled frame", true);
  }
  for (auto& x : ih.extra) {
    if (x.dim_shift != 0) throw ParseError("unsupported: subsampled extra channel", true);
    if (x.depth.is_float) {
      const uint32_t b = x.depth.bits, eb = x.depth.exp_bits;
      if (b > 32 || eb < 2 || eb > 8 || b < eb + 2 || b - eb - 1 > 23 || (b == 32 && eb != 8)) throw ParseError("unsupported: float sample layout", true);
    }
  }
  if (p.modular && ih.depth.is_float && !ih.xyb_encoded) {
    // dec_modular.cc int_to_float: the sample's bit pattern, exp_bits of exponent; what the format allows and a binary32 can hold
    const uint32_t b = ih.depth.bits, eb = ih.depth.exp_bits;
    if (b > 32 || eb < 2 || eb > 8 || b < eb + 2 || b - eb - 1 > 23 || (b == 32 && eb != 8)) throw ParseError("unsupported: float sample layout", true);
  }
  if (p.feat.has_noise && !ih.xyb_encoded) throw ParseError("noise on a non-XYB frame", false);
}

// The preview of image i (headers.cc PreviewHeader; JXL_DEC_PREVIEW_IMAGE, jpegxl-sys decode.rs:999-1025): the preview frame decoded as a one-frame image of the
// preview's size by a batch of its own — the same kernels, the frame tail for colour and write — and copied to `dst`.
ImageHeader Batch::PreviewHeaderOf(int i) const {
  const ImageEntry& e = *images_[pub_[i].first_unit];
  if (!e.ih.have_preview) throw ParseError("the image has no preview", false);
  ImageHeader ph = e.ih;
  ph.xsize = e.ih.preview_x; ph.ysize = e.ih.preview_y; ph.have_preview = false; ph.intrinsic_x = ph.intrinsic_y = 0;
  return ph;
}
size_t Batch::PreviewOutputSize(int i, const OutputSpec& o) const {
  if (o.resized() || o.cropped()) throw ParseError("preview: no resized output", false);
  return OutputSize(PreviewHeaderOf(i), o);
}
void Batch::DecodePreview(int i, const OutputSpec& o, void* dst, size_t cap, void* stream_v) {
  if (o.resized() || o.cropped()) throw ParseError("preview: no resized output", false);
  const ImageEntry& e = *images_[pub_[i].first_unit];
  std::shared_ptr<ImageShared> sh(new ImageShared());
  sh->cs = e.cs; sh->ih = PreviewHeaderOf(i);
  std::unique_ptr<ImageEntry> u(new ImageEntry(sh));
  u->frame_bitpos = e.preview_bitpos; u->frame_index = 0; u->complex = true;
  u->visible_frame_index = 1; u->nonvisible_frame_index = 0;
  ParseFrameStart(sh->cs, sh->ih, u->frame_bitpos, &u->plan);
  if (u->plan.frame_type != 0 || u->plan.use_lf_frame) throw ParseError("the preview must be a regular frame", false);
  u->plan.is_last = true;                              // (whatever the frame says: nothing of the image follows it as far as the preview goes)
  CheckFrameSupported(u->plan, sh->ih);
  Batch tmp(device_);
  ParsedImage pi; pi.complex = true; pi.units.push_back(std::move(u));
  tmp.Append(std::move(pi));
  tmp.SetOutput(0, o);
  if (tmp.image(0).out_size > cap) throw ParseError("preview output buffer too small", false);
  tmp.Prepare(stream_v);
  tmp.Run(stream_v);
  tmp.Finish(stream_v);
  tmp.CopyOutputToHost(0, dst, tmp.image(0).out_size, stream_v);
}

void Batch::ParseImage(const uint8_t* data, size_t size, ParsedImage* out, bool allow_partial) {
  std::shared_ptr<ImageShared> sh(new ImageShared());
  bool have_container = false, has_jbrd = false;
  if (!ExtractCodestream(data, size, &sh->cs, &have_container, &has_jbrd, &sh->boxes) && !allow_partial) throw ParseError("truncated", false);
  uint64_t bitpos = 0, preview_bitpos = 0;
  ParseImageHeader(sh->cs, &sh->ih, &bitpos);
  sh->ih.have_container = have_container;
  const ImageHeader& ih = sh->ih;
  if (ih.xyb_encoded) {
    // stage_from_linear.cc: sRGB, linear, pure gamma (incl. DCI), Rec.709, PQ and HLG
    const bool ok = ih.color_default || ih.want_icc || ih.have_gamma || ih.tf == 13 || ih.tf == 8 || ih.tf == 17 || ih.tf == 1 || ih.tf == 16 || ih.tf == 18;
    if (!ok) throw ParseError("unsupported: output transfer function", true);
  }
  if (ih.have_preview) {
    // decode.cc: the preview is a frame of its own in front of the image's frames, its default size the PreviewHeader's.  It is decoded for callers that
    // subscribe to JXL_DEC_PREVIEW_IMAGE only — jpegxl-rs never does (decode.rs:334-347) —, so the frame is stepped over: header + TOC say where it ends.
    ImageHeader ph = ih;
    ph.xsize = ih.preview_x; ph.ysize = ih.preview_y;
    FramePlan pp;
    ParseFrameStart(sh->cs, ph, bitpos, &pp, /*header_and_toc_only=*/true);
    if (pp.frame_type != 0) throw ParseError("the preview must be a regular frame", false);
    preview_bitpos = bitpos;
    bitpos = pp.frame_end_bitpos;
  }
  // every frame of the image (frame_header.cc): reference-only / zero-duration layers first, the last one is displayed
  vec<std::unique_ptr<ImageEntry>> units;
  std::shared_ptr<ImageEntry> lf_frames[5];     // dec_cache.h dc_frames: the latest LF frame of every level (1 .. 4)
  uint32_t visible = 0, nonvisible = 0;
  for (int k = 0;; k++) {
    if (k >= 4096) throw ParseError("unsupported: more than 4096 frames", true);     // (a bound on what one image may make the host allocate; every frame is a unit of the batch)
    std::unique_ptr<ImageEntry> e(new ImageEntry(sh));
    e->has_jbrd = has_jbrd;
    e->frame_bitpos = bitpos;
    e->frame_index = (int)units.size();   // (position among the units of the image: LF frames are none)
    e->pub_index = 0;                     // (set when the image is appended)
    // (allow_partial: a single-frame image cut off inside its PassGroup sections parses as far as its LF part — what a progressive flush shows)
    ParseFrameStart(sh->cs, ih, bitpos, &e->plan, /*header_and_toc_only=*/false, /*allow_partial=*/allow_partial && units.empty());
    const FramePlan& p = e->plan;
    if (p.partial && !(p.frame_type == 0 && p.is_last && !p.have_crop)) throw ParseError("truncated", false);
    if (p.frame_type == 0 || p.frame_type == 3) { visible++; nonvisible = 0; } else nonvisible++;
    e->visible_frame_index = visible; e->nonvisible_frame_index = nonvisible;
    if (p.use_lf_frame) {
      // frame_header.cc kUseDcFrame: the LF image is the LF frame of the next level's samples, one per 8x8 block of this frame
      const std::shared_ptr<ImageEntry>& src = lf_frames[p.lf_level + 1];
      if (!src) throw ParseError("the LF frame this frame refers to is not in the stream", false);
      if (p.subsampled || src->plan.width != p.bw || src->plan.height != p.bh) throw ParseError("LF frame of the wrong size", false);
      e->lf_source = src;
    }
    CheckFrameSupported(p, ih);
    const bool last = p.is_last;
    bitpos = p.frame_end_bitpos;
    if (p.frame_type == 1) {              // an LF frame: kept aside for the frames that refer to it (decoded by Batch::lf_batch_), never displayed
      // (every frame carries the image's extra channels, an LF frame too — libjxl's encoder fills them with zeros there; they are decoded with the frame and not looked at)
      lf_frames[p.lf_level] = std::shared_ptr<ImageEntry>(e.release());
      continue;
    }
    units.push_back(std::move(e));
    if (last) break;
  }
  bool complex = units.size() > 1;
  for (auto& u : units) {
    const FramePlan& p = u->plan;
    bool replace_all = p.blend.mode == 0;
    for (auto& b : p.ec_blend) if (b.mode != 0) replace_all = false;
    if ((p.flags & (1 | 2 | 16)) || p.have_crop || !replace_all || p.frame_type != 0) complex = true;
    if (p.modular && ih.xyb_encoded) complex = true;      // XYB Modular frames go through the float planes
    if (p.modular && p.upsampling != 1) complex = true;
    // (chroma-subsampled frames without anything else: OutputKernel upsamples the chroma planes as it reads them; in the frame tail of complex images ChromaUpsampleKernel does)
  }
  for (auto& x : ih.extra) if (x.depth.is_float) complex = true;   // float extra channels are converted in the frame tail (IntToFloatSample)
  for (auto& u : units) { u->complex = complex; u->preview_bitpos = preview_bitpos; }
  out->units = std::move(units);
  out->complex = complex;
}

size_t Batch::OutputStride(const ImageHeader& ih, const OutputSpec& o, uint32_t* channels) {
  uint32_t nc = o.num_channels;
  bool alpha = false;
  for (auto& e : ih.extra) if (e.type == 0) alpha = true;
  if (o.alpha_from_extra >= 0 && (size_t)o.alpha_from_extra < ih.extra.size()) alpha = true;
  if (nc == 0) nc = (ih.color_space == 1 ? 1 : 3) + (alpha ? 1 : 0);
  if (channels) *channels = nc;
  const size_t bps = o.type == 0 ? 1 : o.type == 2 ? 4 : 2;
  size_t stride = (size_t)OrientedWidth(ih, o) * (o.planar ? 1 : nc) * bps;      // (planar: the row of one plane)
  if (o.align > 1) stride = (stride + o.align - 1) / o.align * o.align;
  return stride;
}
// Orientations 5..8 transpose the image (codestream_header.rs JxlOrientation); applied unless the caller keeps it.
// (1:8 decode, OutputSpec::downscale == 8: one pixel per 8x8 block of the stored picture, the orientation applied to that picture)
// (libjpeg's scaled decode, OutputSpec::jpeg_scale = 2, 4, 8: ceil(side / jpeg_scale) of the stored picture — jdmaster.c jpeg_calc_output_dimensions —, never both)
static uint32_t Scaled(uint32_t v, const OutputSpec& o) { return o.downscale == 8 ? (v + 7) / 8 : o.jpeg_scale > 1 ? (v + o.jpeg_scale - 1) / o.jpeg_scale : v; }
// (resized output, OutputSpec::resize_w / resize_h: that picture is the source of the resize, the output has the target size)
uint32_t Batch::SourceWidth(const ImageHeader& ih, const OutputSpec& o) { return Scaled((!o.keep_orientation && ih.orientation > 4) ? ih.ysize : ih.xsize, o); }
uint32_t Batch::SourceHeight(const ImageHeader& ih, const OutputSpec& o) { return Scaled((!o.keep_orientation && ih.orientation > 4) ? ih.xsize : ih.ysize, o); }
uint32_t Batch::OrientedWidth(const ImageHeader& ih, const OutputSpec& o) { return o.resized() ? o.resize_w : SourceWidth(ih, o); }
uint32_t Batch::OrientedHeight(const ImageHeader& ih, const OutputSpec& o) { return o.resized() ? o.resize_h : SourceHeight(ih, o); }
static size_t SampleBytes(uint32_t type) { return type == 0 ? 1 : type == 2 ? 4 : 2; }
size_t Batch::OutputSize(const ImageHeader& ih, const OutputSpec& o) { return o.planes.any() ? PlanesLayoutOf(ih, o).total : ColorOutputSize(ih, o); }
size_t Batch::PlaneRowStride(const ImageHeader& ih, const OutputSpec& o, const PlaneRequest& r) {
  size_t stride = (size_t)OrientedWidth(ih, o) * SampleBytes(r.type);
  if (r.align > 1) stride = (stride + r.align - 1) / r.align * r.align;
  return stride;
}
// Every refusal is worded "unsupported: extra planes ..."; what concerns the kind of decode first, then the requests one by one.
std::string Batch::PlanesRefusal(const ImageHeader& ih, const OutputSpec& o) {
  if (!o.planes.any()) return std::string();
  const std::string head = "unsupported: extra planes ";
  if (o.downscale == 8) return head + "of the 1:8 decode (downscale 8)";
  if (o.jpeg_scale != 1 || o.resize_u8) return head + "beside a libjpeg-exact output (jpeg_scale, resize_u8)";
  if (o.planes.req.size() > kMaxOutputPlanes) return head + "beyond " + std::to_string(kMaxOutputPlanes) + " requests";
  for (const PlaneRequest& r : o.planes.req) {
    if (r.index >= ih.extra.size()) return head + "of extra channel " + std::to_string(r.index) + ": the image has " + std::to_string(ih.extra.size()) + " extra channels";
    if (r.type > 3) return head + "of an unknown sample type";
    if (r.affine && r.type != 2 && r.type != 3) return head + "with scale / bias need a float sample type";
  }
  return std::string();
}
PlanesLayout Batch::PlanesLayoutOf(const ImageHeader& ih, const OutputSpec& o) {
  const size_t color = ColorOutputSize(ih, o);
  const std::string why = PlanesRefusal(ih, o);
  if (!why.empty()) throw ParseError(why, true);
  PlanesLayout l;
  if (!o.planes.any()) { l.offset = l.total = color; return l; }
  const size_t rows = OrientedHeight(ih, o);
  size_t tight = 0, sample = 1;      // the largest plane, the largest sample
  for (const PlaneRequest& r : o.planes.req) { tight = std::max(tight, PlaneRowStride(ih, o, r) * rows); sample = std::max(sample, SampleBytes(r.type)); }
  size_t def_offset, def_pitch;
  if (o.planar) {
    uint32_t nc;
    const size_t cstride = OutputStride(ih, o, &nc);
    const size_t cplane = o.plane_stride ? o.plane_stride : cstride * rows;
    def_offset = (size_t)nc * cplane; def_pitch = cplane;
    if (!o.planes.plane_stride && tight > cplane) throw ParseError("extra planes: a plane of this image takes " + std::to_string(tight) + " bytes, the colour layout's plane_stride is " + std::to_string(cplane), false);
  } else {
    def_offset = (color + 15) / 16 * 16; def_pitch = tight;
  }
  l.offset = o.planes.offset ? o.planes.offset : def_offset;
  l.pitch = o.planes.plane_stride ? o.planes.plane_stride : def_pitch;
  if (l.offset < def_offset) throw ParseError("extra planes: offset " + std::to_string(l.offset) + " is below the default, " + std::to_string(def_offset) + " bytes behind the start of the colour output", false);
  if (l.offset % sample) throw ParseError("extra planes: offset must be a multiple of the sample size", false);
  if (l.pitch < std::max(tight, def_pitch)) throw ParseError("extra planes: plane_stride " + std::to_string(l.pitch) + " is below the default, " + std::to_string(std::max(tight, def_pitch)) + " bytes", false);
  if (l.pitch % sample) throw ParseError("extra planes: plane_stride must be a multiple of the sample size", false);
  l.total = l.offset + o.planes.req.size() * l.pitch;
  return l;
}
size_t Batch::ColorOutputSize(const ImageHeader& ih, const OutputSpec& o) {
  // jpegxl-sys decode.rs:1100 JxlDecoderImageOutBufferSize: stride * (h - 1) + w * C * bytes
  uint32_t nc;
  const size_t stride = OutputStride(ih, o, &nc);
  const size_t bps = o.type == 0 ? 1 : o.type == 2 ? 4 : 2;
  const std::string no_resize = ResizeRefusal(ih, o);
  if (!no_resize.empty()) throw ParseError(no_resize, false);
  const std::string why = LayoutRefusal(ih, o);
  if (!why.empty()) throw ParseError(why, false);
  if (o.planar) return (size_t)nc * (o.plane_stride ? o.plane_stride : stride * OrientedHeight(ih, o));
  return stride * (OrientedHeight(ih, o) - 1) + (size_t)OrientedWidth(ih, o) * nc * bps;
}
std::string Batch::LayoutRefusal(const ImageHeader& ih, const OutputSpec& o) {
  if (o.affine && o.type != 2 && o.type != 3) return "affine output needs a float sample type";
  if (o.planar && o.plane_stride) {
    const size_t bps = o.type == 0 ? 1 : o.type == 2 ? 4 : 2;
    const size_t tight = OutputStride(ih, o, nullptr) * OrientedHeight(ih, o);
    if (o.plane_stride < tight) return "planar output: plane_stride " + std::to_string(o.plane_stride) + " is below the " + std::to_string(tight) + " bytes one plane of this image takes";
    if (o.plane_stride % bps) return "planar output: plane_stride must be a multiple of the sample size";
  }
  return std::string();
}
std::string Batch::ResizeRefusal(const ImageHeader& ih, const OutputSpec& o) {
  if (!o.resized()) return o.cropped() ? "resized output: a crop needs a target size" : o.mirror || o.resize_filter ? "resized output: a filter or a mirror needs a target size" : std::string();
  if (o.resize_filter > 1) return "resized output: filter " + std::to_string(o.resize_filter) + " is not known (0 = triangle, 1 = cubic)";
  if (o.resize_w == 0 || o.resize_h == 0) return "resized output: a target side of 0";
  if (o.resize_w > 65535 || o.resize_h > 65535) return "resized output: a target side above 65535";
  if (!o.cropped()) return std::string();
  const uint32_t w = SourceWidth(ih, o), h = SourceHeight(ih, o);
  if (o.crop_w == 0 || o.crop_h == 0) return "resized output: the crop is empty";
  if (o.crop_x0 >= w || o.crop_w > w - o.crop_x0 || o.crop_y0 >= h || o.crop_h > h - o.crop_y0)
    return "resized output: the crop " + std::to_string(o.crop_w) + " x " + std::to_string(o.crop_h) + " at (" + std::to_string(o.crop_x0) + ", " + std::to_string(o.crop_y0) +
           ") leaves the " + std::to_string(w) + " x " + std::to_string(h) + " picture";
  return std::string();
}
// One axis of the resize (OutputSpec::resize_w / resize_h): a filter kernel k of radius r with half-pixel centres, widened by the ratio when it shrinks.  filter 0: the
// triangle, k(x) = max(0, 1 - |x|), r = 1 (Pillow's BILINEAR reduce, torch's interpolate(mode="bilinear", antialias=True)); filter 1: cubic convolution with a = -0.5,
// k(x) = ((a + 2)|x| - (a + 3))|x|^2 + 1 below 1, a(((|x| - 5)|x| + 8)|x| - 4) below 2, r = 2 (Pillow's BICUBIC, torch's mode="bicubic", antialias=True).
// n_in samples -> n_out; scale = n_in / n_out, support = max(scale, 1), output i has its centre at c = scale x (i + 0.5) and takes the samples j of
// [max(0, int(c - r x support + 0.5)), min(n_in, int(c + r x support + 0.5))) with weight k((j - c + 0.5) / support) over the sum of these: the range is cut at the edges and
// the weights renormalised, nothing is mirrored or clamped.  Everything in double; a normalised weight is rounded to f32 once.  Samples of weight 0 at either end of a
// range are left out (they change no sum; at n_in == n_out one tap of weight 1 is left, for either filter: a copy).
// lo[i]: first sample of output i; its weights are weight[first[i]] .. weight[first[i + 1] - 1].
static double ResizeFilterWeight(uint32_t filter, double x) {
  x = std::fabs(x);
  if (filter == 0) return std::max(0.0, 1.0 - x);
  const double a = -0.5;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0;
  if (x < 2.0) return a * (((x - 5.0) * x + 8.0) * x - 4.0);
  return 0.0;
}
static void ResizeAxis(uint32_t filter, uint32_t n_in, uint32_t n_out, vec<uint32_t>* lo, vec<uint32_t>* first, vec<float>* weight) {
  const double scale = (double)n_in / (double)n_out, support = std::max(scale, 1.0), reach = (filter ? 2.0 : 1.0) * support;
  lo->assign(n_out, 0); first->assign((size_t)n_out + 1, 0); weight->clear();
  vec<double> w;
  for (uint32_t i = 0; i < n_out; i++) {
    const double c = scale * ((double)i + 0.5);
    int64_t a = std::max<int64_t>(0, (int64_t)(c - reach + 0.5)), b = std::min<int64_t>((int64_t)n_in, (int64_t)(c + reach + 0.5));
    w.assign((size_t)(b - a), 0.0);
    double sum = 0.0;
    for (int64_t j = a; j < b; j++) { w[(size_t)(j - a)] = ResizeFilterWeight(filter, ((double)j - c + 0.5) / support); sum += w[(size_t)(j - a)]; }
    const int64_t a0 = a;
    while (b - a > 1 && w[(size_t)(b - 1 - a0)] == 0.0) b--;
    while (b - a > 1 && w[(size_t)(a - a0)] == 0.0) a++;
    (*lo)[i] = (uint32_t)a; (*first)[i] = (uint32_t)weight->size();
    for (int64_t j = a; j < b; j++) weight->push_back((float)(w[(size_t)(j - a0)] / sum));
  }
  (*first)[n_out] = (uint32_t)weight->size();
}
// The integer form (OutputSpec::resize_u8; the rule: include/jxl_hip.h): the same ranges and the same normalised double weights — not their f32 roundings —, each as
// kk = int(w x 2^22 + 0.5) for w >= 0, int(w x 2^22 - 0.5) below, truncating: Pillow's 8-bit coefficients (Resample.c normalize_coeffs_8bpc, PRECISION_BITS = 32 - 8 - 2).
// They are not renormalised.  Taps of kk == 0 at either end of a range are left out (they change no sum); one tap always stays.
static void ResizeAxisInt(uint32_t filter, uint32_t n_in, uint32_t n_out, vec<uint32_t>* lo, vec<uint32_t>* first, vec<int32_t>* weight) {
  const double scale = (double)n_in / (double)n_out, support = std::max(scale, 1.0), reach = (filter ? 2.0 : 1.0) * support;
  lo->assign(n_out, 0); first->assign((size_t)n_out + 1, 0); weight->clear();
  vec<double> w;
  vec<int32_t> kk;
  for (uint32_t i = 0; i < n_out; i++) {
    const double c = scale * ((double)i + 0.5);
    int64_t a = std::max<int64_t>(0, (int64_t)(c - reach + 0.5)), b = std::min<int64_t>((int64_t)n_in, (int64_t)(c + reach + 0.5));
    if (b <= a) { a = std::min<int64_t>(a, (int64_t)n_in - 1); b = a + 1; }      // (cannot happen for n_in >= 1: the centre's own sample is inside the reach)
    w.assign((size_t)(b - a), 0.0); kk.assign((size_t)(b - a), 0);
    double sum = 0.0;
    for (int64_t j = a; j < b; j++) { w[(size_t)(j - a)] = ResizeFilterWeight(filter, ((double)j - c + 0.5) / support); sum += w[(size_t)(j - a)]; }
    for (size_t t = 0; t < w.size(); t++) { const double v = w[t] / sum; kk[t] = v < 0.0 ? (int32_t)(v * 4194304.0 - 0.5) : (int32_t)(v * 4194304.0 + 0.5); }
    const int64_t a0 = a;
    while (b - a > 1 && kk[(size_t)(b - 1 - a0)] == 0) b--;
    while (b - a > 1 && kk[(size_t)(a - a0)] == 0) a++;
    (*lo)[i] = (uint32_t)a; (*first)[i] = (uint32_t)weight->size();
    for (int64_t j = a; j < b; j++) weight->push_back(kk[(size_t)(j - a0)]);
  }
  (*first)[n_out] = (uint32_t)weight->size();
}
void Batch::OutputDims(int i, const OutputSpec& o, uint32_t* w, uint32_t* h) const {
  const ImageEntry& first = *images_[pub_[i].first_unit];
  *w = first.ih.xsize; *h = first.ih.ysize;
  if (o.only_frame >= 0 && o.only_frame < pub_[i].num_units) { const FramePlan& p = images_[pub_[i].first_unit + o.only_frame]->plan; *w = p.frame_w; *h = p.frame_h; }
}
size_t Batch::OutputSizeOf(int i, const OutputSpec& o) const {
  ImageHeader dims = images_[pub_[i].first_unit]->ih;       // (OutputStride / OutputSize only look at the size, the orientation and the channel list)
  OutputDims(i, o, &dims.xsize, &dims.ysize);
  if (o.color_set) {      // (what SetOutput would refuse for this image: a pipeline job asks here first and lets the image fail alone)
    const std::string why = ColourRefusal(dims, o);
    if (!why.empty()) throw ParseError(why, true);
  }
  return OutputSize(dims, o);
}
static float IntMul(const OutputSpec& o) { const uint32_t full = o.type == 0 ? 8 : 16; const uint32_t b = o.int_bits && o.int_bits < full ? o.int_bits : full; return (float)((1u << b) - 1); }
// Where the write stage puts the image's pixels (work: the arena that holds the output unless the caller named a device buffer)
// A resized output (OutputSpec::resize_w / resize_h): the write stage leaves the picture — oriented, every slot of the output — as plain interleaved f32 among the pixel planes
// (big: it lives from the write stage to the resize behind it, like the planes the write stage reads), and ResizeKernel writes the caller's destination from it
// (EnqueueResizes, resize_target = true: the destination as it is described otherwise, the orientation applied already)
OutputDesc FillOutput(const ImageEntry& e, uint8_t* work, uint8_t* big, bool resize_target) {
  OutputDesc d{};
  if (e.out.resized() && !resize_target) {
    d.out = big + e.off_resize_src;
    d.out_stride = (size_t)e.src_w * e.out.num_channels * 4; d.out_channels = e.out.num_channels; d.out_type = 2; d.out_int_mul = 1.0f;
    // (OutputSpec::resize_u8: the same picture as interleaved u8 — the libjpeg-exact write stage stores its sample k as k — for ResizeU8Kernel)
    if (e.out.resize_u8) { d.out_stride = (size_t)e.src_w * e.out.num_channels; d.out_type = 0; d.out_int_mul = 255.0f; }
    d.out_orient = e.out.keep_orientation ? 1 : e.ih.orientation; d.is_gray = e.ih.color_space == 1;
    return d;
  }
  d.out = (uint8_t*)(e.out.device_ptr ? e.out.device_ptr : work + e.off_out);
  d.planar = e.out.planar; d.plane_stride = !e.out.planar ? 0 : e.out.plane_stride ? e.out.plane_stride : e.color_size / std::max(1u, e.out.num_channels);
  d.affine = e.out.affine;
  for (int c = 0; c < 4; c++) { d.scale[c] = e.out.scale[c]; d.bias[c] = e.out.bias[c]; }
  d.out_stride = e.out_stride; d.out_channels = e.out.num_channels; d.out_type = e.out.type; d.out_big_endian = e.out.big_endian; d.out_int_mul = IntMul(e.out);
  d.out_orient = e.out.keep_orientation ? 1 : e.ih.orientation; d.is_gray = e.ih.color_space == 1;
  if (resize_target) d.out_orient = 1;
  return d;
}
// Requested extra-channel plane k (OutputSpec::planes) in the caller's destination: slot 0 of a planar one-channel output at planes_layout.offset + k x pitch, in the
// request's own format; never int_bits (a plane is the channel as it is).  The write of a resized output goes to the plane's f32 resize source instead (frame_tail.cc
// TailPlanes builds that descriptor itself); resize_target: the destination as ResizeKernel<1> stores into it, the orientation applied already.
OutputDesc FillPlaneOutput(const ImageEntry& e, size_t k, uint8_t* work, bool resize_target) {
  const PlaneRequest& r = e.out.planes.req[k];
  ImageHeader dims = e.ih;
  dims.xsize = e.out.resized() ? e.out.resize_w : e.src_w; dims.ysize = 1; dims.orientation = 1;      // (PlaneRowStride reads the oriented width alone)
  OutputDesc d{};
  d.out = (uint8_t*)(e.out.device_ptr ? e.out.device_ptr : work + e.off_out) + e.planes_layout.offset + k * e.planes_layout.pitch;
  d.planar = 1; d.plane_stride = e.planes_layout.pitch; d.out_channels = 1;
  d.affine = r.affine ? 1 : 0;
  for (int c = 0; c < 4; c++) { d.scale[c] = r.scale; d.bias[c] = r.bias; }
  d.out_stride = Batch::PlaneRowStride(dims, OutputSpec(), r);
  d.out_type = r.type; d.out_big_endian = r.big_endian; d.out_int_mul = r.type == 0 ? 255.0f : 65535.0f;
  d.out_orient = resize_target || e.out.keep_orientation ? 1 : e.ih.orientation; d.is_gray = 1;
  return d;
}
// What the 1:8 decode takes: single-frame VarDCT images that carry their own LF coefficients and end in their own pixels (no frame tail).
static std::string DownscaleRefusalOf(int num_units, const ImageEntry& e) {
  const FramePlan& p = e.plan;
  const char* what = nullptr;
  if (num_units != 1) what = "an image with several frames";
  else if (p.modular) what = "a Modular frame";
  else if (p.use_lf_frame || e.lf_source) what = "a frame that takes its LF image from an LF frame";
  else if (!e.ih.extra.empty()) what = "an image with extra channels";
  else if (p.upsampling != 1) what = "an upsampled frame";
  else if (e.complex) what = "a frame with patches, splines, noise, a crop or blending";
  return what ? std::string("unsupported: downscaled decode of ") + what : std::string();
}
std::string Batch::DownscaleRefusal(int i) const { return DownscaleRefusalOf(pub_[i].num_units, *images_[pub_[i].first_unit]); }
// Which groups the libjpeg-exact decode of a crop needs (decoder.h jpeg_region), for a single-frame JPEG transcode that decode takes:
//   1. the crop (source picture: oriented, at jpeg_scale s) is mapped back through the orientation — the inverse of pixel_ops.h OutPixelPtr — to rect[] = x0, y0, w, h of
//      the stored picture at scale s, ceil(xsize / s) x ceil(ysize / s);
//   2. a luma block covers n x n of its pixels, n = 8 / s: blocks floor(first / n) .. floor(last / n) per axis;
//   3. widened outwards to whole MCUs of (1 << hs) x (1 << vs) luma blocks (hs / vs: the chroma shifts; grey and 4:4:4: 1 x 1);
//   4. one MCU more on every side — h2v1 / h2v2 fancy upsampling reads chroma sample i +- 1, which lies in the neighbouring chroma block at every scale, a block
//      holding at least one sample; taken at 4:4:4 and grey too: one rule —, clamped to the frame's block grid;
//   5. groups[] = gx0, gy0, gx1, gy1: every group (32 x 32 blocks) that block rectangle touches, gx0 <= gx < gx1, gy0 <= gy < gy1.
static bool JpegRegionRule(const ImageEntry& e, const OutputSpec& o, uint32_t groups[4], uint32_t rect[4]) {
  const FramePlan& p = e.plan;
  const uint32_t s = o.jpeg_scale ? o.jpeg_scale : 1, n = 8 / s;
  const uint32_t w = (e.ih.xsize + s - 1) / s, h = (e.ih.ysize + s - 1) / s;
  if (!n || !w || !h || !p.bw || !p.bh || !o.crop_w || !o.crop_h) return false;
  const uint32_t X0 = o.crop_x0, Y0 = o.crop_y0, X1 = o.crop_x0 + o.crop_w - 1, Y1 = o.crop_y0 + o.crop_h - 1;      // inclusive, in the oriented picture
  const uint32_t orient = o.keep_orientation ? 1 : e.ih.orientation;
  const uint32_t ow = orient > 4 ? h : w, oh = orient > 4 ? w : h;
  if (X1 >= ow || Y1 >= oh) return false;
  uint32_t x0 = X0, x1 = X1, y0 = Y0, y1 = Y1;
  switch (orient) {
    case 2: x0 = w - 1 - X1; x1 = w - 1 - X0; break;
    case 3: x0 = w - 1 - X1; x1 = w - 1 - X0; y0 = h - 1 - Y1; y1 = h - 1 - Y0; break;
    case 4: y0 = h - 1 - Y1; y1 = h - 1 - Y0; break;
    case 5: x0 = Y0; x1 = Y1; y0 = X0; y1 = X1; break;
    case 6: x0 = Y0; x1 = Y1; y0 = h - 1 - X1; y1 = h - 1 - X0; break;
    case 7: x0 = w - 1 - Y1; x1 = w - 1 - Y0; y0 = h - 1 - X1; y1 = h - 1 - X0; break;
    case 8: x0 = w - 1 - Y1; x1 = w - 1 - Y0; y0 = X0; y1 = X1; break;
    default: break;
  }
  rect[0] = x0; rect[1] = y0; rect[2] = x1 - x0 + 1; rect[3] = y1 - y0 + 1;
  const bool grey = e.ih.color_space == 1;
  const uint32_t mx = grey ? 1u : 1u << p.hs[0], my = grey ? 1u : 1u << p.vs[0];      // luma blocks per MCU (Y is channel 1; Cb / Cr share their shifts)
  auto axis = [](uint32_t first, uint32_t last, uint32_t n, uint32_t mcu, uint32_t nblocks, uint32_t* g0, uint32_t* g1) {
    const uint32_t m0 = first / n / mcu, m1 = last / n / mcu;                  // MCUs of the crop's blocks
    const uint32_t b0 = (m0 ? m0 - 1 : 0) * mcu;                                // one MCU more on either side
    const uint32_t b1 = std::min((m1 + 2) * mcu - 1, nblocks - 1);
    *g0 = std::min(b0, nblocks - 1) / 32; *g1 = b1 / 32 + 1;
  };
  axis(x0, x1, n, mx, p.bw, &groups[0], &groups[2]);
  axis(y0, y1, n, my, p.bh, &groups[1], &groups[3]);
  return groups[0] < groups[2] && groups[1] < groups[3] && groups[2] <= p.xgroups && groups[3] <= p.ygroups;
}
void Batch::SetOutput(int i, const OutputSpec& o) {
  ImageEntry& e = *images_[pub_[i].first_unit];
  if (o.planes.any()) {      // (first: a request the decode cannot serve is answered in its own words, whatever else the output asks for)
    const std::string why = PlanesRefusal(e.ih, o);
    if (!why.empty()) throw ParseError(why, true);
  }
  if (o.downscale != 1) {
    if (o.downscale != 8) throw ParseError("downscale must be 1 or 8", false);
    const std::string why = DownscaleRefusal(i);
    if (!why.empty()) throw ParseError(why, true);
    if (o.only_frame >= 0 || o.upto_frame >= 0) throw ParseError("unsupported: downscaled decode of a single frame of an animation", true);
  }
  if (o.jpeg_scale != 1) {
    if (o.jpeg_scale != 2 && o.jpeg_scale != 4 && o.jpeg_scale != 8) throw ParseError("jpeg_scale must be 1, 2, 4 or 8", false);
    if (o.downscale != 1) throw ParseError("unsupported: jpeg_scale " + std::to_string(o.jpeg_scale) + " together with downscale " + std::to_string(o.downscale) + " (one of the two scaled decodes)", true);
    // (only the libjpeg-exact decode writes such an output: what it does not take has no scaled picture at all)
    std::string why;
    if (!CanDecodeJpegPixelsAs(i, o, &why)) throw ParseError(why, true);
  }
  if (o.resize_u8) {
    // the integer resample (OutputSpec::resize_u8) is defined over the u8 picture libjpeg gives: it needs a target, and an image that decode takes
    if (!o.resized()) throw ParseError("unsupported: integer resample without a target size (resize_u8 needs a resized output)", true);
    if (o.downscale != 1) throw ParseError("unsupported: integer resample together with downscale " + std::to_string(o.downscale) + " (the 1:8 decode is not a libjpeg-exact one)", true);
    std::string why;
    if (!CanDecodeJpegPixelsAs(i, o, &why)) throw ParseError("unsupported: integer resample of an image the libjpeg-exact decode does not take (" + why + ")", true);
  }
  if (o.only_frame >= pub_[i].num_units) throw ParseError("non-coalesced output: no such frame", false);
  if (o.color_set) {
    const std::string why = ColourRefusal(e.ih, o);
    if (!why.empty()) throw ParseError(why, true);
  }
  // Everything that can refuse the output — a layout, a resize or a crop the image does not fit, an offset or pitch of the planes below its default — is computed
  // before anything of the entry is assigned: a call that throws leaves the entry, spec and sizes alike, as it was.
  OutputSpec out = o;
  // (a lone frame that fills the image is the same either way: the plain path keeps it)
  if (o.only_frame == 0 && pub_[i].num_units == 1 && !e.plan.have_crop) out.only_frame = -1;
  if (o.upto_frame >= pub_[i].num_units - 1 || o.only_frame >= 0) out.upto_frame = -1;     // (the last frame's composite is the image)
  ImageHeader dims = e.ih;
  OutputDims(i, out, &dims.xsize, &dims.ysize);
  uint32_t nc;
  const size_t out_stride = OutputStride(dims, o, &nc);
  out.num_channels = nc;
  const size_t color_size = ColorOutputSize(dims, o);
  const PlanesLayout planes_layout = PlanesLayoutOf(dims, o);
  e.out = out;
  e.jpeg_dc_eligible = JpegDcEligibleOf(e.plan, o);      // (jpeg_scale 8: CanDecodeJpegPixelsAs has taken the image above)
  e.out_stride = out_stride; e.color_size = color_size; e.planes_layout = planes_layout;
  e.out_size = planes_layout.total;
  e.src_w = SourceWidth(dims, o); e.src_h = SourceHeight(dims, o);
  // (the crop lies inside the source picture: OutputSize above has thrown otherwise)
  e.jpeg_region_eligible = false;
  if (o.cropped() && o.resized() && o.downscale == 1 && CanDecodeJpegPixelsAs(i, o, nullptr)) e.jpeg_region_eligible = JpegRegionRule(e, o, e.region_groups, e.region_rect);
  e.deliver_frames.clear();
  prepared_ = false;
}
bool Batch::JpegRegionOf(int i, uint32_t groups[4]) const {
  const ImageEntry& e = *images_[pub_[i].first_unit];
  if (!e.jpeg_region_eligible || JpegDcOnly(i)) return false;
  for (int k = 0; k < 4; k++) groups[k] = e.region_groups[k];
  return true;
}
bool Batch::JpegRegionUnit(int unit) const {
  const ImageEntry& e = *images_[unit];
  return jpeg_region && e.frame_index == 0 && e.jpeg_region_eligible && !JpegDcOnlyUnit(unit);
}
void Batch::SetOutputAllFrames(int i, const OutputSpec& o, const vec<int>& frames) {
  if (o.device_ptr || o.only_frame >= 0 || frames.empty()) throw ParseError("SetOutputAllFrames: internal output buffers, coalesced frames only", false);
  if (o.planar || o.affine) throw ParseError("SetOutputAllFrames: interleaved output without scale / bias only", false);
  if (o.resized() || o.cropped()) throw ParseError("SetOutputAllFrames: no resized output", false);
  if (o.planes.any()) throw ParseError("unsupported: extra planes of kept animation canvases (all frames in one decode)", true);
  if (ConvertsNonXyb(images_[pub_[i].first_unit]->ih, o)) throw ParseError("unsupported: output colour conversion of kept animation canvases of an image that is not XYB (all frames in one decode)", true);
  for (size_t k = 0; k < frames.size(); k++)
    if (frames[k] < 0 || frames[k] >= pub_[i].num_units || (k && frames[k] <= frames[k - 1])) throw ParseError("SetOutputAllFrames: frame list must be ascending positions among the image's frames", false);
  OutputSpec oo = o;
  oo.upto_frame = -1;
  SetOutput(i, oo);
  images_[pub_[i].first_unit]->deliver_frames = frames;
}

uint64_t Batch::total_pixels() const { uint64_t n = 0; for (auto& pi : pub_) { const ImageHeader& ih = images_[pi.first_unit]->ih; n += (uint64_t)ih.xsize * ih.ysize; } return n; }
uint64_t Batch::compressed_bytes() const { uint64_t n = 0; for (auto& pi : pub_) n += images_[pi.first_unit]->cs.size; return n; }
void Batch::StageBytes(uint64_t out[6]) const {
  // Compulsory (ALGORITHMIC) HBM traffic of each stage as the kernels are actually structured — every input the stage cannot avoid
  // reading once, every output written once:
  //  lf     LfGroup sections -> quantised LF (3 x i32) + block info + coefficient offset per 8x8 block
  //  lfpost LF dequantisation, smoothing, LLF, EPF sigma: 76 B per block
  //  hf     PassGroup sections -> the non-zero coefficients (i32 each; counted by the kernel, known after the first Finish)
  //  idct   coefficient planes as stored (dense i32: 12 B/px) -> 3 f32 planes (12 B/px)
  //  filter gaborish + EPF (+ colour + write when the stage's last kernel writes the pixels — the fused kernel of the headline, the tiled EPF passes of every other
  //         plain frame): 12 B/px in, C x bytes out — ONCE, however many kernels the stage is split into (their intermediate planes are traffic, not algorithmic
  //         bytes: SURVEY.md 8(d)).  Frames whose filters end in the planes (upsampling, the frame tail of complex images): 12 B/px in, 12 B/px out
  //  out    those frames only: 12 B/px in, C x bytes out
  for (int i = 0; i < 6; i++) out[i] = 0;
  for (size_t u = 0; u < images_.size(); u++) {
    const ImageEntry& e = *images_[u];
    const FramePlan& p = e.plan;
    if (p.modular) continue;
    const ImageEntry& first = *images_[pub_[e.pub_index].first_unit];
    const uint64_t nblk = (uint64_t)p.bw * p.bh, npx = (uint64_t)p.width * p.height;
    uint64_t lf_sec = 0, hf_sec = 0;
    if (p.single_section) { lf_sec = e.cs.size / 4; hf_sec = e.cs.size; }
    else {
      for (uint32_t s = 1; s < 1 + p.num_lf_groups; s++) lf_sec += p.sections[s].size;
      for (size_t s = 2 + p.num_lf_groups; s < p.sections.size(); s++) hf_sec += p.sections[s].size;
    }
    const uint64_t bps = first.out.type == 0 ? 1 : first.out.type == 2 ? 4 : 2;
    uint64_t out_px = (uint64_t)first.out.num_channels * bps;
    if (first.out.resized()) {
      // resized output: the write stage's pixels are the f32 intermediate; ResizeKernel reads the resampled rectangle of it and writes the target in the caller's format (once per
      // image; the horizontally filtered rows between its two passes are traffic, not algorithmic bytes)
      out_px = (uint64_t)first.out.num_channels * (first.out.resize_u8 ? 1 : 4);      // (OutputSpec::resize_u8: a u8 intermediate, ResizeU8Kernel)
      if (&e == &first) {
        const uint64_t rect = first.out.cropped() ? (uint64_t)first.out.crop_w * first.out.crop_h : (uint64_t)first.src_w * first.src_h;
        out[5] += rect * out_px + (uint64_t)first.out.resize_w * first.out.resize_h * first.out.num_channels * bps;
      }
    }
    out[0] += lf_sec + nblk * (3 * 4 + 4 + 4);
    out[1] += nblk * (12 + 12 + 12 + 12 + 12 + 16);
    if (first.out.downscale == 8) {      // 1:8 decode: no HF stage, no IDCT, no filters; LfOutputKernel reads three LF samples and writes one pixel per block
      out[5] += (uint64_t)((p.width + 7) / 8) * ((p.height + 7) / 8) * (12 + out_px);
      continue;
    }
    if (JpegDcOnlyUnit((int)u)) {        // DC-only: no HF stage, no IDCT; JpegDcOutKernel reads one DC term (i32) per component and writes one pixel of the scaled picture
      out[5] += (uint64_t)((e.ih.xsize + 7) / 8) * ((e.ih.ysize + 7) / 8) * (4 * (e.ih.color_space == 1 ? 1 : 3) + out_px);
      continue;
    }
    // pixels through the IDCT and through the write stage: the frame's — or, for a frame the libjpeg-exact decode planned last decodes by region (hf_by_region_: not after
    // a Run, which decodes every group whatever lists the frames carry), the sections of the region's groups, the pixels of their blocks, the crop's rectangle
    uint64_t idct_px = npx, write_px = npx;
    if (hf_by_region_ && JpegRegionUnit((int)u) && !p.single_section) {
      const uint32_t* rg = e.region_groups;
      hf_sec = 0;
      for (uint32_t gy = rg[1]; gy < rg[3]; gy++) for (uint32_t gx = rg[0]; gx < rg[2]; gx++) {
        const size_t s = 2 + (size_t)p.num_lf_groups + (size_t)gy * p.xgroups + gx;
        if (s < p.sections.size()) hf_sec += p.sections[s].size;
      }
      idct_px = (uint64_t)(std::min(rg[2] * 32, p.bw) - rg[0] * 32) * (std::min(rg[3] * 32, p.bh) - rg[1] * 32) * 64;
      write_px = (uint64_t)e.region_rect[2] * e.region_rect[3];
    }
    out[2] += hf_sec + (u < hf_written_.size() ? (uint64_t)hf_written_[u] * 4 : 0);
    out[3] += idct_px * (12 + 12);
    ImageHeader colour_store;
    const bool fused = p.lf.gab && p.lf.epf_iters == 1 && e.ih.xyb_encoded && SimpleTransfer(ColourHeader(e.ih, first.out, &colour_store)) && p.upsampling == 1 && !e.complex && !cfg.force_unfused_filters;
    const bool any_filter = p.lf.gab || p.lf.epf_iters > 0;
    const bool epf_writes = !fused && p.lf.epf_iters >= 1 && p.upsampling == 1 && !e.complex && cfg.debug_stop_after == 0;    // kernels.hip EpfWritesOutput
    if (fused || epf_writes) out[4] += npx * (12 + out_px);
    else {
      if (any_filter) out[4] += npx * 24;
      out[5] += write_px * (12 + out_px);
    }
  }
}

// Testing: copies one of the device buffers of image i's first frame to the host (after a decode, JxlHipBatchDebugRead): the planes
// between the stages ("debug_stop_after") and the inputs of the pixel stages.  Returns the bytes the buffer holds; copies min(that, cap).
size_t Batch::DebugRead(int i, const std::string& name, int c, void* dst, size_t cap, void* stream_v) {
  if (!prepared_ || i < 0 || (size_t)i >= pub_.size() || c < 0 || (c > 2 && name != "qtable") || c >= 51) throw ParseError("DebugRead: no such image / channel", false);
  if (name == "qtable") {     // dequantisation table (1 / weight) of quant kind c / 3, channel c % 3: 64 x rows x cols floats (kKindRows / kKindCols)
    const FrameDev& f0 = frames_host_[pub_[i].first_unit];
    const size_t bytes = (size_t)64 * kKindRows[c / 3] * kKindCols[c / 3] * 4;
    if (!f0.qtable[c]) throw ParseError("DebugRead: no such table", false);
    HIP_CHECK(hipStreamSynchronize((hipStream_t)stream_v));
    if (dst && cap) HIP_CHECK(hipMemcpy(dst, f0.qtable[c], std::min(bytes, cap), hipMemcpyDeviceToHost));
    return bytes;
  }
  const int u = pub_[i].first_unit;
  const FrameDev& f = frames_host_[u];
  const FramePlan& p = images_[u]->plan;
  if (p.modular) throw ParseError("DebugRead: not a VarDCT frame", false);
  const size_t nb = (size_t)p.bw * p.bh, npx = nb * 64;
  const void* src = nullptr; size_t bytes = 0;
  if (name == "plane_a") { src = f.plane_a[c]; bytes = npx * 4; }
  else if (name == "plane_b") { src = f.plane_b[c]; bytes = npx * 4; }
  else if (name == "lf") { src = f.lf[c]; bytes = nb * 4; }
  else if (name == "lf_smooth") { src = f.lf_tmp[c]; bytes = nb * 4; }     // the LF samples after the adaptive smoothing
  else if (name == "llf") { src = f.llf[c]; bytes = nb * 4; }
  else if (name == "lfq") { src = f.lfq[c]; bytes = nb * 4; }
  else if (name == "inv_sigma") { src = f.inv_sigma; bytes = nb * 4; }
  else if (name == "blk_info") { src = f.blk_info; bytes = nb * 4; }
  else if (name == "coef_off") { src = f.coef_off; bytes = nb * 4; }
  else if (name == "coeff") { src = f.coeff[c]; bytes = (size_t)p.num_groups * 65536 * 4; }
  else if (name == "qtable") { throw ParseError("DebugRead: qtable takes kind * 3 + channel", false); }
  else if (name == "up_weights") { src = f.up_weights; bytes = p.upsampling == 2 ? 60 : p.upsampling == 4 ? 220 : p.upsampling == 8 ? 840 : 0; }   // the 15 / 55 / 210 stored upsampling weights in use
  else if (name == "ytox") { src = f.ytox; bytes = (size_t)((p.bw + 7) / 8) * ((p.bh + 7) / 8); }
  else if (name == "ytob") { src = f.ytob; bytes = (size_t)((p.bw + 7) / 8) * ((p.bh + 7) / 8); }
  else throw ParseError("DebugRead: unknown buffer " + name, false);
  if (!src) throw ParseError("DebugRead: buffer " + name + " is not allocated for this batch", false);
  HIP_CHECK(hipStreamSynchronize((hipStream_t)stream_v));
  if (dst && cap) HIP_CHECK(hipMemcpy(dst, src, std::min(bytes, cap), hipMemcpyDeviceToHost));
  return bytes;
}

void Batch::HashPostOps(uint64_t* h) const {
  if (lf_batch_) lf_batch_->HashPostOps(h);
  for (auto& op : post_ops_) for (const char* c = op.first;; c++) { *h = (*h ^ (uint8_t)*c) * 1099511628211ull; if (!*c) break; }   // (each name with its terminating zero)
}

int64_t Batch::Info(const std::string& name) const {
  if (name == "lf_simt_frames" || name == "lf_legacy_frames") {
    int64_t simt = 0, legacy = 0;
    for (size_t i = 0; i < frames_host_.size() && i < images_.size(); i++) if (!images_[i]->plan.modular) (frames_host_[i].lf_simt ? simt : legacy)++;
    return name == "lf_simt_frames" ? simt : legacy;
  }
  if (name == "hf_nonzeros") { int64_t t = 0; for (uint32_t v : hf_written_) t += v; return t; }   // non-zero AC coefficients per decode of the batch (known after a Finish)
  // the frame tail's recorded ops, those of the LF frames' batch first (they run first), and FNV-1a (63 bits) over the names of their stages in order
  if (name == "post_ops") return (int64_t)post_ops_.size() + (lf_batch_ ? lf_batch_->Info(name) : 0);
  if (name == "post_ops_hash") { uint64_t h = 1469598103934665603ull; HashPostOps(&h); return (int64_t)(h & 0x7fffffffffffffffull); }
  if (name == "mod_group_lds_bytes") return prepared_ ? (int64_t)ModularGroupLdsBytes(cfg) : -1;
  if (name == "resize_u8_images") return resize_u8_images_;         // images of the last decode whose resize ran in Pillow's 8-bit arithmetic (OutputSpec::resize_u8: ResizeU8Kernel)
  if (name == "resize_launches") return resize_launches_;           // kernel launches the last decode's resizes took (two per group of the table: Batch::EnqueueResizes)
  if (name == "plane_outputs") return plane_outputs_;               // extra-channel planes the last decode wrote beside the colour outputs (OutputSpec::planes: EcPlanesOutKernel)
  if (name == "jpeg_device_images") return jpeg_device_images_;     // images of the last ReconstructJpegs whose scans the device wrote / that went through the host writer
  if (name == "jpeg_host_images") return jpeg_host_images_;
  if (name == "jpeg_device_progressive_images") return jpeg_device_progressive_images_;    // ... of the device's, those with at least one progressive scan
  if (name == "jpeg_gather_launches") return jpeg_gather_launches_;                        // ... launches of JpegGatherKernel: one per group of the gather table
  if (name == "jpeg_pixel_images") return jpeg_pixel_images_;       // images the last DecodeJpegPixels wrote
  if (name == "jpeg_pixel_launches") return jpeg_pixel_launches_;   // ... launches of its pixel kernels (two per group of the image table, one per DC-only group, however many images a group holds)
  if (name == "hf_groups_total") return hf_groups_total_;           // ... groups of the frames that took its HF stage, and those of them that were decoded: equal unless
  if (name == "hf_groups_decoded") return hf_groups_decoded_;       // jpeg_region is on and some image has a region (Batch::JpegRegionOf)
  if (name == "jpeg_dc_only_images") return jpeg_dc_only_images_;   // ... images of it written from their DC terms alone (JpegDcOutKernel; Batch::JpegDcOnly)
  if (name == "lf_simt_lanes") return lf_simt_.num_lanes;
  if (name == "lf_simt_streams") return lf_simt_.num_streams;      // (more streams than lanes: some lane decodes several, one after the other)
  if (name == "lf_spec_lanes") return trace_.lf_spec_lanes;
  if (name == "lf_spec_hits") return LfSpecStats(0);
  if (name == "lf_spec_misses") return LfSpecStats(1);
  if (name == "lf_simt_wp") return lf_simt_.num_lanes ? lf_simt_.any_wp : 0;     // the SIMT launch is the weighted-predictor instantiation
  // the kernels the last decode's LF / HF stage launched (kernels.h kHfVar* / kLfVar* bits) and the LDS sizes that chose them (bytes, after Prepare)
  if (name == "hf_variant") return trace_.hf_variant;
  if (name == "lf_variant") return trace_.lf_variant;
  if (name == "lf_wide_bytes") return trace_.lf_wide_bytes;
  if (name == "lf_wide_only") return trace_.lf_wide_only;
  if (name == "ac_code_bytes") return prepared_ ? cfg.ac_code_bytes : -1;
  if (name == "ac_code_bytes_compact") return prepared_ ? cfg.ac_code_bytes_compact : -1;
  if (name == "mod_code_bytes") return prepared_ ? cfg.mod_code_bytes : -1;
  if (name == "ac_cfg_uniform" || name == "mod_cfg_uniform") {   // every cluster of every AC / global-tree Modular code of the batch shares one hybrid-uint configuration
    const bool ac = name == "ac_cfg_uniform";
    auto uniform = [](const HostCode& c) { for (uint32_t v : c.cfg) if (v != c.cfg[0]) return false; return true; };
    for (size_t i = 0; i < images_.size(); i++) {
      const FramePlan& p = images_[i]->plan;
      if (ac) { if (!p.modular) for (auto& code : p.ac_code) if (!uniform(code)) return 0; }
      else if (p.has_global_tree && !uniform(p.tree_code)) return 0;
    }
    return 1;
  }
  if (!images_.empty() && !images_[0]->plan.modular) {   // geometry / quantiser of the first frame (tests that restate a stage from its defining formula)
    const FramePlan& p = images_[0]->plan;
    if (name == "frame0_bw") return p.bw;
    if (name == "frame0_bh") return p.bh;
    if (name == "frame0_global_scale") return p.global_scale;
    if (name == "frame0_quant_lf") return p.quant_lf;
    if (name == "frame0_color_factor") return p.color_factor;
    if (name == "frame0_x_qm_scale") return p.x_qm_scale;
    if (name == "frame0_b_qm_scale") return p.b_qm_scale;
    if (name == "frame0_xgroups") return p.xgroups;
  }
  if (name == "lf_simt_waves") return lf_simt_.num_lanes ? (lf_simt_.num_lanes + lf_simt_.lanes_per_wave - 1) / lf_simt_.lanes_per_wave : 0;
  return -1;
}

void* Batch::device_output(int i) const {
  const ImageEntry& e = *images_[pub_[i].first_unit];
  return e.out.device_ptr ? e.out.device_ptr : (void*)(dwork_ + e.off_out);
}

// ---- Batch::Prepare: phases over one PrepareState, in the order Prepare lists them --------------------------------------------------------
namespace {
// offsets of one unit's buffers in the work arena (lfq .. end_bitpos, place_*, mod_*, lz_*) and in the coefficient / pixel-plane arenas (coeff, plane_*, up_plane)
struct WorkOffsets {
  size_t lfq[3], lf[3], lf_tmp[3], llf[3], blk_info, coef_off, vb_list, vb_count, ytox, ytob, coeff[3], plane_a[3], plane_b[3], inv_sigma, lf_scratch, wp_scratch, end_bitpos,
      place_rec = 0, place_cnt = 0, band_start = 0,
      mod_scratch, hf_end = 0, mod_wp = 0, up_plane[4] = {0, 0, 0, 0};
  size_t lf_scratch_stride, wp_scratch_stride, mod_scratch_stride, mod_wp_stride = 0, lz_window = (size_t)-1, lz_ac_window = (size_t)-1;
};
struct QCache { const QuantTableSpec* spec; int kind; size_t off[3]; };     // quant tables are shared between frames with identical specs
bool SpecEqual(const QuantTableSpec& a, const QuantTableSpec& b) {
  if (a.mode != b.mode || a.num_bands != b.num_bands || a.num_bands4 != b.num_bands4) return false;
  if (memcmp(a.bands, b.bands, sizeof(a.bands)) || memcmp(a.idw, b.idw, sizeof(a.idw)) || memcmp(a.dct2w, b.dct2w, sizeof(a.dct2w))) return false;
  if (memcmp(a.dct4mul, b.dct4mul, sizeof(a.dct4mul)) || memcmp(a.dct4x8mul, b.dct4x8mul, sizeof(a.dct4x8mul))) return false;
  if (a.mode == 5 && (memcmp(a.afvw, b.afvw, sizeof(a.afvw)) || memcmp(a.bands4, b.bands4, sizeof(a.bands4)))) return false;
  if (a.mode == 7 && (a.raw_den != b.raw_den || a.raw[0] != b.raw[0] || a.raw[1] != b.raw[1] || a.raw[2] != b.raw[2])) return false;
  return true;
}
ConstOffsets::Local PutLocal(Arena& arena, uint32_t unit, const HostTree& tree, const HostCode& code) {    // a sub-stream's own tree and code
  ConstOffsets::Local l;
  l.unit = unit;
  l.tree = arena.Put(tree.nodes.data(), tree.nodes.size() * sizeof(TreeNode));
  PutCode(arena, code, &l.ctx, &l.cfg, &l.alias, &l.pc, &l.po, &l.ps);
  return l;
}
// descriptor of a sub-stream with its own tree and code, from where PutLocal put them
void FillLocalDev(ModLocalDev& d, const HostTree& tree, const HostCode& code, uint64_t data_bitpos, const ConstOffsets::Local& l, const uint8_t* cbase) {
  d.tree = (const TreeNode*)(cbase + l.tree); d.tree_nodes = (uint32_t)tree.nodes.size(); d.uses_wp = tree.uses_wp; d.max_prop = (uint32_t)tree.max_prop;
  d.data_bitpos = data_bitpos;
  d.code = ViewCode(code, cbase, l.ctx, l.cfg, l.alias, l.pc, l.po, l.ps);
}
// The quant tables of `spec` for kind k, put into the arena once per Prepare and spec (qcache); the DCT128/256 tables are large (up to 64K weights per channel) and
// computed once per process and spec.
const size_t* QuantTableOffsets(Arena& arena, vec<QCache>& qcache, const QuantTableSpec& spec, int k) {
  for (const QCache& q : qcache) if (q.kind == k && SpecEqual(*q.spec, spec)) return q.off;
  QCache qc; qc.spec = &spec; qc.kind = k;
  for (int ch = 0; ch < 3; ch++) {
    struct Big { QuantTableSpec spec; int kind, ch; std::vector<float> t; };   // process-lifetime cache: plain allocator
    static std::mutex mu;
    static std::vector<Big> big;
    vec<float> local;
    if (k >= 13) {
      std::lock_guard<std::mutex> lock(mu);
      const Big* found = nullptr;
      for (const Big& b : big) if (b.kind == k && b.ch == ch && SpecEqual(b.spec, spec)) { found = &b; break; }
      if (!found) {
        if (big.size() >= 48) big.clear();
        big.push_back(Big{spec, k, ch, {}});
        { vec<float> tmp; ComputeQuantTable(spec, k, ch, &tmp); big.back().t.assign(tmp.begin(), tmp.end()); }
        found = &big.back();
      }
      local.assign(found->t.begin(), found->t.end());
    } else ComputeQuantTable(spec, k, ch, &local);
    qc.off[ch] = arena.Put(local.data(), local.size() * 4);
  }
  qcache.push_back(qc);
  return qcache.back().off;
}
// LDS bytes of a code's tables (prefix codes / LZ77 streams are read through the tables in global memory: nothing to size the LDS for)
int CodeBytes(const HostCode& c, bool ctx) {
  if (c.use_prefix || c.lz77) return 16;
  return (int)(((c.num_clusters * 4 + 15) & ~15u) + (ctx ? ((c.num_ctx + 15) & ~15u) : 0) + ((size_t)c.num_clusters << c.log_alpha) * 8);
}
int CodeBytesCompact(const HostCode& c) {
  if (c.use_prefix || c.lz77) return 16;
  return (int)(((c.num_clusters * 4 + 15) & ~15u) + ((c.num_ctx + 15) & ~15u) + (((((size_t)c.num_clusters << c.log_alpha) * 6) + 15) & ~(size_t)15));
}
void SizeForModularStream(LaunchCfg& cfg, const HostTree& tree, const HostCode& code) {     // the global tree, a local stream, an LF-local stream
  cfg.max_tree_nodes = std::max<int>(cfg.max_tree_nodes, (int)tree.nodes.size()); cfg.mod_code_bytes = std::max(cfg.mod_code_bytes, CodeBytes(code, false)); cfg.any_wp |= tree.uses_wp ? 1 : 0;
}
// indices of `cost`, the dearest first (ties in index order)
template <class T> vec<uint32_t> OrderByCostDescending(const vec<T>& cost) {
  vec<uint32_t> order(cost.size());
  for (size_t k = 0; k < order.size(); k++) order[k] = (uint32_t)k;
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return cost[a] > cost[b]; });
  return order;
}
// What the SIMT LF plan gathers over the frames: the blob of cluster tables and which instantiation of the kernel the eligible streams need
struct LfSimtTables {
  vec<uint8_t> luts;
  std::map<std::string, uint32_t> lut_of;       // table content -> offset in the blob (frames of one encoder share most tables)
  bool general = false;                         // some eligible stream needs the instantiation with two-property tables / the rarer properties and predictors
  bool wp = false;                              // some eligible stream keeps weighted-predictor state: the batch takes that instantiation of the kernel
  uint32_t Intern(const uint8_t* bytes, size_t size) {
    const std::string key((const char*)bytes, size);
    auto it = lut_of.find(key);
    if (it == lut_of.end()) { it = lut_of.emplace(key, (uint32_t)luts.size()).first; luts.insert(luts.end(), bytes, bytes + size); }
    return it->second;
  }
};
// The LF-group streams of frame `frame` as LfDecodeSimtKernel takes them, in *mine; false: the frame keeps LfDecodeKernel (what its channels interned so far stays in t)
bool ClassifyLfStreams(const FramePlan& p, uint32_t frame, LfSimtTables& t, vec<LfSimtStream>* mine) {
  if (p.modular || !p.has_global_tree || !p.lf_local.empty() || p.tree_code.use_prefix || p.tree_code.lz77 || p.tree_code.log_alpha > 8 || p.tree_code.num_clusters > 256 || p.use_lf_frame) return false;
  // extra-channel sub-channels squeezed by >= 3 sit in the middle of the LfGroup sections: only the one-wavefront-per-stream kernel decodes those
  for (size_t c = p.global_decodable; c < p.gchannels.size(); c++) if (p.gchannels[c].w && p.gchannels[c].h && std::min(p.gchannels[c].hshift, p.gchannels[c].vshift) >= 3) return false;
  for (uint32_t g = 0; g < p.num_lf_groups; g++) {
    LfSimtStream s;
    memset(&s, 0, sizeof(s));
    s.frame = frame; s.group = g;
    for (int c = 0; c < 7; c++) {
      LfChanClass cl;
      if (!ClassifyLfChannel(p.tree, p.tree_code, c < 3 ? c : c - 3, c < 3 ? 1 + g : 1 + 2 * p.num_lf_groups + g, &cl)) return false;
      if (cl.uses_wp && c == 5) return false;      // (the block-info rows are up to 65 536 wide: the per-lane weighted-predictor rows hold 256)
      auto word = [&](const LfRowClass& rc) { return rc.kind | (rc.pred << 2) | (rc.sel_a << 5) | (rc.sel_b << 7) | (cl.uses_wp ? kLfSimtWpLive : 0u) | (rc.cluster << 16); };
      if (cl.rows.size() == 1) {
        s.chan[c].lut_off = cl.rows[0].kind ? t.Intern(cl.rows[0].lut.data(), cl.rows[0].lut.size()) : 0;
        s.chan[c].info = word(cl.rows[0]);
      } else {   // the class depends on the row: [512 bytes: row -> class][classes x {table offset, class word}]
        vec<uint8_t> blob(512 + 8 * cl.rows.size());
        memcpy(blob.data(), cl.row_to_class, 512);
        for (size_t k = 0; k < cl.rows.size(); k++) {
          const uint32_t e[2] = {cl.rows[k].kind ? t.Intern(cl.rows[k].lut.data(), cl.rows[k].lut.size()) : 0u, word(cl.rows[k])};
          memcpy(blob.data() + 512 + 8 * k, e, 8);
        }
        s.chan[c].lut_off = t.Intern(blob.data(), blob.size());
        s.chan[c].info = kLfSimtRows | (cl.uses_wp ? kLfSimtWpLive : 0u);
      }
      if (cl.uses_wp) t.wp = true;
      for (const LfRowClass& rc : cl.rows)      // beyond what the lean instantiation handles: one cluster per row or a table over W + N - NW; zero / W / clamped gradient
        if (rc.kind == 2 || (rc.kind == 1 && rc.sel_a != 0) || !(rc.pred == 0 || rc.pred == 1 || rc.pred == 3)) t.general = true;
    }
    mine->push_back(s);
  }
  return true;
}
// Streams of the given costs (not empty) spread over lanes, longest-processing-time-first; the number of lanes grows from the lower bound (total work / longest
// stream) until no lane carries noticeably more than the longest stream: a lane more costs nothing, a lane with two long streams doubles the stage's latency
vec<vec<uint32_t>> PackLanes(const vec<uint64_t>& cost) {
  uint64_t total = 0, longest = 0;
  for (uint64_t cst : cost) { total += cst; longest = std::max(longest, cst); }
  const vec<uint32_t> order = OrderByCostDescending(cost);
  vec<vec<uint32_t>> lane_streams;
  for (size_t nlanes = std::max<size_t>(1, std::min<size_t>(cost.size(), (size_t)((total + longest - 1) / longest)));; nlanes = std::min(cost.size(), nlanes + std::max<size_t>(1, nlanes / 64))) {
    lane_streams.assign(nlanes, vec<uint32_t>());
    std::priority_queue<std::pair<uint64_t, uint32_t>, std::vector<std::pair<uint64_t, uint32_t>>, std::greater<std::pair<uint64_t, uint32_t>>> pq;
    for (size_t l = 0; l < nlanes; l++) pq.push({0, (uint32_t)l});
    uint64_t makespan = 0;
    for (uint32_t k : order) { auto top = pq.top(); pq.pop(); lane_streams[top.second].push_back(k); makespan = std::max(makespan, top.first + cost[k]); pq.push({top.first + cost[k], top.second}); }
    if (makespan <= longest + longest / 16 || nlanes >= cost.size()) return lane_streams;
  }
}
uint32_t ResizeSlots(const ImageEntry& e) { return std::min(4u, std::max(1u, e.out.num_channels)); }   // (which ResizeKernel<NC> the image takes: sort key and group key)
}  // namespace

// What the phases of one Prepare share.  Each phase's comment says what it reads from here and what it adds; nothing else passes between them but the Batch's members.
struct Batch::PrepareState {
  const int n;                     // units
  hipStream_t stream;
  Arena arena;                     // over hconst_: streams and tables, uploaded as the constant arena
  vec<ConstOffsets> co;            // per unit: where its tables are in the constant arena
  vec<WorkOffsets> wo;             // per unit: where its buffers are in the work / plane arenas
  vec<size_t> cs_bytes;            // per unit: codestream bytes the frame's kernels may look at (FrameDev::cs_size)
  size_t natural_off[13] = {0};    // natural coefficient orders (shared by all frames)
  vec<QCache> qcache;
  vec<uint8_t> simt_frame;         // per unit: its LF-group streams are in the SIMT plan
  size_t place_units_off = 0, simt_streams_off = 0, simt_lanes_off = 0, simt_luts_off = 0;
  bool need_plane_b = false;
  // `take` = the per-batch work arena (everything the LF stage writes, scratch, status, outputs); `take_big` = pixel planes, only touched between HF decode and the
  // write stage (shareable)
  size_t w = 0, wbig = 0;
  size_t take(size_t bytes) { const size_t off = Align(w); w = off + bytes; return off; }
  size_t take_big(size_t bytes) { const size_t off = Align(wbig); wbig = off + bytes; return off; }
  // JXL_HIP_TIME_PREPARE=1: host milliseconds of the phases of Prepare on stderr
  const bool time_phases = getenv("JXL_HIP_TIME_PREPARE") != nullptr;
  std::chrono::steady_clock::time_point t_last = std::chrono::steady_clock::now();
  std::string t_report;
  void mark(const char* what) {
    if (!time_phases) return;
    const auto now = std::chrono::steady_clock::now();
    char buf[64];
    snprintf(buf, sizeof buf, " %s %.2f", what, std::chrono::duration<double, std::milli>(now - t_last).count());
    t_report += buf; t_last = now;
  }
  PrepareState(HostStage& hconst, int units, hipStream_t s) : n(units), stream(s), arena(hconst), co(units), wo(units), cs_bytes(units, 0), simt_frame(units, 0) {}
};

// frames decoded at 1:8 (OutputSpec::downscale == 8; SetOutput only lets single-frame VarDCT images through): their decode ends behind the LF post-processing
bool Batch::DecodedAtEighth(int unit) const { return images_[unit]->frame_index == 0 && images_[unit]->out.downscale == 8; }
// the frame of a DC-only image (decoder.h JpegDcOnly; SetOutput only lets single-frame JPEG transcodes through): its decode ends behind the LF decode
bool Batch::JpegDcOnlyUnit(int unit) const { return jpeg_dc_only && images_[unit]->frame_index == 0 && images_[unit]->jpeg_dc_eligible; }

// Device allocations are kept from one Prepare to the next and only replaced when they are too small (DevReserve): a batch object
// that is refilled step after step (JxlHipBatchReset + AddImages + Prepare, the streaming loop of bench.py) allocates once —
// hipFree synchronises the device, hipMalloc of gigabytes takes milliseconds.  Pointers into somebody else's planes are decided anew (ReserveArenas).
void Batch::ResetForPrepare() {
  if (clear_stream_) (void)hipStreamSynchronize((hipStream_t)clear_stream_);   // a pending clear of the old coefficient planes
  clear_pending_ = false;
  if (coef_owner_) dcoef_ = nullptr;
  if (big_owner_) dbig_ = nullptr;
  if (big_is_ext_) { dbig_ = nullptr; big_cap_ = 0; big_is_ext_ = false; }          // (pointers into the pipeline's planes)
  if (coef_is_ext_) { dcoef_ = nullptr; coef_cap_ = 0; coef_laid_out_ = 0; coef_is_ext_ = false; }
}

void Batch::MarkComplex(PubImage& pi) {
  pi.complex = true;
  for (int u = pi.first_unit; u < pi.first_unit + pi.num_units; u++) images_[u]->complex = true;
}

// Images whose output only the frame tail can write become complex: rendered spot colours (stage_spot.cc; grey images keep one colour plane there: not handled), a single
// frame as coded (its own size, no blending), un-premultiplied alpha (JxlDecoderSetUnpremultiplyAlpha, jpegxl-rs decode.rs:353).  Reads and adds nothing of PrepareState.
// ... and extra-channel planes beside the colour output (OutputSpec::planes): the frame tail is the one place where every extra channel of the finished image is a float
// plane (TailDeliver).  OutputNeedsTail: the rules that do not ask about planes (Batch::ComplexWithoutPlanes).
static bool OutputNeedsTail(const ImageHeader& ih, const OutputSpec& o) {
  bool premul = false, spot = false;
  for (auto& x : ih.extra) if (x.type == 0) { premul = x.alpha_associated; break; }
  for (auto& x : ih.extra) if (x.type == 2) spot = true;
  return (spot && o.render_spotcolors) || o.only_frame >= 0 || (o.unpremul_alpha && premul);
}
void Batch::PromoteToComplex() {
  for (PubImage& pi : pub_) {
    ImageEntry& first = *images_[pi.first_unit];
    bool spot = false;
    for (auto& x : first.ih.extra) if (x.type == 2) spot = true;
    if (spot && first.out.render_spotcolors && first.ih.color_space == 1) throw ParseError("unsupported: spot colours on a grey image", true);
    if (OutputNeedsTail(first.ih, first.out) || first.out.planes.any() || ConvertsNonXyb(first.ih, first.out)) MarkComplex(pi);
  }
}
bool Batch::ComplexWithoutPlanes(int i, const OutputSpec& o) const {
  const PubImage& pi = pub_[i];
  const ImageEntry& first = *images_[pi.first_unit];
  OutputSpec oo = o;      // (as SetOutput normalises it)
  if (oo.only_frame == 0 && pi.num_units == 1 && !first.plan.have_crop) oo.only_frame = -1;
  return pi.parsed_complex || OutputNeedsTail(first.ih, oo);
}

// "tables1".  Adds natural_off, cs_bytes and, per unit, co's codestream, section tables, trees, codes and bcm; fills resize_plans_ (axis tables), the batch maxima and fplan_.
void Batch::PutStreamTables(PrepareState& st) {
  Arena& arena = st.arena;
  hconst_.clear();
  {
    size_t guess = (size_t)1 << 20;      // streams + tables: one allocation instead of a dozen doublings
    for (auto& e : images_) { guess += sizeof(FrameDev) + 4 * sizeof(PassDev) + 1024; if (e->frame_index == 0) guess += e->cs.padded_size() + ((size_t)256 << 10); }
    hconst_.Reserve(guess);
  }
  {
    // (process-wide: the orders of the DCT128/256 buckets are 16K..64K entries each)
    static std::mutex mu;
    static std::vector<uint16_t> natural[13];   // process-lifetime cache: never through a caller's allocator
    std::lock_guard<std::mutex> lock(mu);
    for (int b = 0; b < 13; b++) {
      if (natural[b].empty()) { const vec<uint16_t> v = NaturalCoeffOrder(kBucketStrategy[b]); natural[b].assign(v.begin(), v.end()); }
      st.natural_off[b] = arena.Put(natural[b].data(), natural[b].size() * 2);
    }
  }
  max_lf_groups_ = max_groups_ = max_hf_slots_ = max_w_ = max_h_ = max_bw_ = max_bh_ = 0;
  any_vardct_ = any_modchan_ = any_multipass_ = any_scaled_ = any_full_vardct_ = false;
  fplan_ = FilterPlan();
  resize_plans_.clear(); resize_groups_.clear();
  for (int i = 0; i < st.n; i++) {
    ImageEntry& e = *images_[i];
    FramePlan& p = e.plan;
    ConstOffsets& c = st.co[i];
    if (e.frame_index == 0 && e.out_size == 0) SetOutput(e.pub_index, e.out);
    if (e.frame_index == 0 && e.out.resized()) {     // the two axes' filters of a resized output (ResizeAxis)
      ResizePlan rp;
      rp.unit = i;
      vec<uint32_t> lo, first; vec<float> weight; vec<int32_t> kk;
      for (int ax = 0; ax < 2; ax++) {
        const uint32_t n_in = e.out.cropped() ? (ax ? e.out.crop_h : e.out.crop_w) : (ax ? e.src_h : e.src_w);
        if (e.out.resize_u8) ResizeAxisInt(e.out.resize_filter, n_in, ax ? e.out.resize_h : e.out.resize_w, &lo, &first, &kk);
        else ResizeAxis(e.out.resize_filter, n_in, ax ? e.out.resize_h : e.out.resize_w, &lo, &first, &weight);
        rp.tab[3 * ax] = arena.Put(lo.data(), lo.size() * 4); rp.tab[3 * ax + 1] = arena.Put(first.data(), first.size() * 4);
        rp.tab[3 * ax + 2] = e.out.resize_u8 ? arena.Put(kk.data(), kk.size() * 4) : arena.Put(weight.data(), weight.size() * 4);
      }
      resize_plans_.push_back(rp);
      for (size_t k = 0; k < e.out.planes.req.size(); k++) { rp.plane = (int)k; resize_plans_.push_back(rp); }      // (one-slot entries over the same axis tables)
    }
    st.cs_bytes[i] = e.cs.size;
    if (EndsBehindLf(i) && !p.single_section) {
      // the 1:8 decode and the DC-only one read LfGlobal, the LfGroups and (on the host) HfGlobal: what lies behind the last of them — the AC groups, most of the file — stays on the host
      size_t end = 0;
      for (size_t k = 0; k < 2 + (size_t)p.num_lf_groups && k < p.sections.size(); k++) end = std::max<size_t>(end, p.sections[k].offset + p.sections[k].size);
      st.cs_bytes[i] = std::min(e.cs.size, end);
    }
    if (e.frame_index == 0) c.cs = arena.Put(e.cs.data(), e.cs.padded_size() - (e.cs.size - st.cs_bytes[i])); else c.cs = st.co[i - e.frame_index].cs;   // frames share the codestream
    vec<uint64_t> so, ss;
    for (auto& s : p.sections) { so.push_back(s.offset); ss.push_back(s.size); }
    c.sec_off = arena.Put(so.data(), so.size() * 8);
    c.sec_size = arena.Put(ss.data(), ss.size() * 8);
    if (p.has_global_tree) {
      c.tree = arena.Put(p.tree.nodes.data(), p.tree.nodes.size() * sizeof(TreeNode));
      PutCode(arena, p.tree_code, &c.mod_ctx, &c.mod_cfg, &c.mod_alias, &c.mod_pc, &c.mod_po, &c.mod_ps);
    }
    for (auto& ls : p.local_streams) c.local.push_back(PutLocal(arena, ls.unit, ls.tree, ls.code));
    for (size_t k = 0; k < p.lf_local.size(); k++) if (p.lf_local[k].present) c.lf_local.push_back(PutLocal(arena, (uint32_t)k, p.lf_local[k].tree, p.lf_local[k].code));
    c.bcm = arena.Put(&p.bcm, sizeof(p.bcm));
    if (!p.modular) any_vardct_ = true;      // (single-section frames: HfGlobal is parsed in the pre-run; nothing is reserved for it here)
    max_lf_groups_ = std::max<int>(max_lf_groups_, p.num_lf_groups);
    max_groups_ = std::max<int>(max_groups_, p.num_groups);
    if (!p.modular && !EndsBehindLf(i)) {
      // the groups an HF launch that honours the lists decodes for this frame (RunPart kPartJpegHf): those of its region, or all of them
      uint32_t slots = p.num_groups;
      if (JpegRegionUnit(i)) {
        vec<uint32_t> list;
        for (uint32_t gy = e.region_groups[1]; gy < e.region_groups[3]; gy++) for (uint32_t gx = e.region_groups[0]; gx < e.region_groups[2]; gx++) list.push_back(gy * p.xgroups + gx);
        // (what the kernels rely on: no entry names a group the frame does not have — every per-group address follows from it)
        bool ok = !list.empty() && list.size() <= p.num_groups;
        for (uint32_t g : list) ok = ok && g < p.num_groups;
        if (!ok) throw ParseError("Prepare: the region of image " + std::to_string(e.pub_index) + " leaves its frame's groups", false);
        c.hf_list = arena.Put(list.data(), list.size() * 4); c.hf_count = slots = (uint32_t)list.size();
      }
      max_hf_slots_ = std::max<int>(max_hf_slots_, (int)slots);
    }
    max_w_ = std::max<int>(max_w_, p.width); max_h_ = std::max<int>(max_h_, p.height);
    max_bw_ = std::max<int>(max_bw_, p.bw); max_bh_ = std::max<int>(max_bh_, p.bh);
    if (!p.modular && DecodedAtEighth(i)) any_scaled_ = true;
    if (!p.modular && !EndsBehindLf(i)) any_full_vardct_ = true;
    if (!p.modular && !EndsBehindLf(i)) {
      ImageHeader colour_store;      // (the transfer function of the encoding the image is rendered to: its header's, or the output's target)
      const bool fusable = p.lf.gab && p.lf.epf_iters == 1 && e.ih.xyb_encoded && SimpleTransfer(ColourHeader(e.ih, images_[pub_[e.pub_index].first_unit]->out, &colour_store)) && p.upsampling == 1 && !e.complex;
      if (p.upsampling > 1 && !e.complex) { fplan_.any_upsampled = true; fplan_.max_out_w = std::max<int>(fplan_.max_out_w, e.ih.xsize); fplan_.max_out_h = std::max<int>(fplan_.max_out_h, e.ih.ysize); }
      fplan_.any_fused |= fusable; fplan_.any_unfused |= !fusable;
      fplan_.any_gab |= p.lf.gab != 0; fplan_.max_epf = std::max<int>(fplan_.max_epf, p.lf.epf_iters);
    }
  }
}

// Lays out the work arena, the coefficient planes and the pixel planes.  Reads fplan_ (PutStreamTables); adds wo, the arena cursors, need_plane_b and co's up_weights / mod_chan.
void Batch::LayOutWork(PrepareState& st) {
  const int n = st.n;
  st.need_plane_b = fplan_.any_unfused || cfg.force_unfused_filters;
  mod_plane_offsets_.assign(n, {});
  mod_ops_.assign(n, {});
  cbufs_.assign(n, ComplexBufs());
  for (int i = 0; i < n; i++) for (vec<size_t>* a : {&cbufs_[i].ecf, &cbufs_[i].up_ec, &cbufs_[i].canvas_ec}) a->assign(images_[i]->ih.extra.size(), (size_t)-1);
  for (auto& cb : cbufs_) for (size_t* a : {cb.up, cb.noise, cb.rgb, cb.canvas, cb.pa, cb.pb, cb.color_int}) for (int k = 0; k < 3; k++) a[k] = (size_t)-1;
  post_ops_.clear(); any_complex_ = false;
  vardct_alpha_.assign(n, VarDctAlpha());
  status_off_ = st.take((size_t)n * 4);
  flags_off_ = st.take((size_t)n * 4);
  hfw_off_ = st.take((size_t)n * 4);
  hf_written_.assign(n, 0); decodes_since_finish_ = 0;
  cfg.idct_flags_known = 0; ran_once_ = false; flags_pending_ = false;
  // coefficient buffers of all frames are contiguous so that one memset clears them
  // quantised coefficients: an arena of this batch's own (never shared: it is cleared for the batch's next decode on an
  // internal stream while the next batch's HF stage runs, see ClearCoefficients*)
  size_t wcoef = 0;
  for (int i = 0; i < n; i++) {
    const FramePlan& p = images_[i]->plan;
    if (p.modular || EndsBehindLf(i)) continue;
    for (int c = 0; c < 3; c++) { st.wo[i].coeff[c] = Align(wcoef); wcoef = st.wo[i].coeff[c] + (size_t)p.num_groups * 65536 * 4; }
  }
  coeff_bytes_ = Align(wcoef);
  for (int i = 0; i < n; i++) {
    ImageEntry& e = *images_[i];
    const FramePlan& p = e.plan;
    WorkOffsets& o = st.wo[i];
    o.end_bitpos = st.take(16);
    if (e.frame_index == 0 && !e.out.device_ptr) e.off_out = st.take((e.out_size + 64) * std::max<size_t>(1, e.deliver_frames.size()));
    if (e.frame_index == 0 && e.out.resized()) {
      // resized output: the f32 picture the write stage leaves (every slot of the output, interleaved), and the rows of the resampled rectangle after the horizontal pass —
      // among the pixel planes: written and read between the write stage and the end of the decode, so the jobs of a pipeline share one set (UseSharedPlanes)
      // (OutputSpec::resize_u8: both hold u8 samples, a quarter of it)
      const size_t sample = e.out.resize_u8 ? 1 : 4;
      e.off_resize_src = st.take_big((size_t)e.src_w * e.src_h * e.out.num_channels * sample);
      e.off_resize_tmp = st.take_big((size_t)(e.out.cropped() ? e.out.crop_h : e.src_h) * e.out.resize_w * e.out.num_channels * sample);
      // ... and per requested extra-channel plane one slot of each (OutputSpec::planes): the planes of one decode are resampled together, so each has rows of its own
      e.off_plane_src.clear(); e.off_plane_tmp.clear();
      for (size_t k = 0; k < e.out.planes.req.size(); k++) {
        e.off_plane_src.push_back(st.take_big((size_t)e.src_w * e.src_h * 4));
        e.off_plane_tmp.push_back(st.take_big((size_t)(e.out.cropped() ? e.out.crop_h : e.src_h) * e.out.resize_w * 4));
      }
    }
    if (p.upsampling > 1) {   // kernel weights: custom (image header) or library default
      const int upk = p.upsampling == 2 ? 0 : p.upsampling == 4 ? 1 : 2;
      const float* const kDefault[3] = {kUp2, kUp4, kUp8};
      static const size_t kCount[3] = {15, 55, 210};
      const vec<float>& cw = e.ih.up_weights[upk];
      st.co[i].up_weights = cw.empty() ? st.arena.Put(kDefault[upk], kCount[upk] * 4) : st.arena.Put(cw.data(), cw.size() * 4);
    }
    if (!p.modular) LayOutVarDct(i, st); else LayOutModular(i, st);
    bool lz_local = false;     // (Modular sub-streams with codes of their own)
    if (!p.modular) {
      for (auto& ls : p.local_streams) lz_local |= ls.code.lz77;
      for (auto& l : p.lf_local) lz_local |= l.present && l.code.lz77;
    }
    if (((p.has_global_tree && p.tree_code.lz77) || lz_local) && (!p.gchannels.empty() || !p.modular))   // LZ77 windows of the Modular streams (4 MiB each); VarDCT: + one per LF group
      o.lz_window = st.take((size_t)(1 + p.NumModUnits() + (p.modular ? 0 : p.num_lf_groups)) * (4u << 20));
    if (!p.modular && !EndsBehindLf(i)) {   // LZ77-coded AC streams: a window per group stream (1 MiB each, only for the frames that use them)
      bool lz_ac = p.single_section;    // (a one-section frame's AC code is only parsed once its LF streams have been decoded: always reserved, 1 MiB)
      for (auto& code : p.ac_code) lz_ac |= code.lz77;
      if (lz_ac) o.lz_ac_window = st.take((size_t)p.num_groups * kAcLzWindow * 4);
    }
    if (e.complex) LayOutComplexBufs(i, st);
  }
  work_size_ = Align(st.w);
}

// The Modular channels of a frame (every channel of a Modular frame, the extra channels of a VarDCT frame): planes in the work arena, the plan that undoes the global
// transforms, the channel table.  Adds co[i].mod_chan; fills mod_plane_offsets_[i] and mod_ops_[i].
void Batch::LayOutModChannels(int i, PrepareState& st) {
  const FramePlan& p = images_[i]->plan;
  any_modchan_ = true;
  vec<size_t>& mp = mod_plane_offsets_[i];
  for (auto& ch : p.gchannels) mp.push_back(st.take((size_t)ch.w * ch.h * 4 + 64));
  PlanModularUndo(i, [&st](size_t bytes) { return st.take(bytes); });
  vec<ModChanDev> table;
  for (size_t k = 0; k < p.gchannels.size(); k++) table.push_back(ModChanDev{mp[k], p.gchannels[k].w, p.gchannels[k].h, p.gchannels[k].hshift, p.gchannels[k].vshift});
  st.co[i].mod_chan = st.arena.Put(table.data(), table.size() * sizeof(ModChanDev));
}

// Buffers of a VarDCT unit: LF-stage outputs and scratch in the work arena, pixel planes; with extra channels, their Modular channels.  Reads need_plane_b; adds wo[i].
void Batch::LayOutVarDct(int i, PrepareState& st) {
  const ImageEntry& e = *images_[i]; const FramePlan& p = e.plan;
  WorkOffsets& o = st.wo[i];
  const size_t nb = (size_t)p.bw * p.bh;
  for (int c = 0; c < 3; c++) { o.lfq[c] = st.take(nb * 4); o.lf[c] = st.take(nb * 4); o.lf_tmp[c] = st.take(nb * 4); o.llf[c] = st.take(nb * 4); }
  o.blk_info = st.take(nb * 4); o.coef_off = st.take(nb * 4); o.inv_sigma = st.take(nb * 4);
  o.vb_list = st.take((size_t)p.num_groups * 1024 * 8); o.vb_count = st.take((size_t)p.num_groups * 4);
  o.place_rec = st.take(nb * 16); o.place_cnt = st.take((size_t)p.num_lf_groups * 8 * 4); o.band_start = st.take((size_t)p.num_lf_groups * 8 * 4);
  const size_t ntile = (size_t)((p.bw + 7) / 8) * ((p.bh + 7) / 8);
  o.ytox = st.take(ntile); o.ytob = st.take(ntile);
  const size_t plane = (size_t)p.bw * 8 * p.bh * 8 * 4;
  for (int c = 0; c < 3; c++) {
    if (EndsBehindLf(i)) { o.plane_a[c] = o.plane_b[c] = (size_t)-1; continue; }      // (no full-resolution planes)
    o.plane_a[c] = st.take_big(plane); o.plane_b[c] = (st.need_plane_b || e.complex) ? st.take_big(plane) : (size_t)-1;
  }
  if (p.upsampling > 1 && !e.complex) for (int c = 0; c < 4; c++) o.up_plane[c] = st.take_big((size_t)e.ih.xsize * e.ih.ysize * 4);
  o.lf_scratch_stride = 16 + 2 * 1024 + 3 * 65536;
  o.lf_scratch = st.take(o.lf_scratch_stride * 4 * p.num_lf_groups);
  // weighted-predictor state of an LF-group stream.  LfDecodeSimtKernel: two rows of 258 records of 32 bytes; LfDecodeKernel's global
  // form (channels wider than its LDS slot — only the block-info rows, up to 65 536 wide, can be): five arrays of 2 x (width + 2) ints
  bool wide_wp = false;
  if (p.tree.uses_wp && p.has_global_tree)
    for (uint32_t g = 0; g < p.num_lf_groups && !wide_wp; g++) wide_wp = LfChannelUsesWp(p.tree, 2, 1 + 2 * p.num_lf_groups + g);
  for (uint32_t g = 0; g < p.num_lf_groups && !p.lf_local.empty() && !wide_wp; g++) {   // (local trees: the HF-metadata stream's own, or the global one it uses)
    const FramePlan::LfLocal& l = p.lf_local[3 * (size_t)g + 2];
    wide_wp = l.present ? LfChannelUsesWp(l.tree, 2, 1 + 2 * p.num_lf_groups + g) : (p.tree.uses_wp && LfChannelUsesWp(p.tree, 2, 1 + 2 * p.num_lf_groups + g));
  }
  o.wp_scratch_stride = wide_wp ? 10 * (65536 + 2) : kLfSimtWpInts;
  o.wp_scratch = st.take(o.wp_scratch_stride * 4 * p.num_lf_groups);
  if (p.gchannels.empty()) return;
  LayOutModChannels(i, st);      // extra channels (alpha, ...) ride in the frame's Modular sub-streams
  const size_t gd = p.group_dim;
  o.mod_scratch_stride = (8 + 4) * gd * gd + 4 * 65536;
  o.mod_scratch = st.take(o.mod_scratch_stride * 4 * p.NumModUnits());
  o.hf_end = st.take((size_t)p.num_groups * p.ModUnitPasses() * 8);   // (pass - mod_pass, g)
  // the Modular streams keep their WP state apart from the LF streams'
  o.mod_wp_stride = (p.tree.uses_wp || (!p.local_streams.empty() && p.local_streams[0].tree.uses_wp)) ? 10 * (65536 + 2) : 16;
  o.mod_wp = st.take(o.mod_wp_stride * 4 * (1 + p.NumModUnits()));
}

// Buffers of a Modular unit: its channels, per-unit scratch, weighted-predictor rows; float planes when the frame tail composes it.  Adds wo[i].
void Batch::LayOutModular(int i, PrepareState& st) {
  const ImageEntry& e = *images_[i]; const FramePlan& p = e.plan;
  WorkOffsets& o = st.wo[i];
  LayOutModChannels(i, st);
  const size_t gd = p.group_dim;
  // per-unit scratch: channels of units with transforms of their own are decoded there (worst case 12 planes of a group + palettes: 4 MB per unit, 4.3 GB for the 1040
  // units of an 8192x8192 frame) — the host has read every unit's header: frames without such units get none; weighted-predictor rows: two rows x five arrays of the widest channel
  const bool tight = p.mod_units_scanned && !p.mod_local_transforms;
  o.mod_scratch_stride = tight ? 64 : (8 + 4) * gd * gd + 4 * 65536;
  o.mod_scratch = st.take(o.mod_scratch_stride * 4 * p.NumModUnits());
  size_t widest = gd;
  for (auto& ch : p.gchannels) widest = std::max<size_t>(widest, ch.w);
  o.wp_scratch_stride = (p.tree.uses_wp || p.mod_local_wp) ? (tight ? 10 * (widest + 2) : 10 * (65536 + 2)) : 16;
  o.wp_scratch = st.take(o.wp_scratch_stride * 4 * (1 + p.NumModUnits()));
  if (e.complex) for (int c = 0; c < 3; c++) { o.plane_a[c] = st.take_big((size_t)p.bw * 8 * p.bh * 8 * 4); o.plane_b[c] = (size_t)-1; }
}

// Buffers of the frame tail (PlanPostOps) of a complex unit: float extra channels, upsampled planes, noise planes, colour-transformed planes (only when the
// untransformed ones must survive as a reference frame), canvas (only when the frame is blended).  Reads wo[i]'s planes; fills cbufs_[i].
void Batch::LayOutComplexBufs(int i, PrepareState& st) {
  const ImageEntry& e = *images_[i]; const FramePlan& p = e.plan;
  any_complex_ = true;
  ComplexBufs& cb = cbufs_[i];
  const size_t ne = e.ih.extra.size();
  const size_t coded = (size_t)p.width * p.height * 4, full = (size_t)p.frame_w * p.frame_h * 4, img = (size_t)e.ih.xsize * e.ih.ysize * 4;
  for (size_t k = 0; k < ne; k++) cb.ecf[k] = st.take_big(coded);
  if (p.upsampling > 1) { for (int c = 0; c < 3; c++) cb.up[c] = st.take_big(full); for (size_t k = 0; k < ne; k++) cb.up_ec[k] = st.take_big(full); }
  if (p.feat.has_noise) for (int c = 0; c < 3; c++) cb.noise[c] = st.take_big(full);
  if (p.flags & 2) for (size_t k = 0; k < ne; k++) cb.ec_tmp.push_back(st.take_big(coded));
  const bool can_ref = !p.is_last && p.frame_type != 1 && (p.duration == 0 || p.save_as_reference != 0);
  bool replace_all = p.blend.mode == 0;
  for (auto& b : p.ec_blend) if (b.mode != 0) replace_all = false;
  const bool needs_blending = p.have_crop || !replace_all;
  if (p.frame_type != 2) {
    if (can_ref && p.save_before_ct) for (int c = 0; c < 3; c++) cb.rgb[c] = st.take_big(full);
    if (needs_blending) { for (int c = 0; c < 3; c++) cb.canvas[c] = st.take_big(img); for (size_t k = 0; k < ne; k++) cb.canvas_ec[k] = st.take_big(img); }
  }
  for (int c = 0; c < 3; c++) { cb.pa[c] = st.wo[i].plane_a[c]; cb.pb[c] = st.wo[i].plane_b[c]; }
}

// The work arena with its clear policy, the pixel planes and the coefficient planes (own, an owner's, or the pipeline's shared set), the frame descriptors' device array.
// Reads the arena cursors and need_plane_b; adds nothing.
void Batch::ReserveArenas(PrepareState& st) {
  const int n = st.n;
  hipStream_t stream = st.stream;
  {
    // The arena is cleared when it is new.  A refilled batch of plain VarDCT frames (the streaming loop: 14 MB of LF-stage outputs per 4K frame, 3.6 GB per
    // batch of 256) only gets its status / flag / counter words zeroed: every kernel of that path writes what it reads later (valid streams) or treats what it
    // finds as it treats the content of a damaged stream.  JXL_HIP_POISON_WORK=1 (tests) fills the rest with 0xCD even when new, to prove exactly that.
    const bool fresh = DevReserve((void**)&dwork_, &work_cap_, work_size_);
    static const bool poison = getenv("JXL_HIP_POISON_WORK") != nullptr;
    bool plain = n > 0, cautious = false;     // cautious: one-group frames (the LF stage runs ahead, in this function) and output buffers inside the arena (row padding)
    for (int i = 0; i < n; i++) {
      const ImageEntry& e = *images_[i];
      if (e.plan.modular || !e.plan.gchannels.empty() || e.complex) plain = false;
      if (e.plan.single_section || (e.frame_index == 0 && !e.out.device_ptr)) cautious = true;
    }
    const size_t head = std::min(work_size_, Align(hfw_off_ + (size_t)n * 4));
    if (plain && poison) {
      HIP_CHECK(hipMemsetAsync(dwork_ + head, 0xCD, work_size_ - head, stream));
      HIP_CHECK(hipMemsetAsync(dwork_, 0, head, stream));
      for (int i = 0; i < n; i++) { const ImageEntry& e = *images_[i]; if (e.frame_index == 0 && !e.out.device_ptr) HIP_CHECK(hipMemsetAsync(dwork_ + e.off_out, 0, (e.out_size + 64) * std::max<size_t>(1, e.deliver_frames.size()), stream)); }
    } else if (plain && !cautious && !fresh) HIP_CHECK(hipMemsetAsync(dwork_, 0, head, stream));
    else HIP_CHECK(hipMemsetAsync(dwork_, 0, work_size_, stream));
  }
  big_size_ = Align(st.wbig);
  has_plane_b_ = st.need_plane_b;
  bool plain_planes = n > 0;      // plain VarDCT frames overwrite every sample of the pixel planes they read: they can take planes that hold another decode's leftovers
  for (int i = 0; i < n; i++) { const ImageEntry& e = *images_[i]; if (e.plan.modular || e.complex || e.plan.upsampling > 1) plain_planes = false; }
  if (big_owner_) {
    if (!big_owner_->dbig_ || big_owner_->big_cap_ < big_size_) throw ParseError("ShareBigArena: the owner's buffers are missing or smaller than this batch needs", false);
    dbig_ = big_owner_->dbig_;
  } else if (ext_big_ && ext_big_->p && ext_big_->cap >= big_size_ && plain_planes) {
    if (dbig_) { Pool().Give(dbig_, big_cap_, device_, /*idle=*/big_sharers_ == 0); dbig_ = nullptr; big_cap_ = 0; }
    dbig_ = ext_big_->p; big_is_ext_ = true;
  } else if (DevReserve((void**)&dbig_, &big_cap_, std::max<size_t>(big_size_, 256)) || big_sharers_ == 0) {
    // (planes other batches share are not cleared again when this object is refilled: their decodes may be using them — every sharer,
    // like a refilled owner, then starts from what the decode before left, which plain frames overwrite completely)
    HIP_CHECK(hipMemsetAsync(dbig_, 0, big_cap_, stream));
  }
  if (coef_owner_) {
    if (!coef_owner_->dcoef_ || coef_owner_->coef_cap_ < coeff_bytes_) throw ParseError("ShareCoefArena: the owner's planes are missing or smaller than this batch needs", false);
    dcoef_ = coef_owner_->dcoef_;                      // (whether they are clean is the owner's knowledge: CoefDirty())
  } else if (ext_coef_ && ext_coef_->p && ext_coef_->cap >= coeff_bytes_ && any_vardct_) {
    if (dcoef_) { Pool().Give(dcoef_, coef_cap_, device_, /*idle=*/true); dcoef_ = nullptr; coef_cap_ = 0; }
    dcoef_ = ext_coef_->p; coef_is_ext_ = true;        // (clean or not: ext_coef_->dirty / clean_extent, kept by the decodes that used the set before)
  } else {
    const bool fresh = DevReserve((void**)&dcoef_, &coef_cap_, std::max<size_t>(coeff_bytes_, 256));
    if (fresh) coef_clean_extent_ = 0;                 // (a new allocation: nothing of it is known to be zero)
    if (fresh || coeff_bytes_ != coef_laid_out_) coef_dirty_ = true;   // new planes, or another layout of them: the first decode clears them in its own stream
  }
  coef_laid_out_ = coeff_bytes_;
  DevReserve((void**)&dframes_, &frames_cap_, sizeof(FrameDev) * std::max(n, 1));
  frames_host_.assign(n, FrameDev());
}

// frames_host_[i] from what exists at the time of the call, with the constant arena at `cbase` on the device: called for the one-section frames before HfGlobal is
// parsed (p.ac_code is empty then: no pass tables yet) and for every frame once everything is in the arena.  Reads co[i], wo[i], cs_bytes[i]; adds nothing.
void Batch::FillFrameDev(int i, const uint8_t* cbase, const PrepareState& st) {
  const FramePlan& p = images_[i]->plan;
  FrameDev& f = frames_host_[i];
  memset(&f, 0, sizeof(f));
  FillFrameCommon(i, cbase, st);
  if (!p.modular) FillFrameVarDct(i, cbase, st);
  else { f.hf_start_bitpos = 0; f.mod_wp_scratch = f.wp_scratch; f.mod_wp_stride = f.wp_scratch_stride; }
  if (!p.gchannels.empty()) FillFrameModChannels(i, cbase, st);
}

// geometry, codestream and section tables, the global and local trees and codes, status words, output, LZ77 windows: what every kind of frame has
void Batch::FillFrameCommon(int i, const uint8_t* cbase, const PrepareState& st) {
  ImageEntry& e = *images_[i];
  const FramePlan& p = e.plan;
  const ConstOffsets& c = st.co[i]; const WorkOffsets& o = st.wo[i];
  FrameDev& f = frames_host_[i];
  f.width = p.width; f.height = p.height; f.bw = p.bw; f.bh = p.bh; f.xgroups = p.xgroups; f.ygroups = p.ygroups; f.num_groups = p.num_groups;
  f.xlfgroups = p.xlfgroups; f.num_lf_groups = p.num_lf_groups; f.cw = (p.bw + 7) / 8; f.ch = (p.bh + 7) / 8;
  f.group_dim = p.group_dim; f.is_modular = p.modular; f.plane_stride = p.bw * 8; f.plane_rows = p.bh * 8;
  f.cs = cbase + c.cs; f.cs_size = st.cs_bytes[i];
  f.sec_off = (const uint64_t*)(cbase + c.sec_off); f.sec_size = (const uint64_t*)(cbase + c.sec_size);
  if (c.hf_list != (size_t)-1) { f.hf_list = (const uint32_t*)(cbase + c.hf_list); f.hf_count = c.hf_count; }
  f.single_section = p.single_section;
  f.lf_start_bitpos = p.global_data_bitpos;  // VarDCT without extra channels: LfGroup follows LfGlobal directly
  f.stream_end_bitpos = (uint64_t*)(dwork_ + o.end_bitpos);
  if (p.has_global_tree) {
    f.tree = (const TreeNode*)(cbase + c.tree);
    f.tree_nodes = (uint32_t)p.tree.nodes.size();
    f.mod_code = ViewCode(p.tree_code, cbase, c.mod_ctx, c.mod_cfg, c.mod_alias, c.mod_pc, c.mod_po, c.mod_ps);
    f.mod_cfg_uniform = p.tree_code.cfg.empty() ? 0xFFFFFFFFu : p.tree_code.cfg[0];
    for (uint32_t v : p.tree_code.cfg) if (v != p.tree_code.cfg[0]) f.mod_cfg_uniform = 0xFFFFFFFFu;
  }
  f.uses_wp = p.tree.uses_wp; f.gwp = p.gwp;
  f.mod_unit_passes = p.ModUnitPasses(); f.mod_pass = p.mod_pass;
  for (int k = 0; k < 11; k++) { f.pass_min_shift[k] = p.pass_min_shift[k]; f.pass_max_shift[k] = p.pass_max_shift[k]; }
  f.tree_max_prop = (uint32_t)p.tree.max_prop;
  for (int k = 0; k < 3; k++) { f.hs[k] = p.hs[k]; f.vs[k] = p.vs[k]; }
  f.subsampled = p.subsampled;
  if (!c.local.empty()) {
    // descriptor table of the frame's units (0 = global stream), zero = "uses the frame's tree"
    ModLocalDev* table = &local_host_[local_first_[i]];
    f.mod_local = dlocal_ + local_first_[i];
    for (size_t k = 0; k < c.local.size(); k++) FillLocalDev(table[c.local[k].unit], p.local_streams[k].tree, p.local_streams[k].code, p.local_streams[k].data_bitpos, c.local[k], cbase);
  }
  if (!p.lf_local.empty()) {
    // LfGroup sub-streams: [3 g + k] behind the unit table, zero = "uses the frame's tree"; the frame takes LfDecodeLocalKernel
    const size_t first = local_first_[i] + (p.local_streams.empty() ? 0 : 1 + (size_t)p.NumModUnits());
    ModLocalDev* table = &local_host_[first];
    f.lf_local = dlocal_ + first;
    for (const ConstOffsets::Local& l : c.lf_local) {
      const FramePlan::LfLocal& ll = p.lf_local[l.unit];
      FillLocalDev(table[l.unit], ll.tree, ll.code, ll.data_bitpos, l, cbase);
      f.lf_lz77 |= ll.code.lz77 ? 1u : 0u;
    }
    if (p.has_global_tree && p.tree_code.lz77) f.lf_lz77 = 1;
    f.tree_max_prop = (uint32_t)p.max_prop;      // (every tree the LF streams may use: whether they keep previous-channel references)
  }
  f.bcm = (const BlockCtxDev*)(cbase + c.bcm);
  f.status = (uint32_t*)(dwork_ + status_off_) + i;
  f.frame_flags = (uint32_t*)(dwork_ + flags_off_) + i;
  f.hf_written = (uint32_t*)(dwork_ + hfw_off_) + i;
  f.od = FillOutput(e, dwork_, dbig_);
  f.upsampling = p.upsampling; f.img_w = e.ih.xsize; f.img_h = e.ih.ysize;
  // (an output with jpeg_scale: DecodeJpegPixels writes it from its own table; the write stage of a Run, which fails such an image, stays inside the scaled picture —
  // OutputKernel, the only writer of a frame CanDecodeJpegPixelsAs takes, is bounded by img_w x img_h)
  if (e.frame_index == 0 && e.out.jpeg_scale > 1) { f.img_w = (e.ih.xsize + e.out.jpeg_scale - 1) / e.out.jpeg_scale; f.img_h = (e.ih.ysize + e.out.jpeg_scale - 1) / e.out.jpeg_scale; }
  if (DecodedAtEighth(i)) { f.lf_only = kLfOnlyEighth; f.img_w = (p.width + 7) / 8; f.img_h = (p.height + 7) / 8; }     // (the picture LfOutputKernel writes; out_stride is SetOutput's, of the same picture)
  else if (JpegDcOnlyUnit(i)) f.lf_only = kLfOnlyJpegDc;      // (img_w x img_h: the scaled picture, above; JpegDcOutKernel goes by its own table)
  if (p.upsampling > 1) { f.up_weights = (const float*)(cbase + c.up_weights); for (int k = 0; k < 4; k++) f.up_plane[k] = (float*)(dbig_ + o.up_plane[k]); }
  f.post_mode = e.complex ? 1 : 0;
  f.lz_window = o.lz_window == (size_t)-1 ? nullptr : (uint32_t*)(dwork_ + o.lz_window);
  f.lz_ac_window = o.lz_ac_window == (size_t)-1 ? nullptr : (uint32_t*)(dwork_ + o.lz_ac_window);
  f.lz_lf_base = 1 + p.NumModUnits();
  f.wp_scratch = (int32_t*)(dwork_ + o.wp_scratch); f.wp_scratch_stride = o.wp_scratch_stride;
}

// quantiser, colour and filter parameters, LF-stage buffers, planes and, once HfGlobal has been parsed, the per-pass tables and quant tables of a VarDCT frame
void Batch::FillFrameVarDct(int i, const uint8_t* cbase, const PrepareState& st) {
  const ImageEntry& e = *images_[i]; const FramePlan& p = e.plan;
  const ConstOffsets& c = st.co[i]; const WorkOffsets& o = st.wo[i];
  FrameDev& f = frames_host_[i];
  const float inv_gs = 65536.0f / (float)p.global_scale;
  const float inv_quant_lf = inv_gs / (float)p.quant_lf;
  for (int k = 0; k < 3; k++) f.lf_fac[k] = p.m_lf[k] * inv_quant_lf;
  f.cfl_lf_x = p.base_x + (float)p.ytox_lf * (1.0f / (float)p.color_factor);
  f.cfl_lf_b = p.base_b + (float)p.ytob_lf * (1.0f / (float)p.color_factor);
  f.inv_global_scale = inv_gs;
  f.x_dm = std::pow(0.8f, (float)p.x_qm_scale - 2.0f); f.b_dm = std::pow(0.8f, (float)p.b_qm_scale - 2.0f);
  for (int k = 0; k < 4; k++) f.quant_bias[k] = e.ih.quant_bias[k];
  f.color_scale = 1.0f / (float)p.color_factor; f.base_x = p.base_x; f.base_b = p.base_b;
  f.skip_lf_smoothing = (p.flags & 128) != 0 || p.use_lf_frame;     // (dec_frame.cc FinalizeDC: no adaptive smoothing of an LF frame's samples)
  f.use_lf_frame = p.use_lf_frame ? 1 : 0;
  f.gab = p.lf.gab; f.epf_iters = p.lf.epf_iters;
  for (int k = 0; k < 3; k++) {
    const float w1 = p.lf.gab_w[2 * k], w2 = p.lf.gab_w[2 * k + 1];
    const float div = 1.0f + 4.0f * (w1 + w2);
    f.gab_w[3 * k] = 1.0f / div; f.gab_w[3 * k + 1] = w1 / div; f.gab_w[3 * k + 2] = w2 / div;
  }
  for (int k = 0; k < 8; k++) f.epf_sharp_lut[k] = p.lf.sharp_lut[k];
  for (int k = 0; k < 3; k++) f.epf_channel_scale[k] = p.lf.channel_scale[k];
  f.epf_quant_mul = p.lf.quant_mul; f.epf_quant_scale = (float)p.global_scale / 65536.0f;
  const float scales[3] = {p.lf.pass0_sigma_scale, 1.0f, p.lf.pass2_sigma_scale};
  for (int k = 0; k < 3; k++) { f.epf_sm[k] = scales[k] * 1.65f; f.epf_bsm[k] = f.epf_sm[k] * p.lf.border_sad_mul; }
  ImageHeader colour_store;
  FillColor(ColourHeader(e.ih, images_[pub_[e.pub_index].first_unit]->out, &colour_store), p.do_ycbcr, f);
  for (int k = 0; k < 3; k++) {
    f.lfq[k] = (int32_t*)(dwork_ + o.lfq[k]); f.lf[k] = (float*)(dwork_ + o.lf[k]); f.lf_tmp[k] = (float*)(dwork_ + o.lf_tmp[k]);
    f.llf[k] = (float*)(dwork_ + o.llf[k]); f.coeff[k] = EndsBehindLf(i) ? nullptr : (int32_t*)(dcoef_ + o.coeff[k]);
    f.plane_a[k] = o.plane_a[k] == (size_t)-1 ? nullptr : (float*)(dbig_ + o.plane_a[k]); f.plane_b[k] = o.plane_b[k] == (size_t)-1 ? nullptr : (float*)(dbig_ + o.plane_b[k]);
  }
  f.blk_info = (uint32_t*)(dwork_ + o.blk_info); f.coef_off = (uint32_t*)(dwork_ + o.coef_off);
  f.vb_list = (uint2*)(dwork_ + o.vb_list); f.vb_count = (uint32_t*)(dwork_ + o.vb_count);
  f.place_rec = (uint4*)(dwork_ + o.place_rec); f.place_cnt = (uint32_t*)(dwork_ + o.place_cnt); f.band_start = (uint32_t*)(dwork_ + o.band_start);
  f.ytox = (int8_t*)(dwork_ + o.ytox); f.ytob = (int8_t*)(dwork_ + o.ytob);
  f.inv_sigma = (float*)(dwork_ + o.inv_sigma);
  f.lf_scratch = (int32_t*)(dwork_ + o.lf_scratch); f.lf_scratch_stride = o.lf_scratch_stride;
  // HfGlobal-derived fields (present once parsed)
  if (!p.ac_code.empty()) {
    f.num_passes = cfg.max_passes > 0 ? std::min<uint32_t>(p.num_passes, (uint32_t)cfg.max_passes) : p.num_passes;     // (a progressive flush shows the first passes only; the later ones' sections stay unread)
    f.passes = dpasses_ + pass_first_[i];
    for (uint32_t ps = 0; ps < p.num_passes; ps++) {
      const ConstOffsets::Pass& cp = c.pass[ps];
      PassDev& pd = passes_host_[pass_first_[i] + ps];
      pd.code = ViewCode(p.ac_code[ps], cbase, cp.ac_ctx, cp.ac_cfg, cp.ac_alias, cp.ac_pc, cp.ac_po, cp.ac_ps);
      for (int k = 0; k < 39; k++) pd.orders[k] = (const uint16_t*)(cbase + cp.orders[k]);
      pd.shift = ps + 1 < p.num_passes ? p.pass_shift[ps] : 0; pd.pad = 0;
    }
    f.ac_code = passes_host_[pass_first_[i]].code;
    for (int k = 0; k < 39; k++) f.orders[k] = passes_host_[pass_first_[i]].orders[k];
    for (int k = 0; k < 17 * 3; k++) f.qtable[k] = c.has_qtable[k / 3] ? (const float*)(cbase + c.qtable[k]) : nullptr;
    f.num_hf_presets = p.num_hf_presets;
    uint32_t bits = 0; while ((1u << bits) < p.num_hf_presets) bits++;
    f.preset_bits = bits;
    f.hf_start_bitpos = p.end_bitpos;
  }
}

// the Modular channels of a frame (LayOutModChannels): channel table, scratch; VarDCT frames: their own weighted-predictor rows and the alpha plane the write stage reads
void Batch::FillFrameModChannels(int i, const uint8_t* cbase, const PrepareState& st) {
  const FramePlan& p = images_[i]->plan;
  const WorkOffsets& o = st.wo[i];
  FrameDev& f = frames_host_[i];
  f.mod_nchan = (uint32_t)p.gchannels.size(); f.mod_nb_meta = p.nb_meta_channels;
  f.mod_chan = (const ModChanDev*)(cbase + st.co[i].mod_chan); f.mod_base = dwork_;
  f.mod_global_decodable = p.global_decodable; f.mod_global_bitpos = p.global_data_bitpos;
  f.mod_group_scratch = (int32_t*)(dwork_ + o.mod_scratch); f.mod_group_scratch_stride = o.mod_scratch_stride;
  f.mod_bits = images_[i]->ih.depth.bits;
  if (p.modular) return;
  f.hf_end_bitpos = (uint64_t*)(dwork_ + o.hf_end);
  f.mod_wp_scratch = (int32_t*)(dwork_ + o.mod_wp); f.mod_wp_stride = o.mod_wp_stride;
  f.alpha_plane = vardct_alpha_[i].has ? (const int32_t*)(dwork_ + vardct_alpha_[i].off) : nullptr;
  f.alpha_factor = vardct_alpha_[i].factor;
}

// Descriptors of the sub-streams with their own tree / code, one table per frame that has any: sized and reserved before the one-section pre-run, whose LF decode
// reads them (FillFrameDev fills them).  Reads and adds nothing of PrepareState.
void Batch::SizeLocalTables() {
  const int n = (int)images_.size();
  local_first_.assign(n, 0);
  size_t total = 0;
  for (int i = 0; i < n; i++) {
    const FramePlan& p = images_[i]->plan;
    local_first_[i] = total;
    if (!p.local_streams.empty()) total += 1 + (size_t)p.NumModUnits();
    total += p.lf_local.size();
  }
  local_host_.assign(std::max<size_t>(total, 1), ModLocalDev());
  for (auto& d : local_host_) memset(&d, 0, sizeof(d));
  DevReserve((void**)&dlocal_, &local_cap_, sizeof(ModLocalDev) * local_host_.size());
}

// Single-section VarDCT frames: HfGlobal starts where the device-decoded LfGroup ends.  The LF stage of those frames runs now, from a temporary upload of what the
// constant arena holds so far; the end position is read back and HfGlobal parsed on the host.  Reads co, wo, cs_bytes (FillFrameDev); adds the frames' plan.ac_code etc.
void Batch::PreRunSingleSection(PrepareState& st) {
  hipStream_t stream = st.stream;
  vec<int> single;
  for (int i = 0; i < st.n; i++) if (images_[i]->plan.single_section && !images_[i]->plan.modular) {
    single.push_back(i);
    images_[i]->plan.ac_code.clear();      // (a batch that is prepared again: HfGlobal is parsed afresh below, FillFrameVarDct must not look for its tables yet)
  }
  if (single.empty()) return;
  struct DevFree { uint8_t* p = nullptr; ~DevFree() { (void)hipFree(p); } } tmpc;      // freed on every way out
  HIP_CHECK(hipMalloc((void**)&tmpc.p, Align(hconst_.size())));
  HIP_CHECK(hipMemcpyAsync(tmpc.p, hconst_.data(), hconst_.size(), hipMemcpyHostToDevice, stream));
  vec<FrameDev> tmpf;
  LaunchCfg pcfg = cfg;
  pcfg.any_local_lf = 0;
  for (int i : single) { FillFrameDev(i, tmpc.p, st); tmpf.push_back(frames_host_[i]); if (!images_[i]->plan.lf_local.empty()) pcfg.any_local_lf = 1; }
  HIP_CHECK(hipMemcpyAsync(dframes_, tmpf.data(), sizeof(FrameDev) * tmpf.size(), hipMemcpyHostToDevice, stream));
  HIP_CHECK(hipMemcpyAsync(dlocal_, local_host_.data(), sizeof(ModLocalDev) * local_host_.size(), hipMemcpyHostToDevice, stream));   // (streams with their own trees)
  if (any_modchan_) LaunchModularGlobal(dframes_, (int)tmpf.size(), pcfg, stream);   // extra channels of a one-group frame precede the LfGroup
  LaunchLfDecode(dframes_, (int)tmpf.size(), 1, pcfg, stream);
  HIP_CHECK(hipStreamSynchronize(stream));
  for (size_t k = 0; k < single.size(); k++) {
    const int i = single[k];
    uint32_t status = 0;
    uint64_t endpos[2] = {0, 0};
    HIP_CHECK(hipMemcpy(&status, tmpf[k].status, 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(endpos, tmpf[k].stream_end_bitpos, 16, hipMemcpyDeviceToHost));
    if (status) throw ParseError(status & kErrUnsupported ? "unsupported: stream feature (LF stage)" : "corrupt LF group stream", (status & kErrUnsupported) != 0);
    ParseHfGlobal(images_[i]->cs, images_[i]->ih, endpos[0], &images_[i]->plan);
  }
  HIP_CHECK(hipMemsetAsync(dwork_ + status_off_, 0, (size_t)st.n * 4, stream));
  HIP_CHECK(hipStreamSynchronize(stream));
}

// "hf_tables": HfGlobal's tables, now parsed for every VarDCT frame.  Reads natural_off; adds co's pass tables (AC codes, coefficient orders) and quant tables, qcache.
void Batch::PutHfTables(PrepareState& st) {
  Arena& arena = st.arena;
  for (int i = 0; i < st.n; i++) {
    FramePlan& p = images_[i]->plan;
    ConstOffsets& c = st.co[i];
    if (p.modular) continue;
    c.pass.assign(p.num_passes, ConstOffsets::Pass());
    for (uint32_t ps = 0; ps < p.num_passes; ps++) {
      ConstOffsets::Pass& cp = c.pass[ps];
      PutCode(arena, p.ac_code[ps], &cp.ac_ctx, &cp.ac_cfg, &cp.ac_alias, &cp.ac_pc, &cp.ac_po, &cp.ac_ps);
      for (int b = 0; b < 13; b++) for (int ch = 0; ch < 3; ch++) {
        const auto& cu = p.custom_order[(size_t)ps * 39 + b * 3 + ch];
        cp.orders[b * 3 + ch] = cu.empty() ? st.natural_off[b] : arena.Put(cu.data(), cu.size() * 2);
      }
    }
    if (p.num_passes > 1 && !EndsBehindLf(i)) any_multipass_ = true;     // (what the HF stage must handle: frames decoded at 1:8 never reach it)
    for (int k = 0; k < 17; k++) {
      const size_t* off = QuantTableOffsets(arena, st.qcache, p.qspec[k], k);
      for (int ch = 0; ch < 3; ch++) c.qtable[k * 3 + ch] = off[ch];
      c.has_qtable[k] = true;
    }
  }
}

// LDS right-sizing for the decode kernels and what else of cfg follows from the parsed frames.  Reads and adds nothing of PrepareState.
void Batch::SizeLds() {
  cfg.ac_code_bytes_compact = 16;
  cfg.max_tree_nodes = 1; cfg.mod_code_bytes = 16; cfg.ac_code_bytes = 16; cfg.any_wp = 0; cfg.any_local_trees = 0; cfg.any_local_lf = 0; cfg.any_subsampled = 0; cfg.any_prefix_ac = 0;
  for (int i = 0; i < (int)images_.size(); i++) {
    const FramePlan& p = images_[i]->plan;
    if (p.has_global_tree) SizeForModularStream(cfg, p.tree, p.tree_code);
    for (auto& ls : p.local_streams) { SizeForModularStream(cfg, ls.tree, ls.code); if (ls.unit != 0) cfg.any_local_trees = 1; }
    if (!p.lf_local.empty()) cfg.any_local_lf = 1;
    for (auto& l : p.lf_local) if (l.present) SizeForModularStream(cfg, l.tree, l.code);
    if (!p.modular && EndsBehindLf(i)) continue;     // (the rest sizes and picks the HF / IDCT kernels)
    if (!p.modular) for (auto& code : p.ac_code) { cfg.ac_code_bytes = std::max(cfg.ac_code_bytes, CodeBytes(code, true)); cfg.ac_code_bytes_compact = std::max(cfg.ac_code_bytes_compact, CodeBytesCompact(code)); }
    if (p.subsampled) cfg.any_subsampled = 1;
    if (!p.modular) for (auto& code : p.ac_code) if (code.use_prefix || code.lz77) cfg.any_prefix_ac = 1;
  }
  if (getenv("JXL_HIP_DEBUG_LDS")) fprintf(stderr, "[jxl-hip] LDS sizing: tree nodes %d, modular code %d B, AC code %d B (compact %d B), BlockCtxDev %zu B\n", cfg.max_tree_nodes, cfg.mod_code_bytes, cfg.ac_code_bytes, cfg.ac_code_bytes_compact, sizeof(BlockCtxDev));
}

// per-pass table descriptors (device array next to the frame descriptors; FillFrameVarDct fills them).  Reads and adds nothing of PrepareState.
void Batch::SizePassTables() {
  const int n = (int)images_.size();
  pass_first_.assign(n, 0);
  size_t total = 0;
  for (int i = 0; i < n; i++) { pass_first_[i] = total; total += images_[i]->plan.modular ? 0 : images_[i]->plan.num_passes; }
  passes_host_.assign(std::max<size_t>(total, 1), PassDev());
  DevReserve((void**)&dpasses_, &passes_cap_, sizeof(PassDev) * passes_host_.size());
}

// Varblock placement units: every 32-row band of every LF group of every VarDCT frame, the tallest / widest first (the lanes of a wavefront then carry bands of
// similar length).  Adds place_units_off; starts lf_simt_ anew.
void Batch::PlanPlacementUnits(PrepareState& st) {
  lf_simt_ = LfSimtPlan();
  vec<uint2> units;
  vec<uint32_t> ucost;
  for (int i = 0; i < st.n; i++) {
    const FramePlan& p = images_[i]->plan;
    if (p.modular) continue;
    for (uint32_t g = 0; g < p.num_lf_groups; g++) {
      const uint32_t gx = g % p.xlfgroups, gy = g / p.xlfgroups;
      const uint32_t gbw = std::min<uint32_t>(256, p.bw - gx * 256), gbh = std::min<uint32_t>(256, p.bh - gy * 256);
      for (uint32_t band = 0; band * 32 < gbh; band++) { units.push_back(make_uint2((uint32_t)i, g | (band << 16))); ucost.push_back(std::min<uint32_t>(32, gbh - band * 32) * gbw); }
    }
  }
  vec<uint2> sorted;
  for (uint32_t k : OrderByCostDescending(ucost)) sorted.push_back(units[k]);
  st.place_units_off = st.arena.Put(sorted.data(), sorted.size() * sizeof(uint2));
  lf_simt_.num_units = (uint32_t)sorted.size();
}

// SIMT LF decode plan (cfg.lane_stride_lf < 64): the LF-group streams of the eligible frames, spread over lanes of about equal work.  Adds simt_frame and the
// offsets of the streams, lanes and cluster tables; fills lf_simt_'s counts and flags.
void Batch::PlanLfSimt(PrepareState& st) {
  if (!any_vardct_ || cfg.lane_stride_lf >= 64) return;
  vec<LfSimtStream> streams;
  vec<uint64_t> cost;
  LfSimtTables tables;
  for (int i = 0; i < st.n; i++) {
    const FramePlan& p = images_[i]->plan;
    vec<LfSimtStream> mine;
    if (!ClassifyLfStreams(p, (uint32_t)i, tables, &mine)) continue;
    st.simt_frame[i] = 1;
    for (auto& s : mine) {
      const uint32_t gx = s.group % p.xlfgroups, gy = s.group / p.xlfgroups;
      const uint64_t gbw = std::min<uint32_t>(256, p.bw - gx * 256), gbh = std::min<uint32_t>(256, p.bh - gy * 256);
      streams.push_back(s); cost.push_back(gbw * gbh * 5 + 2048);
    }
  }
  if (streams.empty()) return;
  vec<vec<uint32_t>> lane_streams = PackLanes(cost);
  // lanes of the same frames next to each other (they read the same tables)
  std::stable_sort(lane_streams.begin(), lane_streams.end(), [&](const vec<uint32_t>& a, const vec<uint32_t>& b) { return streams[a[0]].frame < streams[b[0]].frame; });
  vec<LfSimtStream> flat;
  vec<LfSimtLane> lanes;
  for (auto& ls : lane_streams) { lanes.push_back(LfSimtLane{(uint32_t)flat.size(), (uint32_t)ls.size()}); for (uint32_t k : ls) flat.push_back(streams[k]); }
  st.simt_streams_off = st.arena.Put(flat.data(), flat.size() * sizeof(LfSimtStream));
  st.simt_lanes_off = st.arena.Put(lanes.data(), lanes.size() * sizeof(LfSimtLane));
  st.simt_luts_off = st.arena.Put(tables.luts.data(), tables.luts.size());
  lf_simt_.num_lanes = (uint32_t)lanes.size(); lf_simt_.num_streams = (uint32_t)flat.size();
  lf_simt_.lanes_per_wave = (uint32_t)std::max(1, 64 / std::max(1, cfg.lane_stride_lf));
  lf_simt_.any_legacy = 0; lf_simt_.any_wp = tables.wp ? 1 : 0; lf_simt_.any_general = tables.general || tables.wp ? 1 : 0;
  for (int i = 0; i < st.n; i++) if (!images_[i]->plan.modular && !st.simt_frame[i]) lf_simt_.any_legacy = 1;
}

// Resized outputs: the table of ResizeArgs takes its place in the constant arena here (BuildResizeTable fills it once the arena's device address is known);
// resize_plans_ sorted by slot count.  Adds the table's room to the arena.
void Batch::PlaceResizeTable(PrepareState& st) {
  // (the f32 resizes first, the integer ones of OutputSpec::resize_u8 behind them: the two arithmetics take different kernels and never share a launch group)
  auto key = [&](const ResizePlan& r) { return r.plane >= 0 ? 1u : (images_[r.unit]->out.resize_u8 ? 8u : 0u) + ResizeSlots(*images_[r.unit]); };   // (a plane: one f32 slot)
  std::stable_sort(resize_plans_.begin(), resize_plans_.end(), [&](const ResizePlan& a, const ResizePlan& b) { return key(a) < key(b); });
  resize_table_off_ = 0;
  if (resize_plans_.empty()) return;
  resize_table_off_ = st.arena.Put(nullptr, 0);                                                // (an aligned place; Put copies from its source, so the table's room is made here)
  hconst_.Resize(resize_table_off_ + resize_plans_.size() * sizeof(ResizeArgs));                 // (BuildResizeTable writes every entry)
}

// The ResizeArgs of every resized output — on every Prepare, from the arenas as they are now (shared planes may have moved) — and resize_groups_: each run of equal
// slot counts cut into groups of resize_group_max entries.  Needs dconst_, dwork_ and dbig_; reads nothing of PrepareState.
void Batch::BuildResizeTable() {
  const uint32_t group_max = std::max(1u, std::min(resize_group_max, kResizeGroupMax));
  ResizeArgs* table = (ResizeArgs*)(hconst_.data() + resize_table_off_);
  for (size_t k = 0; k < resize_plans_.size(); k++) {
    const ResizePlan& rp = resize_plans_[k];
    const ImageEntry& e = *images_[rp.unit];
    const OutputSpec& o = e.out;
    ResizeArgs a;
    memset(&a, 0, sizeof(a));
    a.src = (const float*)(dbig_ + e.off_resize_src); a.tmp = (float*)(dbig_ + e.off_resize_tmp); a.src_stride = (uint64_t)e.src_w * o.num_channels;   // (resize_u8: bytes, and so is the stride)
    a.u8 = o.resize_u8 ? 1 : 0;
    a.x0 = o.crop_x0; a.y0 = o.crop_y0; a.in_w = o.cropped() ? o.crop_w : e.src_w; a.in_h = o.cropped() ? o.crop_h : e.src_h; a.out_w = o.resize_w; a.out_h = o.resize_h;
    a.mirror = o.mirror ? 1 : 0;
    a.ax = ResizeAxisDev{(const uint32_t*)(dconst_ + rp.tab[0]), (const uint32_t*)(dconst_ + rp.tab[1]), (const float*)(dconst_ + rp.tab[2])};
    a.ay = ResizeAxisDev{(const uint32_t*)(dconst_ + rp.tab[3]), (const uint32_t*)(dconst_ + rp.tab[4]), (const float*)(dconst_ + rp.tab[5])};
    a.od = FillOutput(e, dwork_, dbig_, /*resize_target=*/true);
    if (rp.plane >= 0) {      // requested plane rp.plane of the image: its own source and rows, one slot, its place in the destination
      a.src = (const float*)(dbig_ + e.off_plane_src[(size_t)rp.plane]); a.tmp = (float*)(dbig_ + e.off_plane_tmp[(size_t)rp.plane]); a.src_stride = e.src_w;
      a.od = FillPlaneOutput(e, (size_t)rp.plane, dwork_, /*resize_target=*/true);
    }
    table[k] = a;
    const uint32_t slots = rp.plane >= 0 ? 1u : ResizeSlots(e);
    if (resize_groups_.empty() || resize_groups_.back().slots != slots || resize_groups_.back().u8 != a.u8 || resize_groups_.back().count >= group_max)
      resize_groups_.push_back(ResizeGroup{(uint32_t)k, 0, slots, 0, 0, 0, a.u8});
    ResizeGroup& g = resize_groups_.back();
    g.count++; g.max_out_w = std::max(g.max_out_w, a.out_w); g.max_in_h = std::max(g.max_in_h, a.in_h); g.max_out_h = std::max(g.max_out_h, a.out_h);
  }
}

// Every frame's descriptor with the constant arena at its device address, and lf_simt_'s pointers into it.  Reads co, wo, cs_bytes, simt_frame and the plan offsets.
void Batch::FillFrames(const PrepareState& st) {
  for (int i = 0; i < st.n; i++) { FillFrameDev(i, dconst_, st); frames_host_[i].lf_simt = lf_simt_.num_lanes ? st.simt_frame[i] : 0; }
  lf_simt_.units = (const uint2*)(dconst_ + st.place_units_off);
  if (!lf_simt_.num_lanes) return;
  lf_simt_.streams = (const LfSimtStream*)(dconst_ + st.simt_streams_off); lf_simt_.lanes = (const LfSimtLane*)(dconst_ + st.simt_lanes_off); lf_simt_.luts = dconst_ + st.simt_luts_off;
}

// The descriptor arrays travel through the pinned staging buffer, too (a copy from pageable memory is staged by the runtime and holds the calling thread — and
// others — up for as long as the device is busy): appended behind the constant arena's content, which has been copied out of it before.  Adds them to the arena.
void Batch::UploadDescriptors(PrepareState& st) {
  const size_t o_frames = st.arena.Put(frames_host_.data(), sizeof(FrameDev) * (size_t)st.n);
  const size_t o_passes = st.arena.Put(passes_host_.data(), sizeof(PassDev) * passes_host_.size());
  const size_t o_local = st.arena.Put(local_host_.data(), sizeof(ModLocalDev) * local_host_.size());
  HIP_CHECK(hipMemcpyAsync(dframes_, hconst_.data() + o_frames, sizeof(FrameDev) * (size_t)st.n, hipMemcpyHostToDevice, st.stream));
  HIP_CHECK(hipMemcpyAsync(dpasses_, hconst_.data() + o_passes, sizeof(PassDev) * passes_host_.size(), hipMemcpyHostToDevice, st.stream));
  HIP_CHECK(hipMemcpyAsync(dlocal_, hconst_.data() + o_local, sizeof(ModLocalDev) * local_host_.size(), hipMemcpyHostToDevice, st.stream));
}

// LF frames the units refer to: a batch of their own, every LF frame a one-frame image of its own size that ends in its XYB planes (PlanPostOps).  Reads frames_host_.
void Batch::PrepareLfFrameBatch(void* stream_v, bool wait_upload) {
  const int n = (int)images_.size();
  vec<int> users;
  for (int i = 0; i < n; i++) if (images_[i]->lf_source) users.push_back(i);
  if (users.empty()) lf_batch_.reset();
  else {
    if (!lf_batch_) lf_batch_.reset(new Batch(device_)); else lf_batch_->Reset();
    lf_batch_->lf_targets_.assign(users.size(), LfTarget());
    for (size_t k = 0; k < users.size(); k++) {
      const ImageEntry& user = *images_[users[k]];
      const ImageEntry& src = *user.lf_source;
      std::shared_ptr<ImageShared> sh(new ImageShared());
      sh->cs = src.cs; sh->ih = src.ih;
      sh->ih.xsize = src.plan.width; sh->ih.ysize = src.plan.height; sh->ih.orientation = 1; sh->ih.intrinsic_x = sh->ih.intrinsic_y = 0; sh->ih.have_preview = false;
      std::unique_ptr<ImageEntry> e(new ImageEntry(sh));
      e->plan = src.plan; e->frame_bitpos = src.frame_bitpos; e->frame_index = 0; e->complex = true;
      e->visible_frame_index = src.visible_frame_index; e->nonvisible_frame_index = src.nonvisible_frame_index;
      e->lf_source = src.lf_source;                      // (an LF frame may itself sit on the LF frame of the next level)
      ParsedImage pi; pi.complex = true; pi.units.push_back(std::move(e));
      lf_batch_->Append(std::move(pi));
      LfTarget& t = lf_batch_->lf_targets_[k];
      for (int c = 0; c < 3; c++) t.dst[c] = frames_host_[users[k]].lf[c];
      t.pitch = user.plan.bw; t.w = user.plan.bw; t.h = user.plan.bh;
    }
    lf_batch_->cfg.lane_stride_lf = 64;
    lf_batch_->Prepare(stream_v, wait_upload);
  }
}

// What of cfg follows from partial, progressive and chroma-subsampled frames.  Reads nothing of PrepareState.
void Batch::FinishCfg() {
  const int n = (int)images_.size();
  // (a frame cut off inside its AC groups, FramePlan::partial: the HF kernels leave out the group streams that are not completely there; nothing to do when none is)
  for (int i = 0; i < n; i++) if (images_[i]->plan.partial && images_[i]->plan.partial_ac_sections == 0 && !EndsBehindLf(i)) cfg.skip_hf = 1;
  if (refuse_partial_unscaled)
    for (int i = 0; i < n; i++) if (images_[i]->plan.partial && !EndsBehindLf(i)) throw ParseError("truncated", false);
  cfg.any_multipass = any_multipass_ ? 1 : 0;
  if (any_multipass_) cfg.lane_stride_hf = 1;   // progressive frames: only the SIMT HF kernel walks the passes
  if (cfg.any_subsampled) cfg.lane_stride_hf = 1;   // so do chroma-subsampled frames (per-channel block grids)
}

void Batch::Prepare(void* stream_v, bool wait_upload) {
  HIP_CHECK(hipSetDevice(device_));
  InitDeviceTables(stream_v);
  ResetForPrepare();
  PrepareState st(hconst_, (int)images_.size(), (hipStream_t)stream_v);
  PromoteToComplex();
  PutStreamTables(st);  st.mark("tables1");
  LayOutWork(st);
  ReserveArenas(st);  st.mark("layout+reserve");
  SizeLocalTables();
  PreRunSingleSection(st);
  PutHfTables(st);  st.mark("hf_tables");
  SizeLds();
  SizePassTables();
  if (any_complex_) {
    vec<size_t> upw;
    for (const ConstOffsets& c : st.co) upw.push_back(c.up_weights);
    PlanPostOps(hconst_, upw);
  }
  st.mark("misc");
  PlanPlacementUnits(st);
  PlanLfSimt(st);  st.mark("simt_plan");
  PlaceResizeTable(st);
  const_size_ = Align(hconst_.size());      // the constant arena is complete: reserved and uploaded; what follows points into it at its device address
  DevReserve((void**)&dconst_, &const_cap_, const_size_);
  BuildResizeTable();
  HIP_CHECK(hipMemcpyAsync(dconst_, hconst_.data(), hconst_.size(), hipMemcpyHostToDevice, st.stream));
  FillFrames(st);  st.mark("fill_frames");
  UploadDescriptors(st);  st.mark("h2d_enqueue");
  // (a pipelined caller enqueues the LF stage on the same stream right behind the upload and never waits for it on the host: the pinned staging buffer is not touched
  // again before the object's next Prepare, which comes after this decode has left the GPU)
  if (wait_upload) HIP_CHECK(hipStreamSynchronize(st.stream));
  st.mark("upload_wait");
  if (st.time_phases) fprintf(stderr, "[jxl-hip] Prepare of %d frames (%.1f MB of tables and streams, %.1f MB work arena), ms:%s\n", st.n, hconst_.size() / 1e6, work_size_ / 1e6, st.t_report.c_str());
  PrepareLfFrameBatch(stream_v, wait_upload);
  FinishCfg();
  prepared_ = true; hf_by_region_ = false;      // (until a libjpeg-exact decode is planned over this layout)
}

// JXL_HIP_DEBUG_SYNC=1: name every stage on stderr and wait for it (finding the kernel behind a device fault)
void DebugSync(const char* what, void* stream) {
  static const bool on = getenv("JXL_HIP_DEBUG_SYNC") != nullptr;
  if (!on) return;
  fprintf(stderr, "[jxl-hip] %s ...", what); fflush(stderr);
  const hipError_t e = hipStreamSynchronize((hipStream_t)stream);
  fprintf(stderr, " %s (launch status: %s)\n", hipGetErrorString(e), hipGetErrorString(hipPeekAtLastError())); fflush(stderr);
}

void Batch::Run(void* stream_v) { RunPart(stream_v, kPartWhole, false); }

// Resized outputs: behind everything that writes pixels (the write kernels of plain frames, the Modular tail, the frame tail), on the same stream
// (one launch pair per group of the table Prepare left in the constant arena: kernels_features.hip ResizeKernel)
void Batch::EnqueueResizes(void* stream) {
  resize_launches_ = resize_u8_images_ = 0;
  for (const ResizeGroup& g : resize_groups_) { LaunchResizeGroup((const ResizeArgs*)(dconst_ + resize_table_off_), g, stream); resize_launches_ += 2; if (g.u8) resize_u8_images_ += g.count; }
}

// The HF stage only writes non-zero coefficients into zeroed planes.  The IDCT kernels zero what they consumed (kernels.hip,
// IdctTileKernel pass 0), so a batch that is decoded again and again never clears its planes as a whole; only a decode whose
// tail did not run over them (first decode, JPEG reconstruction, a failed stream) leaves them dirty.
void Batch::ClearCoefficientsBeforeHf(void* stream_v) {
  // The planes are known to be zero over [0, clean extent) of the owner: hipMalloc'd memory is not cleared, and a decode only puts zeros
  // back inside its own layout — a sharer (or a refill) whose layout reaches further than anything cleared so far needs the dense clear too.
  size_t& extent = coef_is_ext_ ? ext_coef_->clean_extent : coef_owner_ ? coef_owner_->coef_clean_extent_ : coef_clean_extent_;
  if (CoefDirty() || coeff_bytes_ > extent) {
    const size_t cap = coef_is_ext_ ? ext_coef_->cap : coef_owner_ ? coef_owner_->coef_cap_ : coef_cap_;
    const size_t bytes = std::min(cap, std::max(extent, coeff_bytes_));
    HIP_CHECK(hipMemsetAsync(dcoef_, 0, bytes, (hipStream_t)stream_v));
    extent = bytes;
  }
  CoefDirty() = true;
}
void Batch::ClearCoefficientsAfterDecode(void*) { CoefDirty() = false; }

void Batch::CheckFilterBuffers() const {
  if ((fplan_.any_unfused || cfg.force_unfused_filters) && !has_plane_b_)
    throw ParseError("force_unfused_filters must be set before Prepare (the second pixel plane is only allocated when a frame needs it)", false);
}

void Batch::RunTimed(void* stream_v) { RunPart(stream_v, kPartWhole, true); }

// A launch the runtime refuses (too much LDS, an empty grid ...) does not fail at the call site: it leaves an error code that the next runtime call of the thread
// reports — possibly somebody else's.  Every enqueued stage ends with this check, so that such a launch fails the decode it belongs to, by name.
static void CheckLaunches(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) throw ParseError(std::string("kernel launch rejected by the runtime (") + what + "): " + hipGetErrorString(e), false);
}

// Enqueues the stages of `part` (decode_parts.h) on the stream, in order.  The parts of one decode may be enqueued on different streams (ordered by the caller with
// events): front and rest, so that the latency-bound LF stage of the next batch overlaps the bandwidth stages of the current one; the HF stage on its own, so that a
// caller can record an event behind it (bench.py starts the LF stage of a later batch when an HF stage has ended, not when it starts); the LF decode apart from the LF
// post-processing, whose kernels wait for wavefront slots beside the pixel kernels of the batch before and which only the IDCT and the filters need; the IDCT apart
// from the pixel stage, so that a caller that rotates coefficient sets lets the next HF stage of that set start behind it.
// (whatever an earlier runtime call of this thread left unread is not this decode's — it is named on stderr once, not silently dropped, and then cleared so that
// the checks behind this part's launches report this part's launches only)
static void ClearStaleLaunchError() {
  if (const hipError_t stale = hipPeekAtLastError()) {
    static std::atomic<bool> told{false};
    if (!told.exchange(true)) fprintf(stderr, "[jxl-hip] a HIP error left pending by an earlier call on this thread (not by this decode) is being cleared: %s\n", hipGetErrorString(stale));
    (void)hipGetLastError();
  }
}
void Batch::RunPart(void* stream_v, DecodePart part, bool timed) {
  if (!prepared_) Prepare(stream_v);
  ClearStaleLaunchError();
  if (any_vardct_) CheckFilterBuffers();
  const PartPlan plan = PlanOf(part);
  const bool tail = plan.has(kStageIdct) || plan.has(kStagePixels);
  if (plan.has(kStageHf)) hf_by_region_ = plan.jpeg && jpeg_region;      // (what StageBytes describes: the HF stage enqueued last)
  if (plan.has(kStageHf) || tail) ran_once_ = true;
  if (plan.has(kStageHf)) decodes_since_finish_++;
  // the row of events a timed part records into: the LF stage opens one; LF post-processing goes into the row opened last, the rest into the oldest row still open
  vec<void*>* marks = nullptr;
  if (timed) {
    if (plan.has(kStageLf) || timed_events_.empty()) timed_events_.emplace_back(kNumMarks, nullptr);
    const bool front = plan.has(kStageLf) || plan.has(kStageLfPost);
    marks = front ? &timed_events_.back() : &timed_events_[std::min(timed_rest_cursor_, timed_events_.size() - 1)];
  }
  const PartRun r{stream_v, plan, timed, marks};
  if (plan.has(kStageLf)) StageLf(r);
  if (plan.has(kStageLfPost)) StageLfPost(r);
  if (plan.has(kStageHf)) StageHf(r);
  if (plan.has(kStageIdct)) StageIdct(r);
  if (plan.has(kStagePixels)) StagePixels(r);
}

void Batch::RecordMark(const PartRun& r, Mark m) {
  if (!r.marks) return;
  hipEvent_t ev; HIP_CHECK(hipEventCreate(&ev)); (*r.marks)[m] = ev;
  HIP_CHECK(hipEventRecord(ev, (hipStream_t)r.stream));
}

void Batch::StageLfBegin(const PartRun& r) {
  RecordMark(r, kMarkLfStart);
  DebugSync("start", r.stream);
  if (any_modchan_) LaunchModularGlobal(dframes_, (int)images_.size(), cfg, r.stream);   // Modular frames; extra channels of VarDCT frames
  DebugSync("modular global", r.stream);
}
void Batch::StageLfRest(const PartRun& r, bool simt_launched) {
  const int n = (int)images_.size();
  cfg.lf_head_start = r.plan.lf_head_start;
  cfg.lf_simt_launched = simt_launched ? 1 : 0;
  if (any_vardct_) LaunchLfDecode(dframes_, n, max_lf_groups_, cfg, r.stream, &lf_simt_, &trace_);
  cfg.lf_wide_once = 0; cfg.lf_simt_launched = 0;
  DebugSync("LF decode", r.stream);
  CheckLaunches("LF stage");
  if (any_vardct_ && !cfg.idct_flags_known && r.plan.split && !cfg.no_flag_wait) EnqueueFlagReadback(r.stream);
  RecordMark(r, kMarkLfEnd);
}

LfGroupKey Batch::LfKey() const {
  LfGroupKey k;
  const LfSimtShape s = LfSimtShapeOf(cfg, &lf_simt_);
  k.eligible = prepared_ && any_vardct_ && !any_modchan_ && !lf_batch_ && !cfg.any_local_lf && s.kernel != kLfSimtNone;
  k.kernel = s.kernel * 4 + (int)s.spec_shift; k.lanes_per_wave = s.lanes_per_wave; k.lf_flags = s.lf_flags;
  return k;
}

void Batch::RunLfGroup(Batch* const* batches, int n, void* stream, bool timed, const std::function<void(int)>& after) {
  if (n < 1 || !batches || !batches[0]) throw ParseError("LF group: no batch", false);
  if (n == 1) { batches[0]->RunPart(stream, kPartLf, timed); if (after) after(0); return; }
  if (n > kLfGroupMax) throw ParseError("LF group: more batches than a launch has parts", false);
  const LfGroupKey key = batches[0]->LfKey();
  for (int i = 0; i < n; i++) {
    if (!batches[i] || batches[i]->device_ != batches[0]->device_) throw ParseError("LF group: batches of different devices", false);
    for (int k = 0; k < i; k++) if (batches[k] == batches[i]) throw ParseError("LF group: a batch appears twice", false);
    const LfGroupKey ki = batches[i]->LfKey();
    if (!ki.eligible || !(ki == key)) throw ParseError("LF group: batches whose SIMT LF launches cannot be shared", false);
  }
  ClearStaleLaunchError();
  const PartPlan plan = PlanOf(kPartLf);
  const LfSimtShape shape = LfSimtShapeOf(batches[0]->cfg, &batches[0]->lf_simt_);
  PartRun runs[kLfGroupMax];
  LfSimtGroupPart parts[kLfGroupMax];
  for (int i = 0; i < n; i++) {
    Batch& b = *batches[i];
    b.CheckFilterBuffers();
    if (timed) b.timed_events_.emplace_back(kNumMarks, nullptr);      // (the LF stage opens a row of events: RunPart)
    runs[i] = PartRun{stream, plan, timed, timed ? &b.timed_events_.back() : nullptr};
    b.StageLfBegin(runs[i]);
    parts[i] = LfSimtGroupPart{b.dframes_, &b.lf_simt_};
  }
  LaunchLfSimtGroup(parts, n, shape, stream);
  for (int i = 0; i < n; i++) {
    batches[i]->StageLfRest(runs[i], /*simt_launched=*/true);
    if (after) after(i);
  }
}

// A caller that enqueues the stages separately: the placement flags travel to pinned host memory behind the LF stage, and the tail —
// enqueued steps later — waits for that copy (long done by then) instead of launching every IDCT kernel variant
void Batch::EnqueueFlagReadback(void* stream) {
  const size_t n = images_.size();
  if (!flags_pinned_ || flags_pinned_n_ < n) {
    if (flags_pinned_) (void)hipHostFree(flags_pinned_);      // (waits for the device: the capacity is generous so that a refilled batch object rarely gets here)
    flags_pinned_ = nullptr;
    const size_t cap = std::max<size_t>(4096, 2 * n);
    HIP_CHECK(hipHostMalloc((void**)&flags_pinned_, cap * 4));
    flags_pinned_n_ = cap;
  }
  if (!flags_event_) { hipEvent_t ev; HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming)); flags_event_ = ev; }
  HIP_CHECK(hipMemcpyAsync(flags_pinned_, dwork_ + flags_off_, n * 4, hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_CHECK(hipEventRecord((hipEvent_t)flags_event_, (hipStream_t)stream));
  flags_pending_ = true;
}
void Batch::WaitForIdctFlags(const PartRun& r) {
  if (cfg.idct_flags_known || !flags_pending_ || !r.plan.split || !any_full_vardct_ || r.plan.jpeg) return;      // (the libjpeg-exact tail has one IDCT kernel: nothing to wait for)
  HIP_CHECK(hipEventSynchronize((hipEvent_t)flags_event_));
  ApplyIdctFlags(flags_pinned_);
  flags_pending_ = false;
}

void Batch::StageLfPost(const PartRun& r) {
  if (!r.plan.jpeg) {
    if (lf_batch_) lf_batch_->RunPart(r.stream, kPartWhole, false);     // LF frames: decoded to the end, their planes copied into the LF planes of the units that refer to them
    if (any_vardct_) LaunchLfPost(dframes_, (int)images_.size(), max_bw_, max_bh_, max_groups_, r.stream);
    DebugSync("LF post", r.stream);
    CheckLaunches("LF post-processing");
  }
  if (r.plan.split) RecordMark(r, kMarkLfPostEnd);      // (the whole decode: the HF stage records it, behind the coefficient clear)
}

// With VarDCT frames in the batch the Modular sub-streams and tail run here (the PassGroup Modular parts start where the HF streams ended); without, in the pixel stage.
void Batch::StageHf(const PartRun& r) {
  const int n = (int)images_.size();
  // the HF decoder only writes non-zero coefficients into cleared planes (outside the per-stage brackets when the halves are timed separately)
  // (a batch of 1:8 frames only, any_full_vardct_ == false: no coefficient plane exists, nothing of this stage, of the IDCT or of the filters is launched)
  if (any_full_vardct_) ClearCoefficientsBeforeHf(r.stream);
  RecordMark(r, r.plan.split ? kMarkHfStart : kMarkLfPostEnd);
  if (any_vardct_) {
    // (progressive flush at the kDC step, cfg.skip_hf: no AC group is decoded — the planes stay zero, the IDCT sees the LF part only)
    const bool by_list = hf_by_region_;      // frames decoded by region decode the groups of their lists only; every other HF stage decodes every group
    cfg.hf_by_list = by_list ? 1 : 0;
    if (!cfg.skip_hf && any_full_vardct_) LaunchHfDecode(dframes_, n, by_list ? max_hf_slots_ : max_groups_, cfg, r.stream, &trace_);
    cfg.hf_by_list = 0;
    DebugSync("HF decode", r.stream);
    if (any_modchan_) EnqueueModularTail(r.stream);
    if (any_full_vardct_) LaunchZeroFailedCoefficients(dframes_, n, r.stream);   // (frames that failed up to here are skipped by the IDCT kernels: their planes are zeroed now)
    CheckLaunches("HF stage / Modular sub-streams");
  }
  RecordMark(r, kMarkHfEnd);
}

void Batch::StageIdct(const PartRun& r) {
  WaitForIdctFlags(r);
  if (any_vardct_) {
    if (r.plan.split) RecordMark(r, kMarkIdctStart);                        // the tail may sit on another stream than the HF stage: its own start mark
    if (r.plan.jpeg) EnqueueJpegIdct(r.stream);
    else if (any_full_vardct_) LaunchIdct(dframes_, (int)images_.size(), max_groups_, max_bw_, max_bh_, cfg, r.stream);
    DebugSync("IDCT", r.stream);
    CheckLaunches("IDCT stage");
  }
  RecordMark(r, kMarkIdctEnd);
  if (any_full_vardct_) ClearCoefficientsAfterDecode(r.stream);   // (the IDCT kernels zeroed what they read)
}

// Restoration filters | colour and write of plain frames, the 1:8 frames' LF image, (batches without VarDCT frames) the Modular sub-streams and tail, the frame tail of
// multi-frame / feature images, resizes.  The libjpeg-exact flavour: chroma upsampling, colour, write, resizes (no image of a batch without VarDCT frames takes it).
void Batch::StagePixels(const PartRun& r) {
  const int n = (int)images_.size();
  WaitForIdctFlags(r);
  if (r.plan.jpeg) {
    RecordMark(r, kMarkFiltersEnd);
    if (any_vardct_) { EnqueueJpegColorOut(r.stream); EnqueueResizes(r.stream); DebugSync("JPEG pixels", r.stream); }
    CheckLaunches(any_vardct_ ? "JPEG pixels" : "Modular sub-streams / frame tail");
  } else {
    const bool stop = any_vardct_ && cfg.debug_stop_after;      // (testing: the planes as they stand behind an earlier stage)
    if (any_vardct_) {
      if (cfg.debug_stop_after != 1 && any_full_vardct_) LaunchFilters(dframes_, n, max_w_, max_h_, fplan_, cfg, r.stream);
      DebugSync("filters", r.stream);
    }
    RecordMark(r, kMarkFiltersEnd);
    if (!any_vardct_ && any_modchan_) EnqueueModularTail(r.stream);
    if (!stop && any_full_vardct_) LaunchOutput(dframes_, n, max_w_, max_h_, fplan_, cfg, r.stream);
    if (!stop && any_scaled_) LaunchLfOutput(dframes_, n, max_bw_, max_bh_, r.stream);   // 1:8 frames: the LF image through the colour transform and the write stage
    plane_outputs_ = 0;
    if (!stop && any_complex_) EnqueuePostOps(r.stream);
    if (!stop) EnqueueResizes(r.stream);
    if (any_vardct_) { FailJpegScaledOutputs(r.stream); DebugSync("output / frame tail", r.stream); }
    CheckLaunches(any_vardct_ ? "filters / output / frame tail" : "Modular sub-streams / frame tail");
  }
  RecordMark(r, kMarkOutputEnd);
  if (r.timed && r.plan.split) timed_rest_cursor_++;
}

// (tracing) when the marks (decode_parts.h Mark, in that order) of the timed decode recorded last were reached, in ms after `ref_event`; -1 = not recorded
void Batch::DebugTimeline(void* ref_event, float out[kNumMarks]) {
  for (int i = 0; i < kNumMarks; i++) out[i] = -1;
  if (timed_events_.empty()) return;
  auto& evs = timed_events_.back();
  for (int i = 0; i < kNumMarks && i < (int)evs.size(); i++) {
    if (!evs[(size_t)i]) continue;
    if (hipEventSynchronize((hipEvent_t)evs[(size_t)i]) != hipSuccess) { (void)hipGetLastError(); continue; }
    float ms = 0;
    if (hipEventElapsedTime(&ms, (hipEvent_t)ref_event, (hipEvent_t)evs[(size_t)i]) == hipSuccess) out[i] = ms; else (void)hipGetLastError();
  }
}

StageTimes Batch::CollectTimes(int* runs) {
  StageTimes t;
  *runs = (int)timed_events_.size();
  // a stage lasts from the end mark of the stage before it — or, where a split decode recorded one, from its own start mark — to its end mark
  const struct { float* ms; Mark from, own_start, to; } stages[6] = {
      {&t.lf_ms, kMarkLfStart, kNumMarks, kMarkLfEnd},         {&t.lfpost_ms, kMarkLfEnd, kNumMarks, kMarkLfPostEnd},         {&t.hf_ms, kMarkLfPostEnd, kMarkHfStart, kMarkHfEnd},
      {&t.idct_ms, kMarkHfEnd, kMarkIdctStart, kMarkIdctEnd}, {&t.filter_ms, kMarkIdctEnd, kNumMarks, kMarkFiltersEnd}, {&t.out_ms, kMarkFiltersEnd, kNumMarks, kMarkOutputEnd}};
  for (auto& evs : timed_events_) {
    bool complete = true;
    for (int m = kMarkLfStart; m <= kMarkOutputEnd; m++) if (!evs[(size_t)m]) complete = false;
    if (!complete) { for (auto e : evs) if (e) (void)hipEventDestroy((hipEvent_t)e); (*runs)--; continue; }
    HIP_CHECK(hipEventSynchronize((hipEvent_t)evs[kMarkOutputEnd]));
    for (auto& st : stages) {
      void* from = st.own_start != kNumMarks && evs[st.own_start] ? evs[st.own_start] : evs[st.from];
      float ms = 0; HIP_CHECK(hipEventElapsedTime(&ms, (hipEvent_t)from, (hipEvent_t)evs[st.to])); *st.ms += ms;
    }
    float tot = 0; HIP_CHECK(hipEventElapsedTime(&tot, (hipEvent_t)evs[kMarkLfStart], (hipEvent_t)evs[kMarkOutputEnd])); t.total_ms += tot;
    for (auto e : evs) if (e) (void)hipEventDestroy((hipEvent_t)e);
  }
  timed_events_.clear();
  timed_rest_cursor_ = 0;
  return t;
}

static std::string DeviceStatusMessage(uint32_t status, int frame, bool* unsupported) {
  *unsupported = (status & kErrUnsupported) != 0;
  if (*unsupported) return "unsupported: stream feature on the device path (frame " + std::to_string(frame) + ")";
  return "corrupt stream (device status " + std::to_string(status) + ", frame " + std::to_string(frame) + ")";
}

// An output with OutputSpec::jpeg_scale != 1 is the picture of libjpeg's scaled decode, which the float pipeline has no way to compute — and one with
// OutputSpec::resize_u8 is resampled from libjpeg's u8 picture, which it has no way to compute either: behind a Run the image's
// status word is set, so that Finish fails it — alone, the others are written — with the reason below.  (Its write stage has stayed inside the scaled picture:
// FrameDev::img_w / img_h.)
void Batch::FailJpegScaledOutputs(void* stream_v) {
  static const uint32_t kRefused = kErrUnsupported;
  for (size_t u = 0; u < images_.size(); u++)
    if (images_[u]->frame_index == 0 && (images_[u]->out.jpeg_scale != 1 || images_[u]->out.resize_u8)) HIP_CHECK(hipMemcpyAsync(dwork_ + status_off_ + u * 4, &kRefused, 4, hipMemcpyHostToDevice, (hipStream_t)stream_v));
}

void Batch::Finish(void* stream_v) {
  vec<uint32_t> status;
  FinishStatus(stream_v, &status);
  for (size_t i = 0; i < status.size(); i++) {
    if (!status[i]) continue;
    bool unsupported = false;
    std::string msg = DeviceStatusMessage(status[i], (int)i, &unsupported);
    if (unsupported && images_[i]->frame_index == 0 && images_[i]->out.jpeg_scale != 1)
      msg = "unsupported: image " + std::to_string(images_[i]->pub_index) + " has an output with jpeg_scale " + std::to_string(images_[i]->out.jpeg_scale) +
            ", which only the libjpeg-exact decode writes (DecodeJpegPixels)";
    else if (unsupported && images_[i]->frame_index == 0 && images_[i]->out.resize_u8)
      msg = "unsupported: integer resample of image " + std::to_string(images_[i]->pub_index) + " under a plain decode: only the libjpeg-exact decode writes an output with resize_u8 (DecodeJpegPixels)";
    throw ParseError(msg, unsupported);
  }
}

// Finish without the throw: waits, hands out the per-unit status words (0 = decoded) and clears the ones that are set, so that a caller can let a damaged
// frame fail alone (ReconstructJpegs)
void Batch::FinishStatus(void* stream_v, vec<uint32_t>* status_out) {
  hipStream_t stream = (hipStream_t)stream_v;
  if (lf_batch_) lf_batch_->Finish(stream_v);            // (a damaged LF frame fails the decode like a damaged frame)
  HIP_CHECK(hipStreamSynchronize(stream));
  const int n = (int)images_.size();
  vec<uint32_t>& status = *status_out;
  status.assign(n, 0);
  HIP_CHECK(hipMemcpy(status.data(), dwork_ + status_off_, (size_t)n * 4, hipMemcpyDeviceToHost));
  for (int i = 0; i < n; i++) {
    if (!status[i]) continue;
    HIP_CHECK(hipMemset(dwork_ + status_off_, 0, (size_t)n * 4));
    CoefDirty() = true;                                  // (a failed stream may have written where no IDCT looked)
    return;                                              // (as when Finish throws: the counters below wait for a decode that succeeds)
  }
  if (any_vardct_ && decodes_since_finish_ > 0) {
    // non-zero coefficients per decode of every frame (deterministic per stream): the HF stage's written bytes for StageBytes
    vec<uint32_t> cnt(n, 0);
    HIP_CHECK(hipMemcpy(cnt.data(), dwork_ + hfw_off_, (size_t)n * 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; i++) hf_written_[i] = cnt[i] / decodes_since_finish_;
    HIP_CHECK(hipMemset(dwork_ + hfw_off_, 0, (size_t)n * 4));
    decodes_since_finish_ = 0;
  }
  if (any_vardct_ && !cfg.idct_flags_known && ran_once_) {
    // the LF stage has classified every frame's varblock placement: later decodes of this batch skip the kernels nobody needs
    vec<uint32_t> flags(n, 0);
    HIP_CHECK(hipMemcpy(flags.data(), dwork_ + flags_off_, (size_t)n * 4, hipMemcpyDeviceToHost));
    ApplyIdctFlags(flags.data());
  }
}

// Per-frame flags of the varblock placement (LfPlaceBand) -> which IDCT kernels a decode of this batch needs.
void Batch::ApplyIdctFlags(const uint32_t* flags) {
  const int n = (int)images_.size();
  cfg.any_irregular_blocks = cfg.any_big_blocks = 0;
  cfg.need_tile4_plain = cfg.need_tile4_special = cfg.need_tile8_plain = cfg.need_tile8_special = 0;
  for (int i = 0; i < n; i++) {
    if (images_[i]->plan.modular) continue;
    const uint32_t v = flags[i];
    cfg.any_irregular_blocks |= (v & 1) != 0; cfg.any_big_blocks |= (v & 2) != 0;
    if (v & 1) continue;                                  // generic IdctKernel frame
    if (v & 4) { if (v & 8) cfg.need_tile8_special = 1; else cfg.need_tile8_plain = 1; }
    else { if (v & 8) cfg.need_tile4_special = 1; else cfg.need_tile4_plain = 1; }
  }
  cfg.idct_flags_known = 1;
}

// ---- JPEG reconstruction -----------------------------------------------------------------------------------------------------------------
// What a lossless JPEG transcode looks like as a frame: one VarDCT frame in YCbCr (or of a grey image), not XYB, without extra channels, upsampling, passes or
// image features.  (The RAW quantisation table belongs to it too, but a one-group frame's is only known after Prepare: the callers look at it then.)
static bool IsPlainJpegFrameOf(int num_units, bool complex, const ImageEntry& e) {
  const FramePlan& p = e.plan;
  if (num_units != 1 || (complex && !p.subsampled) || p.modular || e.ih.xyb_encoded || !p.do_ycbcr && e.ih.color_space != 1) return false;
  if (p.upsampling != 1 || p.num_passes != 1 || !e.ih.extra.empty()) return false;
  if (p.subsampled && ((p.flags & (1 | 2 | 16)) || p.have_crop || p.frame_type != 0)) return false;
  return true;
}
bool Batch::IsPlainJpegFrame(int i) const { return IsPlainJpegFrameOf(pub_[i].num_units, pub_[i].complex, *images_[pub_[i].first_unit]); }

bool Batch::CanReconstructJpeg(int i, std::string* why) {
  auto no = [&](const char* m) { if (why) *why = m; return false; };
  const PubImage& pi = pub_[i];
  const ImageEntry& e = *images_[pi.first_unit];
  if (e.shared->boxes.jbrd.empty()) return no("no jbrd box");
  if (!IsPlainJpegFrame(i)) return no("not a plain JPEG-transcoded frame");
  if (jpeg_data_.size() < pub_.size()) jpeg_data_.resize(pub_.size());
  if (!jpeg_data_[i]) {
    std::unique_ptr<JpegData> jd(new JpegData());
    std::string err;
    const MetadataBoxes& bx = e.shared->boxes;
    if (!ParseJbrd(bx.jbrd.data(), bx.jbrd.size(), jd.get(), &err)) { if (why) *why = err; return false; }
    JpegMetadataSources src;
    src.icc = e.ih.icc.data(); src.icc_size = e.ih.icc.size();
    src.exif = bx.have_exif ? bx.exif.data() : nullptr; src.exif_size = bx.exif.size(); src.exif_brob = bx.exif_brob;
    src.xml = bx.have_xml ? bx.xml.data() : nullptr; src.xml_size = bx.xml.size(); src.xml_brob = bx.xml_brob;
    if (!FillJpegMetadata(jd.get(), src, &err)) { if (why) *why = err; return false; }
    if (jd->components.size() != 3 && jd->components.size() != 1) return no("component count");
    for (uint8_t m : jd->marker_order) if (m == 0xC9 || m == 0xCA) return no("unsupported: arithmetic-coded JPEG");
    jpeg_data_[i] = std::move(jd);
  }
  return true;
}

vec<uint8_t> Batch::ReconstructJpeg(int i, void* stream_v) {
  std::string why;
  if (!CanReconstructJpeg(i, &why)) throw ParseError("JPEG reconstruction: " + why, true);
  hipStream_t stream = (hipStream_t)stream_v;
  if (!prepared_) Prepare(stream_v);
  const int u = pub_[i].first_unit;
  const ImageEntry& e = *images_[u];
  const FramePlan& p = e.plan;
  JpegData& jd = *jpeg_data_[i];
  {
    // quantisation tables from the frame's RAW table (HfGlobal; for one-group frames known only after Prepare): jxl channels X, Y, B
    // = Cb, Y, Cr, and libjxl's coefficient layout is the transpose of JPEG's
    const QuantTableSpec& q = p.qspec[0];
    if (q.mode != 7) throw ParseError("JPEG reconstruction: quantisation table is not a RAW (JPEG) table", true);
    for (size_t c = 0; c < jd.components.size(); c++) {
      const int ch = jd.components.size() == 1 ? 1 : (c == 0 ? 1 : c == 1 ? 0 : 2);
      if (q.raw[ch].size() != 64) throw ParseError("JPEG reconstruction: RAW table size", true);
      JpegQuantTable& t = jd.quant[jd.components[c].quant_idx];
      for (int v = 0; v < 8; v++) for (int u = 0; u < 8; u++) t.values[v * 8 + u] = q.raw[ch][u * 8 + v];
    }
  }
  // entropy decode only: LF stage (LF coefficients = JPEG DC, block metadata) and HF stage (AC coefficients)
  RunPart(stream_v, kPartFront, false);
  RunPart(stream_v, kPartHf, false);
  const size_t ncomp = jd.components.size();
  // component planes: the frame's (padded) block grid shifted by the channel's subsampling; sampling factors for the SOF marker from
  // the frame header (libjxl dec_frame.cc: h_samp_factor = 1 << (max shift - shift), JPEG components Y, Cb, Cr = channels 1, 0, 2)
  size_t comp_blocks[3] = {0, 0, 0}, comp_first[3] = {0, 0, 0}, nblk = 0;
  {
    int max_hs = 0, max_vs = 0;
    for (int c = 0; c < 3; c++) { max_hs = std::max(max_hs, (int)p.hs[c]); max_vs = std::max(max_vs, (int)p.vs[c]); }
    for (size_t c = 0; c < ncomp; c++) {
      const int ch = ncomp == 1 ? 1 : (c == 0 ? 1 : c == 1 ? 0 : 2);
      jd.components[c].h_samp = 1u << (max_hs - p.hs[ch]);
      jd.components[c].v_samp = 1u << (max_vs - p.vs[ch]);
      comp_blocks[c] = (size_t)(p.bw >> p.hs[ch]) * (p.bh >> p.vs[ch]);
      comp_first[c] = nblk;
      nblk += comp_blocks[c];
    }
  }
  int16_t* dcoef = nullptr;
  HIP_CHECK(hipMalloc((void**)&dcoef, nblk * 64 * sizeof(int16_t)));
  struct DevFree { int16_t* p; ~DevFree() { if (p) (void)hipFree(p); } } dcoef_guard{dcoef};   // (released on every exit, incl. exceptions below)
  JpegCoefArgs a;
  memset(&a, 0, sizeof(a));
  a.ncomp = (uint32_t)ncomp;
  for (size_t c = 0; c < ncomp; c++) a.comp_off[c] = (uint32_t)comp_first[c];
  for (size_t c = 0; c < ncomp; c++) for (int k = 0; k < 64; k++) a.qt[c][k] = jd.quant[jd.components[c].quant_idx].values[k];
  a.out = dcoef;
  LaunchJpegCoefficients(dframes_, u, a, p.bw, p.bh, stream_v);
  DebugSync("JPEG coefficients", stream_v);
  vec<int16_t> host(nblk * 64);
  hipError_t err = hipMemcpyAsync(host.data(), dcoef, host.size() * sizeof(int16_t), hipMemcpyDeviceToHost, stream);
  if (err == hipSuccess) err = hipStreamSynchronize(stream);
  if (err != hipSuccess) throw ParseError(std::string("HIP error: ") + hipGetErrorString(err), false);
  Finish(stream_v);
  const int16_t* planes[3] = {host.data(), host.data() + comp_first[1] * 64, host.data() + comp_first[2] * 64};
  vec<uint8_t> out;
  if (!WriteJpeg(jd, e.ih.xsize, e.ih.ysize, planes, &out, &why)) throw ParseError(why, true);
  return out;
}

// ---- batch JPEG reconstruction: one entropy run for all images, sequential scans written by the device (jpeg_write.hip) ---------------------
// What the frame of a JPEG transcode says about the JPEG (as ReconstructJpeg documents it): quantisation tables in JPEG's natural order, sampling factors and, for the
// coefficient arena, the component planes packed one after another — component c (0 Y, 1 Cb, 2 Cr = channels 1, 0, 2) is a grid of grid_w x grid_h blocks from block
// comp_first[c] on.  hs / vs: the component's shifts against the frame's block grid.
struct JpegFrameGrid {
  uint32_t ncomp = 0;
  int32_t qt[3][64];
  uint32_t h_samp[3] = {1, 1, 1}, v_samp[3] = {1, 1, 1}, hs[3] = {0, 0, 0}, vs[3] = {0, 0, 0}, grid_w[3] = {0, 0, 0}, grid_h[3] = {0, 0, 0};
  size_t comp_first[3] = {0, 0, 0}, nblk = 0;
};
namespace {
// `what`: whose error it is ("JPEG reconstruction")
bool JpegGridFromFrame(const FramePlan& p, size_t ncomp, const char* what, JpegFrameGrid* g, std::string* why) {
  const QuantTableSpec& q = p.qspec[0];
  if (q.mode != 7) { *why = std::string(what) + ": quantisation table is not a RAW (JPEG) table"; return false; }
  int max_hs = 0, max_vs = 0;
  for (int c = 0; c < 3; c++) { max_hs = std::max(max_hs, (int)p.hs[c]); max_vs = std::max(max_vs, (int)p.vs[c]); }
  g->ncomp = (uint32_t)ncomp; g->nblk = 0;
  for (size_t c = 0; c < ncomp; c++) {
    const int ch = ncomp == 1 ? 1 : (c == 0 ? 1 : c == 1 ? 0 : 2);
    if (q.raw[ch].size() != 64) { *why = std::string(what) + ": RAW table size"; return false; }
    for (int v = 0; v < 8; v++) for (int u = 0; u < 8; u++) g->qt[c][v * 8 + u] = q.raw[ch][u * 8 + v];      // (libjxl's coefficient layout is the transpose of JPEG's)
    g->hs[c] = p.hs[ch]; g->vs[c] = p.vs[ch];
    g->h_samp[c] = 1u << (max_hs - p.hs[ch]); g->v_samp[c] = 1u << (max_vs - p.vs[ch]);
    g->grid_w[c] = p.bw >> p.hs[ch]; g->grid_h[c] = p.bh >> p.vs[ch];
    g->comp_first[c] = g->nblk;
    g->nblk += (size_t)g->grid_w[c] * g->grid_h[c];
  }
  return true;
}
// ... into the JPEG's own description (reconstruction: the component count is the jbrd box's)
bool FillJpegFromFrame(const FramePlan& p, JpegData* jd, JpegFrameGrid* g, std::string* why) {
  if (!JpegGridFromFrame(p, jd->components.size(), "JPEG reconstruction", g, why)) return false;
  for (size_t c = 0; c < jd->components.size(); c++) {
    JpegQuantTable& t = jd->quant[jd->components[c].quant_idx];
    for (int k = 0; k < 64; k++) t.values[k] = g->qt[c][k];
    jd->components[c].h_samp = g->h_samp[c]; jd->components[c].v_samp = g->v_samp[c];
  }
  return true;
}
}  // namespace

// What the phases of a batch reconstruction share (PlanJpegWrite fills it, the next plan replaces it)
struct Batch::JpegWriteState {
  struct ScanPlan { JpegHuffTable dc[4], ac[4]; uint32_t restart = 0; bool progressive = false; };
  struct Img { bool ok = false, device = false, progressive = false; size_t first_blk = 0; JpegFrameGrid grid; size_t first_scan = 0, num_scans = 0; std::vector<ScanPlan> plans; };
  std::vector<Img> im;
  vec<JpegScanDev> scans;
  vec<JpegHuffDev> tables;
  vec<uint32_t> resets;          // reset points of the AC progressive scans, as batch block numbers
  bool any_progressive = false, fail_refused = false;
  bool head_pending = false;     // the raw size and the flag words are on their way to (or in) pinned memory: EnqueueJpegHeadReadback
  uint64_t num_blocks = 0, num_segs = 0;
  size_t total_blk = 0, images_ok = 0;
  size_t o_coef = 0, o_scans = 0, o_tables = 0, o_flags = 0, o_resets = 0, o_gather = 0, arena_bytes = 0;
  size_t o_bits = 0, o_bitpos = 0, o_segbits = 0, o_segbytes = 0, o_segoff = 0, o_tile = 0, o_meta = 0, o_flush = 0, o_spanidx = 0, o_spanfirst = 0;
  JpegWritePlan wp;              // device pointers: valid from EnqueueJpegPlan on
  vec<JpegPixelImage> gather;    // the gather table (host copy; the upload reads it), the image of every entry, the launch groups over it
  vec<int> gather_image;
  std::vector<JpegPixelGroup> groups;
};

// Pinned staging of the reconstruction's copies to the host: a head of `head` bytes (the raw size and the per-image flag words: 8 + 4 n) and two chunks of
// kJpegStageChunk bytes behind it, which CopyJpegToHost fills in turn.  Small and of a fixed size — pinning memory costs about as much per byte as copying it, and a
// pipeline has a batch object per slot —; it only grows with the number of images (hipHostFree waits for the device).
static constexpr size_t kJpegStageChunk = (size_t)4 << 20;
uint8_t* Batch::JpegPinned(size_t head) {
  const size_t head_cap = (std::max<size_t>(head, 4096) + 4095) & ~(size_t)4095, bytes = head_cap + 2 * kJpegStageChunk;
  if (jpeg_pinned_ && jpeg_pinned_cap_ >= bytes) return jpeg_pinned_;
  if (jpeg_pinned_) (void)hipHostFree(jpeg_pinned_);
  jpeg_pinned_ = nullptr; jpeg_pinned_cap_ = 0;
  const size_t cap = 2 * head_cap + 2 * kJpegStageChunk;
  HIP_CHECK(hipHostMalloc((void**)&jpeg_pinned_, cap));
  jpeg_pinned_cap_ = cap;
  return jpeg_pinned_;
}
// `bytes` from device memory into pageable host memory, on `stream`: hipMemcpyAsync into the two pinned chunks in turn, the host copying chunk k - 1 out while chunk k
// is on its way; waits for the last one.  (Not hipMemcpy: that goes through the null stream and would stall the streams of a pipeline's other jobs.)
void Batch::CopyJpegToHost(void* dst_v, const void* src_v, size_t bytes, void* stream_v) {
  hipStream_t stream = (hipStream_t)stream_v;
  uint8_t* dst = (uint8_t*)dst_v;
  const uint8_t* src = (const uint8_t*)src_v;
  if (!jpeg_pinned_ || jpeg_pinned_cap_ < 2 * kJpegStageChunk) throw ParseError("CopyJpegToHost without staging", false);
  uint8_t* chunk[2] = {jpeg_pinned_ + jpeg_pinned_cap_ - 2 * kJpegStageChunk, jpeg_pinned_ + jpeg_pinned_cap_ - kJpegStageChunk};
  for (int k = 0; k < 2; k++) if (!jpeg_copy_event_[k]) { hipEvent_t ev; HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming)); jpeg_copy_event_[k] = ev; }
  size_t prev_off = 0, prev_len = 0;
  int k = 0;
  for (size_t off = 0; off < bytes; off += kJpegStageChunk, k ^= 1) {
    const size_t len = std::min(kJpegStageChunk, bytes - off);
    HIP_CHECK(hipMemcpyAsync(chunk[k], src + off, len, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipEventRecord((hipEvent_t)jpeg_copy_event_[k], stream));
    if (prev_len) { HIP_CHECK(hipEventSynchronize((hipEvent_t)jpeg_copy_event_[k ^ 1])); memcpy(dst + prev_off, chunk[k ^ 1], prev_len); }
    prev_off = off; prev_len = len;
  }
  if (prev_len) { HIP_CHECK(hipEventSynchronize((hipEvent_t)jpeg_copy_event_[k ^ 1])); memcpy(dst + prev_off, chunk[k ^ 1], prev_len); }
}

// ---- phase 1, host only (after Prepare): which images can be reconstructed, the coefficient planes of all of them in one arena, the gather table over it, and — for the
// images the device writes — scan table, table snapshots and reset points.  An image that cannot be reconstructed gets its jpeg_result now.  Returns the images left.
size_t Batch::PlanJpegWrite() {
  const int n = (int)pub_.size();
  jpeg_results_.clear(); jpeg_results_.resize((size_t)n);
  jpeg_device_images_ = jpeg_host_images_ = jpeg_device_progressive_images_ = 0;
  jpeg_gather_launches_ = 0;
  jw_ = std::make_shared<JpegWriteState>();
  JpegWriteState& w = *jw_;
  typedef JpegWriteState::Img Img;
  typedef JpegWriteState::ScanPlan ScanPlan;
  memset(&w.wp, 0, sizeof(w.wp));
  w.im.resize((size_t)n);
  std::vector<Img>& im = w.im;
  for (int i = 0; i < n; i++) {
    std::string why;
    if (CanReconstructJpeg(i, &why)) im[i].ok = true; else jpeg_results_[i].error = "JPEG reconstruction: " + why;
  }
  if (!prepared_) throw ParseError("PlanJpegWrite: the batch is not prepared", false);
  // ---- coefficient planes of every image in one arena; scan table and table snapshots of the images the device writes
  size_t& total_blk = w.total_blk;
  vec<JpegScanDev>& scans = w.scans;
  vec<JpegHuffDev>& tables = w.tables;
  vec<uint32_t>& resets = w.resets;
  bool& any_progressive = w.any_progressive;
  uint64_t& num_blocks = w.num_blocks;
  uint64_t& num_segs = w.num_segs;
  for (int i = 0; i < n; i++) {
    Img& m = im[i];
    if (!m.ok) continue;
    const int unit = pub_[i].first_unit;
    const ImageEntry& e = *images_[unit];
    const FramePlan& p = e.plan;
    JpegData& jd = *jpeg_data_[i];
    std::string why;
    if (!FillJpegFromFrame(p, &jd, &m.grid, &why)) { m.ok = false; jpeg_results_[i].error = why; continue; }
    // (the tables as the file's components refer to them: components that share a table slot share the table)
    for (size_t c = 0; c < jd.components.size(); c++) for (int k = 0; k < 64; k++) m.grid.qt[c][k] = jd.quant[jd.components[c].quant_idx].values[k];
    {
      // the gather's entry.  Every address of the kernel follows from it and the frame's own block grid: the component grids must lie inside the frame's, the planes
      // that are read must exist
      const JpegFrameGrid& g = m.grid;
      const FrameDev& f = frames_host_[unit];
      const uint32_t ncomp = g.ncomp;
      bool fits = (total_blk + g.nblk) < ((size_t)1 << 31) && !f.lf_only && f.coef_off && f.blk_info && f.status;
      bool walk = ncomp == 3;
      for (uint32_t c = 0; c < ncomp && fits; c++) {
        const int chn = ncomp == 1 ? 1 : (c == 0 ? 1 : c == 1 ? 0 : 2);
        fits = g.grid_w[c] && g.grid_h[c] && g.grid_w[c] <= p.bw && g.grid_h[c] <= p.bh && g.hs[c] < 8 && g.vs[c] < 8 && f.coeff[chn] && f.lfq[chn];
        if (g.hs[c] | g.vs[c]) walk = false;          // 4:4:4 colour: chroma from luma, one position per block of the frame
      }
      if (walk) fits = fits && f.ytox && f.ytob;
      if (!fits) { m.ok = false; jpeg_results_[i].error = "JPEG reconstruction: the frame's block grid does not hold the image"; continue; }
      JpegPixelImage t;
      memset(&t, 0, sizeof(t));
      for (uint32_t c = 0; c < ncomp; c++) {
        t.comp_first[c] = (uint32_t)g.comp_first[c]; t.grid_w[c] = g.grid_w[c]; t.grid_h[c] = g.grid_h[c]; t.comp_hs[c] = g.hs[c]; t.comp_vs[c] = g.vs[c];
        for (int v = 0; v < 8; v++) for (int h = 0; h < 8; h++) {
          const int nat = v * 8 + h, tr = h * 8 + v;           // (the kernel reads the ratios beside the coefficients: the planes' transposed layout)
          t.qt[c][tr] = g.qt[c][nat];
          if (c && walk) t.cfl_ratio[c - 1][tr] = g.qt[c][nat] != 0 ? (int32_t)((int64_t)2048 * g.qt[0][nat] / g.qt[c][nat]) : 0;
        }
      }
      t.npos = walk ? g.grid_w[0] * g.grid_h[0] : (uint32_t)g.nblk; t.ncomp = ncomp; t.frame = (uint32_t)unit;
      t.width = e.ih.xsize; t.height = e.ih.ysize; t.hs = ncomp == 3 ? g.hs[1] : 0; t.vs = ncomp == 3 ? g.vs[1] : 0;
      w.gather.push_back(t); w.gather_image.push_back(i);
    }
    m.first_blk = total_blk; total_blk += m.grid.nblk;
    w.images_ok++;
    if (jpeg_host_writer) continue;
    // the marker walk with an emitter that writes nothing: the scans, the tables in force at each
    vec<uint8_t> scratch;
    bool eligible = true;
    vec<JpegScanDev> mine;
    vec<uint32_t> my_resets;
    bool progressive_scans = false;
    uint64_t blocks = num_blocks, segs = num_segs;
    const size_t table0 = tables.size();
    const bool walked = WriteJpegMarkers(jd, e.ih.xsize, e.ih.ysize, [&](const JpegScanContext& cx, vec<uint8_t>*, std::string*) {
      const JpegScanInfo& s = *cx.scan;
      ScanPlan sp; sp.restart = cx.restart_interval; sp.progressive = cx.is_progressive;
      memcpy(sp.dc, cx.dc_tab, sizeof(sp.dc)); memcpy(sp.ac, cx.ac_tab, sizeof(sp.ac));
      m.plans.push_back(sp);
      // sequential scans, and with jpeg_device_progressive the four progressive kinds: extra zero runs, a progressive scan that codes DC and AC
      // together and whatever the tables below cannot express go to the host writer
      if ((cx.is_progressive && !jpeg_device_progressive) || !s.extra_zero_runs.empty() || s.num_components < 1 || s.num_components > 3) { eligible = false; return true; }
      uint32_t kind = kJpegSequential;
      if (cx.is_progressive) {
        if (s.Ss == 0 && s.Se != 0) { eligible = false; return true; }
        if (s.Ss > 0 && s.num_components != 1) { eligible = false; return true; }
        kind = s.Ss == 0 ? (s.Ah == 0 ? kJpegDcFirst : kJpegDcRefine) : (s.Ah == 0 ? kJpegAcFirst : kJpegAcRefine);
        progressive_scans = true;
      } else if (s.Ss != 0 || s.Se != 63 || s.Ah != 0 || s.Al != 0) { eligible = false; return true; }
      const bool needs_dc = kind == kJpegSequential || kind == kJpegDcFirst, needs_ac = kind == kJpegSequential || kind >= kJpegAcFirst;
      JpegScanDev d;
      memset(&d, 0, sizeof(d));
      d.kind = kind; d.ss = (uint8_t)s.Ss; d.se = (uint8_t)s.Se; d.ah = (uint8_t)s.Ah; d.al = (uint8_t)s.Al;
      uint32_t cols, rows;
      JpegScanGrid(cx, &cols, &rows);
      d.ncomp = s.num_components; d.scan_cols = cols; d.restart = cx.restart_interval;
      d.frame = (uint32_t)pub_[i].first_unit; d.image = (uint32_t)i;
      for (uint32_t k = 0; k < s.num_components; k++) {
        const JpegScanComponent& sc = s.components[k];
        for (uint32_t k2 = 0; k2 < k; k2++) if (s.components[k2].comp_idx == sc.comp_idx) eligible = false;     // (the DC predictor is kept per component)
        const JpegComponentInfo& comp = jd.components[sc.comp_idx];
        if ((needs_dc && !cx.dc_tab[sc.dc_tbl_idx & 3].init) || (needs_ac && !cx.ac_tab[sc.ac_tbl_idx & 3].init)) eligible = false;   // (the host writer names the error)
        d.h[k] = (uint8_t)(s.num_components > 1 ? comp.h_samp : 1); d.v[k] = (uint8_t)(s.num_components > 1 ? comp.v_samp : 1);
        d.plane[k] = (uint32_t)(m.first_blk + m.grid.comp_first[sc.comp_idx]); d.pitch[k] = cx.mcu_cols * comp.h_samp;
        d.dc[k] = (uint16_t)(sc.dc_tbl_idx & 3); d.ac[k] = (uint16_t)(4 + (sc.ac_tbl_idx & 3));       // (slots of this scan's snapshot: rebased below)
        d.blocks_per_mcu += (uint32_t)d.h[k] * d.v[k];
      }
      const uint64_t nb = (uint64_t)cols * rows * d.blocks_per_mcu, per_seg = d.restart ? (uint64_t)d.restart * d.blocks_per_mcu : nb;
      // a block is at most 27 + 63 x 31 + 3 x 16 + 16 bits: segments whose worst case leaves 32 bits stay on the host.  The progressive kinds stay below that: 28 bits
      // (first DC pass), 63 x 31 + 3 x 16 + 30 for the EOBn symbol (first AC pass), 63 x 17 + 3 x 16 + 30 (AC refinement: a symbol and its sign, or one correction bit)
      if (nb == 0 || per_seg * 2044 >= ((uint64_t)1 << 32)) eligible = false;
      d.first_block = (uint32_t)blocks; d.num_blocks = (uint32_t)nb;
      d.first_seg = (uint32_t)segs; d.num_segs = (uint32_t)(d.restart ? ((uint64_t)cols * rows + d.restart - 1) / d.restart : 1);
      blocks += nb; segs += d.num_segs;
      if (blocks >= ((uint64_t)1 << 31) || segs >= ((uint64_t)1 << 31) || table0 + 8 * (mine.size() + 1) > 65000) { eligible = false; return true; }
      if (kind >= kJpegAcFirst) {
        // reset points: blocks in front of which the original file ended its end-of-band run (the host writer walks them with a cursor, so they count only in order)
        d.reset_first = (uint32_t)(resets.size() + my_resets.size());
        uint64_t last = 0;
        for (size_t k = 0; k < s.reset_points.size(); k++) {
          const uint64_t rp = s.reset_points[k];
          if (k > 0 && rp <= last) { eligible = false; return true; }
          last = rp;
          if (rp < nb) my_resets.push_back((uint32_t)(d.first_block + rp));
        }
        d.reset_count = (uint32_t)(resets.size() + my_resets.size()) - d.reset_first;
      }
      // table snapshots: eight slots per scan (tables are few hundred bytes; DHT markers between scans redefine slots)
      const uint32_t base = (uint32_t)(table0 + 8 * mine.size());
      for (uint32_t k = 0; k < s.num_components; k++) { d.dc[k] = (uint16_t)(base + d.dc[k]); d.ac[k] = (uint16_t)(base + d.ac[k]); }
      mine.push_back(d);
      return true;
    }, &scratch, &why);
    if (!walked || !eligible || mine.empty() || total_blk * 64 >= ((uint64_t)1 << 37)) continue;        // host writer (it reports what the walk ran into)
    for (size_t k = 0; k < mine.size(); k++) {
      for (int t = 0; t < 8; t++) {
        const JpegHuffTable& src = t < 4 ? m.plans[k].dc[t] : m.plans[k].ac[t - 4];
        JpegHuffDev hd; memcpy(hd.depth, src.depth, 256); memcpy(hd.code, src.code, 512);
        tables.push_back(hd);
      }
    }
    m.device = true; m.progressive = progressive_scans; m.first_scan = scans.size(); m.num_scans = mine.size();
    any_progressive = any_progressive || progressive_scans;
    scans.insert(scans.end(), mine.begin(), mine.end());
    resets.insert(resets.end(), my_resets.begin(), my_resets.end());
    num_blocks = blocks; num_segs = segs;
  }
  // ---- the launch groups of the gather table
  for (size_t first = 0; first < w.gather.size(); first += kJpegPixelGroupMax) {
    JpegPixelGroup g{(uint32_t)first, (uint32_t)std::min<size_t>(kJpegPixelGroupMax, w.gather.size() - first), 0, 0, 0};
    for (uint32_t k = 0; k < g.count; k++) g.max_npos = std::max(g.max_npos, w.gather[first + k].npos);
    w.groups.push_back(g);
  }
  // ---- arena: coefficients, tables, gather table, per-block and per-segment arrays (one allocation per batch object, kept like the other arenas)
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
  w.o_coef = take(total_blk * 128); w.o_scans = take(scans.size() * sizeof(JpegScanDev)); w.o_tables = take(tables.size() * sizeof(JpegHuffDev));
  w.o_bits = take(num_blocks * 4); w.o_bitpos = take((num_blocks + 1) * 8); w.o_segbits = take(num_segs * 4); w.o_segbytes = take(num_segs * 4);
  w.o_segoff = take((num_segs + 1) * 8); w.o_tile = take((std::max(num_blocks, num_segs) / 1024 + 1) * 8); w.o_flags = take((size_t)n * 4);
  // progressive scans: per-block head / tail, flush flags, span numbers and first blocks, reset points
  const size_t nprog = any_progressive ? num_blocks : 0;
  w.o_meta = take(nprog * 4); w.o_flush = take(nprog * 4); w.o_spanidx = take(any_progressive ? (num_blocks + 1) * 8 : 0); w.o_spanfirst = take(nprog * 4);
  w.o_resets = take(resets.size() * 4);
  w.o_gather = take(w.gather.size() * sizeof(JpegPixelImage));
  w.arena_bytes = off;
  return w.images_ok;
}

// ---- phase 2: the arena, and into it the scan table, the table snapshots, the reset points and the gather table; the flags are cleared.  The host copies stay in the
// plan, so the uploads may still be on their way when this returns.  fail_refused: as in EnqueueJpegPixelTable, for frames that are not in the gather table.
void Batch::EnqueueJpegPlan(void* stream_v, bool fail_refused) {
  if (!jw_) throw ParseError("EnqueueJpegPlan without PlanJpegWrite", false);
  JpegWriteState& w = *jw_;
  hipStream_t stream = (hipStream_t)stream_v;
  const size_t n = pub_.size();
  HIP_CHECK(hipSetDevice(device_));
  DevReserve((void**)&djpeg_, &jpeg_cap_, std::max<size_t>(w.arena_bytes, 256));
  JpegPinned(8 + 4 * n);
  w.fail_refused = fail_refused;
  w.head_pending = false;
  for (size_t k = 0; k < w.gather.size(); k++) w.gather[k].coef_out = (int16_t*)(djpeg_ + w.o_coef) + w.im[(size_t)w.gather_image[k]].first_blk * 64;
  if (!w.scans.empty()) {
    HIP_CHECK(hipMemcpyAsync(djpeg_ + w.o_scans, w.scans.data(), w.scans.size() * sizeof(JpegScanDev), hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipMemcpyAsync(djpeg_ + w.o_tables, w.tables.data(), w.tables.size() * sizeof(JpegHuffDev), hipMemcpyHostToDevice, stream));
    if (!w.resets.empty()) HIP_CHECK(hipMemcpyAsync(djpeg_ + w.o_resets, w.resets.data(), w.resets.size() * 4, hipMemcpyHostToDevice, stream));
  }
  if (!w.gather.empty()) HIP_CHECK(hipMemcpyAsync(djpeg_ + w.o_gather, w.gather.data(), w.gather.size() * sizeof(JpegPixelImage), hipMemcpyHostToDevice, stream));
  HIP_CHECK(hipMemsetAsync(djpeg_ + w.o_flags, 0, n * 4, stream));
  JpegWritePlan& wp = w.wp;
  memset(&wp, 0, sizeof(wp));
  wp.frames = dframes_; wp.scans = (const JpegScanDev*)(djpeg_ + w.o_scans); wp.tables = (const JpegHuffDev*)(djpeg_ + w.o_tables); wp.coef = (const int16_t*)(djpeg_ + w.o_coef);
  wp.num_scans = (uint32_t)w.scans.size(); wp.num_blocks = (uint32_t)w.num_blocks; wp.num_segs = (uint32_t)w.num_segs;
  wp.bits = (uint32_t*)(djpeg_ + w.o_bits); wp.bitpos = (uint64_t*)(djpeg_ + w.o_bitpos); wp.seg_bits = (uint32_t*)(djpeg_ + w.o_segbits); wp.seg_bytes = (uint32_t*)(djpeg_ + w.o_segbytes);
  wp.seg_off = (uint64_t*)(djpeg_ + w.o_segoff); wp.tile_tmp = (uint64_t*)(djpeg_ + w.o_tile); wp.flags = (uint32_t*)(djpeg_ + w.o_flags);
  wp.has_spans = w.any_progressive ? 1 : 0;
  wp.meta = (uint32_t*)(djpeg_ + w.o_meta); wp.flush = (uint32_t*)(djpeg_ + w.o_flush); wp.span_idx = (uint64_t*)(djpeg_ + w.o_spanidx); wp.span_first = (uint32_t*)(djpeg_ + w.o_spanfirst);
  wp.resets = (const uint32_t*)(djpeg_ + w.o_resets);
  if (!fail_refused) return;
  // nobody consumes the coefficients of a frame that is not in the gather table: with its status word set the entropy stages skip it where they can, and what the HF
  // stage wrote for it before is zeroed behind that stage (ZeroFailedCoefKernel), like a damaged frame's
  static const uint32_t kRefused = kErrUnsupported;
  vec<uint8_t> in_table(images_.size(), 0);
  for (int i : w.gather_image) in_table[(size_t)pub_[i].first_unit] = 1;
  for (size_t u = 0; u < images_.size(); u++)
    if (!in_table[u]) HIP_CHECK(hipMemcpyAsync(dwork_ + status_off_ + u * 4, &kRefused, 4, hipMemcpyHostToDevice, stream));
}

// ---- phase 3, behind the HF stage: JpegGatherKernel, one launch per group of the table, then ZeroFailedCoefKernel for the frames it failed (kErrVarblock: consumed in
// part only).  With fail_refused every frame of the batch is either gathered or zeroed whole: the coefficient set is clean behind this.  Without it the planes stay
// marked dirty (an image may have been ineligible, a frame may fail).  Then the sizes pass of the writer.  Nothing here waits on the host.
void Batch::EnqueueJpegGather(void* stream_v) {
  if (!jw_) throw ParseError("EnqueueJpegGather without PlanJpegWrite", false);
  JpegWriteState& w = *jw_;
  const JpegPixelImage* dtable = (const JpegPixelImage*)(djpeg_ + w.o_gather);
  for (const JpegPixelGroup& g : w.groups) { LaunchJpegGatherGroup(dframes_, dtable, g, stream_v); jpeg_gather_launches_++; }
  if (!w.groups.empty()) LaunchZeroFailedCoefficients(dframes_, (int)images_.size(), stream_v);
  DebugSync("JPEG coefficients", stream_v);
  CheckLaunches("JPEG gather");
  if (w.fail_refused && any_full_vardct_) ClearCoefficientsAfterDecode(stream_v);
}
void Batch::EnqueueJpegSizes(void* stream_v) {
  if (!jw_) throw ParseError("EnqueueJpegSizes without PlanJpegWrite", false);
  LaunchJpegSizes(jw_->wp, stream_v);
  CheckLaunches("JPEG writer, sizes");
}
// The one size the device decides (bytes of all segments before stuffing) and the per-image flag words, to pinned memory behind the sizes pass — for callers that
// have a copy stream of their own (the pipeline sends them with the status words); FinishJpegWrite fetches them itself otherwise.
void Batch::EnqueueJpegHeadReadback(void* stream_v) {
  if (!jw_) throw ParseError("EnqueueJpegHeadReadback without PlanJpegWrite", false);
  JpegWriteState& w = *jw_;
  hipStream_t stream = (hipStream_t)stream_v;
  const size_t n = pub_.size();
  uint8_t* pin = JpegPinned(8 + 4 * n);
  memset(pin, 0, 8 + 4 * n);
  if (w.num_segs) {
    HIP_CHECK(hipMemcpyAsync(pin, w.wp.seg_off + w.num_segs, 8, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipMemcpyAsync(pin + 8, w.wp.flags, n * 4, hipMemcpyDeviceToHost, stream));
  }
  w.head_pending = true;
}

// ---- phase 4: with the status words of the entropy run (FinishStatus / HarvestStatus) — the raw size and the flags, the pack and stuffing pass sized from them, the
// stuffed bytes and segment records back, then per image the splice, or the host writer from that image's coefficients.  Every copy is a hipMemcpyAsync on `stream`
// into pinned staging, followed by a wait for it (CopyJpegToHost): nothing goes through the null stream, which would stall the streams of a pipeline's other jobs.
void Batch::FinishJpegWrite(void* stream_v, const vec<uint32_t>& status) {
  if (!jw_) throw ParseError("FinishJpegWrite without PlanJpegWrite", false);
  JpegWriteState& w = *jw_;
  typedef JpegWriteState::Img Img;
  hipStream_t stream = (hipStream_t)stream_v;
  const int n = (int)pub_.size();
  const uint64_t num_blocks = w.num_blocks, num_segs = w.num_segs;
  const JpegWritePlan& wp = w.wp;
  HIP_CHECK(hipSetDevice(device_));
  vec<uint32_t> flags((size_t)n, 0);
  uint64_t raw_bytes = 0;
  vec<JpegSegDev> recs;
  vec<uint8_t> stuffed_bytes;
  const uint8_t* stuffed = nullptr;
  size_t stuffed_size = 0;
  if (num_segs) {
    if (!w.head_pending) { EnqueueJpegHeadReadback(stream_v); HIP_CHECK(hipStreamSynchronize(stream)); }
    w.head_pending = false;
    memcpy(&raw_bytes, jpeg_pinned_, 8);
    memcpy(flags.data(), jpeg_pinned_ + 8, (size_t)n * 4);
    if (raw_bytes > num_blocks * 256) throw ParseError("JPEG writer: segment sizes beyond the per-block bound", false);
    // Everything pass 2 writes is sized from the raw size here, before the launch.
    const uint64_t chunks = (raw_bytes + JpegStuffChunkBytes() - 1) / JpegStuffChunkBytes();
    size_t off2 = 0;
    auto take2 = [&](size_t bytes) { const size_t o = off2; off2 += (bytes + 255) & ~(size_t)255; return o; };
    const size_t o_raw = take2(raw_bytes + 8), o_ffc = take2(chunks * 4), o_ffb = take2((chunks + 1) * 8), o_tile2 = take2((chunks / 1024 + 1) * 8);
    const size_t o_stuffed = take2(raw_bytes * 2 + 8), o_recs = take2(num_segs * sizeof(JpegSegDev));
    DevReserve((void**)&djpeg_out_, &jpeg_out_cap_, std::max<size_t>(off2, 256));
    JpegPackBuffers pb;
    pb.raw = djpeg_out_ + o_raw; pb.raw_bytes = raw_bytes; pb.ff_count = (uint32_t*)(djpeg_out_ + o_ffc); pb.ff_before = (uint64_t*)(djpeg_out_ + o_ffb);
    pb.tile_tmp = (uint64_t*)(djpeg_out_ + o_tile2); pb.stuffed = djpeg_out_ + o_stuffed; pb.stuffed_cap = raw_bytes * 2; pb.recs = (JpegSegDev*)(djpeg_out_ + o_recs);
    // (pass 1 gave the blocks of frames that failed zero bits, which keeps pass 2 off them whether or not their status words are still set)
    LaunchJpegPack(wp, pb, stream_v);
    CheckLaunches("JPEG writer, pack");
    // the stuffing count first (it sizes the copy of the bytes), then the records and the bytes
    uint64_t num_ff = 0;
    CopyJpegToHost(&num_ff, pb.ff_before + chunks, 8, stream_v);
    if (num_ff > raw_bytes) throw ParseError("JPEG writer: stuffing count beyond the buffer", false);
    recs.resize(num_segs);
    CopyJpegToHost(recs.data(), pb.recs, num_segs * sizeof(JpegSegDev), stream_v);
    stuffed_size = raw_bytes + num_ff;
    stuffed_bytes.resize(stuffed_size);
    CopyJpegToHost(stuffed_bytes.data(), pb.stuffed, stuffed_size, stream_v);
    stuffed = stuffed_bytes.data();
  }
  // ---- per image: splice (device path) or Huffman-encode on the host from its coefficients
  vec<int> host_images;
  for (int i = 0; i < n; i++) {
    Img& m = w.im[i];
    if (!m.ok) continue;
    JpegResult& r = jpeg_results_[i];
    const ImageEntry& e = *images_[pub_[i].first_unit];
    const JpegData& jd = *jpeg_data_[i];
    const int unit = pub_[i].first_unit;
    if (const uint32_t st = (size_t)unit < status.size() ? status[(size_t)unit] : 1u) { bool unsupported; r.error = DeviceStatusMessage(st, unit, &unsupported); continue; }
    std::string why;
    if (m.device && flags[i] == 0) {
      size_t scan_k = 0;
      const bool ok = WriteJpegMarkers(jd, e.ih.xsize, e.ih.ysize, [&](const JpegScanContext& cx, vec<uint8_t>* out, std::string* err) {
        if (scan_k >= m.num_scans) { if (err) *err = "JPEG writer: scan count"; return false; }
        const JpegScanDev& d = w.scans[m.first_scan + scan_k++];
        vec<JpegSegmentRecord> segs(d.num_segs);
        for (uint32_t g = 0; g < d.num_segs; g++) {
          const JpegSegDev& rec = recs[d.first_seg + g];
          if (rec.offset + rec.size > stuffed_size) { if (err) *err = "JPEG writer: segment record outside the buffer"; return false; }
          segs[g].bytes = stuffed + rec.offset; segs[g].size = rec.size; segs[g].trail_bits = (uint8_t)(rec.trail >> 8); segs[g].trail_count = (uint8_t)(rec.trail & 0xFF);
        }
        return SpliceJpegScan(cx, segs.data(), segs.size(), out, err);
      }, &r.bytes, &why);
      if (ok) { r.ok = true; jpeg_device_images_++; jpeg_device_progressive_images_ += m.progressive ? 1 : 0; } else { r.bytes.clear(); r.error = why; }
      continue;
    }
    host_images.push_back(i);
  }
  // host writer: progressive files (without "jpeg_device_progressive"), extra zero runs, "jpeg_host_writer" — and images the device flagged: the host writer
  // names their error, or writes the span whose correction bits it flushes on its own
  for (int i : host_images) {
    Img& m = w.im[i];
    JpegResult& r = jpeg_results_[i];
    const ImageEntry& e = *images_[pub_[i].first_unit];
    const JpegData& jd = *jpeg_data_[i];
    std::string why;
    vec<int16_t> host(m.grid.nblk * 64);
    CopyJpegToHost(host.data(), (const int16_t*)(djpeg_ + w.o_coef) + m.first_blk * 64, host.size() * sizeof(int16_t), stream_v);
    const int16_t* planes[3] = {host.data(), host.data() + m.grid.comp_first[1] * 64, host.data() + m.grid.comp_first[2] * 64};
    if (WriteJpeg(jd, e.ih.xsize, e.ih.ysize, planes, &r.bytes, &why)) { r.ok = true; jpeg_host_images_++; } else { r.bytes.clear(); r.error = why; }
  }
}

// The batch call: the four phases in sequence on the caller's stream, around one entropy decode of the batch, with its host waits
void Batch::ReconstructJpegs(void* stream_v) {
  const int n = (int)pub_.size();
  jpeg_results_.clear(); jpeg_results_.resize((size_t)n);
  jpeg_device_images_ = jpeg_host_images_ = jpeg_device_progressive_images_ = 0;
  jpeg_gather_launches_ = 0;
  jw_.reset();
  bool any = false;
  for (int i = 0; i < n; i++) {
    std::string why;
    if (CanReconstructJpeg(i, &why)) any = true; else jpeg_results_[i].error = "JPEG reconstruction: " + why;
  }
  if (!any) return;
  if (!prepared_) Prepare(stream_v);
  HIP_CHECK(hipSetDevice(device_));
  PlanJpegWrite();
  EnqueueJpegPlan(stream_v, /*fail_refused=*/false);
  // ---- one entropy decode of the batch (LF stage: JPEG DC, block metadata; HF stage: AC), coefficients into JPEG layout
  RunPart(stream_v, kPartFront, false);
  RunPart(stream_v, kPartHf, false);
  EnqueueJpegGather(stream_v);
  EnqueueJpegSizes(stream_v);
  vec<uint32_t> status;
  FinishStatus(stream_v, &status);         // (waits; the kernels above and below skip frames whose status word is set — it is cleared only on the host's copy)
  FinishJpegWrite(stream_v, status);
}

// ---- libjpeg-exact pixels of JPEG transcodes: the entropy run of ReconstructJpegs, then integer IDCT, libjpeg's chroma upsampling and colour conversion (jpeg_pixels.hip)
namespace {
// what of a frame's RAW table and sampling the pixel path takes ("" = all of it); only meaningful once HfGlobal has been parsed
std::string JpegPixelTableRefusal(const FramePlan& p) {
  const QuantTableSpec& q = p.qspec[0];
  if (q.mode != 7 || q.raw[0].size() != 64 || q.raw[1].size() != 64 || q.raw[2].size() != 64) return "a frame without a RAW (JPEG) quantisation table";
  return std::string();
}
}  // namespace

bool Batch::CanDecodeJpegPixels(int i, std::string* why) const { return CanDecodeJpegPixelsAs(i, images_[pub_[i].first_unit]->out, why); }
// ... with the output given: SetOutput asks before it takes a spec with jpeg_scale.
// The write stage of a Run relies on this list for such an output (FillFrameCommon sets FrameDev::img_w / img_h to the scaled picture): without gaborish, EPF,
// upsampling, extra channels and image features a frame reaches the caller's buffer through OutputKernel alone, which is bounded by img_w x img_h.  The fused filter
// kernels, the EPF kernels that write, the Modular write and the frame tail are bounded by the frame's own size — whoever lets such a frame in here must bound those too.
bool Batch::CanDecodeJpegPixelsAs(int i, const OutputSpec& out, std::string* why) const {
  const std::string refusal = JpegPixelsRefusalOf(pub_[i].num_units, pub_[i].complex, *images_[pub_[i].first_unit], out);
  if (why && !refusal.empty()) *why = refusal;
  return refusal.empty();
}
// ("" = taken) over an image as it was parsed, in a batch or not yet (AddImagesImpl)
static std::string JpegPixelsRefusalOf(int num_units, bool complex, const ImageEntry& e, const OutputSpec& out) {
  auto no = [&](const std::string& m) { return "unsupported: libjpeg-exact decode of " + m; };
  const FramePlan& p = e.plan;
  if (!IsPlainJpegFrameOf(num_units, complex, e)) return no("an image that is not a plain JPEG-transcoded frame");
  if (complex || p.have_crop || p.frame_type != 0 || (p.flags & (1 | 2 | 16))) return no("a frame with patches, splines, noise, a crop or blending");
  if (p.use_lf_frame || e.lf_source) return no("a frame that takes its LF image from an LF frame");
  if (p.lf.gab || p.lf.epf_iters) return no("a frame with restoration filters");
  // Y at full resolution, both chroma channels with the same shifts: 4:4:4, 4:2:2, 4:2:0 (4:4:0 and the rest: libjpeg has rules for them that no test here could pin)
  if (p.hs[1] || p.vs[1] || p.hs[0] != p.hs[2] || p.vs[0] != p.vs[2] || p.hs[0] > 1 || p.vs[0] > 1 || (p.vs[0] && !p.hs[0]))
    return no("chroma sampling other than 4:4:4, 4:2:2 and 4:2:0");
  if (out.downscale != 1) return no("an output with downscale 8 (libjpeg's scaled IDCTs are other arithmetic)");
  if (e.ih.xsize > 65535 || e.ih.ysize > 65535) return no("an image larger than a JPEG file can be");
  if (!(p.single_section && p.ac_code.empty())) {      // (HfGlobal of a one-group frame is parsed by Prepare)
    const std::string t = JpegPixelTableRefusal(p);
    if (!t.empty()) return no(t);
  }
  return std::string();
}
// libjpeg's 1/8 decode from the DC terms alone (decoder.h JpegDcOnly), for an image JpegPixelsRefusalOf takes: jdmaster.c gives every component the 1 x 1 IDCT unless
// both of its dimensions still need upsampling by two — 4:2:0 chroma ((hs, vs) == (1, 1): the 2 x 2 form, three AC terms per block)
static bool JpegDcEligibleOf(const FramePlan& p, const OutputSpec& out) { return out.jpeg_scale == 8 && out.downscale == 1 && !p.modular && !(p.hs[0] == 1 && p.vs[0] == 1); }

// ---- host plan (after Prepare): which images take the path, their component grids, the image table and the launch groups over it
size_t Batch::PlanJpegPixels() {
  const int n = (int)pub_.size();
  jpeg_pixel_results_.clear(); jpeg_pixel_results_.resize((size_t)n);
  jpeg_pixel_images_ = jpeg_pixel_launches_ = jpeg_dc_only_images_ = 0;
  jpeg_pixel_table_.clear(); jpeg_pixel_table_image_.clear(); jpeg_pixel_groups_.clear();
  if (!prepared_) throw ParseError("PlanJpegPixels: the batch is not prepared", false);
  // entries of scale 1 first, the scaled ones (OutputSpec::jpeg_scale) behind them, the DC-only ones (JpegDcOnly) last: the three kinds take different kernels and never
  // share a launch group
  vec<JpegPixelImage>& table = jpeg_pixel_table_;
  vec<JpegPixelImage> scaled_table, dc_table;
  vec<int> scaled_image, dc_image;
  for (int i = 0; i < n; i++) {
    std::string why;
    if (!CanDecodeJpegPixels(i, &why)) { jpeg_pixel_results_[i].error = why; continue; }
    const int u = pub_[i].first_unit;
    const ImageEntry& e = *images_[u];
    const FramePlan& p = e.plan;
    why = JpegPixelTableRefusal(p);
    if (!why.empty()) { jpeg_pixel_results_[i].error = "unsupported: libjpeg-exact decode of " + why; continue; }
    const uint32_t ncomp = e.ih.color_space == 1 ? 1 : 3;
    JpegFrameGrid g;
    if (!JpegGridFromFrame(p, ncomp, "libjpeg-exact decode", &g, &why)) { jpeg_pixel_results_[i].error = why; continue; }
    const FrameDev& f = frames_host_[u];
    // a DC-only image (Prepare gave its frame neither coefficient nor pixel planes: FrameDev::lf_only) is written by JpegDcOutKernel from lfq and block info alone
    const bool dc = JpegDcOnlyUnit(u);
    // every address of the kernels follows from this entry and the frame's own block grid: the component grids must hold the components' real extents and lie inside
    // the frame's grid, the planes that are read and written must exist
    bool fits = g.nblk < ((size_t)1 << 31) && f.blk_info && f.status;
    if (dc) fits = fits && f.lf_only == kLfOnlyJpegDc && !(ncomp == 3 && g.vs[1]);
    else fits = fits && f.plane_a[0] && f.plane_a[1] && f.plane_a[2] && !f.lf_only && f.coef_off;
    for (uint32_t c = 0; c < ncomp && fits; c++) {
      const int chn = ncomp == 1 ? 1 : (c == 0 ? 1 : c == 1 ? 0 : 2);
      const uint32_t cw = (e.ih.xsize + (1u << g.hs[c]) - 1) >> g.hs[c], ch = (e.ih.ysize + (1u << g.vs[c]) - 1) >> g.vs[c];
      fits = g.grid_w[c] && g.grid_h[c] && (uint64_t)g.grid_w[c] * 8 >= cw && (uint64_t)g.grid_h[c] * 8 >= ch && g.grid_w[c] <= p.bw && g.grid_h[c] <= p.bh && (dc || f.coeff[chn]) && f.lfq[chn];
    }
    const bool walk = ncomp == 3 && !g.hs[1] && !g.vs[1];      // 4:4:4 colour: chroma from luma, one position per block of the frame
    if (walk && !dc) fits = fits && f.ytox && f.ytob;
    if (!fits) { jpeg_pixel_results_[i].error = "unsupported: libjpeg-exact decode of a frame whose block grid does not hold the image"; continue; }
    JpegPixelImage t;
    memset(&t, 0, sizeof(t));
    for (uint32_t c = 0; c < ncomp; c++) {
      t.plane[c] = (uint8_t*)f.plane_a[ncomp == 1 ? 1 : (c == 0 ? 1 : c == 1 ? 0 : 2)];     // (the frame's own pixel planes, which this decode does not use otherwise: bw x bh x 64 floats each; DC-only: none)
      t.comp_first[c] = (uint32_t)g.comp_first[c]; t.grid_w[c] = g.grid_w[c]; t.grid_h[c] = g.grid_h[c];
      for (int v = 0; v < 8; v++) for (int h = 0; h < 8; h++) {
        const int nat = v * 8 + h, tr = h * 8 + v;           // (the kernel reads the tables beside the coefficients: the planes' transposed layout)
        t.qt[c][tr] = g.qt[c][nat];
        if (c && walk) t.cfl_ratio[c - 1][tr] = g.qt[c][nat] > 0 ? (int32_t)((int64_t)2048 * g.qt[0][nat] / g.qt[c][nat]) : 0;
      }
    }
    t.npos = walk ? g.grid_w[0] * g.grid_h[0] : (uint32_t)g.nblk; t.ncomp = ncomp; t.frame = (uint32_t)u;
    t.width = e.ih.xsize; t.height = e.ih.ysize; t.hs = ncomp == 3 ? g.hs[1] : 0; t.vs = ncomp == 3 ? g.vs[1] : 0;
    t.scale = e.out.jpeg_scale;
    // what of the image is decoded: all of it, or (jpeg_region, an image with a region — the groups of FrameDev::hf_list, which Prepare made from the same rectangle) the
    // blocks of the region's groups and the pixels of the crop.  Component block (bx, by) is frame block (bx << hs, by << vs) and a group is 32 x 32 frame blocks, so the
    // component's share of the group rectangle is [32 gx0 >> hs, 32 gx1 >> hs) x [32 gy0 >> vs, 32 gy1 >> vs), cut to its grid.
    const bool by_region = JpegRegionUnit(u) && f.hf_list;
    for (uint32_t c = 0; c < ncomp; c++) { t.reg_x0[c] = t.reg_y0[c] = 0; t.reg_w[c] = g.grid_w[c]; t.reg_h[c] = g.grid_h[c]; }
    t.rect_x0 = t.rect_y0 = 0; t.rect_w = (t.width + t.scale - 1) / t.scale; t.rect_h = (t.height + t.scale - 1) / t.scale;
    if (by_region) {
      bool ok = e.region_rect[2] && e.region_rect[3] && e.region_rect[0] < t.rect_w && e.region_rect[2] <= t.rect_w - e.region_rect[0] && e.region_rect[1] < t.rect_h &&
                e.region_rect[3] <= t.rect_h - e.region_rect[1];
      uint32_t npos = 0;
      for (uint32_t c = 0; c < ncomp && ok; c++) {
        const uint32_t x0 = (e.region_groups[0] * 32) >> g.hs[c], x1 = std::min((e.region_groups[2] * 32) >> g.hs[c], g.grid_w[c]);
        const uint32_t y0 = (e.region_groups[1] * 32) >> g.vs[c], y1 = std::min((e.region_groups[3] * 32) >> g.vs[c], g.grid_h[c]);
        ok = x0 < x1 && y0 < y1;
        if (!ok) break;
        t.reg_x0[c] = x0; t.reg_y0[c] = y0; t.reg_w[c] = x1 - x0; t.reg_h[c] = y1 - y0;
        t.comp_first[c] = npos; npos += t.reg_w[c] * t.reg_h[c];
      }
      if (!ok) { jpeg_pixel_results_[i].error = "unsupported: libjpeg-exact decode of a frame whose block grid does not hold the image"; continue; }
      t.npos = walk ? t.reg_w[0] * t.reg_h[0] : npos;      // (the region's positions only)
      t.rect_x0 = e.region_rect[0]; t.rect_y0 = e.region_rect[1]; t.rect_w = e.region_rect[2]; t.rect_h = e.region_rect[3];
    }
    if (t.scale == 1) { table.push_back(t); jpeg_pixel_table_image_.push_back(i); continue; }
    // libjpeg's scaled decode (jdmaster.c): the smallest IDCT is m = 8 / scale; a component whose sampling factors are below the largest takes twice that as long as
    // both of its dimensions still need upsampling by a factor of two — 4:2:0 chroma does, once (n = 2 m: it then has the picture's extent), 4:2:2 chroma does not
    // (its height has the picture's already).  hmax / h_c = 1 << hs and vmax / v_c = 1 << vs for chroma, 1 for luma.
    const uint32_t m = 8 / t.scale;
    t.out_w = (t.width + t.scale - 1) / t.scale; t.out_h = (t.height + t.scale - 1) / t.scale;
    for (uint32_t c = 0; c < ncomp; c++) {
      const uint32_t rh = c ? 1u << t.hs : 1u, rv = c ? 1u << t.vs : 1u;      // hmax / h_c, vmax / v_c
      uint32_t nn = m;
      while (nn < 8 && (rh * m) % (nn * 2) == 0 && (rv * m) % (nn * 2) == 0) nn *= 2;
      t.n[c] = nn; t.pitch[c] = g.grid_w[c] * nn;
      t.ext_w[c] = (uint32_t)(((uint64_t)t.width * nn + (uint64_t)rh * 8 - 1) / ((uint64_t)rh * 8));
      t.ext_h[c] = (uint32_t)(((uint64_t)t.height * nn + (uint64_t)rv * 8 - 1) / ((uint64_t)rv * 8));
    }
    // (the grids hold the full-size extents — `fits` above —, so grid x n holds these; a plane of grid_w x n by grid_h x n bytes lies inside the frame's float plane)
    t.chroma_up = ncomp == 3 && t.hs && !t.vs ? 1u : 0u;      // 4:2:2: ext_w = ceil(out_w / 2), all of the picture's height
    t.chroma_fancy = m > 1 ? 1u : 0u;                         // (jdsample.c: no fancy upsampling when the smallest IDCT is 1 x 1)
    if (dc) {
      // (what JpegDcOutKernel relies on: one sample per block for every component, chroma as tall as the picture and never interpolated)
      if (t.scale != 8 || t.n[0] != 1 || (ncomp == 3 && (t.n[1] != 1 || t.n[2] != 1 || t.vs || t.chroma_fancy)) || t.out_w > p.bw || t.out_h > p.bh) {
        jpeg_pixel_results_[i].error = "unsupported: libjpeg-exact decode of a frame whose block grid does not hold the image";
        continue;
      }
      dc_table.push_back(t); dc_image.push_back(i);
      continue;
    }
    scaled_table.push_back(t); scaled_image.push_back(i);
  }
  const size_t plain = table.size(), general = plain + scaled_table.size();
  table.insert(table.end(), scaled_table.begin(), scaled_table.end());
  table.insert(table.end(), dc_table.begin(), dc_table.end());
  jpeg_pixel_table_image_.insert(jpeg_pixel_table_image_.end(), scaled_image.begin(), scaled_image.end());
  jpeg_pixel_table_image_.insert(jpeg_pixel_table_image_.end(), dc_image.begin(), dc_image.end());
  auto group_runs = [&](size_t from, size_t to, uint32_t scaled) {
    for (size_t first = from; first < to; first += kJpegPixelGroupMax) {
      JpegPixelGroup g{(uint32_t)first, (uint32_t)std::min<size_t>(kJpegPixelGroupMax, to - first), 0, 0, 0};
      g.scaled = scaled;
      for (uint32_t k = 0; k < g.count; k++) {
        const JpegPixelImage& t = table[first + k];
        g.max_npos = std::max(g.max_npos, t.npos);
        // (the colour launch is sized by the rectangle it writes, JpegPixelImage::rect_*: threads take pixel pairs (2 t, 2 t + 1) from pair rect_x0 >> 1 on)
        g.max_w = std::max(g.max_w, 2 * (((t.rect_x0 + t.rect_w + 1) >> 1) - (t.rect_x0 >> 1))); g.max_h = std::max(g.max_h, t.rect_h);
      }
      jpeg_pixel_groups_.push_back(g);
    }
  };
  group_runs(0, plain, 0);
  group_runs(plain, general, 1);
  group_runs(general, table.size(), kJpegGroupDc);
  // the groups of the frames that take this decode's HF stage (RunPart kPartJpegHf), and how many of them it decodes
  hf_by_region_ = jpeg_region;      // (StageBytes: the plan of a libjpeg-exact decode — a pipeline asks for the bytes of the job it has prepared, before any stage runs)
  hf_groups_total_ = hf_groups_decoded_ = 0;
  for (size_t u = 0; u < images_.size(); u++) {
    const FramePlan& p = images_[u]->plan;
    if (p.modular || EndsBehindLf((int)u)) continue;
    hf_groups_total_ += p.num_groups;
    hf_groups_decoded_ += jpeg_region && frames_host_[u].hf_list ? frames_host_[u].hf_count : p.num_groups;
  }
  return table.size();
}

// The table goes into a buffer of its own (not the constant arena: Prepare's layout does not know about this decode).  The host copy stays in the batch until the
// next plan, so the copy may still be on its way when this returns.
void Batch::EnqueueJpegPixelTable(void* stream_v, bool fail_refused) {
  hipStream_t stream = (hipStream_t)stream_v;
  HIP_CHECK(hipSetDevice(device_));
  if (!jpeg_pixel_table_.empty()) {
    const size_t bytes = jpeg_pixel_table_.size() * sizeof(JpegPixelImage);
    DevReserve((void**)&djpeg_table_, &jpeg_table_cap_, std::max<size_t>(bytes, 256));
    HIP_CHECK(hipMemcpyAsync(djpeg_table_, jpeg_pixel_table_.data(), bytes, hipMemcpyHostToDevice, stream));
  }
  if (!fail_refused) return;
  // nobody consumes the coefficients of a frame that is not in the table: with its status word set the entropy stages skip it where they can, and what the HF stage
  // wrote for it before is zeroed behind that stage (ZeroFailedCoefKernel), like a damaged frame's
  static const uint32_t kRefused = kErrUnsupported;
  vec<uint8_t> in_table(images_.size(), 0);
  for (int i : jpeg_pixel_table_image_) in_table[(size_t)pub_[i].first_unit] = 1;
  for (size_t u = 0; u < images_.size(); u++)
    if (!in_table[u]) HIP_CHECK(hipMemcpyAsync(dwork_ + status_off_ + u * 4, &kRefused, 4, hipMemcpyHostToDevice, stream));
}

void Batch::EnqueueJpegIdct(void* stream_v) {
  const JpegPixelImage* dtable = (const JpegPixelImage*)djpeg_table_;
  // (a DC-only group has no coefficients to transform: a job of such groups only launches nothing here)
  bool any = false;
  for (const JpegPixelGroup& g : jpeg_pixel_groups_) if (g.scaled != kJpegGroupDc) { LaunchJpegIdctGroup(dframes_, dtable, g, stream_v); jpeg_pixel_launches_++; any = true; }
  // (a frame the kernel failed — kErrVarblock — has been consumed in part only: its planes are zeroed whole, as behind the HF stage)
  if (any) LaunchZeroFailedCoefficients(dframes_, (int)images_.size(), stream_v);
}
void Batch::EnqueueJpegColorOut(void* stream_v) {
  const JpegPixelImage* dtable = (const JpegPixelImage*)djpeg_table_;
  for (const JpegPixelGroup& g : jpeg_pixel_groups_) { LaunchJpegColorOutGroup(dframes_, dtable, g, stream_v); jpeg_pixel_launches_++; }
}

// what a status word means for an image of this path: kErrVarblock is set by JpegIdctPlanesKernel itself
static std::string JpegPixelStatusMessage(uint32_t st, int frame) {
  if (st & kErrVarblock) return "corrupt stream: a JPEG-transcoded frame with a transform other than DCT8 (device status " + std::to_string(st) + ", frame " + std::to_string(frame) + ")";
  bool unsupported;
  return DeviceStatusMessage(st, frame, &unsupported);
}
void Batch::HarvestJpegPixels(const vec<uint32_t>& status) {
  jpeg_pixel_images_ = jpeg_dc_only_images_ = 0;
  for (size_t k = 0; k < jpeg_pixel_table_image_.size(); k++) {
    const int i = jpeg_pixel_table_image_[k];
    JpegPixelResult& r = jpeg_pixel_results_[i];
    const int u = pub_[i].first_unit;
    if (const uint32_t st = (size_t)u < status.size() ? status[(size_t)u] : 1u) { r.error = JpegPixelStatusMessage(st, u); continue; }
    r.ok = true; jpeg_pixel_images_++;
    if (JpegDcOnlyUnit(u)) jpeg_dc_only_images_++;
  }
}

// The batch call: plan, one entropy decode of the batch, the pixel kernels, harvest — with a host wait at the end
void Batch::DecodeJpegPixels(void* stream_v) {
  const int n = (int)pub_.size();
  jpeg_pixel_results_.clear(); jpeg_pixel_results_.resize((size_t)n);
  jpeg_pixel_images_ = jpeg_pixel_launches_ = jpeg_dc_only_images_ = 0;
  jpeg_pixel_table_.clear(); jpeg_pixel_table_image_.clear(); jpeg_pixel_groups_.clear();
  if (!n) throw ParseError("DecodeJpegPixels: the batch holds no image", false);
  bool any = false;
  for (int i = 0; i < n; i++) {
    std::string why;
    if (CanDecodeJpegPixels(i, &why)) any = true; else jpeg_pixel_results_[i].error = why;
  }
  if (!any) return;
  if (!prepared_) Prepare(stream_v);
  HIP_CHECK(hipSetDevice(device_));
  if (!PlanJpegPixels()) return;
  EnqueueJpegPixelTable(stream_v, /*fail_refused=*/false);
  // ---- one entropy decode of the batch (LF stage: JPEG DC, block metadata; HF stage: AC)
  RunPart(stream_v, kPartFront, false);
  RunPart(stream_v, kPartJpegHf, false);
  // ---- the pixel half: one launch per kernel and group of the table, then the resizes of resized outputs over the f32 pictures the write stage left
  RunPart(stream_v, kPartJpegIdct, false);
  RunPart(stream_v, kPartJpegPixels, false);
  vec<uint32_t> status;
  FinishStatus(stream_v, &status);          // (a frame that failed leaves the set marked dirty)
  // frames outside the table went through the HF stage too, and nobody consumed their coefficients
  if (jpeg_pixel_table_.size() != images_.size()) CoefDirty() = true;
  HarvestJpegPixels(status);
}

void Batch::CopyOutputSlotToHost(int i, int slot, void* dst, size_t size, void* stream_v) {
  const ImageEntry& e = *images_[pub_[i].first_unit];
  if (slot < 0 || (size_t)slot >= e.deliver_frames.size() || e.out.device_ptr) throw ParseError("CopyOutputSlotToHost: no such slot", false);
  HIP_CHECK(hipMemcpyAsync(dst, dwork_ + e.off_out + (size_t)slot * (e.out_size + 64), std::min(size, e.out_size), hipMemcpyDeviceToHost, (hipStream_t)stream_v));
  HIP_CHECK(hipStreamSynchronize((hipStream_t)stream_v));
}
void Batch::CopyOutputToHost(int i, void* dst, size_t size, void* stream_v) {
  const ImageEntry& e = *images_[pub_[i].first_unit];
  HIP_CHECK(hipMemcpyAsync(dst, device_output(i), std::min(size, e.out_size), hipMemcpyDeviceToHost, (hipStream_t)stream_v));
  HIP_CHECK(hipStreamSynchronize((hipStream_t)stream_v));
}
void Batch::CopyOutputRangeToHost(int i, size_t offset, void* dst, size_t size, void* stream_v) {
  const ImageEntry& e = *images_[pub_[i].first_unit];
  if (offset > e.out_size || size > e.out_size - offset) throw ParseError("CopyOutputRangeToHost: the range leaves the output", false);
  HIP_CHECK(hipMemcpyAsync(dst, (const uint8_t*)device_output(i) + offset, size, hipMemcpyDeviceToHost, (hipStream_t)stream_v));
  HIP_CHECK(hipStreamSynchronize((hipStream_t)stream_v));
}

}  // namespace jxlhip
