// jxl-hip: device-side frame descriptor + kernel launch interface (implemented in kernels.hip).
#pragma once
#include "jxl_dev.h"
#include "lf_group_plan.h"
#if !defined(__HIPCC__)
// host-only builds of the library's host sources (the sanitizer build, tests/test_sanitizers.py): the runtime API and the vector types, no device code
#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>
#endif

namespace jxlhip {

// One channel of a Modular frame's global image as the sub-streams see it (after the global transforms' MetaApply):
// plane location in the work arena, dimensions and the squeeze shifts that decide which section carries it.
struct ModChanDev { uint64_t off; uint32_t w, h; int32_t hshift, vshift; };

// Per-pass tables of a VarDCT frame (HfPass in the codestream): entropy code, coefficient orders, left shift of the values.
struct PassDev { DevCode code; const uint16_t* orders[39]; uint32_t shift; uint32_t pad; };

// One per frame of a batch; array lives in device memory.  All pointers are device pointers.
// A Modular sub-stream that carries its own MA tree and entropy code (GroupHeader.use_global_tree = 0, parsed on the host for
// Modular frames, where every section starts with its stream).
struct ModLocalDev { const TreeNode* tree; uint32_t tree_nodes, uses_wp, max_prop, pad; uint64_t data_bitpos; DevCode code; };

// Where and how the write stage puts an image's pixels (pixel_ops.h StorePixel), filled by decoder.cc FillOutput; the image size travels beside it.
struct OutputDesc {
  uint8_t* out;
  uint64_t out_stride;            // bytes per row
  uint32_t out_channels, out_type /*0 u8 1 u16 2 f32 3 f16*/, out_big_endian;
  float out_int_mul;              // integer output: sample = round(clamp(v, 0, 1) x this) — 255 / 65535, or 2^bits - 1 (JxlDecoderSetImageOutBitDepth)
  uint32_t out_orient;            // 1..8: orientation applied while writing (1 = none)
  uint32_t is_gray;               // grey image: one- and two-channel output takes R (= G = B), of a colour image G
  // OutputSpec's layout: planar = channel slot c (grey or G, alpha / R, G, B, alpha) is a plane of its own at out + c x plane_stride, out_stride the row pitch of one plane;
  // affine = float samples are stored as fmaf(v, scale[c], bias[c]).  Both 0: interleaved samples as they are, no multiply anywhere.
  uint32_t planar, affine;
  uint64_t plane_stride;          // bytes from one plane to the next (planar)
  float scale[4], bias[4];        // per slot (affine)
};

struct FrameDev {
  // geometry
  uint32_t width, height, bw, bh, xgroups, ygroups, num_groups, xlfgroups, num_lf_groups, cw, ch;
  uint32_t group_dim, is_modular, plane_stride, plane_rows;
  // codestream + sections (byte offsets); for single-section frames the *_bitpos fields are used instead
  const uint8_t* cs;
  uint64_t cs_size;
  const uint64_t* sec_off;
  const uint64_t* sec_size;
  uint32_t single_section;
  uint64_t lf_start_bitpos;      // single-section: where LfGroup starts
  uint64_t hf_start_bitpos;      // single-section: where PassGroup starts
  uint64_t* stream_end_bitpos;   // [0] = end of LfGroup stream (single-section), [1] = end of global modular stream
  // entropy codes / tree
  const TreeNode* tree;
  uint32_t tree_nodes;
  DevCode mod_code;
  uint32_t uses_wp;
  WPHeader gwp;
  // chroma subsampling (YCbCr JPEG transcodes): channel c lives on a grid of (bw >> hs[c]) x (bh >> vs[c]) blocks, packed into the
  // top-left corner of the frame-sized LF / pixel planes; coefficients keep the offsets of the full-resolution block a cell starts at
  uint32_t hs[3], vs[3], subsampled;
  uint32_t tree_max_prop;         // largest property index in any MA tree of the frame (>= 16: previous-channel properties)
  const ModLocalDev* mod_local;   // Modular sub-streams with a tree and code of their own, indexed 0 = global stream, 1 + unit = LfGroup /
                                  // PassGroup unit (entries with tree == nullptr use the frame's tree); nullptr: none in this frame
  const ModLocalDev* lf_local;    // VarDCT frames whose LfGroup sub-streams bring trees / codes of their own (LfDecodeLocalKernel): [3 g + k], k = 0 LF coefficients,
                                  // 1 ModularLfGroup, 2 HF metadata (tree == nullptr: the global tree); nullptr: the frame takes the global-tree LF kernels
  uint32_t lf_lz77;               // some LfGroup sub-stream of the frame is LZ77-coded (lz_window holds a window per LF group from lz_lf_base on)
  DevCode ac_code;
  const uint16_t* orders[39];
  const BlockCtxDev* bcm;
  uint32_t num_hf_presets, preset_bits;
  uint32_t num_passes;            // progressive passes: PassGroup section (p, g) adds value << passes[p].shift to the coefficients
  const PassDev* passes;          // [num_passes]; ac_code / orders above are pass 0's
  // dequant
  float lf_fac[3], cfl_lf_x, cfl_lf_b;
  float inv_global_scale, x_dm, b_dm, quant_bias[4], color_scale, base_x, base_b;
  const float* qtable[17 * 3];
  uint32_t skip_lf_smoothing;
  // loop filter + colour
  uint32_t gab, epf_iters;
  float gab_w[9];                 // per channel: n0, n1, n2 (normalised)
  float epf_sharp_lut[8], epf_channel_scale[3], epf_quant_mul, epf_quant_scale;
  float epf_sm[3], epf_bsm[3];    // per pass sad multipliers (normal, border)
  float opsin_inv[9], neg_bias[3], neg_bias_cbrt[3];
  uint32_t color_mode;            // 0: XYB->sRGB, 1: XYB->linear, 2: YCbCr->RGB, 3: none (RGB as is), 4: XYB->gamma (FastPowf), 5: XYB->Rec.709, 6: XYB->PQ, 7: XYB->HLG
  // VarDCT buffers
  int32_t* lfq[3];
  float* lf[3];
  float* lf_tmp[3];
  float* llf[3];
  uint32_t* blk_info;
  uint32_t* coef_off;
  uint2* vb_list;                 // per group: up to 1024 {strategy | log2 cx << 5 | log2 cx cy << 8 | order bucket << 12 | x << 16 | y << 21 | block-context bucket << 26, coefficient offset}
  uint32_t* vb_count;             // per group: number of varblocks
  int8_t* ytox; int8_t* ytob;
  int32_t* coeff[3];
  float* plane_a[3];
  float* plane_b[3];
  float* inv_sigma;
  int32_t* lf_scratch;            // per LF group scratch (HF metadata channels)
  uint64_t lf_scratch_stride;     // ints per LF group
  int32_t* wp_scratch;            // per stream WP state
  uint64_t wp_scratch_stride;
  // modular buffers
  const ModChanDev* mod_chan;     // channel table of the global image *before* undoing global transforms (meta channels first)
  uint8_t* mod_base;              // work arena base the table's offsets refer to
  uint32_t mod_nchan;
  uint32_t mod_nb_meta;
  uint32_t mod_global_decodable;
  uint64_t mod_global_bitpos;
  int32_t* mod_group_scratch;     // per group scratch
  uint64_t mod_group_scratch_stride;
  uint32_t mod_bits;
  int32_t* mod_wp_scratch;        // weighted-predictor state of the Modular sub-streams: global, then one per LfGroup / PassGroup unit
  uint64_t mod_wp_stride;
  uint64_t* hf_end_bitpos;        // VarDCT frames with extra channels: where the HF coefficient stream of PassGroup (mod_pass + k, g) ended, at [k * num_groups + g] (its Modular part starts there)
  const int32_t* alpha_plane;     // VarDCT frames: decoded alpha extra channel (image-sized), or null
  float alpha_factor;             // 1 / (2^bits - 1)
  OutputDesc od;                  // output
  // upsampling (frame coded at 1/upsampling of the image size): width/height above are the CODED size
  uint32_t upsampling, img_w, img_h;   // img_*: image size the write stage covers (= width/height when upsampling == 1)
  const float* up_weights;        // 15 / 55 / 210 coefficients of the symmetric (5N x 5N) kernel matrix, N = upsampling / 2
  float* up_plane[4];             // upsampled X, Y, B (and alpha as float) planes, img_w x img_h
  uint32_t mod_cfg_uniform;       // the hybrid-integer configuration shared by every cluster of mod_code, or 0xFFFFFFFF
  uint4* place_rec;               // varblock placement records (one per varblock, grouped per band: BandRecordBase), bw x bh entries
  uint32_t* place_cnt;            // [LF group * 8 + band] records of the band
  uint32_t* band_start;           // [LF group * 8 + band] index of the band's first entry in the LF group's strategy list (0xFFFFFFFF: damaged)
  uint32_t mod_unit_passes;       // Modular sub-streams per group: the frame's passes (Modular frames); VarDCT frames: the passes mod_pass, mod_pass + 1, ... that carry extra
  uint32_t mod_pass;              // channels — one, unless squeezed extra channels are spread over several passes (FramePlan::mod_passes)
  int32_t pass_min_shift[11], pass_max_shift[11];   // passes.h GetDownsamplingBracket per pass: the channels (by min(hshift, vshift)) a PassGroup of that pass carries
  uint32_t lz_lf_base;            // LZ77-coded LF-group streams of a VarDCT frame: index of LF group 0's window in lz_window (the Modular units' windows come first)
  uint32_t use_lf_frame;          // frame_header.cc kUseDcFrame: no LF coefficients in the LfGroups, the LF image is an LF frame's samples (no dequantisation, no smoothing, LF context 0)
  uint32_t lf_simt;               // the LF-group streams of this frame are decoded by LfDecodeSimtKernel (one stream per lane), placement by LfPlaceKernel
  uint32_t* status;
  uint32_t* frame_flags;          // [0] != 0: some varblock is not contained in a 64x64 tile (generic IDCT path)
  uint32_t* hf_written;           // running count of non-zero AC coefficients the HF stage wrote for this frame (bench accounting)
  uint32_t* lz_ac_window;         // LZ77-coded AC streams: kAcLzWindow entries per group stream (reused pass after pass); null otherwise
  uint32_t* lz_window;            // LZ77-coded Modular streams: 2^20-entry windows, one per stream (global, then LfGroup / PassGroup units)
  uint32_t post_mode;             // 1: the frame ends in its float planes (after the restoration filters); upsampling, colour transform and the
                                  // write stage are done by the host-planned frame tail (kernels_features.hip) — multi-frame images, image features
  float inverse_gamma;            // colour mode 4 (XYB -> gamma transfer)
  float hdr_par[5];               // colour mode 6 (PQ): [0] intensity_target / 10000; 7 (HLG): [0] OOTF exponent, [1] apply it, [2..4] luminances
  uint32_t lf_only;               // != 0: the decode of this frame ends behind the LF stage — the HF stage, the IDCT, the filters and OutputKernel leave the frame alone, it has no
                                  // coefficient or pixel planes.  kLfOnlyEighth: the 1:8 decode (OutputSpec::downscale == 8), the output is the LF image, one pixel per 8x8 block,
                                  // written by LfOutputKernel — img_w / img_h / out_stride describe that bw x bh picture.  kLfOnlyJpegDc: libjpeg's 1/8 decode of a JPEG transcode
                                  // whose components all take the 1 x 1 IDCT (OutputSpec::jpeg_scale == 8, not 4:2:0): JpegDcOutKernel writes it from lfq, the DC terms
  const uint32_t* hf_list;        // libjpeg-exact decode of a crop (Batch::JpegRegion): the hf_count groups its region holds, raster order, each < num_groups (the host asserts it);
  uint32_t hf_count;              // honoured by the HF launches of that decode alone (LaunchCfg::hf_by_list) — stream slot k decodes group hf_list[k].  nullptr: every group
};
constexpr uint32_t kLfOnlyEighth = 1, kLfOnlyJpegDc = 2;

struct LaunchCfg {
  int lane_stride_lf = 64;   // lanes between active decode threads (64 = one stream per wave, 1 = one per lane)
  int lane_stride_hf = 64;
  int lane_stride_mod = 64;
  int any_wp = 0;            // some MA tree of the batch uses the weighted predictor (the Modular kernels then reserve LDS for its state)
  int any_subsampled = 0;    // some frame is chroma-subsampled (its own IDCT kernel; the SIMT HF kernel only)
  int any_multipass = 0;     // some frame has progressive passes (the general instantiation of the SIMT HF kernel)
  int any_prefix_ac = 0;     // some VarDCT frame's AC code is a prefix code or LZ77-coded (HfDecodeKernel beside the SIMT kernel)
  int any_local_trees = 0;   // some Modular sub-stream carries its own MA tree / code (second launch of the group kernel)
  int any_local_lf = 0;      // some VarDCT frame's LfGroup sub-streams carry their own trees / codes (LfDecodeLocalKernel)
  // filled by Batch::Prepare: LDS needs of the batch (bytes of cfg + ctx map + alias tables, MA-tree nodes)
  int max_tree_nodes = 1024, mod_code_bytes = 1 << 20, ac_code_bytes = 1 << 20, ac_code_bytes_compact = 1 << 20;   // (compact: 6 bytes per alias slot, StageCodeCompact)
  int force_generic_idct = 0;
  // filled by Batch::Finish from the per-frame flags the LF stage sets (deterministic per stream): once known, the
  // kernels for varblocks outside a 64x64 tile / the DCT128-256 family are only launched when some frame needs them
  int lf_wide_once = 0;              // the next LF launch takes the one-wavefront-per-stream kernel for every frame, SIMT-eligible or not (a pipeline that starts
                                     // on an idle GPU: 100 instead of 250 ms until the first batch can go on); reset by the launch
  int lf_simt_launched = 0;          // the batch's SIMT LF kernel went out already, as a part of a grouped launch (LaunchLfSimtGroup): LaunchLfDecode runs what follows it only —
                                     // LfDecodeKernel for handed-back streams and legacy frames, the placement kernels; reset by the caller
  int lf_wp_narrow_test = 0;        // testing: the SIMT LF kernel's weighted-predictor lanes hand a stream back at |sample| > 16 instead of 2^20
  int lf_force_big = 0;              // testing: the launch shape of LfDecodeKernel (kernels.hip LaunchLfDecode)
  int lf_spec_lanes = 0;             // SIMT LF launches without the weighted predictor: lanes per stream, each with a candidate cluster whose alias slot it reads ahead (kernels.hip
                                     // LfDecodeSimtKernel SPEC).  0: kLfSpecLanesDefault; 1: the one-lane form; 2, 4, 8: that many — never more than 64 / lane_stride_lf leaves idle
  int lf_head_start = 0;             // the LF launch waits until the next HF launch is resident (set for pipelined front-only calls)
  int idct_flags_known = 0, any_irregular_blocks = 1, any_big_blocks = 1;
  int hf_lanes_per_wave = 0, hf_lanes_per_wg = 0;   // SIMT HF decode: group streams per wavefront / per workgroup (0: the throughput defaults — a frame's streams on four wavefronts of one workgroup)
  int skip_hf = 0;                   // the HF stage is left out: every AC coefficient stays zero (progressive flush at the kDC step, decoder.h AddImage allow_partial)
  int max_passes = 0;                // > 0: at most this many passes of every group are decoded (progressive flush at a kLastPasses / kPasses step)
  int no_flag_wait = 0;              // latency mode (pipeline.h small-job scheduler): the tail never waits on the host for the placement flags of the LF stage, every IDCT kernel variant is launched
  int need_tile4_plain = 1, need_tile4_special = 1, need_tile8_plain = 1, need_tile8_special = 1;   // IdctTileKernel<TB, SPECIAL> variants some frame takes
  int debug_stop_after = 0;          // testing: the tail of a decode stops after 1 = IDCT, 2 = gaborish, 3 / 4 / 5 = EPF pass 0 / 1 / 2 (stage-by-stage filters only)
  int force_unfused_filters = 0;     // testing: stage-by-stage gaborish / EPF / output kernels even for fusable frames        // testing: run the generic (non-tiled) IDCT kernel even for tile-regular frames
  int hf_block_threads = 512;        // threads per HF-decode block (streams per block = threads / lane_stride_hf)
  int hf_by_list = 0;                // this HF launch belongs to a libjpeg-exact decode (Batch::RunPart kPartJpegHf): frames with FrameDev::hf_list decode the groups of that list only, packed into
                                     // the first stream slots; every other launch — Run, the float decode of the same prepared batch — decodes every group
  int lds_code_budget = 64 * 1024;   // bytes of LDS the entropy-code tables (cfg, ctx map, alias) may take per block
};

void InitDeviceTables(void* stream);

// ---- SIMT LF decode (LfDecodeSimtKernel): one LF-group stream (three LF coefficient channels + four HF-metadata channels, ~275 000 tokens
// for a 2048x2048 region) per LANE instead of per wavefront.  The host classifies every channel of every stream from the frame's MA tree
// (decoder.cc ClassifyLfChannel): after the static splits (channel index, stream id) and per class of rows (splits on the row, property 2)
// the subtree may test at most two of {W + N - NW (9), W (7), N (6), largest weighted-predictor error (15)} and its leaves share one
// predictor with offset 0, multiplier 1.  A row class is an 8-byte entry {table offset, class word}; its table — 1024 bytes either way —
// maps the clamped property value(s) to the cluster and is read through the L2 like the alias tables: nothing about a stream lives in LDS
// (measured in round 4: even 2 KB of LDS per LF workgroup — resident for hundreds of milliseconds on every CU — fragments the LDS the 80 KB
// HF workgroups need: HF stage 56 -> 71 ms, with the tables in LDS too 80 ms, although the LF stage itself got 12 % shorter).
// Class word: bits 0-1 kind (0: one cluster, bits 16-23; 1: table over property A, value in [-512, 511]; 2: table over A x B, values in
// [-16, 15]); bits 2-4 predictor (0 zero, 1 W, 2 N, 3 clamped gradient, 4 weighted, 5 (W + N) / 2, 6 select, 7 NE); bits 5-6 / 7-8
// property A / B (0: W + N - NW, 1: W, 2: N, 3: weighted-predictor error); bit 10: the channel keeps weighted-predictor state.
// Channel entry: a row class when every row of the channel has the same one; with bit 9 set, lut_off points at
// [512 bytes: row (clamped to 511) -> index][8-byte row classes].
constexpr uint32_t kLfSimtRows = 1u << 9, kLfSimtWpLive = 1u << 10;
constexpr uint32_t kLfSimtWpInts = 2 * 258 * 8;            // ints of weighted-predictor state per stream: 2 rows x 258 records {four sub-predictor errors, true error, pad}
constexpr int32_t kLfRedoMark = 0x5eed;                    // lf_scratch[2] of an LF group: the SIMT kernel handed the stream back (LfDecodeKernel decodes it again)
struct LfSimtChan { uint32_t lut_off; uint32_t info; };    // lut_off: byte offset in the batch's table blob; info: class word
struct LfSimtStream { uint32_t frame, group; LfSimtChan chan[7]; };   // channels: LF Y, X, B, then ytox, ytob, block info, sharpness
struct LfSimtLane { uint32_t first, count; };               // a lane decodes streams [first, first + count) one after the other
constexpr uint32_t kLfSpecLanesDefault = 8;
struct LfSimtPlan {
  const LfSimtStream* streams = nullptr; const LfSimtLane* lanes = nullptr; const uint8_t* luts = nullptr;   // device pointers
  const uint2* units = nullptr; uint32_t num_units = 0;     // varblock placement: {frame, LF group | band << 16} of every 32-row band of every VarDCT frame, longest first
  uint32_t num_lanes = 0, lanes_per_wave = 16, num_streams = 0;
  int any_legacy = 1;          // some VarDCT frame of the batch still takes LfDecodeKernel (one wavefront per stream)
  int any_general = 0;         // some SIMT stream needs more than the lean instantiation offers (kernels.hip LfDecodeSimtKernel<WP, GEN>)
  int any_wp = 0;              // some SIMT stream keeps weighted-predictor state (the kernel's WP instantiation; LfDecodeKernel follows for the streams it hands back)
};

// Which entropy-decode kernels the last LF / HF launch took (Batch::Info hf_variant, lf_variant, lf_wide_bytes, lf_wide_only): bit masks, one bit per kernel
// instantiation — tests assert the path they meant to reach was the one that ran.
enum : int {
  kHfVarWave = 1, kHfVarSimtPlain = 2, kHfVarSimtAllLds = 4, kHfVarSimtGlobal = 8, kHfVarLaneStride = 16, kHfVarPrefix = 32,   // HfDecodeWaveKernel, HfDecodeSimtKernel
  // <true,false,false> / <true,true,true> / <false,true,true>, HfDecodeKernel (lane-stride batches), HfDecodeKernel beside the SIMT kernel (prefix-coded / LZ77 AC codes)
  kLfVarSimtLean = 1, kLfVarSimtGen = 2, kLfVarSimtWp = 4, kLfVarSimtWpQuad = 8, kLfVarBig = 16, kLfVarSmall = 32, kLfVarLocal = 64,   // LfDecodeSimtKernel<false,false> / <false,true> /
  // <true,true> / <true,true,true>, LfDecodeKernel<true> (four groups per workgroup, register-capped) / <false> (one group per wavefront, or four uncapped),
  // LfDecodeLocalKernel (LF groups with trees / codes of their own)
};
struct LaunchTrace {
  int hf_variant = 0, lf_variant = 0;
  uint32_t lf_wide_bytes = 0;   // LDS bytes of the wave-wide decoder's copy of the Modular code's alias tables (0: the lane-0 serial path without it)
  int lf_wide_only = 0;         // the plain layout was left out (LdAliasAt puts entries together from the wide one)
  int lf_spec_lanes = 0;        // lanes per stream of the SIMT LF launch without the weighted predictor (1: the one-lane form); 0: no such launch
};
// One SIMT LF launch for several batches (pipeline.cc: the LF stages of the jobs that became ready while the LF stream was busy).  The kernel is latency-bound and uses
// 64 of the chip's 1024 SIMDs for 256 frames: the parts of a launch run side by side, so M jobs cost one launch time.  A part is one batch's descriptors and the first
// wavefront that works on them; the table is passed by value (kernel arguments).  Unused slots: first_wave = ~0.
struct LfSimtPart { const FrameDev* frames; const LfSimtStream* streams; const LfSimtLane* lanes; const uint8_t* luts; uint32_t first_wave, num_lanes; };
struct LfSimtPartTable { LfSimtPart part[kLfGroupMax]; };
// What LaunchLfDecode decides about a batch's SIMT launch: batches with equal shapes can share one (lf_group_plan.h LfGroupKey).
enum : int { kLfSimtNone = 0, kLfSimtWpQuad, kLfSimtWp, kLfSimtGen, kLfSimtLean };
struct LfSimtShape {
  int kernel = kLfSimtNone;      // kLfSimtNone: no SIMT launch (no plan, or the wide one-wavefront-per-stream launch takes every frame)
  uint32_t spec_shift = 0;       // log2 of the candidate lanes per stream (kLfSimtGen / kLfSimtLean)
  uint32_t lanes_per_wave = 0;   // streams a wavefront carries (quads: at most 16)
  int lf_flags = 0, waves_per_wg = 1;
};
LfSimtShape LfSimtShapeOf(const LaunchCfg& cfg, const LfSimtPlan* simt);
struct LfSimtGroupPart { const FrameDev* frames; const LfSimtPlan* simt; };
// The SIMT kernel of `shape` over n <= kLfGroupMax batches that all have that shape; every part starts at a workgroup boundary.
void LaunchLfSimtGroup(const LfSimtGroupPart* parts, int n, const LfSimtShape& shape, void* stream);
int64_t LfSpecStats(int which);   // JXL_HIP_LF_SPEC_STATS: samples of this device's candidate-lane LF launches so far whose cluster was a candidate (0) / was not (1); -1 without the variable

// VarDCT stages.  max_* are maxima over the batch (grid sizing); nframes = frames in batch.  trace: filled with the kernels launched (nullptr: not recorded).
void LaunchLfDecode(const FrameDev* frames, int nframes, int max_lf_groups, const LaunchCfg& cfg, void* stream, const LfSimtPlan* simt = nullptr, LaunchTrace* trace = nullptr);
void LaunchLfPost(const FrameDev* frames, int nframes, int max_bw, int max_bh, int max_groups, void* stream);
void LaunchHfDecode(const FrameDev* frames, int nframes, int max_groups, const LaunchCfg& cfg, void* stream, LaunchTrace* trace = nullptr);
void LaunchZeroFailedCoefficients(const FrameDev* frames, int nframes, void* stream);   // behind the HF stage: a failed frame's coefficient planes go back to zero
void LaunchIdct(const FrameDev* frames, int nframes, int max_groups, int max_bw, int max_bh, const LaunchCfg& cfg, void* stream);
struct FilterPlan {
  bool any_upsampled = false;    // some frame needs UpsampleKernel before the write stage
  int max_out_w = 0, max_out_h = 0; bool any_fused = false, any_unfused = false, any_gab = false; int max_epf = 0; };   // over the VarDCT frames of a batch
void LaunchFilters(const FrameDev* frames, int nframes, int max_w, int max_h, const FilterPlan& fp, const LaunchCfg& cfg, void* stream);
void LaunchOutput(const FrameDev* frames, int nframes, int max_w, int max_h, const FilterPlan& fp, const LaunchCfg& cfg, void* stream);
// 1:8 decode: the LF image of every frame with lf_only set -> colour transform -> the caller's layout (LfOutputKernel); needs the LF post-processing only
void LaunchLfOutput(const FrameDev* frames, int nframes, int max_bw, int max_bh, void* stream);
// Modular stages
struct ModOutputArgs { const int32_t* color[3]; const int32_t* alpha; uint32_t ncolor; float color_factor, alpha_factor; uint32_t float_bits, float_exp_bits; };   // float_bits != 0: colour samples are float bit patterns
void LaunchModularGlobal(const FrameDev* frames, int nframes, const LaunchCfg& cfg, void* stream);
uint32_t ModularGroupLdsBytes(const LaunchCfg& cfg);
void LaunchModularGroups(const FrameDev* frames, int nframes, int max_units, const LaunchCfg& cfg, void* stream);   // max_units: most LF groups + groups x passes of a frame
// inverse Squeeze of one channel: (avg, res) -> out; horizontal: avg aw x h, res rw x h, out (aw+rw) x h; vertical: avg w x ah, res w x rh
void LaunchModInvSqueeze(const int32_t* avg, const int32_t* res, int32_t* out, int horizontal, uint32_t aw, uint32_t ah, uint32_t rw, uint32_t rh, void* stream);
// the same step of n <= kSqueezeBatch equally shaped, independent channels (one per image of a batch) in one launch
constexpr int kSqueezeBatch = 16;
struct SqueezeBatch { const int32_t* avg[kSqueezeBatch]; const int32_t* res[kSqueezeBatch]; int32_t* out[kSqueezeBatch]; };
void LaunchModInvSqueezeBatch(const SqueezeBatch& b, int n, int horizontal, uint32_t aw, uint32_t ah, uint32_t rw, uint32_t rh, void* stream);
void LaunchModRct(int32_t* a, int32_t* b, int32_t* c, size_t n, uint32_t rct_type, void* stream);
void LaunchModPalette(const int32_t* pal, int32_t* const* out, uint32_t nb_colors, uint32_t num_c, uint32_t bit_depth, size_t n, void* stream);
// a channel subsampled by (hs, vs), packed top-left in src -> out_w x out_h samples in dst (pixel_ops.h SubsampledSample)
void LaunchChromaUpsample(const float* src, uint32_t src_stride, float* dst, uint32_t dst_stride, uint32_t hs, uint32_t vs, uint32_t out_w, uint32_t out_h, void* stream);
void LaunchModPaletteDelta(const int32_t* pal, int32_t* const* out, uint32_t nb_colors, uint32_t num_c, uint32_t bit_depth, uint32_t nb_deltas, uint32_t predictor,
                           uint32_t w, uint32_t h, const WPHeader& wp, int32_t* wp_scratch, uint32_t wp_stride, void* stream);
void LaunchModOutput(const FrameDev* frames, int fidx, const ModOutputArgs& a, int w, int h, void* stream);

// ---- frame tail of images with several frames or image features (kernels_features.hip); explicit arguments, device pointers ----
// The three colour planes travel in the argument blocks.  A frame's extra channels — any number of them — are described by a per-frame channel table in device
// memory (EcChanDev, built by Batch::PlanPostOps in the constant arena); the per-channel kernels run over (channel, y, x) with the channel on blockIdx.z, so a
// table entry is wave-uniform.  A frame without extra channels has no table and its extra-channel launches are skipped.
struct SplineSegmentDev;   // host_parse.h
struct EcChanDev {
  const int32_t* src_int;            // decoded samples (coded size, row stride = coded width)
  float* plane;                      // float samples, coded size
  float* up;                         // upsampled to the frame size (null: the frame is not upsampled)
  float* tmp;                        // patch blending: the channel's value after a patch, until every channel of the pixel has read the values before it
  const float* fg;                   // what blending reads: `up` or `plane`
  const float* bg;                   // the blending source's plane of this channel (null: an empty reference slot, zeros)
  const float* bg_alpha;             // the same source's plane of channel blend_alpha (modes blend / alpha-weighted add)
  float* canvas;                     // where the blended channel goes (image size)
  uint32_t fg_stride, bg_stride, canvas_stride;
  uint32_t mode;                     // BlendMode | alpha channel << 8 | clamp << 16
  uint32_t premul;                   // alpha_associated (channels of type alpha)
  uint32_t float_bits, float_exp_bits;   // float samples: IntToFloatSample instead of the factor
  float factor;                      // 1 / (2^bits - 1)
  uint32_t type;                     // ExtraChannelType (2 = spot colour)
  float spot[4];                     // spot colour and solidity
};
struct EcFrameArgs { const EcChanDev* table; uint32_t num_extra, w, h, ow, oh, up; const float* up_weights; };
void LaunchEcIntToFloat(const EcFrameArgs& a, void* stream);      // table[c].src_int -> table[c].plane, w x h
void LaunchEcUpsample(const EcFrameArgs& a, void* stream);        // table[c].plane (w x h) -> table[c].up (ow x oh)
// One placement of a patch: source rectangle (pointers already at its top-left sample) -> frame position (x, y); mode = PatchBlendMode | alpha channel << 8 | clamp << 16
// of the colour.  Per placement and extra channel, PatchEcDev [placement * num_extra + channel]: source plane (at the same sample) and the channel's mode word.
struct PatchEntryDev { const float* src[3]; uint32_t src_stride, esrc_stride; int32_t x, y; uint32_t xs, ys; uint32_t mode, pad; };
struct PatchEcDev { const float* src; uint32_t mode, pad; };
struct PatchFrameArgs { float* p[3]; uint32_t stride, ec_stride, w, h, num_extra; };
struct NoiseArgs { float* p[3]; uint32_t stride, w, h; float* noise[3]; uint32_t noise_stride, group_dim, visible_frame_index, nonvisible_frame_index; float lut[8]; float ytox, ytob; };
// mode: 3 = transfer function only (after a spot-colour stage in linear light); 0 XYB -> linear -> transfer function (tf_kind: FrameDev::color_mode's values 0, 1, 4..7), 1 YCbCr -> RGB, 2 copy
// convert (modes 1 and 2 only; decoder.cc FillColourConversion): the samples of an image that is not XYB go on to a requested output encoding — src_tf (color_mode's
// values) with src_par decodes them to linear light (gamma: par[0] = 1 / exponent; PQ: par[0] = 10000 / intensity target; HLG: par = {OOTF exponent, apply?, luminances of
// the source's primaries}), conv is the row-major matrix between the two sets of primaries (conv_identity: left out), tf_kind / inverse_gamma / hdr_par are the target's
struct ColorArgs { const float* src[3]; float* dst[3]; uint32_t src_stride, dst_stride, w, h, mode, tf_kind; float inverse_gamma, opsin_inv[9], neg_bias[3], neg_bias_cbrt[3], hdr_par[5];
                   uint32_t convert, conv_identity, src_tf; float src_par[5], conv[9]; };
// Blending of the colour: mode = BlendMode | alpha channel << 8 | clamp << 16; bg pointers are null when the source slot is empty (treated as zeros); bg_alpha: the colour
// source's plane of the alpha channel.  The foreground alpha and every extra channel go through the table.
struct BlendArgs {
  const float* fg[3]; uint32_t fg_stride, fw, fh; int32_t x0, y0;
  const float* bg[3]; uint32_t bg_stride; const float* bg_alpha; uint32_t bg_alpha_stride;
  float* canvas[3]; uint32_t canvas_stride, img_w, img_h, num_extra, mode;
};
struct WriteArgs { const float* p[3]; const float* alpha; uint32_t stride, alpha_stride, img_w, img_h, unpremul; OutputDesc od; };
void LaunchIntToFloat(const int32_t* src, uint32_t src_stride, float* dst, uint32_t dst_stride, uint32_t w, uint32_t h, float factor, void* stream, uint32_t float_bits = 0,
                      uint32_t float_exp_bits = 0);   // float_bits != 0: the integers are float bit patterns (IntToFloatSample)
void LaunchXybModToFloat(const int32_t* cy, const int32_t* cx, const int32_t* cb, uint32_t src_stride, float* const dst[3], uint32_t dst_stride, uint32_t w, uint32_t h, const float fac[3], void* stream);
// table / pec: null for a frame without extra channels
void LaunchPatches(const PatchFrameArgs& a, const EcChanDev* table, const PatchEntryDev* entries, const PatchEcDev* pec, const uint32_t* tile_start, const uint32_t* tile_list,
                   void* stream);
void LaunchSplines(float* const p[3], uint32_t stride, uint32_t w, uint32_t h, const SplineSegmentDev* segs, const uint32_t* row_start, const uint32_t* indices, void* stream);
void LaunchUpsamplePlane(const float* src, uint32_t src_stride, uint32_t w, uint32_t h, float* dst, uint32_t dst_stride, uint32_t ow, uint32_t oh, uint32_t up, const float* weights, void* stream);
void LaunchNoise(const NoiseArgs& a, void* stream);
void LaunchColor(const ColorArgs& a, void* stream);
// the colour kernel, then the extra channels' (it reads foreground planes and the sources' planes only, never a canvas plane)
void LaunchBlend(const BlendArgs& a, const EcChanDev* table, void* stream);
// stage_spot.cc: p[c] = mix * color[c] + (1 - mix) * p[c], mix = solidity * plate, for the spot-colour channels in header order, channel after channel per pixel (the
// mix is order-dependent); use_canvas: the plates are the blended planes (else fg)
void LaunchSpot(float* const p[3], uint32_t stride, const EcChanDev* table, uint32_t num_extra, uint32_t use_canvas, uint32_t w, uint32_t h, void* stream);
void LaunchWrite(const WriteArgs& a, void* stream);
// Extra-channel planes beside the colour output (OutputSpec::planes; EcPlanesOutKernel): one table entry per requested plane in the constant arena — the float plane of the
// finished image it is taken from (w x h samples, src_stride floats per row) and where it goes: od is a one-slot planar output (pixel_ops.h OutPixelPtr / SlotValue /
// StoreSample: type, byte order, orientation, row pitch, scale[0] / bias[0]), the caller's destination or — resized outputs — the plane's oriented f32 resize source.
struct EcPlaneOutDev { const float* src; uint32_t src_stride, pad; OutputDesc od; };
struct EcPlanesOutArgs { const EcPlaneOutDev* table; uint32_t num_planes, w, h; };
void LaunchEcPlanesOut(const EcPlanesOutArgs& a, void* stream);
// JPEG reconstruction: quantised coefficients of a JPEG-transcoded frame in JPEG layout — component c (0 Y, 1 Cb, 2 Cr), block raster
// order, 64 coefficients in natural (row-major) order: DC from the quantised LF image, AC from the coefficient planes with the integer
// chroma-from-luma of the transcoder undone (dec_group.cc, jpeg branch).  qt: the JPEG quantisation tables, natural order.
struct JpegCoefArgs { int16_t* out; uint32_t ncomp; int32_t qt[3][64]; uint32_t comp_off[3]; };   // comp_off: first block of a component's plane (subsampled frames)
void LaunchJpegCoefficients(const FrameDev* frames, int fidx, const JpegCoefArgs& a, uint32_t bw, uint32_t bh, void* stream);
// ---- device-side writer of Huffman JPEG scans (jpeg_write.hip).  One JpegScanDev per (image, scan) of the batch that takes the device path: the blocks
// of all scans, and their restart segments, are numbered through in table order (first_block / first_seg).
// kind: what a block of the scan codes.  Sequential: DC difference, AC coefficients, end of block.  The four progressive kinds (spectral band Ss..Se, successive
// approximation Ah / Al): first DC pass (difference of c0 >> Al), DC refinement (one bit), first AC pass (|c| >> Al of the band; trailing zeros join an end-of-band
// run), AC refinement (newly non-zero coefficients as symbols, one correction bit for every coefficient that already was non-zero).
enum JpegScanKind : uint32_t { kJpegSequential = 0, kJpegDcFirst = 1, kJpegDcRefine = 2, kJpegAcFirst = 3, kJpegAcRefine = 4 };
struct JpegScanDev {
  uint32_t first_block, num_blocks, first_seg, num_segs;
  uint32_t frame, image;                 // FrameDev whose status word says whether the coefficients exist; slot of the per-image error flags
  uint32_t ncomp, blocks_per_mcu, scan_cols, restart;   // restart: MCUs per restart segment, 0 = the scan is one segment
  uint32_t plane[4], pitch[4];           // per scan component: first block of its coefficient plane in the batch's arena, blocks per plane row
  uint8_t h[4], v[4]; uint16_t dc[4], ac[4];      // blocks per MCU across / down (1 x 1 in a single-component scan); Huffman tables, as indices into JpegWritePlan::tables
  uint32_t kind;                         // JpegScanKind
  uint8_t ss, se, ah, al;
  uint32_t reset_first, reset_count;     // AC kinds: the scan's reset points in JpegWritePlan::resets (batch block numbers, ascending)
};
struct JpegHuffDev { uint8_t depth[256]; uint16_t code[256]; };      // one table slot as defined at one scan (depth 127: no code)
struct JpegSegDev { uint64_t offset; uint32_t size, trail; };        // a restart segment in the stuffed buffer; trail: (last incomplete byte << 8) | its bit count
struct JpegWritePlan {
  const FrameDev* frames; const JpegScanDev* scans; const JpegHuffDev* tables; const int16_t* coef;
  uint32_t num_scans, num_blocks, num_segs;
  uint32_t has_spans;      // some scan is of a progressive kind: the span pass runs and the arrays at the end exist
  uint32_t* bits;          // [num_blocks] pass 1 (progressive AC kinds: head + tail; the span pass adds the EOBn symbol of a run head)
  uint64_t* bitpos;        // [num_blocks + 1] exclusive scan of bits
  uint32_t* seg_bits;      // [num_segs]
  uint32_t* seg_bytes;     // [num_segs] = ceil(seg_bits / 8): every segment starts on a byte
  uint64_t* seg_off;       // [num_segs + 1] exclusive scan of seg_bytes; the last entry is the size of the raw (unstuffed) buffer
  uint64_t* tile_tmp;      // [ceil(max(num_blocks, num_segs) / 1024)] scratch of the scans
  uint32_t* flags;         // per image: 1 DC category out of range, 2 AC category >= 16, 4 symbol without a code, 8 a span's correction bits exceed what the
                           // canonical writer buffers (zeroed by the caller); any of them sends the image through the host writer
  // progressive scans (jpeg_write.hip, "spans"): a block's code is head | EOBn if it heads an end-of-band run | tail
  uint32_t* meta;          // [num_blocks] head bits | tail bits << 12 | joins the end-of-band run << 20
  uint32_t* flush;         // [num_blocks] 1: a flush point (the block emits bits of its own, is a reset point or starts a restart segment); 0 elsewhere and outside AC kinds
  uint64_t* span_idx;      // [num_blocks + 1] exclusive scan of flush: spans in front of a block
  uint32_t* span_first;    // [num_blocks] the flush points in order: first block of every span
  const uint32_t* resets;  // reset points of all scans
};
struct JpegPackBuffers {
  uint8_t* raw; uint64_t raw_bytes;        // = seg_off[num_segs], read back by the host; allocated up to the next multiple of 4
  uint32_t* ff_count; uint64_t* ff_before; // [chunks], [chunks + 1]: 0xFF bytes per JpegStuffChunkBytes() of raw, and their exclusive scan
  uint64_t* tile_tmp;                      // [ceil(chunks / 1024)]
  uint8_t* stuffed; uint64_t stuffed_cap;  // raw with 00 behind every FF: at most 2 x raw_bytes
  JpegSegDev* recs;                        // [num_segs]
};
void LaunchJpegSizes(const JpegWritePlan& p, void* stream);
void LaunchJpegPack(const JpegWritePlan& p, const JpegPackBuffers& o, void* stream);
uint32_t JpegStuffChunkBytes();
// ---- libjpeg-exact pixels of JPEG transcodes (jpeg_pixels.hip; decoder.cc Batch::DecodeJpegPixels).  One JpegPixelImage per image that takes the path, in a device
// table; both kernels run over a group of the table with the image on blockIdx.z.  The coefficients are read from the frame's own planes (FrameDev::coeff / lfq / coef_off),
// where the HF stage left them.  qt: the JPEG quantisation tables; cfl_ratio[c - 1]: 2048 x qt[0][i] / qt[c][i] (4:4:4 colour: chroma from luma, JpegCoefKernel's formula) —
// both in the layout of the coefficient planes, the transpose of JPEG's natural order (index u * 8 + v).  plane[c]: u8 samples of component c (0 Y, 1 Cb, 2 Cr) after the
// integer IDCT, grid_w[c] x 8 bytes per row, the whole padded grid.  hs / vs: the chroma components' shifts against luma (0 / 1) = against the frame's block grid.
struct alignas(16) JpegPixelImage {
  uint8_t* plane[3];
  uint32_t grid_w[3], grid_h[3];         // the component's padded grid, in blocks
  uint32_t comp_first[3];                // grey and subsampled images: first position of component c (4:4:4 colour: unused, a position is one block of all three)
  uint32_t npos;                         // positions JpegIdctPlanesKernel walks: the blocks of all components, or at 4:4:4 colour the blocks of the luma grid
  uint32_t ncomp;
  uint32_t frame;                        // FrameDev of the image: status word, block info, coefficient planes, OutputDesc
  uint32_t width, height, hs, vs;
  // what of the image is decoded (Batch::JpegRegion; an image without a region: the whole of it).  reg_*[c]: the block rectangle of component c that JpegIdctBody walks —
  // whole 256x256 groups of the frame, so that every coefficient the HF stage wrote is read and zeroed; comp_first / npos count its positions.  rect_*: the pixel
  // rectangle of the stored picture (at `scale`) the colour kernels write — the crop mapped back through the orientation — and nothing outside it
  uint32_t reg_x0[3], reg_y0[3], reg_w[3], reg_h[3];
  uint32_t rect_x0, rect_y0, rect_w, rect_h;
  // libjpeg's scaled decode (OutputSpec::jpeg_scale = 2, 4, 8; entries of scale 1 leave all of this 0 apart from `scale`): component c takes the n[c] x n[c] IDCT
  // (jdmaster.c: 8 / scale, twice that for 4:2:0 chroma), its plane has pitch[c] = grid_w[c] x n[c] bytes per row and n[c] rows per block row, of which ext_w[c] x
  // ext_h[c] are real samples; the picture is out_w x out_h = ceil(width / scale) x ceil(height / scale).  chroma_up: 0 = the chroma planes have the picture's
  // extent, 1 = half its width (4:2:2): h2v1 upsampling, "fancy" if chroma_fancy (8 / scale > 1) and the plane is more than two samples wide, else replication
  uint32_t scale, n[3], pitch[3], ext_w[3], ext_h[3], out_w, out_h, chroma_up, chroma_fancy;
  // JpegGatherKernel (reconstruction: Batch::PlanJpegWrite fills the same entry, without planes): where the image's int16 coefficients go — natural order, component c
  // from block comp_first[c] on (at 4:4:4 too), 16-byte aligned — and every component's own shifts against the frame's block grid
  int16_t* coef_out;
  uint32_t comp_hs[3], comp_vs[3];
  alignas(16) int32_t qt[3][64];
  alignas(16) int32_t cfl_ratio[2][64];
};
constexpr uint32_t kJpegPixelGroupMax = 32768;       // images per launch (gridDim.z is limited to 65535)
// a run of the table served by one launch per kernel, the grids sized for its largest image (max_w x max_h: of the pictures that are written); scaled: 1 = a run of
// entries with scale 2, 4, 8, which take the two ...Scaled kernels; kJpegGroupDc = a run of DC-only entries (scale 8, every component at the 1 x 1 IDCT; their frames
// have FrameDev::lf_only == kLfOnlyJpegDc and neither coefficient nor pixel planes), which take no IDCT launch at all and JpegDcOutKernel — the kinds never share a run
constexpr uint32_t kJpegGroupDc = 2;
struct JpegPixelGroup { uint32_t first, count, max_npos, max_w, max_h, scaled = 0; };
void LaunchJpegIdctGroup(const FrameDev* frames, const JpegPixelImage* table, const JpegPixelGroup& g, void* stream);       // JpegIdctPlanesKernel / JpegIdctScaledKernel; nothing for a DC-only run
void LaunchJpegColorOutGroup(const FrameDev* frames, const JpegPixelImage* table, const JpegPixelGroup& g, void* stream);   // JpegColorOutKernel / JpegColorOutScaledKernel, behind it on the same stream; JpegDcOutKernel
void LaunchJpegGatherGroup(const FrameDev* frames, const JpegPixelImage* table, const JpegPixelGroup& g, void* stream);     // JpegGatherKernel (max_w / max_h unused)
void LaunchCopyPlane(const float* src, uint32_t src_stride, float* dst, uint32_t dst_stride, uint32_t w, uint32_t h, void* stream);
// ---- resized output (OutputSpec::resize_w / resize_h): separable antialiased filter (triangle or cubic convolution), horizontal pass then vertical, f32 throughout.
// One axis' filter as the host built it (decoder.cc ResizeAxis): output index i takes the taps first[i] .. first[i + 1] - 1 of `weight` (normalised, double rounded once to f32)
// from the input samples lo[i], lo[i] + 1, ...; the number of taps is whatever the ratio asks for.
struct ResizeAxisDev { const uint32_t* lo; const uint32_t* first; const float* weight; };
// src: interleaved f32 picture of od.out_channels slots, src_stride floats per row, of which the rectangle (x0, y0) in_w x in_h is resampled to out_w x out_h; tmp:
// in_h x out_w x slots floats (the horizontally filtered rows); od: the caller's destination, out_orient 1 — the source is oriented already; mirror: target column ox is
// stored at out_w - 1 - ox
// u8 (the integer resample of libjpeg-exact outputs, OutputSpec::resize_u8 — ResizeU8Kernel): src and tmp are bytes (src_stride in bytes, tmp in_h x out_w x slots bytes) and
// the two axes' `weight` are int32 (decoder.cc ResizeAxisInt: the normalised double weight x 2^22, rounded half away from zero); everything else as above
struct ResizeArgs { const float* src; float* tmp; uint64_t src_stride; uint32_t x0, y0, in_w, in_h, out_w, out_h, mirror, u8; ResizeAxisDev ax, ay; OutputDesc od; };
// The resizes of a decode are one device table of ResizeArgs, sorted by arithmetic (f32, then u8) and slot count; a group is a run of `count` entries from `first` on with the same arithmetic and number of slots,
// served by one launch per pass (image on blockIdx.z, the grid sized for the group's largest extents).  count <= kResizeGroupMax (gridDim.z is limited to 65535).
constexpr uint32_t kResizeGroupMax = 32768;
struct ResizeGroup { uint32_t first, count, slots, max_out_w, max_in_h, max_out_h, u8 = 0; };   // u8: a group of ResizeU8Kernel's entries (a group never mixes the two arithmetics)
void LaunchResizeGroup(const ResizeArgs* table, const ResizeGroup& g, void* stream);

// names of the kernels (for profiling summaries)
extern const char* const kKernelNames[];

}  // namespace jxlhip
