// jxl-hip: batch decoder — owns device memory for a batch of frames and enqueues the kernel pipeline.
// A batch of one frame backs the libjxl-compatible JxlDecoder ABI (jxl_abi.cc); larger batches back the resident
// batch API used by bench.py (include/jxl_hip.h).
#pragma once
#include "host_parse.h"
#include "kernels.h"
#include "jpeg_recon.h"
#include "decode_parts.h"
#include <memory>
#include <string>
#include <functional>
#include <vector>

namespace jxlhip {

// One extra-channel plane written beside the colour output (OutputSpec::planes): channel `index` as it is — the values alpha_from_extra = index puts into the alpha
// slot, never un-premultiplied, untouched by spot rendering and int_bits — as one sample per pixel in a format of its own; float types may be stored as
// fmaf(v, scale, bias).  The public calls give every plane the colour output's format; jxl_abi.cc serves buffers of differing formats.
struct PlaneRequest {
  uint32_t index = 0;          // extra channel
  uint32_t type = 0;           // 0 u8, 1 u16, 2 f32, 3 f16
  uint32_t big_endian = 0;
  size_t align = 0;            // row pitch = oriented width x sample size, rounded up to this
  bool affine = false; float scale = 1.0f, bias = 0.0f;
};
// The planes sit behind the colour output, plane k at offset + k x pitch of the destination; they follow the colour output's geometry (orientation, resize, crop, filter, mirror).
// offset 0 = num_channels x plane_stride of a planar colour output (colour and extras form one [C + m, H, W] block), the colour size rounded up to 16 bytes of an
// interleaved one; plane_stride 0 = the colour layout's plane_stride when the colour is planar, else tight (rows x row pitch).  Either may be given: at least the default
// and a multiple of the sample size (Batch::PlanesLayoutOf).  Indices may repeat.
struct OutputPlanes {
  std::vector<PlaneRequest> req;
  size_t offset = 0, plane_stride = 0;
  bool any() const { return !req.empty(); }
};
struct PlanesLayout { size_t offset = 0, pitch = 0, total = 0; };
constexpr size_t kMaxOutputPlanes = 4096;      // (the format's limit on channels)

struct OutputSpec {
  uint32_t num_channels = 0;   // 0 = colour + alpha
  uint32_t type = 0;           // 0 u8, 1 u16, 2 f32, 3 f16
  uint32_t big_endian = 0;
  size_t align = 0;
  void* device_ptr = nullptr;  // optional caller-owned device destination
  bool keep_orientation = false;  // false: the header's orientation is applied to the output (libjxl's default)
  bool unpremul_alpha = false;    // JxlDecoderSetUnpremultiplyAlpha: premultiplied colour is divided by alpha in the write stage
  int upto_frame = -1;            // >= 0: coalesced output of an animation frame — the canvas as it stands after frame `upto_frame` has been blended (the frames behind it are not shown)
  int only_frame = -1;            // >= 0: non-coalesced output (JxlDecoderSetCoalescing(false)) — frame `only_frame` of the image as coded: its own size, its own
                                  // pixels after the colour transform, not blended onto the canvas
  int alpha_from_extra = -1;      // which extra channel fills the alpha slot of 2 / 4-channel output: -1 = the first one of type alpha; >= 0: that extra channel, as it is
                                  // (JxlDecoderSetExtraChannelBuffer hands out the extra channels of simple images through this slot, a decode per plane; `planes` below
                                  // delivers any number of them from one decode, through the frame tail)
  uint32_t int_bits = 0;          // integer output: 0 = the full range of the sample type, else samples in [0, 2^int_bits - 1] (JxlDecoderSetImageOutBitDepth)
  bool render_spotcolors = true;  // JxlDecoderSetRenderSpotcolors: spot-colour extra channels are mixed into the colour channels (stage_spot.cc)
  uint32_t downscale = 1;         // 1, or 8: the 1:8 decode — the output is the frame's LF image, ceil(w / 8) x ceil(h / 8) pixels, one per 8x8 block, through the colour transform and the
                                  // write stage (LfOutputKernel); no AC coefficient is decoded, no IDCT, no restoration filter runs.  Single-frame VarDCT images without extra
                                  // channels, patches, splines, noise or upsampling (Batch::DownscaleRefusal)
  uint32_t jpeg_scale = 1;        // 1, 2, 4, 8: libjpeg's scaled decode of a JPEG transcode (scale_num / scale_denom = 1 / jpeg_scale: jdmaster.c, jidctred.c) — the picture is the
                                  // ceil(w / jpeg_scale) x ceil(h / jpeg_scale) one libjpeg gives for the original file, from reduced IDCTs.  Other than 1: only with downscale 1, only
                                  // for images Batch::CanDecodeJpegPixels takes (SetOutput), and written by Batch::DecodeJpegPixels alone — Run fails such an image
  // ---- layout (Batch and Pipeline outputs; the libjxl look-alike API, previews and kept animation canvases are interleaved)
  bool planar = false;            // channel slot c (grey or G, alpha / R, G, B, alpha) is a plane of its own at c x plane_stride: rows of one sample per pixel, oriented width x sample size
                                  // rounded up to `align` apart; the output is num_channels x plane_stride bytes
  size_t plane_stride = 0;        // 0 = tight (oriented height x row stride), else at least that and a multiple of the sample size
  bool affine = false;            // float16 / float32 output: slot c is stored as fmaf(v, scale[c], bias[c])
  float scale[4] = {1.0f, 1.0f, 1.0f, 1.0f}, bias[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  // ---- resize (Batch and Pipeline outputs): the picture the output would have held without it — oriented, at downscale 1 or 8 or at jpeg_scale, the "source" — is resampled to
  // resize_w x resize_h with the antialiased filter resize_filter (ResizeAxis, decoder.cc); the output's size, strides and layout go by the target size
  uint32_t resize_w = 0, resize_h = 0;     // 0 x 0 = off, else 1 .. 65535 each
  uint32_t crop_x0 = 0, crop_y0 = 0, crop_w = 0, crop_h = 0;   // rectangle of the source that is resampled (all 0 = the whole picture): exactly crop first, then resize
  uint32_t resize_filter = 0;              // 0 = triangle, 1 = cubic convolution with a = -0.5 (resized outputs only)
  bool mirror = false;                     // resized outputs only: target column ox is stored at column resize_w - 1 - ox, a flip of the finished target
  bool resize_u8 = false;                  // resized outputs of the libjpeg-exact decode only (Batch::CanDecodeJpegPixels, downscale 1): the resample is Pillow's 8-bit one over the
                                           // u8 picture libjpeg gives (include/jxl_hip.h, JxlHipBatchSetOutputJpegResampled: int32 weights of 22 fraction bits, rounded and clamped
                                           // to u8 behind each pass), byte for byte im.crop(box).resize(size, filter); the intermediate is u8.  Written by DecodeJpegPixels alone
  // ---- extra-channel planes behind the colour output (Batch and Pipeline outputs; an image with any becomes complex, the frame tail delivers them: EcPlanesOutKernel)
  OutputPlanes planes;
  // ---- output colour (Batch, Pipeline and JxlHipDecoderSetOutputColorProfile): XYB images are rendered to `color` instead of the encoding their header names — the colour
  // stage's parameters and the kernel choice go by it (Batch::ColourHeader); an image that is not XYB keeps its samples unless color_non_xyb is set, and is then
  // converted in the frame tail (ColorKernel; the image becomes complex) when its encoding differs from the target
  bool color_set = false;
  ColorTarget color;
  uint32_t color_non_xyb = 0;              // 0 leave (libjxl's rule), 1 convert
  bool resized() const { return resize_w || resize_h; }
  bool cropped() const { return crop_x0 || crop_y0 || crop_w || crop_h; }
};

// What the frames of one image share: the codestream and the image header.
struct ImageShared { Codestream cs; ImageHeader ih; MetadataBoxes boxes; };   // jbrd: payload of the JPEG-reconstruction box, if any

// One *frame* of an image: the unit the decode stages work on (one FrameDev each).  A single-frame image without image
// features is one unit that writes its pixels itself; the frames of other ("complex") images end in float planes and a
// host-planned tail (patches, splines, noise, colour transform, blending, write) composes them (Batch::PlanPostOps).
struct ImageEntry {
  std::shared_ptr<ImageShared> shared;
  Codestream& cs;
  ImageHeader& ih;
  FramePlan plan;
  uint64_t frame_bitpos = 0;
  OutputSpec out;                      // (first unit of the image)
  size_t out_stride = 0, out_size = 0; // out_size: the whole destination, the colour output and the planes behind it
  size_t color_size = 0;               // (first unit) the colour output alone (= out_size without planes)
  PlanesLayout planes_layout;          // (first unit) where out.planes go in the destination
  vec<size_t> off_plane_src, off_plane_tmp;   // (first unit, resized output with planes; pixel-plane arena) per requested plane: the oriented f32 plane EcPlanesOutKernel leaves for
                                              // ResizeKernel<1>, the horizontally filtered rows
  vec<int> deliver_frames;             // (first unit) coalesced animation decoded once: the canvas after each of these frames goes to its own slot of the output area (SetOutputAllFrames)
  bool has_jbrd = false;
  int pub_index = 0, frame_index = 0;  // image the frame belongs to, position among its frames
  bool complex = false;                // frame of a complex image
  uint32_t visible_frame_index = 0, nonvisible_frame_index = 0;   // noise seeds (dec_frame.cc)
  uint64_t preview_bitpos = 0;             // where the preview frame starts (images with a preview: ih.have_preview)
  std::shared_ptr<ImageEntry> lf_source;   // the LF frame (frame type 1) a frame with use_lf_frame takes its LF image from; not a unit of the batch itself
  // arena offsets
  size_t off_cs = 0, off_sec = 0, off_tree = 0, off_bcm = 0;
  size_t off_out = 0;
  size_t off_resize_src = 0, off_resize_tmp = 0;   // (first unit, resized output; pixel-plane arena) the f32 picture the write stage leaves for ResizeKernel, the horizontally filtered rows
                                                   // (OutputSpec::resize_u8: both in u8, for ResizeU8Kernel)
  uint32_t src_w = 0, src_h = 0;                   // (first unit) size of that picture: SetOutput
  bool jpeg_dc_eligible = false;                   // (first unit) SetOutput: the output is libjpeg's 1/8 decode and every component takes the 1 x 1 IDCT (Batch::JpegDcOnly)
  // (first unit) SetOutput: the output is a crop of a picture the libjpeg-exact decode takes (Batch::JpegRegion) — region_groups: gx0, gy0, gx1, gy1, the rectangle of
  // 256x256 groups the crop needs; region_rect: x0, y0, w, h of the crop in the stored picture at jpeg_scale (mapped back through the orientation)
  bool jpeg_region_eligible = false;
  uint32_t region_groups[4] = {0, 0, 0, 0}, region_rect[4] = {0, 0, 0, 0};
  explicit ImageEntry(std::shared_ptr<ImageShared> s) : shared(std::move(s)), cs(shared->cs), ih(shared->ih) {}
};

// growable byte buffer in pinned host memory: the constant arena is assembled in it and uploaded from it (decoder.cc)
class HostStage {
 public:
  HostStage() = default;
  HostStage(const HostStage&) = delete;
  HostStage& operator=(const HostStage&) = delete;
  ~HostStage();
  size_t size() const { return n_; }
  uint8_t* data() { return p_; }
  const uint8_t* data() const { return p_; }
  void clear() { n_ = 0; }
  void Resize(size_t n);
  void Reserve(size_t n);      // capacity only
  bool pinned() const { return pinned_; }
 private:
  void Release();
  uint8_t* p_ = nullptr; size_t n_ = 0, cap_ = 0; bool pinned_ = false;
  std::vector<std::pair<uint8_t*, bool>> retired_;     // outgrown blocks, freed with the object
};

// Coefficient / pixel planes that belong to somebody else (a Pipeline): a batch whose layout fits uses them instead of arenas of its own (Batch::UseSharedPlanes).
// `dirty` / `clean_extent` are the coefficient planes' bookkeeping (see Batch::ClearCoefficientsBeforeHf); the owner serialises the decodes that share one set.
struct SharedPlanes { uint8_t* p = nullptr; size_t cap = 0; bool dirty = true; size_t clean_extent = 0; };

struct JpegFrameGrid;      // quantisation tables, sampling factors and component grids of a JPEG-transcoded frame (decoder.cc)

struct StageTimes { float lf_ms = 0, lfpost_ms = 0, hf_ms = 0, idct_ms = 0, filter_ms = 0, out_ms = 0, total_ms = 0; };

class Batch {
 public:
  explicit Batch(int device);
  ~Batch();
  // Parses headers (container, image header, frame header, TOC, global sections).  Throws ParseError.
  // allow_partial: a single-frame VarDCT image whose bytes end inside its PassGroup sections is accepted as far as its LF part (LfGlobal, LfGroups, HfGlobal complete):
  // it decodes with every AC coefficient zero — what JxlDecoderFlushImage shows at the kDC progression step
  int AddImage(const uint8_t* data, size_t size, bool allow_partial = false);
  bool is_partial(int i) const;
  // The same for n images, parsed on `threads` host threads and appended in order; returns the index of the first.
  int AddImages(const uint8_t* const* datas, const size_t* sizes, int n, int threads, bool allow_partial = false);
  // "" when image i can be decoded at 1:8 (OutputSpec::downscale == 8), else the reason, "unsupported: downscaled decode of ..."; SetOutput throws it
  std::string DownscaleRefusal(int i) const;
  // Same, but an image that does not parse is left out instead of failing the call: (*index)[i] = its index in the batch or -1, (*errors)[i] = what it threw.
  // for_downscale: the images are going to be decoded at 1:8 — a stream may end behind its LF part (allow_partial as for AddImage), and an image that decode does not take is
  // left out with DownscaleRefusal's message
  // for_jpeg_dc: the images are going to be decoded at libjpeg's scale 1/8 (OutputSpec::jpeg_scale == 8) — a stream may end behind its LF part too, and one that does
  // and is not DC-only at that scale (JpegDcOnly: 4:2:0 needs AC terms; what the libjpeg-exact decode does not take) is left out as "truncated"
  void AddImagesTolerant(const uint8_t* const* datas, const size_t* sizes, int n, int threads, vec<int>* index, std::vector<std::string>* errors, bool for_downscale = false,
                         bool for_jpeg_dc = false);
  // Forgets the images, keeps device arenas / staging buffer / buffer sharing: the object can be filled and prepared again.
  void Reset();
  size_t size() const { return pub_.size(); }
  ImageEntry& image(int i) { return *images_[pub_[i].first_unit]; }
  int num_units() const { return (int)images_.size(); }          // frames of all images, in decode order
  const ImageEntry& unit(int i) const { return *images_[i]; }
  static size_t OutputStride(const ImageHeader& ih, const OutputSpec& o, uint32_t* channels);
  static uint32_t OrientedWidth(const ImageHeader& ih, const OutputSpec& o);
  static uint32_t OrientedHeight(const ImageHeader& ih, const OutputSpec& o);
  // size of the picture a resize reads (OrientedWidth / OrientedHeight of the same output without its resize)
  static uint32_t SourceWidth(const ImageHeader& ih, const OutputSpec& o);
  static uint32_t SourceHeight(const ImageHeader& ih, const OutputSpec& o);
  static size_t OutputSize(const ImageHeader& ih, const OutputSpec& o);      // the colour output and, behind it, o.planes
  static size_t ColorOutputSize(const ImageHeader& ih, const OutputSpec& o); // the colour output alone
  // "" when o.planes can be written for an image with ih's extra channels, else the reason, "unsupported: extra planes ..."; OutputSize and SetOutput throw it
  static std::string PlanesRefusal(const ImageHeader& ih, const OutputSpec& o);
  // where o.planes go: offset of the first, pitch from one to the next, size of the whole destination; throws what does not fit (an offset or pitch below the default ...)
  static PlanesLayout PlanesLayoutOf(const ImageHeader& ih, const OutputSpec& o);
  // row pitch of requested plane k, bytes
  static size_t PlaneRowStride(const ImageHeader& ih, const OutputSpec& o, const PlaneRequest& r);
  // Output colour (OutputSpec::color).  ColourRefusal: "" when `o`'s target can be served for an image with header ih, else the reason, "unsupported: output colour ...";
  // SetOutput throws it.  ColourHeader: the header the colour stage and the kernel choice go by — for an XYB image under a target, ih's colour fields replaced by the
  // target (built in *store), else ih itself.  ConvertsNonXyb: the image is not XYB and `o` asks for its conversion to another encoding than its own (frame tail).
  static std::string ColourRefusal(const ImageHeader& ih, const OutputSpec& o);
  static const ImageHeader& ColourHeader(const ImageHeader& ih, const OutputSpec& o, ImageHeader* store);
  static bool ConvertsNonXyb(const ImageHeader& ih, const OutputSpec& o);
  // "" when the layout of `o` (planar, plane_stride, affine) can be written for an image of ih's size, else the reason; OutputSize and SetOutput throw it
  static std::string LayoutRefusal(const ImageHeader& ih, const OutputSpec& o);
  // "" when the resize of `o` can be done for an image of ih's size (a target side of 0 or above 65535, a crop that is empty or leaves the picture), else the reason;
  // OutputSize and SetOutput throw it
  static std::string ResizeRefusal(const ImageHeader& ih, const OutputSpec& o);
  // size of the rectangle output `o` of image i covers: the image, or — non-coalesced output — frame o.only_frame as coded (before orientation)
  void OutputDims(int i, const OutputSpec& o, uint32_t* w, uint32_t* h) const;
  size_t OutputSizeOf(int i, const OutputSpec& o) const;
  // Coalesced animation in one decode: the canvas as it stands after every frame of `frames` (ascending positions among the image's frames) is written to slot k of the
  // image's output area in device memory (internal buffers only); CopyOutputSlotToHost hands them out.  Throws "unsupported" for what needs the canvas changed in place on
  // delivery (spot colours, a transfer function deferred behind them): the caller then decodes frame by frame (OutputSpec::upto_frame).
  void SetOutputAllFrames(int i, const OutputSpec& o, const vec<int>& frames);
  void CopyOutputSlotToHost(int i, int slot, void* dst, size_t size, void* stream);
  // image i takes the frame tail under output `o` whether or not planes are asked for (what PromoteToComplex decides without its clause for OutputSpec::planes): host only
  bool ComplexWithoutPlanes(int i, const OutputSpec& o) const;
  int num_frames(int i) const { return pub_[i].num_units; }
  const ImageEntry& frame(int i, int k) const { return *images_[pub_[i].first_unit + k]; }
  void SetOutput(int i, const OutputSpec& o);
  // Allocates device memory, uploads streams + tables (inputs become HBM-resident).  stream: hipStream_t.
  // wait_upload = false: returns with the upload still in flight on `stream` (the caller enqueues the first stage of the decode on that same stream)
  void Prepare(void* stream, bool wait_upload = true);
  // Enqueues the whole decode of every frame of the batch.  No host synchronisation inside.
  void Run(void* stream);
  // Waits, checks device status words; throws ParseError on stream errors.
  void Finish(void* stream);
  // JPEG bit-stream reconstruction of image i (decode.rs:493 reconstruct): true if the image carries a usable `jbrd` box and is a plain
  // single-frame JPEG transcode (DCT8 only, RAW quant table, 4:4:4).  ReconstructJpeg runs the entropy-decode stages on the GPU, gathers
  // the quantised coefficients in JPEG layout and serialises the file on the host; throws ParseError if something does not fit.
  bool CanReconstructJpeg(int i, std::string* why = nullptr);
  vec<uint8_t> ReconstructJpeg(int i, void* stream);
  // The same for every image of the batch from one run of the entropy stages.  Images whose scans are all sequential Huffman scans get their entropy-coded
  // segments written on the device (jpeg_write.hip) and spliced between the markers on the host; progressive files (unless jpeg_device_progressive), scans with extra zero runs and
  // cfg.jpeg_host_writer go through WriteJpeg, from coefficients copied to the host for those images only.  An image that cannot be reconstructed, or whose
  // stream is damaged, fails alone: jpeg_result(i).  Throws only for what concerns the whole batch (HIP errors, Prepare).
  struct JpegResult { bool ok = false; std::string error; vec<uint8_t> bytes; };
  void ReconstructJpegs(void* stream);
  bool jpeg_host_writer = false;          // every image through the host writer (tests, measurements)
  // progressive files too get their scans written on the device where every scan is a first DC pass, a DC refinement, a first AC pass or an AC refinement of one
  // component (DESIGN.md §5 lists what stays with the host writer); off: progressive files go through the host writer
  bool jpeg_device_progressive = false;
  uint32_t resize_group_max = kResizeGroupMax;   // testing: images per resize launch (1 .. kResizeGroupMax)
  // ReconstructJpegs in its phases, for callers that order the stages themselves (Pipeline jobs of this kind); ReconstructJpegs is the four in sequence on one stream:
  //   PlanJpegWrite             host only, after Prepare: CanReconstructJpeg per image, the marker walk (scans, table snapshots, reset points), the arena layout, the gather
  //                             table, and which images the device writes (jpeg_host_writer, jpeg_device_progressive); an image that cannot be reconstructed
  //                             gets its jpeg_result now.  Returns the number of images left.
  //   EnqueueJpegPlan           uploads scan table, tables, resets and gather table on `stream`, clears the flags; fail_refused: the status words of the frames that are
  //                             NOT in the gather table are set (kErrUnsupported), so that ZeroFailedCoefKernel puts zeros back where nobody will consume coefficients
  //   EnqueueJpegGather         behind the HF stage (RunPart kPartHf): JpegGatherKernel, one launch per group of at most kJpegPixelGroupMax images — the last stage that touches
  //                             the coefficient planes; with fail_refused they are clean behind it
  //   EnqueueJpegSizes          the sizes pass of the device writer.  Neither waits on the host.
  //   EnqueueJpegHeadReadback   (optional) the raw size and the flag words to pinned memory on a copy stream of the caller's, who waits for it before FinishJpegWrite
  //   FinishJpegWrite           with the status words (FinishStatus / HarvestStatus): pack and stuffing pass, bytes and records back, splice or host writer per image.
  //                             Every copy is a hipMemcpyAsync on `stream` into pinned staging followed by a wait for that stream.  Fills jpeg_result(i) and the counters.
  size_t PlanJpegWrite();
  void EnqueueJpegPlan(void* stream, bool fail_refused);
  void EnqueueJpegGather(void* stream);
  void EnqueueJpegSizes(void* stream);
  void EnqueueJpegHeadReadback(void* stream);
  void FinishJpegWrite(void* stream, const vec<uint32_t>& per_unit);
  JpegResult* mutable_jpeg_result(int i) { return i >= 0 && (size_t)i < jpeg_results_.size() ? &jpeg_results_[(size_t)i] : nullptr; }   // (a pipeline job moves the bytes out)
  const JpegResult* jpeg_result(int i) const { return i >= 0 && (size_t)i < jpeg_results_.size() ? &jpeg_results_[(size_t)i] : nullptr; }
  // The samples libjpeg gives for the original file of a JPEG transcode, instead of libjxl's rendering of the frame (Run): integer dequantisation and IDCT, libjpeg's
  // "fancy" chroma upsampling and fixed-point YCbCr -> RGB (jpeg_pixels.hip), written through the write stage to the outputs set with SetOutput.  Takes the frame
  // conditions of CanReconstructJpeg without those on the `jbrd` box, 4:4:4 / 4:2:2 / 4:2:0 or grey, at downscale 1; CanDecodeJpegPixels is host-only and says
  // "unsupported: libjpeg-exact decode of ..." otherwise (the quantisation table of a one-group frame is only known after Prepare: DecodeJpegPixels looks again).
  // DecodeJpegPixels runs the entropy stages once for the whole batch; an image that is not eligible, or whose stream is damaged, fails alone: jpeg_pixel_result(i).
  // Throws only for what concerns the whole batch (HIP errors, no prepared images).  An output with OutputSpec::jpeg_scale = 2, 4, 8 is libjpeg's scaled decode of the
  // file (jidctred.c's reduced IDCTs): such images take JpegIdctScaledKernel / JpegColorOutScaledKernel, in launch groups of their own behind those of scale 1.
  struct JpegPixelResult { bool ok = false; std::string error; };
  bool CanDecodeJpegPixels(int i, std::string* why = nullptr) const;
  bool CanDecodeJpegPixelsAs(int i, const OutputSpec& out, std::string* why) const;      // the same for an output that is not set yet (SetOutput)
  // The DC-only frame kind.  An image whose output is libjpeg's 1/8 decode (OutputSpec::jpeg_scale == 8; SetOutput has asked CanDecodeJpegPixelsAs) and whose sampling is
  // grey, 4:4:4 or 4:2:2 takes the 1 x 1 "IDCT" for every component: each sample is one DC term, and the DC terms are FrameDev::lfq, written by the LF stage.  Its decode
  // ends behind the LF stage like a 1:8 frame's (EndsBehindLf): no HF stage, no coefficient or pixel planes, a stream that ends behind its LF part will do;
  // JpegDcOutKernel writes the picture.  4:2:0 takes the 2 x 2 IDCT for chroma, hence AC terms, and keeps the general path.  Known from the frame header and the
  // output alone.  jpeg_dc_only = false keeps the general path for every image (the A/B of the tests; read by the next Prepare).
  bool jpeg_dc_only = true;
  void SetJpegDcOnly(bool on) { if (on != jpeg_dc_only) { jpeg_dc_only = on; prepared_ = false; } }      // (another layout of the arenas: the batch is prepared again)
  bool JpegDcOnly(int i) const { return jpeg_dc_only && images_[pub_[i].first_unit]->jpeg_dc_eligible; }
  // Decoding by region (off by default; DESIGN.md §3 has the rule).  An image whose output DecodeJpegPixels writes, that is not DC-only and whose output carries a crop
  // needs only the blocks the crop covers, widened to whole MCUs plus one MCU on every side (fancy chroma upsampling reads chroma sample i +- 1, which lies in the
  // neighbouring chroma block at every scale): with jpeg_region on, the HF stage of DecodeJpegPixels (RunPart kPartJpegHf) and of the pipeline jobs built from its steps decodes
  // only the 256x256 groups that rectangle touches — Prepare uploads their indices per frame (FrameDev::hf_list) —, the integer IDCT walks only those groups' blocks and
  // the colour kernels write only the crop's rectangle.  The bytes delivered are those of the decode without the option.  Run, the float decode of the same prepared
  // batch, decodes every group whatever the option says.  Known from the frame header and the output alone (SetOutput); read by the next Prepare.
  bool jpeg_region = false;
  void SetJpegRegion(bool on) { if (on != jpeg_region) { jpeg_region = on; prepared_ = false; } }      // (the lists are Prepare's: the batch is prepared again)
  // the region image i would be decoded by with jpeg_region on (false: it would be decoded whole — no crop, DC-only, not taken by the libjpeg-exact decode); host only
  bool JpegRegionOf(int i, uint32_t groups[4]) const;
  void DecodeJpegPixels(void* stream);
  // DecodeJpegPixels in its steps, for callers that order the stages themselves (Pipeline jobs of this kind):
  //   PlanJpegPixels            host only, after Prepare: eligibility, the component grids, the image table and its launch groups; an image that is refused gets its
  //                             jpeg_pixel_result now.  Returns the number of images in the table.
  //   EnqueueJpegPixelTable     uploads the table into a buffer of its own on `stream`; fail_refused: the status words of the frames that are NOT in the table are set
  //                             (kErrUnsupported), so that the HF stage's ZeroFailedCoefKernel puts zeros back where nobody will consume their coefficients
  //   RunPart(stream, kPartJpegIdct / kPartJpegPixels)   the integer IDCT over the HF planes (the last stage that touches the coefficient set, which is clean behind it); colour, write and resizes
  //   HarvestJpegPixels         the status words (FinishStatus / HarvestStatus) -> jpeg_pixel_result of the images in the table
  size_t PlanJpegPixels();
  void EnqueueJpegPixelTable(void* stream, bool fail_refused);
  void HarvestJpegPixels(const vec<uint32_t>& per_unit);
  // (after PlanJpegPixels) the launches of the pixel kernels its groups take: two per group, one per DC-only group
  size_t jpeg_pixel_launch_count() const { size_t n = 0; for (const JpegPixelGroup& g : jpeg_pixel_groups_) n += g.scaled == kJpegGroupDc ? 1 : 2; return n; }
  const JpegPixelResult* jpeg_pixel_result(int i) const { return i >= 0 && (size_t)i < jpeg_pixel_results_.size() ? &jpeg_pixel_results_[(size_t)i] : nullptr; }
  void FinishStatus(void* stream, vec<uint32_t>* per_unit);
  // Copies frame i's pixels to host memory (after Finish).
  void CopyOutputToHost(int i, void* dst, size_t size, void* stream);
  void CopyOutputRangeToHost(int i, size_t offset, void* dst, size_t size, void* stream);   // bytes [offset, offset + size) of it (one plane of OutputSpec::planes)
  // the preview of image i (JXL_DEC_PREVIEW_IMAGE): its header (the image header with the preview's size), the size of its output, the decode into host memory
  ImageHeader PreviewHeaderOf(int i) const;
  size_t PreviewOutputSize(int i, const OutputSpec& o) const;
  void DecodePreview(int i, const OutputSpec& o, void* dst, size_t cap, void* stream);
  void* device_output(int i) const;
  // Same as Run but brackets every stage with HIP events recorded on `stream` (no host sync).  CollectTimes() waits for
  // all recorded runs and returns the per-stage sums (ms) and the number of runs; used by bench.py for the roofline.
  void RunTimed(void* stream);
  void RunPart(void* stream, DecodePart part, bool timed);   // parts: decode_parts.h; the libjpeg-exact flavours come after PlanJpegPixels
  // The LF stage (kPartLf) of several prepared batches on one stream, their SIMT LF kernels as ONE launch (kernels.h LaunchLfSimtGroup).  LfKey: what the batch's next LF stage
  // launches, as lf_group_plan.h compares it (cfg as it stands: lf_wide_once, lf_spec_lanes); eligible are plain VarDCT batches — no Modular channels, no LF frames, no LF groups
  // with trees of their own — whose SIMT plan is not overridden by the wide launch.  RunLfGroup takes one group of PlanLfGroups: n = 1 is RunPart(kPartLf) — exactly those
  // launches —, n > 1 (equal eligible keys, one device; anything else throws) opens every member's timing bracket, launches the kernel once and then runs, member by member in
  // order, what follows it (LfDecodeKernel for handed-back streams, placement, the flag read-back), with after(i) behind member i.  So the group kernel's time lies inside
  // every member's "lf" bracket.
  LfGroupKey LfKey() const;
  static void RunLfGroup(Batch* const* batches, int n, void* stream, bool timed, const std::function<void(int)>& after = nullptr);
  StageTimes CollectTimes(int* runs);
  void DebugTimeline(void* ref_event, float out[kNumMarks]);
  // ALGORITHMIC bytes per stage for one Run of the batch: 0 lf, 1 lfpost, 2 hf, 3 idct, 4 filters, 5 out
  void StageBytes(uint64_t out[6]) const;
  LaunchCfg cfg;
  bool refuse_partial_unscaled = false;   // Prepare throws "truncated" for an image cut off behind its LF part (AddImage allow_partial) that is not decoded at 1:8 — callers that let
                                          // such streams in for the sake of 1:8 decodes only (JxlHipBatch*)
  size_t const_bytes() const { return const_size_; }
  size_t work_bytes() const { return work_size_ + (coef_owner_ || coef_is_ext_ ? 0 : coeff_bytes_) + (big_owner_ || big_is_ext_ ? 0 : big_size_); }
  void ShareBigArena(Batch* owner);
  void ShareCoefArena(Batch* owner);
  // Planes owned by the caller (pipeline.cc): used by the next Prepare when they are large enough for the batch's layout, otherwise the batch falls back to arenas of
  // its own (big_bytes_wanted / coef_bytes_wanted say what it would have taken).  nullptr = back to own arenas.  The caller orders the decodes that share a set.
  void UseSharedPlanes(SharedPlanes* big, SharedPlanes* coef);
  size_t big_bytes_wanted() const { return big_size_; }
  size_t coef_bytes_wanted() const { return coeff_bytes_; }
  bool uses_shared_big() const { return big_is_ext_; }
  bool uses_shared_coef() const { return coef_is_ext_; }
  // Stream-ordered form of Finish for pipelined callers: EnqueueStatusReadback copies the per-unit status words to pinned host memory behind whatever `stream` holds
  // and records an event; HarvestStatus waits for that event only and returns the words (0 = decoded).  Nothing touches the legacy NULL stream.
  void EnqueueStatusReadback(void* stream);
  void HarvestStatus(vec<uint32_t>* per_unit);
  int first_unit_of(int i) const { return pub_[i].first_unit; }
  int num_units_of(int i) const { return pub_[i].num_units; }
  int device() const { return device_; }
  int64_t Info(const std::string& name) const;
  size_t DebugRead(int i, const std::string& name, int c, void* dst, size_t cap, void* stream);
  uint64_t total_pixels() const;
  uint64_t compressed_bytes() const;

 private:
  int device_;
  vec<std::unique_ptr<ImageEntry>> images_;   // decode units (frames), in image order
  struct PubImage { int first_unit = 0, num_units = 1; bool complex = false, parsed_complex = false; };   // parsed_complex: complex as parsed, before any output promoted it
  vec<PubImage> pub_;                          // images as the caller counts them
  // ---- the phases of Prepare, in the order it calls them (decoder.cc); what they share beyond the members is in PrepareState
  struct PrepareState;
  void ResetForPrepare(); void PromoteToComplex(); void MarkComplex(PubImage& pi);
  void PutStreamTables(PrepareState& st);
  void LayOutWork(PrepareState& st);      // per unit: LayOutVarDct or LayOutModular (both through LayOutModChannels), LayOutComplexBufs
  void LayOutVarDct(int i, PrepareState& st); void LayOutModular(int i, PrepareState& st); void LayOutModChannels(int i, PrepareState& st); void LayOutComplexBufs(int i, PrepareState& st);
  void ReserveArenas(PrepareState& st);
  void SizeLocalTables(); void PreRunSingleSection(PrepareState& st);
  void PutHfTables(PrepareState& st);
  void SizeLds(); void SizePassTables();
  void PlanPlacementUnits(PrepareState& st); void PlanLfSimt(PrepareState& st);
  void PlaceResizeTable(PrepareState& st); void BuildResizeTable();
  void FillFrames(const PrepareState& st);     // per unit FillFrameDev: FillFrameCommon, then FillFrameVarDct, then FillFrameModChannels
  void FillFrameDev(int i, const uint8_t* cbase, const PrepareState& st); void FillFrameCommon(int i, const uint8_t* cbase, const PrepareState& st);
  void FillFrameVarDct(int i, const uint8_t* cbase, const PrepareState& st); void FillFrameModChannels(int i, const uint8_t* cbase, const PrepareState& st);
  void UploadDescriptors(PrepareState& st);
  void PrepareLfFrameBatch(void* stream, bool wait_upload);
  void FinishCfg();
  bool DecodedAtEighth(int unit) const;      // the unit is decoded at 1:8 (OutputSpec::downscale == 8): its decode ends behind the LF post-processing
  bool JpegDcOnlyUnit(int unit) const;       // the unit is the frame of a DC-only image (JpegDcOnly): its decode ends behind the LF decode
  bool JpegRegionUnit(int unit) const;       // the unit is the frame of an image decoded by region (jpeg_region on, JpegRegionOf): its FrameDev carries a group list
  bool EndsBehindLf(int unit) const { return DecodedAtEighth(unit) || JpegDcOnlyUnit(unit); }   // either: no HF stage, no IDCT, no filters, no coefficient or pixel planes
  // ---- frame tail of complex images
  struct ComplexBufs {      // big-arena offsets of one complex unit ((size_t)-1: not allocated)
    size_t up[3], noise[3], rgb[3], canvas[3], pa[3], pb[3];
    vec<size_t> ecf, up_ec, canvas_ec;   // per extra channel: float planes (coded size), upsampled, blended onto the canvas
    vec<size_t> ec_tmp;                  // frames with patches: one plane (coded size) per extra channel, where the patch kernel parks new values
    vec<size_t> ec_int;     // work-arena offsets of the decoded extra channels (int32, coded size)
    size_t color_int[3];            // Modular frames: work-arena offsets of the colour channels after the inverse transforms
    uint32_t nb_color_int = 0;
  };
  vec<ComplexBufs> cbufs_;
  vec<std::pair<const char*, std::function<void(void*)>>> post_ops_;   // the recorded ops, each beside the name of its stage (frame_tail.cc)
  void HashPostOps(uint64_t* h) const;
  void PostOp(const char* stage, std::function<void(void*)> op) { post_ops_.emplace_back(stage, std::move(op)); }
  // ---- LF frames: the frames that units of this batch take their LF image from are decoded by a batch of their own (each as a one-frame image that ends
  // in its XYB planes), run in front of this batch's LF post-processing; its frame tail copies the planes into the referring unit's LF planes
  struct LfTarget { float* dst[3] = {nullptr, nullptr, nullptr}; uint32_t pitch = 0, w = 0, h = 0; };
  std::unique_ptr<Batch> lf_batch_;
  vec<LfTarget> lf_targets_;                   // (of the batch that decodes LF frames: per image, where its planes go)
  vec<std::unique_ptr<JpegData>> jpeg_data_;   // per image, parsed lazily by CanReconstructJpeg
  std::vector<JpegResult> jpeg_results_;       // per image, of the last ReconstructJpegs
  std::vector<JpegPixelResult> jpeg_pixel_results_;   // per image, of the last DecodeJpegPixels
  int64_t jpeg_pixel_images_ = 0, jpeg_pixel_launches_ = 0;   // images the last DecodeJpegPixels wrote; launches of its pixel kernels (two per group of the image table, one per DC-only group)
  int64_t hf_groups_total_ = 0, hf_groups_decoded_ = 0;       // ... groups of the frames that took its HF stage, and those of them that were decoded (fewer with jpeg_region)
  bool hf_by_region_ = false;                                  // StageBytes counts by region: a libjpeg-exact decode with jpeg_region was planned (PlanJpegPixels) and no Run has enqueued an HF stage since
  int max_hf_slots_ = 0;                                       // Prepare: the most stream slots a frame fills in an HF launch that honours the lists (<= max_groups_)
  int64_t jpeg_dc_only_images_ = 0;                            // ... images of it that were written from their DC terms alone (JpegDcOutKernel)
  vec<JpegPixelImage> jpeg_pixel_table_;       // PlanJpegPixels: the image table (host copy; the upload reads it), the image of every entry, the launch groups
  vec<int> jpeg_pixel_table_image_;
  std::vector<JpegPixelGroup> jpeg_pixel_groups_;
  void FailJpegScaledOutputs(void* stream);    // Run's tail: the status words of images with OutputSpec::jpeg_scale != 1, which only DecodeJpegPixels writes
  uint8_t* djpeg_table_ = nullptr; size_t jpeg_table_cap_ = 0;   // the table on the device
  void EnqueueJpegIdct(void* stream);          // JpegIdctPlanesKernel per group, then ZeroFailedCoefKernel for the frames it failed
  void EnqueueJpegColorOut(void* stream);      // JpegColorOutKernel per group
  bool IsPlainJpegFrame(int i) const;          // the frame conditions CanReconstructJpeg and CanDecodeJpegPixels share
  struct JpegWriteState;                       // what the phases of ReconstructJpegs share (decoder.cc): the plan of the last PlanJpegWrite
  std::shared_ptr<JpegWriteState> jw_;
  uint8_t* jpeg_pinned_ = nullptr; size_t jpeg_pinned_cap_ = 0;   // pinned staging of the reconstruction's copies to the host: a head and two chunks
  void* jpeg_copy_event_[2] = {nullptr, nullptr};
  uint8_t* JpegPinned(size_t head);
  void CopyJpegToHost(void* dst, const void* src, size_t bytes, void* stream);
  int jpeg_device_images_ = 0, jpeg_host_images_ = 0, jpeg_device_progressive_images_ = 0;
  int64_t jpeg_gather_launches_ = 0;           // launches of JpegGatherKernel of the last reconstruction (one per group of the gather table)
  uint8_t* djpeg_ = nullptr; size_t jpeg_cap_ = 0;           // ReconstructJpegs: coefficient planes in JPEG layout, scan table, per-block / per-segment arrays
  uint8_t* djpeg_out_ = nullptr; size_t jpeg_out_cap_ = 0;   // ... raw and stuffed segment bytes, segment records
  bool any_complex_ = false;
  // the frame tail (frame_tail.cc): PlanPostOps walks the frames of every complex image through the stages below, which record the ops EnqueuePostOps replays
  struct TailImage; struct TailUnit;
  void PlanPostOps(HostStage& hconst, const vec<size_t>& up_weights_off);
  void TailToFloat(TailImage& im, TailUnit& t); void TailPatches(TailImage& im, TailUnit& t); void TailSplines(TailImage& im, TailUnit& t); void TailUpsample(TailImage& im, TailUnit& t);
  void TailNoise(TailUnit& t); void TailLfHandOver(TailUnit& t); void TailColour(TailImage& im, TailUnit& t); void TailOwnFrame(TailImage& im, TailUnit& t);
  void TailBlend(TailImage& im, TailUnit& t); void TailDeliver(TailImage& im, TailUnit& t, int slot);
  void TailPlanes(TailImage& im, const char* stage, const vec<size_t>& ec, uint32_t ec_stride, uint32_t w, uint32_t h);   // OutputSpec::planes: the delivery op behind LaunchWrite
  int64_t plane_outputs_planned_ = 0, plane_outputs_ = 0;   // planes the recorded ops write (PlanPostOps); planes the last decode wrote (EnqueuePostOps)
  WriteArgs TailWriteArgs(const TailImage& im, const size_t p[3], uint32_t stride, const vec<size_t>& ec, uint32_t ec_stride, uint32_t w, uint32_t h);
  void TailDeferredTf(const TailUnit& t, const char* stage, const size_t p[3], uint32_t stride, uint32_t w, uint32_t h);
  float* BigPlane(size_t off) const { return (float*)(dbig_ + off); }                                // (read when an op runs as well as when it is planned)
  const EcChanDev* EcTable(size_t off) const { return (const EcChanDev*)(dconst_ + off); }
  void EnqueuePostOps(void* stream);
  // resized outputs: per image one ResizeArgs (kernels.h), built by Prepare into a table of the constant arena — sorted by slot count, cut into groups of at most
  // resize_group_max entries — and launched group by group behind everything that writes pixels
  struct ResizePlan { int unit; size_t tab[6]; int plane = -1; };    // constant-arena offsets of the two axes' tables: lo, first, weights of x, then of y; plane >= 0: the one-slot
                                                                     // entry of requested plane `plane` of the image (OutputSpec::planes), which shares the image's tables
  vec<ResizePlan> resize_plans_;
  vec<ResizeGroup> resize_groups_;
  size_t resize_table_off_ = 0;
  int64_t resize_launches_ = 0;                      // kernel launches of the last EnqueueResizes
  int64_t resize_u8_images_ = 0;                     // ... images of it that took ResizeU8Kernel (OutputSpec::resize_u8)
  void EnqueueResizes(void* stream);
  vec<FrameDev> frames_host_;
  HostStage hconst_;
  struct ParsedImage { vec<std::unique_ptr<ImageEntry>> units; bool complex = false; };
  static void ParseImage(const uint8_t* data, size_t size, ParsedImage* out, bool allow_partial = false);
  int AddImagesImpl(const uint8_t* const* datas, const size_t* sizes, int n, int threads, bool tolerant, vec<int>* index, std::vector<std::string>* errors, bool allow_partial = false, bool only_downscalable = false,
                    bool partial_only_jpeg_dc = false);
  int Append(ParsedImage&& im);
  bool DevReserve(void** ptr, size_t* cap, size_t bytes);
  size_t const_cap_ = 0, work_cap_ = 0, big_cap_ = 0, coef_cap_ = 0, coef_laid_out_ = 0, frames_cap_ = 0, passes_cap_ = 0, local_cap_ = 0;
  uint8_t* dconst_ = nullptr; size_t const_size_ = 0;
  uint8_t* dwork_ = nullptr; size_t work_size_ = 0;
  uint8_t* dbig_ = nullptr; size_t big_size_ = 0;   // coefficient + pixel planes (rest half only); may alias big_owner_'s
  Batch* big_owner_ = nullptr; int big_sharers_ = 0;
  // The coefficient planes must be zero when the HF stage starts.  A 7 ms memset per 256 4K frames with nothing else
  // running is avoided like this: every batch has coefficient planes of its own (288 GB of HBM: three batches in flight
  // hold 82 GB of them), and a decode that is done with them clears them again on an internal stream — which the GPU
  // runs under the next batch's latency-bound HF stage.  The next decode of this batch only waits for that event.
  uint8_t* dcoef_ = nullptr;
  void* clear_stream_ = nullptr; void* clear_event_ = nullptr; void* idct_event_ = nullptr;
  bool clear_pending_ = false, coef_dirty_ = true;
  Batch* coef_owner_ = nullptr;
  size_t coef_clean_extent_ = 0;   // bytes of this object's own coefficient planes known to be zero after a completed decode
  SharedPlanes* ext_big_ = nullptr; SharedPlanes* ext_coef_ = nullptr; bool big_is_ext_ = false, coef_is_ext_ = false;
  uint32_t* status_pinned_ = nullptr; size_t status_pinned_n_ = 0; void* status_event_ = nullptr; bool status_pending_ = false;
  bool& CoefDirty() { return coef_is_ext_ ? ext_coef_->dirty : coef_owner_ ? coef_owner_->coef_dirty_ : coef_dirty_; }
  void ClearCoefficientsBeforeHf(void* stream);
  void ClearCoefficientsAfterDecode(void* stream);
  bool has_plane_b_ = false;
  uint32_t* flags_pinned_ = nullptr; size_t flags_pinned_n_ = 0; void* flags_event_ = nullptr; bool flags_pending_ = false;   // placement flags on their way to the host
  void ApplyIdctFlags(const uint32_t* flags);
  void CheckFilterBuffers() const;
  FrameDev* dframes_ = nullptr;
  PassDev* dpasses_ = nullptr;
  vec<PassDev> passes_host_;
  vec<size_t> pass_first_;
  ModLocalDev* dlocal_ = nullptr;      // descriptors of Modular sub-streams with their own tree / code (FrameDev::mod_local)
  vec<ModLocalDev> local_host_;
  vec<size_t> local_first_;
  bool any_multipass_ = false;
  size_t flags_off_ = 0, hfw_off_ = 0;
  vec<uint32_t> hf_written_;   // per unit: non-zero AC coefficients per decode (from the device counter, read by Finish)
  uint32_t decodes_since_finish_ = 0;
  bool ran_once_ = false;         // a complete decode (incl. the LF stage) has been enqueued since Prepare
  size_t coeff_bytes_ = 0, status_off_ = 0;
  bool prepared_ = false;
  int max_lf_groups_ = 0, max_groups_ = 0, max_w_ = 0, max_h_ = 0, max_bw_ = 0, max_bh_ = 0;
  bool any_vardct_ = false;
  bool any_scaled_ = false, any_full_vardct_ = false;   // some VarDCT frame is decoded at 1:8 / goes through the HF stage (a batch of 1:8 and DC-only frames skips the HF stage, the IDCT and the filters)
  FilterPlan fplan_;
  LaunchTrace trace_;             // the entropy-decode kernels the last LF / HF launch took (Info: hf_variant, lf_variant, lf_wide_bytes, lf_wide_only)
  LfSimtPlan lf_simt_;            // SIMT LF decode: device descriptors of the eligible frames' LF-group streams (cfg.lane_stride_lf < 64)
  vec<vec<size_t>> mod_plane_offsets_;   // per frame: work-arena offsets of the planes of its Modular channels
  // one kernel launch of the host-planned tail of a Modular image: inverse global transforms, then the write stage
  struct ModOp {
    enum Kind { kRct, kPalette, kSqueeze, kOutput } kind = kRct;
    size_t in[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0};   // work-arena offsets
    size_t n = 0;
    uint32_t param = 0, num_c = 0, bits = 0, aw = 0, ah = 0, rw = 0, rh = 0;
    uint32_t nb_deltas = 0, predictor = 0, wp_stride = 0; size_t wp_scratch = 0;   // palette with delta entries / a predictor
    bool has_alpha = false;
    float color_factor = 1.0f, alpha_factor = 1.0f;
    uint32_t float_bits = 0, float_exp_bits = 0;          // float samples: IntToFloatSample instead of the factor
  };
  vec<vec<ModOp>> mod_ops_;
  struct VarDctAlpha { bool has = false; size_t off = 0; float factor = 1.0f; };
  vec<VarDctAlpha> vardct_alpha_;
  bool any_modchan_ = false;      // some frame carries Modular channels (Modular frames, VarDCT frames with extra channels)
  struct ModChan;
  void EnqueueModularTail(void* stream); void RunModOp(int i, const ModOp& op, void* stream);
  void PlanModularUndo(int i, const std::function<size_t(size_t)>& take); void PlanModularOutput(int i, const vec<ModChan>& list);
  // ---- RunPart: one function per stage of the part (decode_parts.h), over what the call shares
  struct PartRun { void* stream; PartPlan plan; bool timed; vec<void*>* marks; };
  void RecordMark(const PartRun& r, Mark m);
  void StageLf(const PartRun& r) { StageLfBegin(r); StageLfRest(r, false); }
  void StageLfBegin(const PartRun& r); void StageLfRest(const PartRun& r, bool simt_launched);      // (between the two: the batch's SIMT LF launch, or the grouped one that takes it along)
  void StageLfPost(const PartRun& r); void StageHf(const PartRun& r); void StageIdct(const PartRun& r); void StagePixels(const PartRun& r);
  void EnqueueFlagReadback(void* stream); void WaitForIdctFlags(const PartRun& r);
  vec<vec<void*>> timed_events_;
  size_t timed_rest_cursor_ = 0;       // timed decodes run in parts (RunPart): which entry of timed_events_ the next "rest" part records into; CollectTimes starts it over
};

// device arena pool (decoder.cc): blocks a batch or a pipeline lets go of are kept for the next one that asks for that much memory on that device
size_t DeviceArenaPoolTrim();      // gives every pooled block back to the runtime; returns the bytes released
size_t DeviceArenaPoolHeld();
void* DeviceArenaTake(size_t want, size_t* cap, int device);
void DeviceArenaGive(void* p, size_t cap, int device, bool idle = false);   // idle: nothing on the device refers to the block (no device-wide wait)

}  // namespace jxlhip
