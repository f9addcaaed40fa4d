/* jxl_hip.h — C ABI of the MI355X-native JPEG XL decode path.
 *
 * This is the drop-in boundary: the symbols below are exactly the libjxl / libjxl_threads entry points that
 * inflation/jpegxl-rs binds through jpegxl-sys (extern "C-unwind"), with identical names, argument meaning, struct
 * layouts and status codes, exported from libjxl.so / libjxl_threads.so look-alikes so that
 * `DEP_JXL_LIB=<dir> cargo build -p jpegxl-rs` links against this implementation with zero Rust changes
 * (jpegxl-sys/build.rs:30-34).  Each declaration cites the reference line it replaces.
 * The second part (JxlHip*) is an extension without reference counterpart: a device-resident batch decode used by
 * bench.py and by batch users — the reference decodes batches by looping decode_with (jpegxl-rs/benches/decode.rs:16-19).
 */
#ifndef JXL_HIP_H_
#define JXL_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- common types (jpegxl-sys/src/common/types.rs:25-148) -------------------------------------------------------- */
typedef int JXL_BOOL;                                                     /* types.rs:25-31 */
typedef enum { JXL_TYPE_FLOAT = 0, JXL_TYPE_UINT8 = 2, JXL_TYPE_UINT16 = 3, JXL_TYPE_FLOAT16 = 5 } JxlDataType;   /* types.rs:40-55 */
typedef enum { JXL_NATIVE_ENDIAN = 0, JXL_LITTLE_ENDIAN = 1, JXL_BIG_ENDIAN = 2 } JxlEndianness;                  /* types.rs:60-72 */
typedef struct { uint32_t num_channels; JxlDataType data_type; JxlEndianness endianness; size_t align; } JxlPixelFormat; /* types.rs:83-103 */

/* jpegxl-sys/src/common/memory_manager.rs:22-64 */
typedef void* (*jpegxl_alloc_func)(void* opaque, size_t size);
typedef void (*jpegxl_free_func)(void* opaque, void* address);
typedef struct { void* opaque; jpegxl_alloc_func alloc; jpegxl_free_func free; } JxlMemoryManager;

/* jpegxl-sys/src/metadata/codestream_header.rs:38-241 (204 bytes) */
typedef enum { JXL_ORIENT_IDENTITY = 1 } JxlOrientation;
typedef struct { uint32_t xsize, ysize; } JxlPreviewHeader;
typedef struct { uint32_t tps_numerator, tps_denominator, num_loops; JXL_BOOL have_timecodes; } JxlAnimationHeader;
typedef struct {
  JXL_BOOL have_container;
  uint32_t xsize, ysize, bits_per_sample, exponent_bits_per_sample;
  float intensity_target, min_nits;
  JXL_BOOL relative_to_max_display;
  float linear_below;
  JXL_BOOL uses_original_profile, have_preview, have_animation;
  int32_t orientation;
  uint32_t num_color_channels, num_extra_channels, alpha_bits, alpha_exponent_bits;
  JXL_BOOL alpha_premultiplied;
  JxlPreviewHeader preview;
  JxlAnimationHeader animation;
  uint32_t intrinsic_xsize, intrinsic_ysize;
  uint8_t padding[100];
} JxlBasicInfo;

/* jpegxl-sys/src/decode.rs:43-54, 84-247, 284-287 */
typedef enum { JXL_SIG_NOT_ENOUGH_BYTES = 0, JXL_SIG_INVALID = 1, JXL_SIG_CODESTREAM = 2, JXL_SIG_CONTAINER = 3 } JxlSignature;
typedef enum {
  JXL_DEC_SUCCESS = 0, JXL_DEC_ERROR = 1, JXL_DEC_NEED_MORE_INPUT = 2, JXL_DEC_NEED_PREVIEW_OUT_BUFFER = 3,
  JXL_DEC_NEED_IMAGE_OUT_BUFFER = 5, JXL_DEC_JPEG_NEED_MORE_OUTPUT = 6, JXL_DEC_BOX_NEED_MORE_OUTPUT = 7,
  JXL_DEC_BASIC_INFO = 0x40, JXL_DEC_COLOR_ENCODING = 0x100, JXL_DEC_PREVIEW_IMAGE = 0x200, JXL_DEC_FRAME = 0x400,
  JXL_DEC_FULL_IMAGE = 0x1000, JXL_DEC_JPEG_RECONSTRUCTION = 0x2000, JXL_DEC_BOX = 0x4000, JXL_DEC_FRAME_PROGRESSION = 0x8000,
  JXL_DEC_BOX_COMPLETE = 0x10000
} JxlDecoderStatus;
typedef enum { JXL_COLOR_PROFILE_TARGET_ORIGINAL = 0, JXL_COLOR_PROFILE_TARGET_DATA = 1 } JxlColorProfileTarget;

/* jpegxl-sys/src/metadata/codestream_header.rs:286-388 (frame header of a displayed frame or non-coalesced layer) */
typedef enum { JXL_BLEND_REPLACE = 0, JXL_BLEND_ADD = 1, JXL_BLEND_BLEND = 2, JXL_BLEND_MULADD = 3, JXL_BLEND_MUL = 4 } JxlBlendMode;
typedef struct { JxlBlendMode blendmode; uint32_t source, alpha; JXL_BOOL clamp; } JxlBlendInfo;
typedef struct { JXL_BOOL have_crop; int32_t crop_x0, crop_y0; uint32_t xsize, ysize; JxlBlendInfo blend_info; uint32_t save_as_reference; } JxlLayerInfo;
typedef struct { uint32_t duration, timecode, name_length; JXL_BOOL is_last; JxlLayerInfo layer_info; } JxlFrameHeader;

typedef struct JxlDecoderStruct JxlDecoder;

/* jpegxl-sys/src/threads/parallel_runner.rs:46-122 */
typedef int JxlParallelRetCode;
typedef JxlParallelRetCode (*JxlParallelRunInit)(void* jpegxl_opaque, size_t num_threads);
typedef void (*JxlParallelRunFunction)(void* jpegxl_opaque, uint32_t value, size_t thread_id);
typedef JxlParallelRetCode (*JxlParallelRunner)(void* runner_opaque, void* jpegxl_opaque, JxlParallelRunInit init,
                                                JxlParallelRunFunction func, uint32_t start_range, uint32_t end_range);

/* ---- live decoder entry points (the 22 symbols jpegxl-rs/src/decode.rs calls) ----------------- */
uint32_t JxlDecoderVersion(void);                                                             /* decode.rs:370 -> 11002 */
JxlSignature JxlSignatureCheck(const uint8_t* buf, size_t len);                               /* decode.rs:385 */
JxlDecoder* JxlDecoderCreate(const JxlMemoryManager* memory_manager);                         /* decode.rs:400; on device JXL_HIP_DEVICE (default 0).  -1: a host-only decoder — headers, events up to JXL_DEC_FRAME, getters and settings need no GPU; the preview, a frame and JxlDecoderFlushImage fail, "a host-only decoder ..." */
void JxlDecoderReset(JxlDecoder* dec);                                                        /* decode.rs:408 */
void JxlDecoderDestroy(JxlDecoder* dec);                                                      /* decode.rs:414 */
JxlDecoderStatus JxlDecoderSetParallelRunner(JxlDecoder* dec, JxlParallelRunner runner, void* opaque);   /* decode.rs:487 */
JxlDecoderStatus JxlDecoderSubscribeEvents(JxlDecoder* dec, int events_wanted);               /* decode.rs:525 */
JxlDecoderStatus JxlDecoderSetKeepOrientation(JxlDecoder* dec, JXL_BOOL skip_reorientation);  /* decode.rs:563 */
JxlDecoderStatus JxlDecoderSetUnpremultiplyAlpha(JxlDecoder* dec, JXL_BOOL unpremul_alpha);   /* decode.rs:585 */
JxlDecoderStatus JxlDecoderSetRenderSpotcolors(JxlDecoder* dec, JXL_BOOL render_spotcolors);  /* decode.rs:602 */
/* decode.rs:622.  coalescing = FALSE: every regular frame of the image arrives as coded — JXL_DEC_FRAME, JXL_DEC_NEED_IMAGE_OUT_BUFFER (a buffer of
 * the FRAME's size: JxlDecoderImageOutBufferSize follows), JXL_DEC_FULL_IMAGE per frame — its pixels after the colour transform, not blended,
 * cropped frames at their own size; JxlDecoderGetFrameHeader says where it goes and how it blends. */
JxlDecoderStatus JxlDecoderSetCoalescing(JxlDecoder* dec, JXL_BOOL coalescing);
void JxlDecoderRewind(JxlDecoder* dec);                                                       /* decode.rs:438: back to the start, settings kept; set the input again */
void JxlDecoderSkipFrames(JxlDecoder* dec, size_t amount);                                    /* decode.rs:457: the next `amount` frames are not announced nor decoded */
JxlDecoderStatus JxlDecoderSkipCurrentFrame(JxlDecoder* dec);                                 /* decode.rs:472: after JXL_DEC_FRAME: do not decode this frame */
JxlDecoderStatus JxlDecoderGetFrameHeader(const JxlDecoder* dec, JxlFrameHeader* header);     /* decode.rs:1040: valid after JXL_DEC_FRAME */
JxlDecoderStatus JxlDecoderGetFrameName(const JxlDecoder* dec, char* name, size_t size);      /* decode.rs:1058 */
JxlDecoderStatus JxlDecoderGetExtraChannelBlendInfo(const JxlDecoder* dec, size_t index, JxlBlendInfo* blend_info);   /* decode.rs:1077 */
JxlDecoderStatus JxlDecoderProcessInput(JxlDecoder* dec);                                     /* decode.rs:662 — runs the HIP hot path */
JxlDecoderStatus JxlDecoderSetInput(JxlDecoder* dec, const uint8_t* data, size_t size);
/* jpegxl-sys/src/decode.rs:706: releases the input set by JxlDecoderSetInput; returns the number of bytes the decoder has not consumed
 * (everything while the headers could not be parsed yet, 0 afterwards: the decoder keeps its own copy of the codestream). */
size_t JxlDecoderReleaseInput(JxlDecoder* dec);       /* decode.rs:680 */
void JxlDecoderCloseInput(JxlDecoder* dec);                                                   /* decode.rs:724 */
JxlDecoderStatus JxlDecoderGetBasicInfo(const JxlDecoder* dec, JxlBasicInfo* info);           /* decode.rs:738 */
JxlDecoderStatus JxlDecoderGetICCProfileSize(const JxlDecoder* dec, JxlColorProfileTarget target, size_t* size);              /* decode.rs:862 */
JxlDecoderStatus JxlDecoderGetColorAsICCProfile(const JxlDecoder* dec, JxlColorProfileTarget target, uint8_t* icc, size_t size); /* decode.rs:884 */
JxlDecoderStatus JxlDecoderSetDesiredIntensityTarget(JxlDecoder* dec, float desired_intensity_target);                         /* decode.rs:921 */
JxlDecoderStatus JxlDecoderImageOutBufferSize(const JxlDecoder* dec, const JxlPixelFormat* format, size_t* size);              /* decode.rs:1100 */
JxlDecoderStatus JxlDecoderSetImageOutBuffer(JxlDecoder* dec, const JxlPixelFormat* format, void* buffer, size_t size);        /* decode.rs:1123 */
// jpegxl-sys/src/color/color_encoding.rs:125-159 and metadata/codestream_header.rs:247-279 (read-only descriptions of the image; jpegxl-rs itself reads JxlBasicInfo and the ICC profile only)
typedef struct {
  int color_space;                 // JxlColorSpace: 0 RGB, 1 grey, 2 XYB, 3 unknown
  int white_point;                 // JxlWhitePoint: 1 D65, 2 custom, 10 E, 11 DCI
  double white_point_xy[2];
  int primaries;                   // JxlPrimaries: 1 sRGB, 2 custom, 9 BT.2100, 11 P3
  double primaries_red_xy[2], primaries_green_xy[2], primaries_blue_xy[2];
  int transfer_function;           // JxlTransferFunction: 1 BT.709, 2 unknown, 8 linear, 13 sRGB, 16 PQ, 17 DCI, 18 HLG, 65535 gamma
  double gamma;
  int rendering_intent;            // 0 perceptual, 1 relative, 2 saturation, 3 absolute
} JxlColorEncoding;
typedef struct {
  int type;                        // JxlExtraChannelType: 0 alpha, 1 depth, 2 spot colour, 3 selection mask, 4 black, 5 CFA, 6 thermal, 15 unknown, 16 optional
  uint32_t bits_per_sample, exponent_bits_per_sample, dim_shift, name_length;
  JXL_BOOL alpha_premultiplied;
  float spot_color[4];
  uint32_t cfa_channel;
} JxlExtraChannelInfo;
// decode.rs:833: the colour encoding as enumerated values (error for images that carry an ICC profile instead: JxlDecoderGetColorAsICCProfile is the way then)
JxlDecoderStatus JxlDecoderGetColorAsEncodedProfile(const JxlDecoder* dec, JxlColorProfileTarget target, JxlColorEncoding* color_encoding);
// decode.rs:756 / :777
JxlDecoderStatus JxlDecoderGetExtraChannelInfo(const JxlDecoder* dec, size_t index, JxlExtraChannelInfo* info);
JxlDecoderStatus JxlDecoderGetExtraChannelName(const JxlDecoder* dec, size_t index, char* name, size_t size);
// decode.rs:509: bytes of input that make JxlDecoderGetBasicInfo likely to succeed; decode.rs:1495: the whole image is always decoded (ratio 1)
size_t JxlDecoderSizeHintBasicInfo(const JxlDecoder* dec);
size_t JxlDecoderGetIntendedDownsamplingRatio(const JxlDecoder* dec);
// jpegxl-sys/src/decode.rs:999-1025: the preview image (JXL_DEC_PREVIEW_IMAGE / JXL_DEC_NEED_PREVIEW_OUT_BUFFER; JxlBasicInfo.have_preview, .preview) — the preview frame is
// decoded on the GPU like an image of its own.  jpegxl-rs itself never subscribes to it (decode.rs:334-347).
JxlDecoderStatus JxlDecoderPreviewOutBufferSize(const JxlDecoder* dec, const JxlPixelFormat* format, size_t* size);
JxlDecoderStatus JxlDecoderSetPreviewOutBuffer(JxlDecoder* dec, const JxlPixelFormat* format, void* buffer, size_t size);
/* Pixel output through a callback instead of a buffer (decode.rs:289-309, :1172): called once per row (x = 0, num_pixels = xsize) from
 * the thread inside JxlDecoderProcessInput after the image has been decoded; the row memory is only valid during the call. */
typedef void (*JxlImageOutCallback)(void* opaque, size_t x, size_t y, size_t num_pixels, const void* pixels);
JxlDecoderStatus JxlDecoderSetImageOutCallback(JxlDecoder* dec, const JxlPixelFormat* format, JxlImageOutCallback callback, void* opaque);   /* decode.rs:1172 */
/* decode.rs:1200 (callback types :324-361): the rows are handed out after the image has been decoded on the device — init(init_opaque, 1 thread,
 * xsize pixels per call), run(..., thread 0, x = 0, y, xsize, row) for every row, destroy. */
typedef void* (*JxlImageOutInitCallback)(void* init_opaque, size_t num_threads, size_t num_pixels_per_thread);
typedef void (*JxlImageOutRunCallback)(void* run_opaque, size_t thread_id, size_t x, size_t y, size_t num_pixels, const void* pixels);
typedef void (*JxlImageOutDestroyCallback)(void* run_opaque);
JxlDecoderStatus JxlDecoderSetMultithreadedImageOutCallback(JxlDecoder* dec, const JxlPixelFormat* format, JxlImageOutInitCallback init_callback,
                                                            JxlImageOutRunCallback run_callback, JxlImageOutDestroyCallback destroy_callback, void* init_opaque);
/* decode.rs:1224 / :1258: a separate plane for an extra channel (one sample per pixel in `format`'s type, num_channels ignored), any of the image's extra channels: each
 * plane costs one more pass of the frame with that channel in the alpha slot of the interleaved output. */
JxlDecoderStatus JxlDecoderExtraChannelBufferSize(const JxlDecoder* dec, const JxlPixelFormat* format, size_t* size, uint32_t index);
JxlDecoderStatus JxlDecoderSetExtraChannelBuffer(JxlDecoder* dec, const JxlPixelFormat* format, void* buffer, size_t size, uint32_t index);
/* decode.rs:1326-1470: the boxes of the container (JXL_DEC_BOX once per box, signature and codestream boxes included; contents through a caller buffer with
 * JXL_DEC_BOX_NEED_MORE_OUTPUT when it is full; `brob` boxes decompressed on request when the system has libbrotlidec).  Boxes up to the first codestream
 * box are announced before JXL_DEC_BASIC_INFO, the others after the last frame. */
typedef struct { char type[4]; } JxlBoxType;                                                  /* types.rs:147 */
JxlDecoderStatus JxlDecoderSetBoxBuffer(JxlDecoder* dec, uint8_t* data, size_t size);
size_t JxlDecoderReleaseBoxBuffer(JxlDecoder* dec);
JxlDecoderStatus JxlDecoderSetDecompressBoxes(JxlDecoder* dec, JXL_BOOL decompress);
JxlDecoderStatus JxlDecoderGetBoxType(JxlDecoder* dec, JxlBoxType* type, JXL_BOOL decompressed);
JxlDecoderStatus JxlDecoderGetBoxSizeRaw(JxlDecoder* dec, uint64_t* size);
JxlDecoderStatus JxlDecoderGetBoxSizeContents(JxlDecoder* dec, uint64_t* size);
/* decode.rs:1482: which JXL_DEC_FRAME_PROGRESSION events are wanted (0 frames, 1 DC, 2 last passes, 3 passes are accepted, the finer ones rejected like libjxl
 * does); frames are decoded whole on the device, so no progression event is ever emitted.  decode.rs:1513: nothing partial exists to flush: JXL_DEC_ERROR
 * ("no flush was done"), as libjxl answers when no new image data is available. */
JxlDecoderStatus JxlDecoderSetProgressiveDetail(JxlDecoder* dec, int detail);
JxlDecoderStatus JxlDecoderFlushImage(JxlDecoder* dec);
/* decode.rs:1528 (types.rs:111-144): integer output is scaled to the full range of the buffer's type by default (JXL_BIT_DEPTH_FROM_PIXEL_FORMAT = 0); FROM_CODESTREAM (1) /
 * CUSTOM (2): samples in [0, 2^bits - 1] (the write stage's multiplier), bits <= the sample type's; float buffers keep their values.  Call after the image out buffer is set;
 * the setting lasts for that buffer. */
typedef struct { int type; uint32_t bits_per_sample, exponent_bits_per_sample; } JxlBitDepth;
JxlDecoderStatus JxlDecoderSetImageOutBitDepth(JxlDecoder* dec, const JxlBitDepth* bit_depth);
JxlDecoderStatus JxlDecoderSetJPEGBuffer(JxlDecoder* dec, uint8_t* data, size_t size);        /* decode.rs:1283 */
size_t JxlDecoderReleaseJPEGBuffer(JxlDecoder* dec);                                          /* decode.rs:1305 */

/* ---- libjxl_threads (threads/thread_parallel_runner.rs:44-65, resizable_parallel_runner.rs:42-67) ---------------- */
JxlParallelRetCode JxlThreadParallelRunner(void* runner_opaque, void* jpegxl_opaque, JxlParallelRunInit init, JxlParallelRunFunction func,
                                           uint32_t start_range, uint32_t end_range);
void* JxlThreadParallelRunnerCreate(const JxlMemoryManager* memory_manager, size_t num_worker_threads);
void JxlThreadParallelRunnerDestroy(void* runner_opaque);
size_t JxlThreadParallelRunnerDefaultNumWorkerThreads(void);
JxlParallelRetCode JxlResizableParallelRunner(void* runner_opaque, void* jpegxl_opaque, JxlParallelRunInit init, JxlParallelRunFunction func,
                                              uint32_t start_range, uint32_t end_range);
void* JxlResizableParallelRunnerCreate(const JxlMemoryManager* memory_manager);
void JxlResizableParallelRunnerSetThreads(void* runner_opaque, size_t num_threads);
uint32_t JxlResizableParallelRunnerSuggestThreads(uint64_t xsize, uint64_t ysize);
void JxlResizableParallelRunnerDestroy(void* runner_opaque);

/* The remaining symbols declared by jpegxl-sys (encoder, CMS, gain map, output colour profile ...) are exported as
 * error-returning stubs so the Rust crate links (csrc/jxl_stubs.cc, generated by tools/gen_stubs.py). */

/* ---- extension: device-resident batch decode ------------------------------------------------------------------- */
typedef struct JxlHipBatchStruct JxlHipBatch;
typedef struct {
  float lf_ms, lfpost_ms, hf_ms, idct_ms, filter_ms, out_ms, total_ms;
} JxlHipStageTimes;

/* Last error message of the calling thread ("" if none). */
const char* JxlHipLastError(void);
/* Lets `batch` use `owner`'s coefficient and pixel planes instead of allocating its own (they are only touched by part 2 of a
 * decode, so two batches whose part-2 halves run one after the other on one stream can share them: halves device memory of a
 * double-buffered pipeline).  Call before JxlHipBatchPrepare(batch); owner must be prepared, at least as large, and outlive batch. */
int JxlHipBatchShareBuffers(JxlHipBatch* batch, JxlHipBatch* owner);
/* The same for the quantised-coefficient planes (written by the HF stage of a decode, consumed and zeroed again by its IDCT stage): batches
 * whose [HF ... IDCT] intervals never overlap may use one set.  A deep pipeline alternates between two owners, so that the HF stage of
 * batch k + 1 runs beside the IDCT of batch k.  Call before JxlHipBatchPrepare(batch); owner must be prepared, at least as large, and
 * outlive batch.  Without it every batch holds planes of its own (106 MB per 4K frame). */
int JxlHipBatchShareCoefficients(JxlHipBatch* batch, JxlHipBatch* owner);
/* Host-only: parses the signature/container and image header of `data` and writes the ICC profile JxlDecoderGetColorAsICCProfile
 * would return (pass icc_out == NULL to query *icc_size).  Needs no GPU.  Returns 0 on success. */
int JxlHipColorProfileFromHeaders(const uint8_t* data, size_t size, uint8_t* icc_out, size_t* icc_size);
/* Host-only (needs no GPU): the dequantisation table (1 / weight, libjxl's coefficient layout) the decoder uses for library-default
 * quantisation kind `kind` (0..16, quant_weights.h), channel c (0 X, 1 Y, 2 B).  Writes min(n, cap) floats, returns n (0 on error). */
size_t JxlHipLibraryQuantTable(int kind, int c, float* out, size_t cap);
/* Host-only (needs no GPU): the serialisation half of JPEG reconstruction — parses a `jbrd` box payload and writes the JPEG file from
 * quantised coefficients (components x blocks x 64 int16, natural order, 4:4:4) and quantisation tables (components x 64, natural order).
 * *out_size: capacity in, bytes needed / written out.  Returns 0 on success, 2 if the buffer is too small, 1 on error. */
int JxlHipDebugWriteJpeg(const uint8_t* jbrd, size_t jbrd_size, uint32_t width, uint32_t height, const int16_t* coefficients, const int32_t* quant_tables,
                         uint8_t* out, size_t* out_size);
/* Same with JPEG sampling factors: sampling = (h, v) per component (NULL = all 1x1); the component planes follow one another, each
 * (mcu_rows * v) x (mcu_cols * h) blocks, the MCU grid being ceil(size / (8 * max factor)). */
int JxlHipDebugWriteJpegSampled(const uint8_t* jbrd, size_t jbrd_size, uint32_t width, uint32_t height, const uint32_t* sampling, const int16_t* coefficients,
                                const int32_t* quant_tables, uint8_t* out, size_t* out_size);
/* Host-only (no GPU): parse everything the host side parses and describe the image / its frames, one line each, into out
   (NUL-terminated, truncated to cap).  0 = accepted, 1 = rejected (JxlHipLastError()). */
int JxlHipDebugDescribe(const uint8_t* data, size_t size, char* out, size_t cap);
/* Creates a batch bound to HIP device `device`. */
JxlHipBatch* JxlHipBatchCreate(int device);   /* device -1: a host-only batch (no GPU needed) — images are parsed, outputs set, the host-only queries answered; it cannot be prepared or decoded */
void JxlHipBatchDestroy(JxlHipBatch* batch);
/* Parses one image (headers, TOC, global tables) and appends it; returns its index or -1. */
int JxlHipBatchAddImage(JxlHipBatch* batch, const uint8_t* data, size_t size);
/* The same for `n` images at once, parsed on `num_threads` host threads (the per-image work — container, headers, TOC, entropy-code tables
 * of the global sections — is independent) and appended in order.  Returns the index of the first image, -1 on error (nothing is appended
 * then).  What a streaming caller feeds fresh compressed frames with, step after step. */
int JxlHipBatchAddImages(JxlHipBatch* batch, const uint8_t* const* datas, const size_t* sizes, int n, int num_threads);
/* Forgets the images of the batch but keeps its device arenas, its pinned staging buffer and the sharing set up with JxlHipBatchShare*:
 * the object can be filled (AddImage(s), SetOutput) and prepared again without allocating.  No decode of the old content may be in flight. */
void JxlHipBatchReset(JxlHipBatch* batch);
/* Basic info / required output size of image `index` for `format`. */
JxlDecoderStatus JxlHipBatchGetBasicInfo(const JxlHipBatch* batch, int index, JxlBasicInfo* info);
JxlDecoderStatus JxlHipBatchOutBufferSize(const JxlHipBatch* batch, int index, const JxlPixelFormat* format, size_t* size);
/* Output format (and optional caller-owned *device* destination; NULL = batch-owned) of image `index`. */
JxlDecoderStatus JxlHipBatchSetOutput(JxlHipBatch* batch, int index, const JxlPixelFormat* format, void* device_buffer);
/* ---- the 1:8 decode (thumbnails) --------------------------------------------------------------------------------------------------
 * downscale = 8: the image comes out at ceil(xsize / 8) x ceil(ysize / 8) pixels, one per 8x8 block — the frame's LF image, which the format stores in front of
 * the AC groups.  Output pixel (bx, by) is LF sample (bx, by) of each channel after LF dequantisation and (unless the frame header skips it) adaptive LF smoothing —
 * exactly what the IDCT stage reads as its lowest-frequency input — through the per-pixel tail of the full decode: inverse opsin / YCbCr -> RGB / identity, transfer
 * function, grey handling, then the write stage with every output type, byte order, row alignment and bit depth.  Gaborish, EPF and noise are defined on
 * full-resolution pixels and are not applied.  Chroma-subsampled YCbCr frames (JPEG transcodes): a channel with shift (hs, vs) is sampled on the LF grid with the
 * (1/4, 3/4) taps of the full decode's chroma upsampling, horizontal then vertical, clamped at the channel's own edges.  The alpha slot of 2- / 4-channel output is
 * 1.0.  The orientation is applied to the small picture as the full decode applies it to the large one (unless kept).  No AC coefficient is decoded, no IDCT and no
 * filter runs, and a batch of such images only allocates neither coefficient nor pixel planes; the stream may end anywhere behind its LF part (LfGlobal, the LfGroups
 * and HfGlobal: JxlHipBatchSetOption("allow_partial", 1) before adding such a prefix to a batch; pipeline jobs take them as they are) and decodes to the same bytes as
 * the whole file.  Taken: single-frame VarDCT images with their own LF coefficients, without extra channels, patches, splines, noise or upsampling; anything else
 * fails with "unsupported: downscaled decode of ...".  downscale = 1 is the call without the suffix; any other value returns JXL_DEC_ERROR (-1 from Submit) with a
 * message in JxlHipLastError().  A batch may mix scaled and unscaled images. */
JxlDecoderStatus JxlHipBatchOutBufferSizeScaled(const JxlHipBatch* batch, int index, const JxlPixelFormat* format, int downscale, size_t* size);
JxlDecoderStatus JxlHipBatchSetOutputScaled(JxlHipBatch* batch, int index, const JxlPixelFormat* format, void* device_buffer, int downscale);
/* ---- output layout: planar (CHW) planes and a per-channel scale and bias ---------------------------------------------------------
 * A JxlPixelFormat describes interleaved samples.  JxlHipOutputLayout beside it puts every channel slot into a plane of its own and / or stores float samples as
 * v x scale + bias, so that a consumer of [N, C, H, W] tensors, normalised per channel, needs no second pass over the decoded pixels.
 *   planar        the sample of slot c at oriented position (ox, oy) goes to out + c * plane_stride + oy * row_stride + ox * bytes_per_sample.  Slots in the order of the
 *                 interleaved samples: grey (or G) then alpha for 1 / 2 channels, R G B then alpha for 3 / 4.  row_stride = oriented width x sample size rounded up to
 *                 format->align; the output is num_channels x plane_stride bytes.
 *   plane_stride  0 = tight (oriented height x row_stride); else at least that and a multiple of the sample size, or the call fails with a message.
 *   affine        float16 / float32 output only (an integer type fails: "affine output needs a float sample type"): slot c is stored as fmaf(v, scale[c], bias[c]) in
 *                 float32, v being the sample a call without it stores; applies to interleaved and planar output alike.  affine = 0: scale / bias are not read.
 * A NULL layout is the call without the suffix.  Orientation, keep_orientation, byte order, bit depth and downscale (1 or 8) keep their meaning.  Taken by batches and
 * pipelines, device and pinned-host destinations, every image kind those decode.  The libjxl API above (JxlDecoder*), previews and animation canvases stay interleaved. */
typedef struct { JXL_BOOL planar; size_t plane_stride; JXL_BOOL affine; float scale[4]; float bias[4]; } JxlHipOutputLayout;
JxlDecoderStatus JxlHipBatchOutBufferSizeLayout(const JxlHipBatch* batch, int index, const JxlPixelFormat* format, int downscale, const JxlHipOutputLayout* layout, size_t* size);
JxlDecoderStatus JxlHipBatchSetOutputLayout(JxlHipBatch* batch, int index, const JxlPixelFormat* format, void* device_buffer, int downscale, const JxlHipOutputLayout* layout);
/* ---- output of a requested size: antialiased resize, and crop, at the write stage -------------------------------------------------------------
 * JxlHipOutputResize makes the output xsize x ysize pixels whatever the image's size, so that a job of differently sized images lands in one [N, C, H, W] tensor.
 * The source of the resize is the picture the call without it would have written: after the orientation (or as stored, keep_orientation), at downscale 1 or 8; the
 * crop rectangle is in that picture's coordinates (crop_xsize = crop_ysize = 0 and a zero origin: all of it) and the result is exactly that of cropping first.  Every
 * channel slot is resampled separately, horizontally then vertically in float32, with the triangle filter with half-pixel centres, widened by the ratio where it shrinks:
 * per axis with n_in source and n_out target samples, scale = n_in / n_out, support = max(scale, 1), target sample i is centred at c = scale x (i + 0.5) and is the
 * weighted mean of the source samples j in [max(0, int(c - support + 0.5)), min(n_in, int(c + support + 0.5))) with weights max(0, 1 - |(j - c + 0.5) / support|) —
 * the filter of Pillow's BILINEAR resize and of torch.nn.functional.interpolate(mode="bilinear", antialias=True, align_corners=False).  At the edges the range is cut
 * and the weights are renormalised.  The filtered float32 sample is then stored like any other: sample type, byte order, bit depth, align, planar / plane_stride and
 * scale / bias of `format` and `layout` keep their meaning, and the sizes the calls report are those of an xsize x ysize picture.
 * Refused with a message in JxlHipLastError(): a target side of 0 or above 65535, an empty crop, a crop that leaves the picture (known per image: such an image of a pipeline
 * job fails alone).  A NULL resize is the ...Layout call.  The resize does not choose `downscale`: ask for 8 together with a small target for the cost of a thumbnail.
 * The picture is decoded whole, into a float32 intermediate of the batch's own (counted by JxlHipBatchDeviceBytes), whatever the crop. */
typedef struct { uint32_t xsize, ysize; uint32_t crop_x0, crop_y0, crop_xsize, crop_ysize; } JxlHipOutputResize;
JxlDecoderStatus JxlHipBatchOutBufferSizeResized(const JxlHipBatch* batch, int index, const JxlPixelFormat* format, int downscale, const JxlHipOutputLayout* layout,
                                                 const JxlHipOutputResize* resize, size_t* size);
JxlDecoderStatus JxlHipBatchSetOutputResized(JxlHipBatch* batch, int index, const JxlPixelFormat* format, void* device_buffer, int downscale, const JxlHipOutputLayout* layout,
                                             const JxlHipOutputResize* resize);
/* ---- resampled output: the resize above with a filter and a mirror of the image's own --------------------------------------------------------------------
 * JxlHipOutputResample is JxlHipOutputResize — same meaning of xsize, ysize and the crop, same refusals — with two more choices:
 *   filter   0 = the antialiased triangle filter of JxlHipOutputResize; 1 = antialiased cubic convolution with a = -0.5, the filter of Pillow's BICUBIC resize and of
 *            torch.nn.functional.interpolate(mode="bicubic", antialias=True, align_corners=False).  Any other value is refused.
 *            Both are one rule per axis with a kernel k of radius r (triangle: k(x) = max(0, 1 - |x|), r = 1; cubic: k(x) = ((a + 2)|x| - (a + 3))|x|^2 + 1 for |x| < 1,
 *            a(((|x| - 5)|x| + 8)|x| - 4) for 1 <= |x| < 2, 0 beyond, r = 2): with n_in source and n_out target samples, scale = n_in / n_out, s = max(scale, 1), target
 *            sample i is centred at c = scale x (i + 0.5) and takes the source samples j of [max(0, int(c - r x s + 0.5)), min(n_in, int(c + r x s + 0.5))) with the weights
 *            k((j - c + 0.5) / s) over their sum: at the edges the range is cut and the weights renormalised.  Weights are computed and normalised in double and rounded
 *            to float32 once; the sums are float32, horizontally then vertically.  The cubic's negative lobes let a float result leave the range of its samples; integer
 *            sample types clamp it.  A target of the source's size is a bit-exact copy with either filter.
 *   mirror   target column ox of the resampled picture is stored at column xsize - 1 - ox: a horizontal flip of the finished target, after crop, orientation and
 *            resize — exactly the output without mirror with its columns reversed, in every sample type and layout.
 * filter = 0, mirror = 0 is the ...Resized call, byte for byte.  A pipeline job takes one JxlHipOutputResample per image (each[i] belongs to image i): crop, filter and
 * mirror are the image's own; xsize x ysize must be the same in all n entries (the destinations are slices of one tensor, JxlHipImageOutSizeResized bytes each), else the
 * submission is refused, as it is for a NULL `each`, a filter above 1 and everything JxlHipPipelineSubmitResized refuses.  An image its crop leaves fails alone.
 * The resizes of one decode are launched together: one launch pair (horizontal, vertical) per group of images with the same number of channel slots.
 * JxlHipBatchGetInfo(batch, "resize_launches") is the number of resize launches of the last decode. */
typedef struct { uint32_t xsize, ysize, crop_x0, crop_y0, crop_xsize, crop_ysize; uint32_t filter; JXL_BOOL mirror; } JxlHipOutputResample;
JxlDecoderStatus JxlHipBatchOutBufferSizeResampled(const JxlHipBatch* batch, int index, const JxlPixelFormat* format, int downscale, const JxlHipOutputLayout* layout,
                                                   const JxlHipOutputResample* resample, size_t* size);
JxlDecoderStatus JxlHipBatchSetOutputResampled(JxlHipBatch* batch, int index, const JxlPixelFormat* format, void* device_buffer, int downscale, const JxlHipOutputLayout* layout,
                                               const JxlHipOutputResample* resample);
/* ---- extra-channel planes beside the colour output, all from one decode ---------------------------------------------------------------------------------
 * JxlHipOutputPlanes asks for extra channels of the image — depth, masks, spectral bands, any channel by its index, indices may repeat — as planes of one sample per
 * pixel behind the colour output of the same destination.  Plane k holds channel extra_index[k] "as it is": of the coalesced canvas (or of the frame's own planes for a
 * non-coalesced output), converted by the channel's own bit depth (float channels through their bit pattern), never un-premultiplied, untouched by spot-colour
 * rendering and by the output bit depth.  Its sample type, byte order and row alignment are those of the colour output's JxlPixelFormat; its geometry follows the
 * colour output: orientation (or keep_orientation) and, with a resized output, the same crop, target size, filter and mirror, each plane resampled on its own.
 *   offset        where plane 0 starts in the destination.  0 = num_channels x plane_stride behind a planar colour output, so that colour and extras form one
 *                 [C + m, H, W] block; behind an interleaved one the colour size rounded up to 16 bytes.
 *   plane_stride  bytes from plane k to plane k + 1.  0 = the layout's plane_stride when the colour is planar, else tight (rows x aligned row pitch).
 *                 Either may be given: at least its default and a multiple of the sample size, or the call fails with a message.
 *   scale, bias   NULL, or num_planes values: float16 / float32 plane k is stored as fmaf(v, scale[k], bias[k]) (a NULL one of the two: 1 / 0).
 * The destination is offset + num_planes x plane_stride bytes: JxlHipBatchOutputPlanesLayout (host only) and JxlHipImageOutSizePlanes say so; the capacity checks of a
 * pipeline job include the planes.  JxlHipBatchSetOutputPlanes is called after the JxlHipBatchSetOutput... call of that image, whose device buffer then takes both; a
 * later JxlHipBatchSetOutput... call clears the planes, as do a NULL `planes` or num_planes = 0.  At most 4096 planes.
 * An image with requested planes takes the frame tail (the path of layered, patched and animated images): EcPlanesOutKernel writes every plane of it in one launch
 * behind the colour write, whatever their number — no decode per plane.  JxlHipBatchGetInfo(batch, "plane_outputs"): planes the last decode wrote.
 * Refused, "unsupported: extra planes ..." in JxlHipLastError() (an image of a pipeline job fails alone): an index at or beyond the image's number of extra channels;
 * scale / bias with an integer sample type; downscale 8; libjpeg-exact outputs (jpeg_scale, the integer resample); kept animation canvases ("output_all_frames").
 * Jobs of libjpeg-exact pixels (JxlHipPipelineSubmitJpegPixels...) and previews (JxlDecoderSetPreviewOutBuffer) have no argument that carries planes.
 * Host destinations (host_out of a pipeline job, JxlHipBatchCopyOutput) receive the destination as one run of `total` bytes: the bytes between the colour output and
 * plane 0 — up to 15 behind an interleaved colour output, more under an explicit offset — and behind each plane's rows under an explicit plane_stride are overwritten
 * with unspecified values, as the gaps of a padded planar layout are.  A device destination is written at the samples alone. */
typedef struct { uint32_t num_planes; const uint32_t* extra_index; size_t offset; size_t plane_stride; const float* scale; const float* bias; } JxlHipOutputPlanes;
/* The libjxl API: the buffers of JxlDecoderSetExtraChannelBuffer are served by the frame's main decode, each in its own JxlPixelFormat, when the image takes the frame
 * tail under its colour output anyway (several frames, patches, splines, noise, rendered spot colours, non-coalesced output, un-premultiplied alpha) and its canvases
 * are not kept from one decode of an animation; every other image still takes one more decode per buffer.  JxlHipDecoderInfo(decoder, "frame_decodes"): the decodes
 * the last delivered frame took (1 + the buffers served by a decode of their own; 0: the frame came from kept canvases); -1 for an unknown name. */
int64_t JxlHipDecoderInfo(const JxlDecoder* decoder, const char* name);
JxlDecoderStatus JxlHipBatchSetOutputPlanes(JxlHipBatch* batch, int index, const JxlHipOutputPlanes* planes);
JxlDecoderStatus JxlHipBatchOutputPlanesLayout(const JxlHipBatch* batch, int index, size_t* offset, size_t* plane_stride, size_t* total);
/* JxlHipImageOutSizeResized with a filter-and-mirror resample (NULL: the image's own size) and the planes: *out_size is the whole destination */
JxlDecoderStatus JxlHipImageOutSizePlanes(const uint8_t* data, size_t size, const JxlPixelFormat* format, int downscale, const JxlHipOutputLayout* layout,
                                          const JxlHipOutputResample* resample, const JxlHipOutputPlanes* planes, JxlBasicInfo* info, size_t* out_size);
/* ---- output colour: decode to a requested colour encoding ----------------------------------------------------------------------------------------------------------
 * Every image is decoded into the encoding its own header names; JxlHipOutputColor asks for another one, so that a job of sRGB, Display-P3, PQ and HLG files lands in one
 * space.  The rule:
 *   linear light  display light with 1.0 = the image's intensity_target (what the XYB -> linear stage produces).  The intensity target is always the image's own; a
 *                 target encoding never changes it.  No gamut mapping and no tone mapping: what leaves the target's range clips at the write stage (float output keeps it).
 *   target        a JxlColorEncoding with color_space 0 (RGB) or 1 (grey), any white point / primaries (enumerated or custom xy: the xy fields count under the custom
 *                 enums only) and transfer function 1, 8, 13, 16, 17, 18 or 65535 (gamma in (0, 1], kept in units of 1e-7 as the codestream keeps it).  Refused with a
 *                 message: color_space 2 / 3, transfer function 2, a chromaticity with y <= 0, singular primaries, a grey target for a colour image or the reverse.
 *   XYB images    come out exactly — bit for bit — as the same codestream under a header that names the target at the same intensity target: the inverse opsin matrix is
 *                 multiplied by inv(AdaptToXyzD50(w_t) x PrimariesToXyz(p_t, w_t)) x AdaptToXyzD50(D65) x PrimariesToXyz(sRGB, D65) in double and rounded to float32 once,
 *                 the target's luminances feed the HLG inverse OOTF, and the transfer function — hence the kernel: sRGB and linear targets take the fused filter kernel, the
 *                 others the stage-by-stage one — follows from the target.  An embedded ICC profile does not matter: XYB pixels are absolute.
 *   other images  (lossless Modular RGB, YCbCr transcodes) keep their samples under non_xyb = 0, libjxl's rule.  Under non_xyb = 1 an image with enumerated encoding A is
 *                 converted to the target T per pixel, behind blending and spot colours, in float32: A's transfer function undone to linear light; the matrix
 *                 inv(AdaptToXyzD50(w_T) x PrimariesToXyz(p_T, w_T)) x AdaptToXyzD50(w_A) x PrimariesToXyz(p_A, w_A) (double, rounded once; left out between equal
 *                 chromaticities); T's transfer function as for XYB images.  Inverse transfer functions: sRGB (IEC 61966-2-1), Rec.709, gamma; PQ: the ST 2084 EOTF x
 *                 10000 / intensity_target; HLG: the BT.2100 inverse OETF, then the OOTF display = scene x Y_s^(gamma - 1) with gamma = 1.2 x 1.111^log2(intensity_target /
 *                 1000) and Y_s from A's primaries, skipped in the band the forward path skips its inverse in (|1 / gamma - 1| <= 0.01).  Negative samples: odd extension;
 *                 gamma gives 0 at or below 1e-5.  A grey image converts its transfer function only.  T equal to A (the same xy and transfer function; linear = gamma 1,
 *                 DCI = gamma 1 / 2.6): nothing happens, the image takes the path and gives the bytes of the plain decode.  Such an image takes the frame tail (ColorKernel).
 *                 An image whose colour is only an ICC profile fails, "unsupported: output colour of an image whose colour is an ICC profile needs a CMS".  So does one whose own encoding cannot
 *                 be taken to linear light (an unknown transfer function or colour space): "unsupported: output colour of an image whose own encoding cannot be converted ...".
 * JxlHipBatchSetOutputColor is called after the JxlHipBatchSetOutput... call of that image, like JxlHipBatchSetOutputPlanes; a later JxlHipBatchSetOutput... call or a
 * NULL clears it; a refused call leaves the output that was set.  downscale 8, every layout, resize and extra planes compose with it (planes are never colour-converted).
 * Refused, "unsupported: output colour ...": libjpeg-exact outputs (jpeg_scale, the integer resample: those are libjpeg's samples; jobs of libjpeg-exact pixels have no
 * argument that carries a colour); non_xyb = 1 on kept animation canvases ("output_all_frames") of an image that is not XYB.
 * JxlHipColorConversionMatrix (host only): the row-major linear-light matrix of the rule from `from` to `to`, in double; the identity, exactly, between equal
 * chromaticities.  Returns 0, or 1 with a message for an encoding the rule refuses. */
/* The libjxl-style decoder takes the same request through JxlHipDecoderSetOutputColorProfile, which has the argument list and the contract of libjxl's call of that name for a
 * decoder without a CMS (jpegxl-sys decode.rs:891-973): XYB images come out in the encoding, images that are not XYB keep their samples and the call still succeeds, a
 * non-NULL icc_data is JXL_DEC_ERROR (it needs a CMS).  Call it between JXL_DEC_COLOR_ENCODING and the first frame: JXL_DEC_ERROR with a message before the headers are known,
 * after the frame decode (or a progressive flush) has begun — so an animation decoded once keeps one target —, without an encoding, and for everything the rule above
 * refuses.  Afterwards JxlDecoderGetColorAsEncodedProfile and the two ICC profile calls with target DATA describe the requested encoding for XYB images, also for those with
 * an embedded ICC profile, and ORIGINAL stays the image's own; JxlDecoderFlushImage shows the target's pixels.  JxlDecoderReset clears the request, JxlDecoderRewind keeps it.
 * libjxl's own pair of names for this stays among the error-returning stubs (csrc/jxl_stubs.cc) beside the CMS hook: the ABI test pins that list, and a caller that links
 * against libjxl's names gets the answer it got before.  Forwarding them here is one line each. */
typedef struct { JxlColorEncoding encoding; uint32_t non_xyb; } JxlHipOutputColor;
JxlDecoderStatus JxlHipDecoderSetOutputColorProfile(JxlDecoder* dec, const JxlColorEncoding* color_encoding, const uint8_t* icc_data, size_t icc_size);
JxlDecoderStatus JxlHipBatchSetOutputColor(JxlHipBatch* batch, int index, const JxlHipOutputColor* color);
int JxlHipColorConversionMatrix(const JxlColorEncoding* from, const JxlColorEncoding* to, double m[9]);
/* JPEG bit-stream reconstruction of a whole batch (jpegxl-rs decode.rs:493 `reconstruct`, for many files at once).  JxlHipBatchCanReconstructJpeg: 1 if image
 * `index` is a lossless JPEG transcode with usable reconstruction data (a `jbrd` box whose markers find their ICC / Exif / XMP payloads, a Huffman-coded source),
 * else 0 with the reason in JxlHipLastError().  JxlHipBatchReconstructJpegs runs the LF and HF entropy stages once for all images of the batch (it prepares the batch
 * if need be; no image needs an output set) and writes the files: sequential Huffman scans are entropy-coded on the GPU and only their bytes cross to the host,
 * which serialises the markers around them; progressive files (by default) and scans with extra zero runs are Huffman-coded on the host from that image's coefficients.
 * An image that cannot be reconstructed or whose stream is damaged fails alone — the call still returns JXL_DEC_SUCCESS; JxlHipBatchJpegStatus(index) is
 * JXL_DEC_SUCCESS or JXL_DEC_ERROR with that image's reason in JxlHipLastError().  JxlHipBatchJpegSize / JxlHipBatchCopyJpeg hand out the bytes (size 0: no file),
 * valid until the next JxlHipBatchReconstructJpegs or JxlHipBatchReset.  JxlHipBatchSetOption("jpeg_host_writer", 1): every image through the host writer.
 * JxlHipBatchSetOption("jpeg_device_progressive", 1): progressive files (SOF2) are written by the device too, where every scan is a first DC pass, a DC refinement,
 * a first AC pass or an AC refinement of one component; the default 0 sends progressive files through the host writer, and "jpeg_host_writer" wins over it.
 * JxlHipBatchGetInfo "jpeg_device_images" / "jpeg_host_images": files of the last call written by the device / by the host writer;
 * "jpeg_device_progressive_images": those of the device's files that have at least one progressive scan; "jpeg_gather_launches": launches of the kernel that
 * gathers the coefficients of all images into the writer's arena (one per 32768 images).  The same as jobs of a pipeline: JxlHipPipelineSubmitJpegs below. */
int JxlHipBatchCanReconstructJpeg(JxlHipBatch* batch, int index);
JxlDecoderStatus JxlHipBatchReconstructJpegs(JxlHipBatch* batch, void* hip_stream);
JxlDecoderStatus JxlHipBatchJpegStatus(const JxlHipBatch* batch, int index);
size_t JxlHipBatchJpegSize(const JxlHipBatch* batch, int index);
JxlDecoderStatus JxlHipBatchCopyJpeg(JxlHipBatch* batch, int index, uint8_t* dst, size_t cap);
/* The samples libjpeg gives for the original file of a JPEG transcode — a second way from the batch to pixels, beside JxlHipBatchDecode, which keeps giving libjxl's
 * rendering of the frame.  Integer arithmetic throughout: coefficient x quantiser, libjpeg's jpeg_idct_islow, its "fancy" chroma upsampling (replication for chroma planes
 * at most two samples wide) and its fixed-point YCbCr -> RGB; integer sample k enters the write stage as (float)k x (1 / 255), so every output format, layout, orientation
 * and the resized / resampled outputs work as for JxlHipBatchDecode (u8 gives k, u16 gives 257 k).  For files that a JPEG encoder wrote from 8-bit samples the u8 output
 * equals libjpeg's / libjpeg-turbo's default decode sample for sample.
 * JxlHipBatchCanDecodeJpegPixels (host only): 1 if image `index` is eligible, else 0 with the reason, "unsupported: libjpeg-exact decode of ...", in JxlHipLastError().
 * Eligible: one VarDCT frame in YCbCr (or of a grey image), not XYB, no extra channels, upsampling 1, one pass, a RAW quantisation table, no gaborish, no EPF, no patches /
 * splines / noise / crop; luma at full resolution and both chroma channels at 4:4:4, 4:2:2 or 4:2:0; an output at downscale 1.  No `jbrd` box is needed: a transcode
 * stored without reconstruction data, or as a bare codestream, qualifies.  (The quantisation table of a one-group frame is only known once the batch is prepared:
 * JxlHipBatchDecodeJpegPixels looks again and fails that image alone.)
 * JxlHipBatchDecodeJpegPixels runs the LF and HF entropy stages once for all images (it prepares the batch if need be), then the integer pixel path, and writes to the
 * destinations set with JxlHipBatchSetOutput / ...Layout / ...Resized / ...Resampled; it waits for the result.  An image that is not eligible or whose stream is damaged
 * fails alone — the call still returns JXL_DEC_SUCCESS; it fails only for what concerns the whole batch (HIP errors, no images, an image that cannot be prepared).
 * JxlHipBatchJpegPixelsStatus(index): JXL_DEC_SUCCESS, or JXL_DEC_ERROR with that image's reason in JxlHipLastError().  JxlHipBatchDeviceOutput / JxlHipBatchCopyOutput
 * hand out the pixels as after a decode.  JxlHipBatchGetInfo "jpeg_pixel_images": images the last call wrote; "jpeg_pixel_launches": launches of its two pixel kernels
 * (two per 32768 images).  A JxlHipBatchDecode or JxlHipBatchReconstructJpegs of the same batch afterwards gives what it gives on a fresh one.
 * The integer IDCT reads the coefficients where the HF stage left them and zeroes what it read, as the float IDCT does: after a call in which every image of the batch
 * was decoded, the coefficient planes are clean for the next decode.  The same decode as jobs of a pipeline: JxlHipPipelineSubmitJpegPixels below. */
int JxlHipBatchCanDecodeJpegPixels(JxlHipBatch* batch, int index);
JxlDecoderStatus JxlHipBatchDecodeJpegPixels(JxlHipBatch* batch, void* hip_stream);
JxlDecoderStatus JxlHipBatchJpegPixelsStatus(const JxlHipBatch* batch, int index);
/* libjpeg's scaled decodes, exact: jpeg_scale = 2, 4, 8 gives the samples libjpeg gives for the original file at scale_num / scale_denom = 1 / jpeg_scale (what
 * PIL.Image.draft asks for) — the ceil(xsize / s) x ceil(ysize / s) picture, s = jpeg_scale.  It is not the 1:8 decode of `downscale` (libjxl's float rendering of the LF
 * image); the two cannot be combined.  jpeg_scale = 1 is JxlHipBatchSetOutput... at downscale 1, byte for byte; any other value is refused ("jpeg_scale must be 1, 2, 4
 * or 8").  layout and resample may be NULL (interleaved samples; the picture's own size).  The scaled picture takes the place of the full-size one as the source of
 * everything behind it: orientation, sample types, layouts, scale / bias, resize, crop (coordinates in the scaled picture) and mirror.  An output with jpeg_scale != 1 can
 * only be set for an image JxlHipBatchCanDecodeJpegPixels takes (else JXL_DEC_ERROR with that call's reason) and is written by JxlHipBatchDecodeJpegPixels alone: a
 * JxlHipBatchDecode writes the other images and JxlHipBatchFinish fails with "unsupported: image i has an output with jpeg_scale ...".
 * The arithmetic (libjpeg-turbo jdmaster.c, jidctred.c, jdsample.c; CONST_BITS 13, PASS1_BITS 2, DESCALE(x, n) = (x + 2^(n-1)) >> n), with m = 8 / s:
 *  1. IDCT size per component: n = m; while n < 8 and (hmax m) % (h_c n 2) == 0 and (vmax m) % (v_c n 2) == 0: n = 2 n.  Grey, 4:4:4, every luma and 4:2:2 chroma take
 *     n = m; 4:2:0 chroma takes n = 2 m and needs no upsampling at all.  A block gives n x n samples; the component's real extent is
 *     ceil(xsize h_c n / (hmax 8)) x ceil(ysize v_c n / (vmax 8)).
 *  2. Dequantised input for every n: d[v][u] = coefficient x quantiser, as at full size (chroma from luma at 4:4:4 and the DC term included).
 *  3. n = 8: jpeg_idct_islow.
 *  4. n = 4: columns u = 0, 1, 2, 3, 5, 6, 7 (column 4 is never read); with i0 .. i7 the column's rows (i4 unused): t0 = i0 << 14, t2 = 15137 i2 - 6270 i6,
 *     a0 = -1730 i7 + 11893 i5 - 17799 i3 + 8697 i1, a2 = -4176 i7 - 4926 i5 + 7373 i3 + 20995 i1; out0 = DESCALE(t0 + t2 + a2, 12), out1 = DESCALE(t0 - t2 + a0, 12),
 *     out2 = DESCALE(t0 - t2 - a0, 12), out3 = DESCALE(t0 + t2 - a2, 12).  Pass 2: the same on the four workspace rows over entries 0, 1, 2, 3, 5, 6, 7, DESCALE(., 19).
 *  5. n = 2: columns u = 0, 1, 3, 5, 7; t10 = i0 << 15, t0 = -5906 i7 + 6967 i5 - 10426 i3 + 29692 i1, outputs DESCALE(t10 +- t0, 13).  Pass 2: the same on the two rows
 *     over entries 0, 1, 3, 5, 7, DESCALE(., 20).
 *  6. n = 1: DESCALE(d[0][0], 3).
 *  7. + 128, clamped to [0, 255], in all forms.
 *  8. Upsampling of a component whose extent is half the output's (4:2:2 chroma only): the h2v1 "fancy" rule if m > 1 and its width > 2, else replication (every
 *     s = 8 case: libjpeg turns fancy upsampling off when the smallest IDCT is 1 x 1).
 *  9. Colour conversion as at full size.
 * "jpeg_pixel_launches" counts two launches per group of the image table; images of scale 1 and scaled images form groups of their own (a batch that mixes them: four). */
JxlDecoderStatus JxlHipBatchOutBufferSizeJpegScaled(const JxlHipBatch* batch, int index, const JxlPixelFormat* format, int jpeg_scale, const JxlHipOutputLayout* layout,
                                                    const JxlHipOutputResample* resample, size_t* size);
JxlDecoderStatus JxlHipBatchSetOutputJpegScaled(JxlHipBatch* batch, int index, const JxlPixelFormat* format, void* device_buffer, int jpeg_scale, const JxlHipOutputLayout* layout,
                                                const JxlHipOutputResample* resample);
/* jpeg_scale = 8 from the DC terms alone.  At that scale grey, 4:4:4 and 4:2:2 images take the 1 x 1 IDCT for every component (rules 1 and 6 above): a sample is
 * clamp(DESCALE(dc x q[0], 3) + 128) of one DC term, and the DC terms are what the LF stage of the decode writes.  Such an image is DC-only: the HF entropy stage, the
 * integer IDCT and the intermediate planes are left out for it, it takes neither coefficient nor pixel planes, and one kernel writes the picture — byte for byte what
 * the general path gives.  4:2:0 needs the 2 x 2 chroma IDCT, hence AC terms, and keeps the general path, as does every image at scale 1, 2 and 4.
 * JxlHipBatchJpegDcOnly(index), host only, after the image's output has been set: 1 if the image will be decoded from its DC terms, else 0.
 * Prefixes: a DC-only image may end anywhere behind the LF part of its frame (LfGlobal, the LfGroups, HfGlobal — a fifth of a typical quality-85 transcode), as for the
 * 1:8 decode: add it under JxlHipBatchSetOption "allow_partial" = 1.  A prefix that ends inside the LF part is "truncated"; so is one whose image is not DC-only —
 * when the batch is prepared, as for a prefix that is not decoded at 1:8.  A one-section frame (one group) has no LF prefix: it is DC-only from the whole file only.
 * Jobs of JxlHipPipelineSubmitJpegPixelsScaled / ...Resampled with jpeg_scale = 8 take prefixes as they are; a prefix that is not enough fails alone, "truncated".
 * JxlHipLfPartSize: *bytes = the number of leading bytes of the FILE (container boxes included) that hold the LF part of the first frame — the smallest n for which
 * data[0 .. n) is accepted by the 1:8 decode and by a DC-only decode.  It needs the headers and the frame's TOC only, so any prefix that holds those gives the same
 * answer as the whole file; JXL_DEC_ERROR with "truncated" when the TOC is not there yet (or the codestream goes on in a box that is not).  *bytes = 0: the whole file
 * is needed (a one-section frame, a Modular frame, sections stored out of order).
 * JxlHipBatchSetOption "jpeg_dc_only" (default 1; 0: the general path for every image, read by the next JxlHipBatchPrepare — what a doubted result is compared with;
 * pipelines always take the DC-only path).  JxlHipBatchGetInfo / JxlHipPipelineGetInfo "jpeg_dc_only_images": images of the last call / the job finished last that were
 * written from their DC terms; they count in "jpeg_pixel_images" as before.  A group of DC-only images adds one launch to "jpeg_pixel_launches", not two. */
int JxlHipBatchJpegDcOnly(const JxlHipBatch* batch, int index);
/* Crops decoded by region: JxlHipBatchSetOption "jpeg_region" = 1 (default 0; read by the next JxlHipBatchPrepare), JxlHipPipelineSetOption "jpeg_region" for the jobs
 * submitted after it.  An output written by JxlHipBatchDecodeJpegPixels (or a libjpeg-exact pipeline job) that carries a crop then decodes only the 256x256 groups the
 * crop needs — HF entropy stage, integer IDCT and colour stage —; the bytes delivered are exactly those of the decode without the option.  The rule, for an image that
 * decode takes, that is not DC-only and whose output has a crop (jpeg_scale s = 1, 2, 4, 8):
 *   1. the crop — given in the oriented picture at scale s — is mapped back through the orientation to a rectangle of the stored picture at scale s;
 *   2. a luma block covers n x n of its pixels, n = 8 / s: the crop's luma blocks are floor(first / n) .. floor(last / n) per axis;
 *   3. that range is widened outwards to whole MCUs of (1 << hs) x (1 << vs) luma blocks, hs / vs the chroma shifts (grey and 4:4:4: 1 x 1);
 *   4. plus one MCU on every side (fancy chroma upsampling reads the neighbouring chroma sample; taken at 4:4:4 and grey too), clamped to the frame's block grid;
 *   5. the region is every group (32 x 32 blocks) that block rectangle touches: gx0 <= gx < gx1, gy0 <= gy < gy1.
 * Images without a crop, DC-only images and images the libjpeg-exact decode does not take have no region and are decoded whole.  A damaged stream in a skipped group
 * goes unnoticed.  JxlHipBatchDecode, the float decode of the same batch, decodes every group whatever the option says.
 * JxlHipBatchJpegRegion(index, groups), host only, after the image's output has been set: 1 and groups = {gx0, gy0, gx1, gy1} if the image would be decoded by region
 * under the option (whether or not the option is set), 0 if it would be decoded whole.
 * JxlHipBatchGetInfo "hf_groups_total" / "hf_groups_decoded" (JxlHipPipelineGetInfo: of the job prepared last): the groups of the frames that took the HF stage of the
 * last JxlHipBatchDecodeJpegPixels, and those of them that were decoded — equal with the option off.  JxlHipBatchStageBytes counts the HF, IDCT and output stages of an
 * image with a region by its region after JxlHipBatchDecodeJpegPixels (JxlHipPipelineStageBytes: for a libjpeg-exact job), and by the whole picture after JxlHipBatchDecode.
 * JxlHipBatchJpegRegion also answers 1 for a cropped output set through the float calls (JxlHipBatchSetOutputResampled): it says what JxlHipBatchDecodeJpegPixels would do. */
int JxlHipBatchJpegRegion(const JxlHipBatch* batch, int index, uint32_t groups[4]);
JxlDecoderStatus JxlHipLfPartSize(const uint8_t* data, size_t size, size_t* bytes);
/* The integer resample of libjpeg-exact outputs: Pillow's 8-bit resize, byte for byte.  JxlHipBatchSetOutputJpegResampled is JxlHipBatchSetOutputJpegScaled with
 * `flags`; flags = 0 is that call, byte for byte; bit 0, JXL_HIP_RESAMPLE_U8, selects the integer resample; every other bit is refused.  Sizes are those of
 * JxlHipBatchOutBufferSizeJpegScaled / JxlHipImageOutSizeJpegScaled.  With the flag the u8 output equals
 * numpy.asarray(PIL.Image.open(file).crop(box).resize((xsize, ysize), BILINEAR | BICUBIC)) (after draft() for jpeg_scale, after the orientation) byte for byte: crop, then
 * resize — not resize(size, box=box), which reads taps outside the box.
 * The rule.  The source is the u8 picture the output would have held without a resize: libjpeg's samples after jpeg_scale, after the orientation (or as stored, under
 * "keep_orientation"), in the output's channel slots (grey replicated, the alpha slot 255), cut to the crop — an axis sees n_in = the crop's side.  Per axis, n_in -> n_out,
 * with kernel k and radius r of `filter` as given for JxlHipOutputResample above:
 *   scale = n_in / n_out and s = max(scale, 1), in double; target sample i is centred at c = scale x (i + 0.5) and takes the source samples j of
 *   [max(0, int(c - r s + 0.5)), min(n_in, int(c + r s + 0.5))); the double weights are w_j = k((j - c + 0.5) / s), each divided by their sum (the weights of
 *   JxlHipOutputResample before they are rounded to float32);
 *   the integer weight is kk_j = int(w_j x 2^22 + 0.5) for w_j >= 0 and int(w_j x 2^22 - 0.5) for w_j < 0, int truncating towards zero; the integer weights are not
 *   renormalised;
 *   a sample is clamp((2^21 + sum_j p_j x kk_j) >> 22, 0, 255): the sum in int32 (sum |kk| x 255 < 2^31 for both filters), the shift arithmetic.
 * The horizontal pass runs first, over the rows of the crop, and gives u8; the vertical pass runs over that u8 result.  The clamp between the passes is part of the
 * definition: cubic overshoot is cut twice.  A target of the crop's own size needs no special case (the single weight is 2^22: a copy).  Taps of kk = 0 at either end of a
 * range may be left out.  The finished u8 value k is stored as the libjpeg-exact decode stores a sample: u8 k, u16 257 k, float16 / float32 (float)k x (1 / 255), through
 * scale / bias — every sample type, byte order, 1 - 4 channels, row alignment and planar layout follow from the u8 result; `mirror` is the flip of the finished target.
 * Such an output's intermediates are u8 (JxlHipBatchDeviceBytes: a quarter of the float32 ones of the other resized outputs).
 * Refused, each as "unsupported: integer resample ...": the flag without a resample (no target size); the flag for an image JxlHipBatchCanDecodeJpegPixels does not take
 * (in a pipeline job that image fails alone); together with downscale 8 (the bindings' keyword: these calls have no downscale).  Like an output with jpeg_scale != 1 it is
 * written by JxlHipBatchDecodeJpegPixels alone: a JxlHipBatchDecode writes the other images and JxlHipBatchFinish fails with "unsupported: integer resample of image i ...".
 * The launches are those of the other resized outputs (one pair per group of equal slot count; integer and float32 resamples never share a group).
 * JxlHipBatchGetInfo(batch, "resize_u8_images"): images of the last decode that were resampled this way. */
#define JXL_HIP_RESAMPLE_U8 1u
JxlDecoderStatus JxlHipBatchSetOutputJpegResampled(JxlHipBatch* batch, int index, const JxlPixelFormat* format, void* device_buffer, int jpeg_scale,
                                                   const JxlHipOutputLayout* layout, const JxlHipOutputResample* resample, uint32_t flags);
/* Decode-thread packing: lanes between active entropy-decode threads (64 = one stream per wavefront, 1 = 64 per wavefront). */
void JxlHipBatchSetLaneStride(JxlHipBatch* batch, int lf, int hf);
/* Tuning / testing knobs: "force_generic_idct", "hf_block_threads", "lds_code_budget", "debug_stop_after", "lf_wide_once" (the next LF stage of the batch takes the
 * one-wavefront-per-stream kernel whatever the lane stride: shorter latency on an idle GPU), "lf_wp_narrow_test" (testing: the SIMT LF kernel's
 * weighted-predictor lanes hand a stream back to the one-wavefront-per-stream kernel at |sample| > 16 instead of 2^20), "allow_partial" (images added afterwards may
 * end behind their LF part: they decode at 1:8 only, JxlHipBatchSetOutputScaled; otherwise JxlHipBatchPrepare fails with "truncated"), "jpeg_region" (crops of libjpeg-exact outputs decode only the groups they need: JxlHipBatchJpegRegion).
 * Unknown names are ignored. */
void JxlHipBatchSetOption(JxlHipBatch* batch, const char* name, int value);
/* Uploads streams and tables (inputs become HBM-resident) and allocates work buffers.  hip_stream: hipStream_t or NULL. */
JxlDecoderStatus JxlHipBatchPrepare(JxlHipBatch* batch, void* hip_stream);
/* Enqueues the decode of the whole batch on hip_stream (no host sync). */
JxlDecoderStatus JxlHipBatchDecode(JxlHipBatch* batch, void* hip_stream);
/* Same, bracketing every stage with HIP events recorded on hip_stream (still no host sync). */
JxlDecoderStatus JxlHipBatchDecodeTimed(JxlHipBatch* batch, void* hip_stream);
/* Enqueues one part of a decode: 0 = everything, 1 = front (LF decode, LF post-processing), 2 = rest (HF decode, IDCT,
 * filters, output); the rest may also be enqueued in two pieces, 3 = HF decode, 4 = IDCT, filters, output, and so may the front,
 * 5 = LF decode (all the HF decode needs), 6 = LF post-processing (needed by piece 4 only); piece 4 in turn as 7 = IDCT (the last stage
 * that touches the coefficient planes) and 8 = restoration filters, colour, write.  (9, 10 and 11 are the pieces of the libjpeg-exact decode that
 * JxlHipBatchDecodeJpegPixels and the pipeline enqueue in the places of 7, 8 and 6; they need that decode's plan and do nothing without it.)  Front and rest may
 * go to different streams; the caller orders them with events, which lets the latency-bound LF stage of later batches overlap
 * the other stages of the current one (bench.py: three batches in flight, LF stages on two side streams). */
JxlDecoderStatus JxlHipBatchDecodePart(JxlHipBatch* batch, void* hip_stream, int part, int timed);
/* Piece 5 (LF decode) of n prepared batches on one stream, as the pipeline enqueues it for jobs that are ready together: adjacent batches whose LF streams take the same
 * SIMT kernel (plain VarDCT frames, equal lane strides) share ONE launch of it, at most 8 batches a launch; every other batch gets exactly the launches of
 * JxlHipBatchDecodePart(batch, stream, 5, timed).  Order is kept.  The remaining pieces of each batch follow through JxlHipBatchDecodePart. */
JxlDecoderStatus JxlHipBatchDecodeLfGrouped(JxlHipBatch* const* batches, int n, void* hip_stream, int timed);
/* Waits for all timed decodes so far; returns per-stage sums in ms and the number of timed decodes. */
JxlDecoderStatus JxlHipBatchCollectTimes(JxlHipBatch* batch, JxlHipStageTimes* times, int* runs);
/* Waits for completion and checks per-frame device status. */
JxlDecoderStatus JxlHipBatchFinish(JxlHipBatch* batch, void* hip_stream);
/* Device pointer of the decoded pixels of image `index`; copy to host. */
void* JxlHipBatchDeviceOutput(const JxlHipBatch* batch, int index);
JxlDecoderStatus JxlHipBatchCopyOutput(JxlHipBatch* batch, int index, void* host_dst, size_t size, void* hip_stream);
/* Accounting for roofline reports. */
uint64_t JxlHipBatchTotalPixels(const JxlHipBatch* batch);
uint64_t JxlHipBatchCompressedBytes(const JxlHipBatch* batch);
/* Algorithmic (compulsory) HBM bytes of one decode per stage: lf, lfpost, hf, idct, filters, out. */
void JxlHipBatchStageBytes(const JxlHipBatch* batch, uint64_t out[6]);
uint64_t JxlHipBatchDeviceBytes(const JxlHipBatch* batch);
/* Facts about a prepared batch, by name (-1: unknown name): "lf_simt_frames" / "lf_legacy_frames" = VarDCT frames whose LF-group streams
 * take the SIMT kernel (one stream per lane, lane stride < 64) / the one-wavefront-per-stream kernel, "lf_simt_lanes", "lf_simt_waves", "lf_simt_wp" (1: the SIMT launch is the instantiation with weighted-predictor state), "lf_simt_streams" (more than "lf_simt_lanes": some lane decodes several streams),
 * "lf_spec_lanes" (after a decode: lanes per stream of the SIMT launch without the weighted predictor, batch option "lf_spec_lanes"; 0: no such launch), "lf_spec_hits" / "lf_spec_misses" (with
 * JXL_HIP_LF_SPEC_STATS set: samples of this device's launches so far whose cluster was / was not one of the lanes' candidates; -1 otherwise), "hf_nonzeros" = non-zero AC coefficients of one decode of the batch (after a Finish). */
int64_t JxlHipBatchGetInfo(const JxlHipBatch* batch, const char* name);
/* Testing: after a decode, copies a device buffer of image `index`'s first (VarDCT) frame to the host — "plane_a" / "plane_b" (the padded
 * float XYB planes the stages ping-pong between, 8 bw x 8 bh samples per channel), "lf" / "llf" / "lfq", "inv_sigma", "blk_info", "coef_off" (one
 * value per 8x8 block), "coeff" (dense quantised coefficients, 65536 per group), "ytox" / "ytob".  With JxlHipBatchSetOption("debug_stop_after", s)
 * the tail of the decode stops after stage s (1 IDCT, 2 gaborish, 3 / 4 / 5 EPF pass 0 / 1 / 2; stage-by-stage filters: "force_unfused_filters"),
 * which is how tests/test_stage_formulas.py compares single stages with float64 restatements of their defining formulas.
 * Returns the size of the buffer in bytes (0 on error), copies min(size, cap). */
size_t JxlHipBatchDebugRead(JxlHipBatch* batch, int index, const char* name, int channel, void* dst, size_t cap, void* hip_stream);

/* ---- extension: the streaming decode pipeline of one GPU ----------------------------------------------------------------------
 * No counterpart in the reference: jpegxl-rs decodes batches by looping decode_with over files (jpegxl-rs/benches/decode.rs:16-19).  A pipeline object
 * owns what keeps a GPU busy with a stream of compressed images: a ring of batch objects, the coefficient sets and pixel planes all jobs share, its own
 * non-blocking HIP streams, the host threads that parse / build tables / upload / enqueue the latency-bound LF stage several jobs ahead, and the thread
 * that issues HF stages and tails in submission order (csrc/pipeline.h).  bench.py's headline is produced by these calls.
 * Concurrent callers of the libjxl API above share one such pipeline per device (csrc/scheduler.cc). */
typedef struct JxlHipPipelineStruct JxlHipPipeline;
typedef struct {
  int32_t jobs_in_flight;    /* jobs in flight on the GPU; 0 = default (11) */
  int32_t lf_streams;        /* side streams for the LF stages, at most; 0 = default (11).  In use: as many as the hardware queues leave room for (JxlHipPipelineSetOption "lf_streams_effective") */
  int32_t hf_streams;        /* HF stages in flight beside the tail, one coefficient set each + one; 0 = default (2) */
  int32_t prepare_threads;   /* host threads that each prepare one job at a time; 0 = default (3) */
  int32_t parse_threads;     /* host threads one job's images are parsed on; 0 = default (8) */
  int32_t lane_stride_lf, lane_stride_hf;   /* see JxlHipBatchSetLaneStride; 0 = defaults (8, 1) */
  int32_t wide_first;        /* LF stages at the start of a cold pipeline that take the one-wavefront-per-stream kernel; < 0 = default (4) */
  int32_t small_job_frames;  /* jobs of at most this many frames always take it, and sparse wavefronts in the HF stage (latency over occupancy); 0 = never */
  int32_t timed;             /* bracket the stages with HIP events: JxlHipPipelineCollectTimes */
  int32_t reserve_frames, reserve_width, reserve_height;   /* size the shared planes for jobs of this shape at creation (0: grown when the pipeline is idle) */
  int32_t reserve_plane_sets; /* 2: the frames take the stage-by-stage restoration filters (anything but gaborish + one EPF pass) and need a second set of pixel planes */
} JxlHipPipelineOptions;
JxlHipPipeline* JxlHipPipelineCreate(int device, const JxlHipPipelineOptions* options /* NULL = defaults */);
void JxlHipPipelineDestroy(JxlHipPipeline* pipeline);
/* Submits a job of n compressed images, all decoded to `format`.  Exactly one of device_out / host_out is given: n caller-owned destinations (device memory /
 * host memory — pinned, JxlHipHostAlloc, for full-speed copies that overlap later jobs), each at least JxlHipImageOutSize bytes; out_capacity (optional) is
 * checked per image.  The compressed bytes and the destinations must stay valid until JxlHipPipelineWait(ticket) returns.  Blocks while the ring is full.
 * An image that does not parse or decode fails alone.  Returns the job's ticket (>= 0) or -1 (JxlHipLastError). */
int64_t JxlHipPipelineSubmit(JxlHipPipeline* pipeline, const uint8_t* const* datas, const size_t* sizes, int n, const JxlPixelFormat* format, void* const* device_out,
                             void* const* host_out, const size_t* out_capacity);
/* The same job decoded at 1:8 (downscale = 8, see JxlHipBatchSetOutputScaled; destinations of JxlHipImageOutSizeScaled bytes): streams may end behind their LF part;
 * an image the 1:8 decode does not take fails alone. */
int64_t JxlHipPipelineSubmitScaled(JxlHipPipeline* pipeline, const uint8_t* const* datas, const size_t* sizes, int n, const JxlPixelFormat* format, void* const* device_out,
                                   void* const* host_out, const size_t* out_capacity, int downscale);
/* The same with an output layout (JxlHipOutputLayout above; NULL = interleaved) and downscale 1 or 8: destinations of JxlHipImageOutSizeLayout bytes.  An image whose size
 * does not fit layout->plane_stride fails alone. */
int64_t JxlHipPipelineSubmitLayout(JxlHipPipeline* pipeline, const uint8_t* const* datas, const size_t* sizes, int n, const JxlPixelFormat* format, void* const* device_out,
                                   void* const* host_out, const size_t* out_capacity, int downscale, const JxlHipOutputLayout* layout);
/* The same with every image resized (JxlHipOutputResize above; NULL = JxlHipPipelineSubmitLayout): destinations of JxlHipImageOutSizeResized bytes, the same for every
 * image of the job.  An image the crop leaves fails alone. */
int64_t JxlHipPipelineSubmitResized(JxlHipPipeline* pipeline, const uint8_t* const* datas, const size_t* sizes, int n, const JxlPixelFormat* format, void* const* device_out,
                                    void* const* host_out, const size_t* out_capacity, int downscale, const JxlHipOutputLayout* layout, const JxlHipOutputResize* resize);
/* The same with a resample per image (JxlHipOutputResample above, n entries; every entry the same xsize x ysize). */
int64_t JxlHipPipelineSubmitResampled(JxlHipPipeline* pipeline, const uint8_t* const* datas, const size_t* sizes, int n, const JxlPixelFormat* format, void* const* device_out,
                                      void* const* host_out, const size_t* out_capacity, int downscale, const JxlHipOutputLayout* layout, const JxlHipOutputResample* each);
/* The same with extra-channel planes behind every image's colour output (JxlHipOutputPlanes above: one request list for the job).  `each` may be NULL: every image at
 * its own size.  A destination holds the colour output and the planes (JxlHipImageOutSizePlanes bytes; out_capacity is checked against that); an image the planes are
 * refused for — a channel it does not have — fails alone with the reason. */
int64_t JxlHipPipelineSubmitPlanes(JxlHipPipeline* pipeline, const uint8_t* const* datas, const size_t* sizes, int n, const JxlPixelFormat* format, void* const* device_out,
                                   void* const* host_out, const size_t* out_capacity, int downscale, const JxlHipOutputLayout* layout, const JxlHipOutputResample* each,
                                   const JxlHipOutputPlanes* planes);
/* The same with an output colour for the job (JxlHipOutputColor above; NULL = JxlHipPipelineSubmitPlanes): an image the target is refused for — a grey target on a colour
 * image, non_xyb = 1 on an image whose colour is only an ICC profile — fails alone with the reason. */
int64_t JxlHipPipelineSubmitColor(JxlHipPipeline* pipeline, const uint8_t* const* datas, const size_t* sizes, int n, const JxlPixelFormat* format, void* const* device_out,
                                  void* const* host_out, const size_t* out_capacity, int downscale, const JxlHipOutputLayout* layout, const JxlHipOutputResample* each,
                                  const JxlHipOutputPlanes* planes, const JxlHipOutputColor* color);
/* A job of libjpeg-exact pixels: every image is decoded to the samples libjpeg gives for the JPEG file it was transcoded from (JxlHipBatchDecodeJpegPixels above, as
 * stages of the pipeline: the job shares coefficient sets and pixel planes with plain jobs, which may be mixed with it freely).  Eligible is what
 * JxlHipBatchCanDecodeJpegPixels takes; an image that is not eligible fails alone with that call's reason ("unsupported: libjpeg-exact decode of ..."), and so does an
 * image whose stream is damaged — a frame with a transform other than DCT8 is named as such.  layout: NULL = interleaved; each: NULL, or n JxlHipOutputResample of one
 * target size (crop, filter and mirror the image's own), as for JxlHipPipelineSubmitResampled.  There is no downscale (the 1:8 LF decode is libjxl's rendering, not libjpeg's
 * samples); libjpeg's own scaled decodes: JxlHipPipelineSubmitJpegPixelsScaled below.
 * Destinations are sized as for JxlHipPipelineSubmitLayout / ...Resampled at downscale 1. */
int64_t JxlHipPipelineSubmitJpegPixels(JxlHipPipeline* pipeline, const uint8_t* const* datas, const size_t* sizes, int n, const JxlPixelFormat* format, void* const* device_out,
                                       void* const* host_out, const size_t* out_capacity, const JxlHipOutputLayout* layout /* NULL = interleaved */,
                                       const JxlHipOutputResample* each /* NULL, or n entries of one target size */);
/* The same at one of libjpeg's scales (JxlHipBatchSetOutputJpegScaled above: jpeg_scale = 1, 2, 4, 8; a job takes one scale, another value refuses the submission):
 * destinations are sized with JxlHipImageOutSizeJpegScaled, crops are in the scaled picture.  The other Submit calls have no jpeg_scale: only this decode writes it. */
int64_t JxlHipPipelineSubmitJpegPixelsScaled(JxlHipPipeline* pipeline, const uint8_t* const* datas, const size_t* sizes, int n, const JxlPixelFormat* format,
                                             void* const* device_out, void* const* host_out, const size_t* out_capacity, const JxlHipOutputLayout* layout /* NULL = interleaved */,
                                             const JxlHipOutputResample* each /* NULL, or n entries of one target size */, int jpeg_scale);
/* The same with flags (JxlHipBatchSetOutputJpegResampled above): JXL_HIP_RESAMPLE_U8 makes the integer resample the property of the job — every image of it is
 * resampled in Pillow's 8-bit arithmetic; flags = 0 is the call above, byte for byte; other bits, and the flag with a NULL `each`, refuse the submission.  An image the
 * libjpeg-exact decode does not take fails alone ("unsupported: integer resample of ...").  Such jobs mix with every other kind of job over the same buffer sets. */
int64_t JxlHipPipelineSubmitJpegPixelsResampled(JxlHipPipeline* pipeline, const uint8_t* const* datas, const size_t* sizes, int n, const JxlPixelFormat* format,
                                                void* const* device_out, void* const* host_out, const size_t* out_capacity, const JxlHipOutputLayout* layout /* NULL = interleaved */,
                                                const JxlHipOutputResample* each /* n entries of one target size */, int jpeg_scale, uint32_t flags);
/* A reconstruction job: the original JPEG file of every image, byte for byte (JxlHipBatchReconstructJpegs above, as stages of the pipeline: the entropy stages run
 * ahead on the side streams, one gather launch per job moves the coefficients out of the shared coefficient set — which is clean behind it —, and the pack pass, the
 * copies and the host splice of a job run in the thread that collects it, beside the entropy stages of the jobs behind it).  Such jobs mix freely with plain, 1:8,
 * resized and libjpeg-exact jobs.  There is no pixel format and there are no destinations: nobody can size a JPEG file from its transcode, so the files stay with
 * the pipeline until they are collected.  flags: the two switches of the batch call; unknown bits refuse the submission.  An image the batch call refuses fails alone
 * with that call's reason ("JPEG reconstruction: no jbrd box", ...), and so does an image whose stream is damaged; what a reconstruction job refuses is exactly what
 * JxlHipBatchReconstructJpegs refuses.  A job in which no image can be reconstructed fails as a whole (every image carries the reason) without touching the GPU.
 * JxlHipPipelineWaitJpegs waits like JxlHipPipelineWait and also gives the files' sizes (jpeg_sizes[i], n entries, optional; 0: no file); it keeps the files until
 * JxlHipPipelineReleaseJpegs(ticket), after which the ticket is unknown.  On a ticket of another kind it is an error of the call, and that ticket stays waitable.
 * Between the two, JxlHipPipelineJpegStatus(ticket, i) is JXL_DEC_SUCCESS or JXL_DEC_ERROR with that image's reason in JxlHipLastError(), and JxlHipPipelineCopyJpeg
 * copies image i's file (refused if `capacity` is smaller than the file).  JxlHipPipelineWait on a reconstruction ticket gives the statuses and releases the files.
 * A finished reconstruction job that nobody waits for, or that is never released, holds its files until the pipeline's bounded history of uncollected jobs drops it. */
#define JXL_HIP_JPEG_DEVICE_PROGRESSIVE 1u   /* batch option jpeg_device_progressive */
#define JXL_HIP_JPEG_HOST_WRITER        2u   /* batch option jpeg_host_writer; wins */
int64_t JxlHipPipelineSubmitJpegs(JxlHipPipeline* pipeline, const uint8_t* const* datas, const size_t* sizes, int n, uint32_t flags);
JxlDecoderStatus JxlHipPipelineWaitJpegs(JxlHipPipeline* pipeline, int64_t ticket, int* image_status, size_t* jpeg_sizes, int n, float* end_ms);
JxlDecoderStatus JxlHipPipelineJpegStatus(JxlHipPipeline* pipeline, int64_t ticket, int i);
JxlDecoderStatus JxlHipPipelineCopyJpeg(JxlHipPipeline* pipeline, int64_t ticket, int i, void* dst, size_t capacity);
void JxlHipPipelineReleaseJpegs(JxlHipPipeline* pipeline, int64_t ticket);
/* Waits until the job has left the GPU (pixels written, host copies done).  image_status[i] (n entries, optional): 0 decoded, 1 failed; *end_ms (optional): when the
 * job's last byte was written, ms after JxlHipPipelineResetClock.  JXL_DEC_SUCCESS if every image decoded, else JXL_DEC_ERROR (JxlHipLastError names the first).
 * A ticket can be waited for once; jobs complete in submission order. */
JxlDecoderStatus JxlHipPipelineWait(JxlHipPipeline* pipeline, int64_t ticket, int* image_status, int n, float* end_ms);
JxlDecoderStatus JxlHipPipelineWaitAll(JxlHipPipeline* pipeline);        /* every job submitted so far has left the GPU (results stay collectable) */
JxlDecoderStatus JxlHipPipelineResetClock(JxlHipPipeline* pipeline);     /* waits for idle; end_ms and the prepare-time counters start over */
JxlDecoderStatus JxlHipPipelineCollectTimes(JxlHipPipeline* pipeline, JxlHipStageTimes* times, int* runs);   /* options.timed: per-stage sums (ms) over the jobs since the last call */
void JxlHipPipelineStageBytes(JxlHipPipeline* pipeline, uint64_t out[6]);   /* algorithmic bytes per stage of the job prepared last (JxlHipBatchStageBytes) */
/* "jobs", "slots", "coefficient_sets", "device_bytes", "shared_big_bytes", "shared_coef_bytes", "private_plane_jobs" (jobs that did not fit the shared planes),
 * "prepare_us_total" / "prepared_jobs" (host time of the prepare threads since the last clock reset), and of the job prepared / finished last: "frames",
 * "compressed_bytes", "total_pixels", "hf_nonzeros", "lf_simt_frames", "lf_legacy_frames", "lf_simt_wp", "jpeg_pixel_images" (images of a libjpeg-exact job that took
 * that path; after the job has finished: that were decoded; 0 for a plain job), "jpeg_pixel_launches" (launches of its two pixel kernels: two per 32768 such images);
 * of the job finished last, 0 unless it was a reconstruction job: "jpeg_device_images", "jpeg_host_images", "jpeg_device_progressive_images" (as JxlHipBatchGetInfo),
 * "jpeg_gather_launches" (launches of the gather kernel: one per 32768 images); "lf_groups" / "lf_grouped_jobs" (LF stages enqueued since the last clock reset — a
 * launch may serve several jobs — and the jobs in them), "lf_group_largest", "lf_streams_effective" (LF streams in use), "lf_group_max".  -1: unknown name. */
int64_t JxlHipPipelineGetInfo(JxlHipPipeline* pipeline, const char* name);
/* Options that apply to the jobs submitted after the call: "jpeg_region" (0 / 1, default 0: libjpeg-exact jobs decode crops by region, JxlHipBatchJpegRegion; GetInfo
 * "hf_groups_total" / "hf_groups_decoded" of the job prepared last); "lf_group_max" (1 .. 8, default 4: jobs that are ready together while the LF stream is busy share
 * one launch of the SIMT LF kernel, at most this many; 1: every job its own launch); "lf_streams_effective" (LF streams in use, at most options.lf_streams; default 0 =
 * min(lf_streams, 6, max(3, Q - 2 - hf_streams)) with Q = GPU_MAX_HW_QUEUES of the process, 4 if unset: streams that share a hardware queue serialise).  Both also as
 * JXL_HIP_LF_GROUP_MAX / JXL_HIP_LF_STREAMS_EFFECTIVE in the environment, read when a pipeline is created: there the environment takes precedence over the defaults,
 * a JxlHipPipelineSetOption call afterwards over the environment.  Unknown names are ignored. */
void JxlHipPipelineSetOption(JxlHipPipeline* pipeline, const char* name, int value);
/* Pinned host memory for host_out destinations (hipHostMalloc / hipHostFree). */
void* JxlHipHostAlloc(size_t bytes);
void JxlHipHostFree(void* p);
/* Host-only (needs no GPU): basic info and output size of an image for `format` from its headers — what a caller of JxlHipPipelineSubmit sizes its buffers with. */
JxlDecoderStatus JxlHipImageOutSize(const uint8_t* data, size_t size, const JxlPixelFormat* format, JxlBasicInfo* info, size_t* out_size);
/* The same for the 1:8 decode: `info` stays the full-size JxlBasicInfo, *out_size is that of the ceil(xsize / 8) x ceil(ysize / 8) picture; a prefix of the file that holds
 * the headers is enough. */
JxlDecoderStatus JxlHipImageOutSizeScaled(const uint8_t* data, size_t size, const JxlPixelFormat* format, int downscale, JxlBasicInfo* info, size_t* out_size);
/* The same for an output layout (JxlHipOutputLayout; NULL = interleaved) at downscale 1 or 8. */
JxlDecoderStatus JxlHipImageOutSizeLayout(const uint8_t* data, size_t size, const JxlPixelFormat* format, int downscale, const JxlHipOutputLayout* layout, JxlBasicInfo* info,
                                          size_t* out_size);
/* The same for a resized output (JxlHipOutputResize; NULL = JxlHipImageOutSizeLayout): the size of the xsize x ysize picture. */
JxlDecoderStatus JxlHipImageOutSizeResized(const uint8_t* data, size_t size, const JxlPixelFormat* format, int downscale, const JxlHipOutputLayout* layout,
                                           const JxlHipOutputResize* resize, JxlBasicInfo* info, size_t* out_size);
/* The same for libjpeg's scaled decode (JxlHipBatchSetOutputJpegScaled: jpeg_scale = 1, 2, 4, 8; layout and resample may be NULL): the size of the
 * ceil(xsize / jpeg_scale) x ceil(ysize / jpeg_scale) picture, or of the target it is resampled to.  Whether the image is a JPEG transcode is not looked at here. */
JxlDecoderStatus JxlHipImageOutSizeJpegScaled(const uint8_t* data, size_t size, const JxlPixelFormat* format, int jpeg_scale, const JxlHipOutputLayout* layout,
                                              const JxlHipOutputResample* resample, JxlBasicInfo* info, size_t* out_size);
/* Device arenas that batches and pipelines let go of are pooled per process (hipMalloc / hipFree of tens of GB cost seconds): JXL_HIP_ARENA_POOL_MB bounds the pool
 * (default 60 % of the device's memory, 0 = off); Trim hands every pooled block back to the runtime — for processes that share the GPU with another allocator —
 * and returns the bytes released; Held = bytes pooled right now. */
size_t JxlHipArenaPoolTrim(void);
size_t JxlHipArenaPoolHeld(void);
/* The scheduler behind the libjxl API (one shared pipeline per device; JXL_HIP_SCHEDULER=0 turns it off): jobs submitted / images decoded so far; Shutdown joins its
 * threads and frees its pipelines (tests). */
void JxlHipSchedulerStats(int device, int64_t* jobs, int64_t* images);
void JxlHipSchedulerShutdown(void);

/* ---- extension: lossless batch encoder (csrc/encode_lossless.cc, csrc/encode_lossless.hip) -----------------------------------------
 * Writes bare JPEG XL codestreams that decode to the input exactly: one prefix-coded Modular frame per image (group dimension 256, one pass, RCT type 6 over three colour
 * channels, one fixed MA tree, codes built from the image's own histograms; no Squeeze, palette, LZ77 or ANS).  Tokens, bit counts and the bits themselves are computed on the
 * GPU for all images of a call at once; the host writes headers, TOC and code tables.  libjxl's own encoder names stay error-returning stubs.
 *
 * One input: interleaved samples, `num_channels` 1 (grey), 2 (grey + alpha), 3 (RGB), 4 (RGBA); sRGB (grey: the sRGB transfer function), orientation 1;
 * bits_per_sample 1..16; data_type JXL_TYPE_UINT8 (up to 8 bits) or JXL_TYPE_UINT16 (little endian, any depth); row_pitch in bytes, 0 = tight; pixels in host memory, or in
 * device memory when on_device is set.
 * Refused per image, with a message in the last-error text: a side of 0 or above 16384, channels outside 1..4, bits outside 1..16, a type that does not fit the depth, a
 * pitch below one row, NULL pixels, a device pointer on a host-only encoder, a sample above 2^bits_per_sample - 1. */
typedef struct JxlHipEncoderStruct JxlHipEncoder;
typedef struct {
  const void* pixels; JXL_BOOL on_device; uint32_t xsize, ysize, num_channels, bits_per_sample; JxlDataType data_type; size_t row_pitch; JXL_BOOL alpha_premultiplied;
} JxlHipEncodeImage;
/* device -1: a host-only encoder (needs no GPU) — bounds and refusals work, encoding does not. */
JxlHipEncoder* JxlHipEncoderCreate(int device);
void JxlHipEncoderDestroy(JxlHipEncoder* enc);
/* Host only.  The worst-case size of the image's codestream (`pixels` is not looked at), derived from the stream shape:
 *   48 (image + frame header) + 8192 (LfGlobal: tree, code tables, context map) + 2 + 6 * toc_entries + ceil(xsize * ysize * num_channels * (15 + extra) / 8)
 * where toc_entries = 1 for an image of one 256 x 256 group, else 2 + ceil(xsize / 2048) * ceil(ysize / 2048) + ceil(xsize / 256) * ceil(ysize / 256); 15 is the
 * longest prefix code; extra, the most extra bits of a token, is n - 2 for n = bits_per_sample + (1 if num_channels >= 3: the RCT), 0 if n < 4.
 * Returns 0, or 1 for a description that would be refused. */
int JxlHipEncodeLosslessBound(const JxlHipEncodeImage* image, size_t* bytes);
/* Encodes `num_images` images in one set of launches on hip_stream (NULL: the default stream); the results are complete when it returns.  An image that is refused fails
 * alone.  The bytes of an image do not depend on the other images of the call.  Returns 0 if every image was encoded, else 1 (the text names the first failure). */
int JxlHipEncoderEncodeLossless(JxlHipEncoder* enc, const JxlHipEncodeImage* images, size_t num_images, void* hip_stream);
/* Results of the last call: Status 0 = encoded, 1 = failed (with that image's message as the last-error text); Size 0 for a failed image; Copy returns 1 and writes nothing if
 * `capacity` is below Size.  MaxToken: the largest hybrid-uint token of the image (71 is the largest there is). */
int JxlHipEncoderStatus(JxlHipEncoder* enc, size_t index);
size_t JxlHipEncoderSize(JxlHipEncoder* enc, size_t index);
int JxlHipEncoderCopy(JxlHipEncoder* enc, size_t index, uint8_t* dst, size_t capacity);
uint32_t JxlHipEncoderMaxToken(JxlHipEncoder* enc, size_t index);
/* Wall-clock ms of the last call's phases: upload, tokenise + histogram readback, host code build, count + scans + size readback, pack, copy back, splice. */
#define JXL_HIP_ENCODE_PHASES 7
void JxlHipEncoderPhaseTimes(JxlHipEncoder* enc, float* ms);

/* ---- extension: the gather of decoded pixels over RCCL / xGMI (csrc/gather.cc) --------------------------------------------------
 * The multi-GPU path shards independent frames over one process per GPU and has ONE exchange step: the decoded pixels go to the consumer rank.  These
 * calls put it behind the C ABI so that a caller needs no PyTorch: rank 0 makes an id, the job hands it to the other ranks (file, environment, MPI ...), every rank
 * creates its communicator (world = 1 needs no id exchange and no RCCL).  librccl.so is loaded on first use.  All calls return 0 on success (JxlHipLastError). */
#define JXL_HIP_COMM_ID_BYTES 128
typedef struct JxlHipCommStruct JxlHipComm;
int JxlHipCommGetUniqueId(uint8_t id[JXL_HIP_COMM_ID_BYTES]);
JxlHipComm* JxlHipCommCreate(int device, int rank, int world, const uint8_t id[JXL_HIP_COMM_ID_BYTES]);
void JxlHipCommDestroy(JxlHipComm* comm);
/* Every rank holds `frames` decoded frames of frame_bytes each at `send` (device memory); `root` receives them at recv[rank][frame] (device memory, world x frames x
 * frame_bytes; ignored elsewhere) as point-to-point messages of chunk_frames frames, all peers of a chunk in one group — each over its own xGMI link — enqueued on
 * hip_stream.  The root's own shard is a device copy (skipped when send already points into recv). */
int JxlHipGatherFrames(JxlHipComm* comm, const void* send, size_t frame_bytes, int frames, void* recv, int root, int chunk_frames, void* hip_stream);
/* Shards of unequal length (1024 frames over 3, 5, 6, 7 GPUs): rank r holds frames_per_rank[r] frames, the root receives them in rank order (the frame order of the
 * unsharded job). */
int JxlHipGatherFramesRagged(JxlHipComm* comm, const void* send, size_t frame_bytes, const int* frames_per_rank, void* recv, int root, int chunk_frames, void* hip_stream);
/* Sum over the ranks, in place (per-rank consumers exchange checksums, not pixels). */
int JxlHipAllReduceSumI64(JxlHipComm* comm, int64_t* device_values, size_t count, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* JXL_HIP_H_ */
