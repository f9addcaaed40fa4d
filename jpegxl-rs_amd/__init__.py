"""jpegxl-rs_amd — host-side mirror of the jpegxl-rs decoder API on top of the MI355X-native C ABI (include/jxl_hip.h).

The reference's host language (Rust) is not available in the build image, so the layer above the C ABI is mirrored
here in Python with the same names, argument meaning and error behaviour as jpegxl-rs:

    decoder_builder()                      -> jpegxl-rs/src/decode.rs:535  (bon builder; options are keyword args)
    JxlDecoder.decode(data)                -> decode.rs:440   (pixel type inferred from the header)
    JxlDecoder.decode_with(data, dtype)    -> decode.rs:461   (decode_with::<T>)
    JxlDecoder.reconstruct(data)           -> decode.rs:493
    Metadata / Pixels / PixelFormat        -> decode/result.rs:26-76, decode.rs:49-82
    DecodeError subclasses                 -> errors.rs:27-52
    ThreadsRunner / ResizableRunner        -> parallel/threads_runner.rs, parallel/resizable_runner.rs
    check_valid_signature                  -> utils.rs:25-33

Everything goes through ctypes into lib/libjxl.so (hand-written HIP kernels); there is no CPU fallback: without the
built library or without a GPU the calls fail loudly.
"""
import ctypes as C
import os
import sys
from dataclasses import dataclass
from typing import Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(_HERE, "lib")
LIBJXL_PATH = os.environ.get("JXL_HIP_LIBJXL") or os.path.join(LIB_DIR, "libjxl.so")      # (override: A/B runs of kernel variants)
LIBTHREADS_PATH = os.path.join(LIB_DIR, "libjxl_threads.so")

# ---- C types (include/jxl_hip.h) ------------------------------------------------------------------------------------
JXL_TYPE_FLOAT, JXL_TYPE_UINT8, JXL_TYPE_UINT16, JXL_TYPE_FLOAT16 = 0, 2, 3, 5
JXL_NATIVE_ENDIAN, JXL_LITTLE_ENDIAN, JXL_BIG_ENDIAN = 0, 1, 2
(JXL_DEC_SUCCESS, JXL_DEC_ERROR, JXL_DEC_NEED_MORE_INPUT, JXL_DEC_NEED_PREVIEW_OUT_BUFFER, JXL_DEC_NEED_IMAGE_OUT_BUFFER,
 JXL_DEC_JPEG_NEED_MORE_OUTPUT, JXL_DEC_BOX_NEED_MORE_OUTPUT) = 0, 1, 2, 3, 5, 6, 7
JXL_DEC_BASIC_INFO, JXL_DEC_COLOR_ENCODING, JXL_DEC_PREVIEW_IMAGE, JXL_DEC_FRAME = 0x40, 0x100, 0x200, 0x400
JXL_DEC_FULL_IMAGE, JXL_DEC_JPEG_RECONSTRUCTION, JXL_DEC_BOX, JXL_DEC_FRAME_PROGRESSION, JXL_DEC_BOX_COMPLETE = 0x1000, 0x2000, 0x4000, 0x8000, 0x10000
JXL_HIP_JPEG_DEVICE_PROGRESSIVE, JXL_HIP_JPEG_HOST_WRITER = 1, 2      # flags of JxlHipPipelineSubmitJpegs


class JxlPixelFormat(C.Structure):
    _fields_ = [("num_channels", C.c_uint32), ("data_type", C.c_int), ("endianness", C.c_int), ("align", C.c_size_t)]


class JxlBasicInfo(C.Structure):
    _fields_ = [("have_container", C.c_int), ("xsize", C.c_uint32), ("ysize", C.c_uint32), ("bits_per_sample", C.c_uint32),
                ("exponent_bits_per_sample", C.c_uint32), ("intensity_target", C.c_float), ("min_nits", C.c_float),
                ("relative_to_max_display", C.c_int), ("linear_below", C.c_float), ("uses_original_profile", C.c_int),
                ("have_preview", C.c_int), ("have_animation", C.c_int), ("orientation", C.c_int32), ("num_color_channels", C.c_uint32),
                ("num_extra_channels", C.c_uint32), ("alpha_bits", C.c_uint32), ("alpha_exponent_bits", C.c_uint32),
                ("alpha_premultiplied", C.c_int), ("preview_xsize", C.c_uint32), ("preview_ysize", C.c_uint32),
                ("tps_numerator", C.c_uint32), ("tps_denominator", C.c_uint32), ("num_loops", C.c_uint32), ("have_timecodes", C.c_int),
                ("intrinsic_xsize", C.c_uint32), ("intrinsic_ysize", C.c_uint32), ("padding", C.c_uint8 * 100)]


class JxlMemoryManager(C.Structure):
    _fields_ = [("opaque", C.c_void_p), ("alloc", C.c_void_p), ("free", C.c_void_p)]


class JxlColorEncoding(C.Structure):
    """jpegxl-sys color/color_encoding.rs:125-159"""
    _fields_ = [("color_space", C.c_int), ("white_point", C.c_int), ("white_point_xy", C.c_double * 2), ("primaries", C.c_int), ("primaries_red_xy", C.c_double * 2),
                ("primaries_green_xy", C.c_double * 2), ("primaries_blue_xy", C.c_double * 2), ("transfer_function", C.c_int), ("gamma", C.c_double), ("rendering_intent", C.c_int)]


class JxlExtraChannelInfo(C.Structure):
    """jpegxl-sys metadata/codestream_header.rs:247-279"""
    _fields_ = [("type", C.c_int), ("bits_per_sample", C.c_uint32), ("exponent_bits_per_sample", C.c_uint32), ("dim_shift", C.c_uint32), ("name_length", C.c_uint32),
                ("alpha_premultiplied", C.c_int), ("spot_color", C.c_float * 4), ("cfa_channel", C.c_uint32)]


class JxlBlendInfo(C.Structure):
    """jpegxl-sys/src/metadata/codestream_header.rs:305-315"""
    _fields_ = [("blendmode", C.c_int), ("source", C.c_uint32), ("alpha", C.c_uint32), ("clamp", C.c_int)]


class JxlLayerInfo(C.Structure):
    """codestream_header.rs:323-353"""
    _fields_ = [("have_crop", C.c_int), ("crop_x0", C.c_int32), ("crop_y0", C.c_int32), ("xsize", C.c_uint32), ("ysize", C.c_uint32),
                ("blend_info", JxlBlendInfo), ("save_as_reference", C.c_uint32)]


class JxlFrameHeader(C.Structure):
    """codestream_header.rs:358-388"""
    _fields_ = [("duration", C.c_uint32), ("timecode", C.c_uint32), ("name_length", C.c_uint32), ("is_last", C.c_int), ("layer_info", JxlLayerInfo)]


class JxlHipStageTimes(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("lf_ms", "lfpost_ms", "hf_ms", "idct_ms", "filter_ms", "out_ms", "total_ms")]


class JxlHipPipelineOptions(C.Structure):
    """include/jxl_hip.h JxlHipPipelineOptions (0 / negative = the library's default)"""
    _fields_ = [(n, C.c_int32) for n in ("jobs_in_flight", "lf_streams", "hf_streams", "prepare_threads", "parse_threads", "lane_stride_lf", "lane_stride_hf", "wide_first",
                                         "small_job_frames", "timed", "reserve_frames", "reserve_width", "reserve_height", "reserve_plane_sets")]


class JxlHipOutputLayout(C.Structure):
    """include/jxl_hip.h JxlHipOutputLayout: planar (CHW) planes and / or a per-slot scale and bias for float output"""
    _fields_ = [("planar", C.c_int), ("plane_stride", C.c_size_t), ("affine", C.c_int), ("scale", C.c_float * 4), ("bias", C.c_float * 4)]


class JxlHipOutputResize(C.Structure):
    """include/jxl_hip.h JxlHipOutputResize: the output's size, and the rectangle of the decoded picture that is resampled into it (all zero: the whole picture)"""
    _fields_ = [(n, C.c_uint32) for n in ("xsize", "ysize", "crop_x0", "crop_y0", "crop_xsize", "crop_ysize")]


class JxlHipOutputResample(C.Structure):
    """include/jxl_hip.h JxlHipOutputResample: JxlHipOutputResize with a filter (0 triangle, 1 cubic) and a mirror of the image's own"""
    _fields_ = [(n, C.c_uint32) for n in ("xsize", "ysize", "crop_x0", "crop_y0", "crop_xsize", "crop_ysize", "filter")] + [("mirror", C.c_int)]


class JxlHipOutputPlanes(C.Structure):
    """include/jxl_hip.h JxlHipOutputPlanes: extra channels as planes behind the colour output (indices, where the first plane starts, the pitch, per-plane scale / bias)"""
    _fields_ = [("num_planes", C.c_uint32), ("extra_index", C.POINTER(C.c_uint32)), ("offset", C.c_size_t), ("plane_stride", C.c_size_t),
                ("scale", C.POINTER(C.c_float)), ("bias", C.POINTER(C.c_float))]


class JxlHipOutputColor(C.Structure):
    """include/jxl_hip.h JxlHipOutputColor: the colour encoding the output is asked for in, and what becomes of images that are not XYB (0 leave, 1 convert)"""
    _fields_ = [("encoding", JxlColorEncoding), ("non_xyb", C.c_uint32)]


assert C.sizeof(JxlBasicInfo) == 204 and C.sizeof(JxlPixelFormat) == 24 and C.sizeof(JxlMemoryManager) == 24

_lib = None
_threads = None


class JxlHipEncodeImage(C.Structure):
    _fields_ = [("pixels", C.c_void_p), ("on_device", C.c_int), ("xsize", C.c_uint32), ("ysize", C.c_uint32), ("num_channels", C.c_uint32),
                ("bits_per_sample", C.c_uint32), ("data_type", C.c_int), ("row_pitch", C.c_size_t), ("alpha_premultiplied", C.c_int)]


class JxlBitDepth(C.Structure):
    """jpegxl-sys/src/common/types.rs:133-144"""
    _fields_ = [("type", C.c_int), ("bits_per_sample", C.c_uint32), ("exponent_bits_per_sample", C.c_uint32)]


class NativeLibraryMissing(RuntimeError):
    pass


def libjxl():
    """Loads lib/libjxl.so (the HIP decode path).  Fails loudly if it has not been built — there is no fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIBJXL_PATH):
            raise NativeLibraryMissing(f"{LIBJXL_PATH} not built: run __graft_entry__.build() (hipcc --offload-arch=gfx950)")
        L = C.CDLL(LIBJXL_PATH, mode=C.RTLD_GLOBAL)
        vp, u8p, sz = C.c_void_p, C.c_char_p, C.c_size_t
        sig = {
            "JxlDecoderVersion": (C.c_uint32, []), "JxlSignatureCheck": (C.c_int, [u8p, sz]),
            "JxlDecoderCreate": (vp, [vp]), "JxlDecoderReset": (None, [vp]), "JxlDecoderDestroy": (None, [vp]),
            "JxlDecoderSetParallelRunner": (C.c_int, [vp, vp, vp]), "JxlDecoderSubscribeEvents": (C.c_int, [vp, C.c_int]),
            "JxlDecoderSetKeepOrientation": (C.c_int, [vp, C.c_int]), "JxlDecoderSetUnpremultiplyAlpha": (C.c_int, [vp, C.c_int]),
            "JxlDecoderSetRenderSpotcolors": (C.c_int, [vp, C.c_int]), "JxlDecoderSetCoalescing": (C.c_int, [vp, C.c_int]),
            "JxlDecoderProcessInput": (C.c_int, [vp]), "JxlDecoderSetInput": (C.c_int, [vp, vp, sz]), "JxlDecoderCloseInput": (None, [vp]),
            "JxlDecoderGetBasicInfo": (C.c_int, [vp, C.POINTER(JxlBasicInfo)]),
            "JxlDecoderGetICCProfileSize": (C.c_int, [vp, C.c_int, C.POINTER(sz)]),
            "JxlDecoderGetColorAsICCProfile": (C.c_int, [vp, C.c_int, vp, sz]),
            "JxlDecoderSetDesiredIntensityTarget": (C.c_int, [vp, C.c_float]),
            "JxlDecoderImageOutBufferSize": (C.c_int, [vp, C.POINTER(JxlPixelFormat), C.POINTER(sz)]),
            "JxlDecoderSetImageOutBuffer": (C.c_int, [vp, C.POINTER(JxlPixelFormat), vp, sz]),
            "JxlDecoderGetColorAsEncodedProfile": (C.c_int, [vp, C.c_int, C.POINTER(JxlColorEncoding)]),
            "JxlDecoderGetExtraChannelInfo": (C.c_int, [vp, sz, C.POINTER(JxlExtraChannelInfo)]),
            "JxlDecoderGetExtraChannelName": (C.c_int, [vp, sz, C.c_char_p, sz]),
            "JxlDecoderSizeHintBasicInfo": (sz, [vp]),
            "JxlDecoderGetIntendedDownsamplingRatio": (sz, [vp]),
            "JxlDecoderPreviewOutBufferSize": (C.c_int, [vp, C.POINTER(JxlPixelFormat), C.POINTER(sz)]),
            "JxlDecoderSetPreviewOutBuffer": (C.c_int, [vp, C.POINTER(JxlPixelFormat), vp, sz]),
            "JxlDecoderReleaseInput": (sz, [vp]), "JxlDecoderSetJPEGBuffer": (C.c_int, [vp, vp, sz]), "JxlDecoderReleaseJPEGBuffer": (sz, [vp]),
            "JxlDecoderGetFrameHeader": (C.c_int, [vp, C.POINTER(JxlFrameHeader)]), "JxlDecoderGetFrameName": (C.c_int, [vp, C.c_char_p, sz]),
            "JxlDecoderGetExtraChannelBlendInfo": (C.c_int, [vp, sz, C.POINTER(JxlBlendInfo)]), "JxlDecoderSkipFrames": (None, [vp, sz]),
            "JxlDecoderSkipCurrentFrame": (C.c_int, [vp]), "JxlDecoderRewind": (None, [vp]),
            "JxlDecoderSetMultithreadedImageOutCallback": (C.c_int, [vp, C.POINTER(JxlPixelFormat), vp, vp, vp, vp]),
            "JxlDecoderExtraChannelBufferSize": (C.c_int, [vp, C.POINTER(JxlPixelFormat), C.POINTER(sz), C.c_uint32]),
            "JxlDecoderSetExtraChannelBuffer": (C.c_int, [vp, C.POINTER(JxlPixelFormat), vp, sz, C.c_uint32]),
            "JxlDecoderSetBoxBuffer": (C.c_int, [vp, vp, sz]), "JxlDecoderReleaseBoxBuffer": (sz, [vp]),
            "JxlDecoderSetDecompressBoxes": (C.c_int, [vp, C.c_int]), "JxlDecoderGetBoxType": (C.c_int, [vp, C.c_char_p, C.c_int]),
            "JxlDecoderGetBoxSizeRaw": (C.c_int, [vp, C.POINTER(C.c_uint64)]), "JxlDecoderGetBoxSizeContents": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
            "JxlDecoderSetProgressiveDetail": (C.c_int, [vp, C.c_int]), "JxlDecoderFlushImage": (C.c_int, [vp]),
            "JxlDecoderSetImageOutBitDepth": (C.c_int, [vp, C.POINTER(JxlBitDepth)]),
            "JxlHipLastError": (C.c_char_p, []), "JxlHipBatchCreate": (vp, [C.c_int]), "JxlHipBatchDestroy": (None, [vp]),
            "JxlHipBatchAddImage": (C.c_int, [vp, vp, sz]), "JxlHipBatchGetBasicInfo": (C.c_int, [vp, C.c_int, C.POINTER(JxlBasicInfo)]),
            "JxlHipBatchOutBufferSize": (C.c_int, [vp, C.c_int, C.POINTER(JxlPixelFormat), C.POINTER(sz)]),
            "JxlHipBatchSetOutput": (C.c_int, [vp, C.c_int, C.POINTER(JxlPixelFormat), vp]),
            "JxlHipBatchOutBufferSizeScaled": (C.c_int, [vp, C.c_int, C.POINTER(JxlPixelFormat), C.c_int, C.POINTER(sz)]),
            "JxlHipBatchSetOutputScaled": (C.c_int, [vp, C.c_int, C.POINTER(JxlPixelFormat), vp, C.c_int]),
            "JxlHipPipelineSubmitScaled": (C.c_int64, [vp, C.POINTER(C.c_char_p), C.POINTER(sz), C.c_int, C.POINTER(JxlPixelFormat), C.POINTER(vp), C.POINTER(vp), C.POINTER(sz), C.c_int]),
            "JxlHipImageOutSizeScaled": (C.c_int, [vp, sz, C.POINTER(JxlPixelFormat), C.c_int, C.POINTER(JxlBasicInfo), C.POINTER(sz)]),
            "JxlHipBatchOutBufferSizeLayout": (C.c_int, [vp, C.c_int, C.POINTER(JxlPixelFormat), C.c_int, C.POINTER(JxlHipOutputLayout), C.POINTER(sz)]),
            "JxlHipBatchSetOutputLayout": (C.c_int, [vp, C.c_int, C.POINTER(JxlPixelFormat), vp, C.c_int, C.POINTER(JxlHipOutputLayout)]),
            "JxlHipPipelineSubmitLayout": (C.c_int64, [vp, C.POINTER(C.c_char_p), C.POINTER(sz), C.c_int, C.POINTER(JxlPixelFormat), C.POINTER(vp), C.POINTER(vp), C.POINTER(sz), C.c_int,
                                                       C.POINTER(JxlHipOutputLayout)]),
            "JxlHipImageOutSizeLayout": (C.c_int, [vp, sz, C.POINTER(JxlPixelFormat), C.c_int, C.POINTER(JxlHipOutputLayout), C.POINTER(JxlBasicInfo), C.POINTER(sz)]),
            "JxlHipBatchOutBufferSizeResized": (C.c_int, [vp, C.c_int, C.POINTER(JxlPixelFormat), C.c_int, C.POINTER(JxlHipOutputLayout), C.POINTER(JxlHipOutputResize), C.POINTER(sz)]),
            "JxlHipBatchSetOutputResized": (C.c_int, [vp, C.c_int, C.POINTER(JxlPixelFormat), vp, C.c_int, C.POINTER(JxlHipOutputLayout), C.POINTER(JxlHipOutputResize)]),
            "JxlHipPipelineSubmitResized": (C.c_int64, [vp, C.POINTER(C.c_char_p), C.POINTER(sz), C.c_int, C.POINTER(JxlPixelFormat), C.POINTER(vp), C.POINTER(vp), C.POINTER(sz), C.c_int,
                                                        C.POINTER(JxlHipOutputLayout), C.POINTER(JxlHipOutputResize)]),
            "JxlHipImageOutSizeResized": (C.c_int, [vp, sz, C.POINTER(JxlPixelFormat), C.c_int, C.POINTER(JxlHipOutputLayout), C.POINTER(JxlHipOutputResize), C.POINTER(JxlBasicInfo),
                                                    C.POINTER(sz)]),
            "JxlHipBatchOutBufferSizeResampled": (C.c_int, [vp, C.c_int, C.POINTER(JxlPixelFormat), C.c_int, C.POINTER(JxlHipOutputLayout), C.POINTER(JxlHipOutputResample), C.POINTER(sz)]),
            "JxlHipBatchSetOutputResampled": (C.c_int, [vp, C.c_int, C.POINTER(JxlPixelFormat), vp, C.c_int, C.POINTER(JxlHipOutputLayout), C.POINTER(JxlHipOutputResample)]),
            "JxlHipPipelineSubmitResampled": (C.c_int64, [vp, C.POINTER(C.c_char_p), C.POINTER(sz), C.c_int, C.POINTER(JxlPixelFormat), C.POINTER(vp), C.POINTER(vp), C.POINTER(sz), C.c_int,
                                                          C.POINTER(JxlHipOutputLayout), C.POINTER(JxlHipOutputResample)]),
            "JxlHipBatchSetOutputPlanes": (C.c_int, [vp, C.c_int, C.POINTER(JxlHipOutputPlanes)]),
            "JxlHipBatchOutputPlanesLayout": (C.c_int, [vp, C.c_int, C.POINTER(sz), C.POINTER(sz), C.POINTER(sz)]),
            "JxlHipPipelineSubmitPlanes": (C.c_int64, [vp, C.POINTER(C.c_char_p), C.POINTER(sz), C.c_int, C.POINTER(JxlPixelFormat), C.POINTER(vp), C.POINTER(vp), C.POINTER(sz), C.c_int,
                                                       C.POINTER(JxlHipOutputLayout), C.POINTER(JxlHipOutputResample), C.POINTER(JxlHipOutputPlanes)]),
            "JxlHipImageOutSizePlanes": (C.c_int, [vp, sz, C.POINTER(JxlPixelFormat), C.c_int, C.POINTER(JxlHipOutputLayout), C.POINTER(JxlHipOutputResample), C.POINTER(JxlHipOutputPlanes),
                                                   C.POINTER(JxlBasicInfo), C.POINTER(sz)]),
            "JxlHipDecoderSetOutputColorProfile": (C.c_int, [vp, C.POINTER(JxlColorEncoding), vp, sz]),
            "JxlHipBatchSetOutputColor": (C.c_int, [vp, C.c_int, C.POINTER(JxlHipOutputColor)]),
            "JxlHipColorConversionMatrix": (C.c_int, [C.POINTER(JxlColorEncoding), C.POINTER(JxlColorEncoding), C.POINTER(C.c_double * 9)]),
            "JxlHipPipelineSubmitColor": (C.c_int64, [vp, C.POINTER(C.c_char_p), C.POINTER(sz), C.c_int, C.POINTER(JxlPixelFormat), C.POINTER(vp), C.POINTER(vp), C.POINTER(sz), C.c_int,
                                                      C.POINTER(JxlHipOutputLayout), C.POINTER(JxlHipOutputResample), C.POINTER(JxlHipOutputPlanes), C.POINTER(JxlHipOutputColor)]),
            "JxlHipDecoderInfo": (C.c_int64, [vp, C.c_char_p]),
            "JxlHipBatchCanReconstructJpeg": (C.c_int, [vp, C.c_int]), "JxlHipBatchReconstructJpegs": (C.c_int, [vp, vp]),
            "JxlHipBatchJpegStatus": (C.c_int, [vp, C.c_int]), "JxlHipBatchJpegSize": (sz, [vp, C.c_int]), "JxlHipBatchCopyJpeg": (C.c_int, [vp, C.c_int, vp, sz]),
            "JxlHipPipelineSubmitJpegPixels": (C.c_int64, [vp, C.POINTER(C.c_char_p), C.POINTER(sz), C.c_int, C.POINTER(JxlPixelFormat), C.POINTER(vp), C.POINTER(vp), C.POINTER(sz),
                                                           C.POINTER(JxlHipOutputLayout), C.POINTER(JxlHipOutputResample)]),
            "JxlHipPipelineSubmitJpegPixelsScaled": (C.c_int64, [vp, C.POINTER(C.c_char_p), C.POINTER(sz), C.c_int, C.POINTER(JxlPixelFormat), C.POINTER(vp), C.POINTER(vp), C.POINTER(sz),
                                                                 C.POINTER(JxlHipOutputLayout), C.POINTER(JxlHipOutputResample), C.c_int]),
            "JxlHipPipelineSubmitJpegPixelsResampled": (C.c_int64, [vp, C.POINTER(C.c_char_p), C.POINTER(sz), C.c_int, C.POINTER(JxlPixelFormat), C.POINTER(vp), C.POINTER(vp), C.POINTER(sz),
                                                                    C.POINTER(JxlHipOutputLayout), C.POINTER(JxlHipOutputResample), C.c_int, C.c_uint32]),
            "JxlHipBatchSetOutputJpegResampled": (C.c_int, [vp, C.c_int, C.POINTER(JxlPixelFormat), vp, C.c_int, C.POINTER(JxlHipOutputLayout), C.POINTER(JxlHipOutputResample), C.c_uint32]),
            "JxlHipBatchOutBufferSizeJpegScaled": (C.c_int, [vp, C.c_int, C.POINTER(JxlPixelFormat), C.c_int, C.POINTER(JxlHipOutputLayout), C.POINTER(JxlHipOutputResample), C.POINTER(sz)]),
            "JxlHipBatchSetOutputJpegScaled": (C.c_int, [vp, C.c_int, C.POINTER(JxlPixelFormat), vp, C.c_int, C.POINTER(JxlHipOutputLayout), C.POINTER(JxlHipOutputResample)]),
            "JxlHipImageOutSizeJpegScaled": (C.c_int, [vp, sz, C.POINTER(JxlPixelFormat), C.c_int, C.POINTER(JxlHipOutputLayout), C.POINTER(JxlHipOutputResample), C.POINTER(JxlBasicInfo),
                                                       C.POINTER(sz)]),
            "JxlHipBatchCanDecodeJpegPixels": (C.c_int, [vp, C.c_int]), "JxlHipBatchDecodeJpegPixels": (C.c_int, [vp, vp]), "JxlHipBatchJpegPixelsStatus": (C.c_int, [vp, C.c_int]),
            "JxlHipBatchJpegDcOnly": (C.c_int, [vp, C.c_int]), "JxlHipBatchJpegRegion": (C.c_int, [vp, C.c_int, C.POINTER(C.c_uint32 * 4)]),
            "JxlHipPipelineSetOption": (None, [vp, C.c_char_p, C.c_int]), "JxlHipLfPartSize": (C.c_int, [vp, sz, C.POINTER(sz)]),
            "JxlHipBatchSetLaneStride": (None, [vp, C.c_int, C.c_int]), "JxlHipBatchSetOption": (None, [vp, C.c_char_p, C.c_int]),
            "JxlHipBatchPrepare": (C.c_int, [vp, vp]), "JxlHipBatchDecode": (C.c_int, [vp, vp]),
            "JxlHipBatchDecodeTimed": (C.c_int, [vp, vp]), "JxlHipBatchFinish": (C.c_int, [vp, vp]),
            "JxlHipBatchDecodePart": (C.c_int, [vp, vp, C.c_int, C.c_int]),
            "JxlHipBatchCollectTimes": (C.c_int, [vp, C.POINTER(JxlHipStageTimes), C.POINTER(C.c_int)]),
            "JxlHipBatchDeviceOutput": (vp, [vp, C.c_int]), "JxlHipBatchCopyOutput": (C.c_int, [vp, C.c_int, vp, sz, vp]),
            "JxlHipBatchTotalPixels": (C.c_uint64, [vp]), "JxlHipBatchCompressedBytes": (C.c_uint64, [vp]),
            "JxlHipBatchStageBytes": (None, [vp, C.POINTER(C.c_uint64 * 6)]), "JxlHipBatchDeviceBytes": (C.c_uint64, [vp]),
            "JxlHipBatchGetInfo": (C.c_int64, [vp, C.c_char_p]), "JxlHipBatchReset": (None, [vp]),
            "JxlHipBatchDebugRead": (sz, [vp, C.c_int, C.c_char_p, C.c_int, vp, sz, vp]),
            "JxlHipBatchAddImages": (C.c_int, [vp, C.POINTER(C.c_char_p), C.POINTER(sz), C.c_int, C.c_int]),
            "JxlHipBatchShareBuffers": (C.c_int, [vp, vp]), "JxlHipBatchShareCoefficients": (C.c_int, [vp, vp]),
            "JxlHipPipelineCreate": (vp, [C.c_int, C.POINTER(JxlHipPipelineOptions)]), "JxlHipPipelineDestroy": (None, [vp]),
            "JxlHipPipelineSubmit": (C.c_int64, [vp, C.POINTER(C.c_char_p), C.POINTER(sz), C.c_int, C.POINTER(JxlPixelFormat), C.POINTER(vp), C.POINTER(vp), C.POINTER(sz)]),
            "JxlHipPipelineWait": (C.c_int, [vp, C.c_int64, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_float)]),
            "JxlHipPipelineSubmitJpegs": (C.c_int64, [vp, C.POINTER(C.c_char_p), C.POINTER(sz), C.c_int, C.c_uint32]),
            "JxlHipPipelineWaitJpegs": (C.c_int, [vp, C.c_int64, C.POINTER(C.c_int), C.POINTER(sz), C.c_int, C.POINTER(C.c_float)]),
            "JxlHipPipelineJpegStatus": (C.c_int, [vp, C.c_int64, C.c_int]), "JxlHipPipelineCopyJpeg": (C.c_int, [vp, C.c_int64, C.c_int, vp, sz]),
            "JxlHipPipelineReleaseJpegs": (None, [vp, C.c_int64]),
            "JxlHipPipelineWaitAll": (C.c_int, [vp]), "JxlHipPipelineResetClock": (C.c_int, [vp]),
            "JxlHipPipelineCollectTimes": (C.c_int, [vp, C.POINTER(JxlHipStageTimes), C.POINTER(C.c_int)]),
            "JxlHipPipelineStageBytes": (None, [vp, C.POINTER(C.c_uint64 * 6)]), "JxlHipPipelineGetInfo": (C.c_int64, [vp, C.c_char_p]),
            "JxlHipHostAlloc": (vp, [sz]), "JxlHipHostFree": (None, [vp]),
            "JxlHipImageOutSize": (C.c_int, [vp, sz, C.POINTER(JxlPixelFormat), C.POINTER(JxlBasicInfo), C.POINTER(sz)]),
            "JxlHipArenaPoolTrim": (sz, []), "JxlHipArenaPoolHeld": (sz, []),
            "JxlHipCommGetUniqueId": (C.c_int, [vp]), "JxlHipCommCreate": (vp, [C.c_int, C.c_int, C.c_int, vp]), "JxlHipCommDestroy": (None, [vp]),
            "JxlHipGatherFrames": (C.c_int, [vp, vp, sz, C.c_int, vp, C.c_int, C.c_int, vp]),
            "JxlHipGatherFramesRagged": (C.c_int, [vp, vp, sz, C.POINTER(C.c_int), vp, C.c_int, C.c_int, vp]),
            "JxlHipAllReduceSumI64": (C.c_int, [vp, vp, sz, vp]),
            "JxlHipSchedulerStats": (None, [C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]), "JxlHipSchedulerShutdown": (None, []),
            "JxlHipEncoderCreate": (vp, [C.c_int]), "JxlHipEncoderDestroy": (None, [vp]),
            "JxlHipEncodeLosslessBound": (C.c_int, [C.POINTER(JxlHipEncodeImage), C.POINTER(sz)]),
            "JxlHipEncoderEncodeLossless": (C.c_int, [vp, C.POINTER(JxlHipEncodeImage), sz, vp]),
            "JxlHipEncoderStatus": (C.c_int, [vp, sz]), "JxlHipEncoderSize": (sz, [vp, sz]), "JxlHipEncoderCopy": (C.c_int, [vp, sz, vp, sz]),
            "JxlHipEncoderMaxToken": (C.c_uint32, [vp, sz]), "JxlHipEncoderPhaseTimes": (None, [vp, C.POINTER(C.c_float * 7)]),
        }
        for name, (res, args) in sig.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def libjxl_threads():
    global _threads
    if _threads is None:
        if not os.path.exists(LIBTHREADS_PATH):
            raise NativeLibraryMissing(f"{LIBTHREADS_PATH} not built: run __graft_entry__.build()")
        T = C.CDLL(LIBTHREADS_PATH)
        vp = C.c_void_p
        T.JxlThreadParallelRunnerCreate.restype = vp; T.JxlThreadParallelRunnerCreate.argtypes = [vp, C.c_size_t]
        T.JxlThreadParallelRunnerDestroy.argtypes = [vp]
        T.JxlThreadParallelRunnerDefaultNumWorkerThreads.restype = C.c_size_t
        T.JxlResizableParallelRunnerCreate.restype = vp; T.JxlResizableParallelRunnerCreate.argtypes = [vp]
        T.JxlResizableParallelRunnerDestroy.argtypes = [vp]
        T.JxlResizableParallelRunnerSetThreads.argtypes = [vp, C.c_size_t]
        T.JxlResizableParallelRunnerSuggestThreads.restype = C.c_uint32
        T.JxlResizableParallelRunnerSuggestThreads.argtypes = [C.c_uint64, C.c_uint64]
        _threads = T
    return _threads


def last_error() -> str:
    return libjxl().JxlHipLastError().decode()


# ---- errors (jpegxl-rs/src/errors.rs:27-52) ---------------------------------------------------------------------------
class DecodeError(Exception):
    pass


class CannotCreateDecoder(DecodeError):
    pass


class GenericError(DecodeError):
    pass


class InvalidInput(DecodeError):
    pass


class UnsupportedBitWidth(DecodeError):
    pass


class InternalError(DecodeError):
    pass


class UnknownStatus(DecodeError):
    pass


class NotImplementedFeature(DecodeError):
    pass


def check_dec_status(status: int):
    """errors.rs:93-99"""
    if status == JXL_DEC_SUCCESS:
        return
    if status == JXL_DEC_ERROR:
        raise GenericError(last_error())
    raise UnknownStatus(status)


def check_valid_signature(buf: bytes) -> Optional[bool]:
    """utils.rs:25-33: None = not enough bytes, False = invalid, True = codestream or container."""
    r = libjxl().JxlSignatureCheck(buf, len(buf))
    if r == 0:
        return None
    return r in (2, 3)


# ---- common (jpegxl-rs/src/common.rs) -----------------------------------------------------------------------------------
def icc_profile_from_headers(buf: bytes) -> bytes:
    """Extension (host-only, no GPU): the ICC profile JxlDecoderGetColorAsICCProfile reports for this file (decode.rs:368-385)."""
    L = libjxl()
    L.JxlHipColorProfileFromHeaders.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_size_t)]
    L.JxlHipColorProfileFromHeaders.restype = C.c_int
    size = C.c_size_t(0)
    if L.JxlHipColorProfileFromHeaders(buf, len(buf), None, C.byref(size)):
        raise GenericError(last_error())
    out = (C.c_uint8 * size.value)()
    if L.JxlHipColorProfileFromHeaders(buf, len(buf), out, C.byref(size)):
        raise GenericError(last_error())
    return bytes(out)


class Endianness:
    Native, Little, Big = JXL_NATIVE_ENDIAN, JXL_LITTLE_ENDIAN, JXL_BIG_ENDIAN


_PIXEL_TYPES = {  # numpy dtype name -> (JxlDataType, bits, exponent bits)   common.rs:59-124
    "uint8": (JXL_TYPE_UINT8, 8, 0), "uint16": (JXL_TYPE_UINT16, 16, 0), "float32": (JXL_TYPE_FLOAT, 32, 8), "float16": (JXL_TYPE_FLOAT16, 16, 5)}


@dataclass
class PixelFormat:
    """decode.rs:49-82 — num_channels 0 = colour channels + alpha (if present)."""
    num_channels: int = 0
    endianness: int = Endianness.Native
    align: int = 0


@dataclass
class Metadata:
    """decode/result.rs:26-49"""
    width: int
    height: int
    intensity_target: float
    min_nits: float
    orientation: int
    num_color_channels: int
    has_alpha_channel: bool
    intrinsic_width: int
    intrinsic_height: int
    icc_profile: Optional[bytes] = None


# ---- parallel runners ---------------------------------------------------------------------------------------------------
class ThreadsRunner:
    """parallel/threads_runner.rs:30-89"""

    def __init__(self, num_workers: Optional[int] = None):
        T = libjxl_threads()
        n = T.JxlThreadParallelRunnerDefaultNumWorkerThreads() if num_workers is None else num_workers
        self._ptr = T.JxlThreadParallelRunnerCreate(None, n)
        if not self._ptr:
            raise CannotCreateDecoder("thread runner")

    def runner(self):
        return C.cast(libjxl_threads().JxlThreadParallelRunner, C.c_void_p)

    def as_opaque_ptr(self):
        return self._ptr

    def callback_basic_info(self, info):
        pass

    def __del__(self):
        if getattr(self, "_ptr", None):
            libjxl_threads().JxlThreadParallelRunnerDestroy(self._ptr)
            self._ptr = None


class ResizableRunner:
    """parallel/resizable_runner.rs:29-87"""

    def __init__(self):
        self._ptr = libjxl_threads().JxlResizableParallelRunnerCreate(None)
        if not self._ptr:
            raise CannotCreateDecoder("resizable runner")

    def runner(self):
        return C.cast(libjxl_threads().JxlResizableParallelRunner, C.c_void_p)

    def as_opaque_ptr(self):
        return self._ptr

    def callback_basic_info(self, info):  # resizable_runner.rs:78-80
        T = libjxl_threads()
        T.JxlResizableParallelRunnerSetThreads(self._ptr, T.JxlResizableParallelRunnerSuggestThreads(info.xsize, info.ysize))

    def __del__(self):
        if getattr(self, "_ptr", None):
            libjxl_threads().JxlResizableParallelRunnerDestroy(self._ptr)
            self._ptr = None


# ---- decoder (jpegxl-rs/src/decode.rs) ---------------------------------------------------------------------------------
class JxlDecoder:
    """Mirror of jpegxl_rs::decode::JxlDecoder.  All option fields are public and mutable after build (decode.rs:85-154)."""

    def __init__(self, pixel_format: Optional[PixelFormat] = None, skip_reorientation=None, unpremul_alpha=None,
                 render_spotcolors=None, coalescing=None, desired_intensity_target=None, decompress=None, progressive_detail=None,
                 icc_profile: bool = False, init_jpeg_buffer: int = 512 * 1024, parallel_runner=None, memory_manager=None):
        self.pixel_format = pixel_format
        self.skip_reorientation = skip_reorientation
        self.unpremul_alpha = unpremul_alpha
        self.render_spotcolors = render_spotcolors
        self.coalescing = coalescing
        self.desired_intensity_target = desired_intensity_target
        self.decompress = decompress                      # stored, never forwarded (decode.rs:129 vs 327-366)
        self.progressive_detail = progressive_detail      # ditto (decode.rs:135)
        self.icc_profile = icc_profile
        self.init_jpeg_buffer = init_jpeg_buffer
        self.parallel_runner = parallel_runner
        self.memory_manager = memory_manager
        L = libjxl()
        self._dec = L.JxlDecoderCreate(C.byref(memory_manager) if memory_manager is not None else None)  # decode.rs:177-182
        if not self._dec:
            raise CannotCreateDecoder()

    def __del__(self):
        if getattr(self, "_dec", None):
            libjxl().JxlDecoderDestroy(self._dec)  # decode.rs:519
            self._dec = None

    # decode.rs:327-366
    def _setup_decoder(self, icc: bool, reconstruct_jpeg: bool):
        L = libjxl()
        if self.parallel_runner is not None:
            check_dec_status(L.JxlDecoderSetParallelRunner(self._dec, self.parallel_runner.runner(), self.parallel_runner.as_opaque_ptr()))
        events = JXL_DEC_BASIC_INFO | JXL_DEC_FULL_IMAGE
        if icc:
            events |= JXL_DEC_COLOR_ENCODING
        if reconstruct_jpeg:
            events |= JXL_DEC_JPEG_RECONSTRUCTION
        check_dec_status(L.JxlDecoderSubscribeEvents(self._dec, events))
        if self.skip_reorientation is not None:
            check_dec_status(L.JxlDecoderSetKeepOrientation(self._dec, int(self.skip_reorientation)))
        if self.unpremul_alpha is not None:
            check_dec_status(L.JxlDecoderSetUnpremultiplyAlpha(self._dec, int(self.unpremul_alpha)))
        if self.render_spotcolors is not None:
            check_dec_status(L.JxlDecoderSetRenderSpotcolors(self._dec, int(self.render_spotcolors)))
        if self.coalescing is not None:
            check_dec_status(L.JxlDecoderSetCoalescing(self._dec, int(self.coalescing)))
        if self.desired_intensity_target is not None:
            check_dec_status(L.JxlDecoderSetDesiredIntensityTarget(self._dec, float(self.desired_intensity_target)))

    # decode.rs:368-385
    def _get_icc_profile(self) -> bytes:
        L = libjxl()
        size = C.c_size_t()
        check_dec_status(L.JxlDecoderGetICCProfileSize(self._dec, 1, C.byref(size)))
        buf = (C.c_uint8 * size.value)()
        check_dec_status(L.JxlDecoderGetColorAsICCProfile(self._dec, 1, buf, size.value))
        return bytes(buf)

    # decode.rs:387-434
    def _output(self, info: JxlBasicInfo, data_type: Optional[int], fmt: JxlPixelFormat):
        L = libjxl()
        if data_type is None:
            bits, exp = info.bits_per_sample, info.exponent_bits_per_sample
            if exp > 0:
                if bits == 16:
                    data_type = JXL_TYPE_FLOAT16
                elif bits == 32:
                    data_type = JXL_TYPE_FLOAT
                else:
                    raise UnsupportedBitWidth(bits)
            elif bits <= 8:
                data_type = JXL_TYPE_UINT8
            elif bits <= 16:
                data_type = JXL_TYPE_UINT16
            else:
                raise UnsupportedBitWidth(bits)
        f = self.pixel_format or PixelFormat()
        nc = f.num_channels if f.num_channels else info.num_color_channels + (1 if info.alpha_bits > 0 else 0)
        fmt.num_channels, fmt.data_type, fmt.endianness, fmt.align = nc, data_type, f.endianness, f.align
        size = C.c_size_t()
        check_dec_status(L.JxlDecoderImageOutBufferSize(self._dec, C.byref(fmt), C.byref(size)))
        pixels = np.zeros(size.value, dtype=np.uint8)  # Vec::resize(size, 0)
        check_dec_status(L.JxlDecoderSetImageOutBuffer(self._dec, C.byref(fmt), pixels.ctypes.data, size.value))
        return pixels

    # decode.rs:207-325
    def _decode_internal(self, data: bytes, data_type: Optional[int], with_icc: bool, reconstruct: bool):
        L = libjxl()
        sig = check_valid_signature(data)
        if sig is None or not sig:
            raise InvalidInput()
        self._setup_decoder(with_icc, reconstruct)
        inbuf = np.frombuffer(data, dtype=np.uint8)
        check_dec_status(L.JxlDecoderSetInput(self._dec, inbuf.ctypes.data, len(data)))
        L.JxlDecoderCloseInput(self._dec)
        info = JxlBasicInfo()
        fmt = JxlPixelFormat()
        pixels = np.zeros(0, dtype=np.uint8)
        icc = None
        jpeg = None
        while True:
            status = L.JxlDecoderProcessInput(self._dec)
            if status in (JXL_DEC_NEED_MORE_INPUT, JXL_DEC_ERROR):
                raise GenericError(last_error())          # NB: no Reset on error paths (decode.rs:241)
            elif status == JXL_DEC_BASIC_INFO:
                check_dec_status(L.JxlDecoderGetBasicInfo(self._dec, C.byref(info)))
                if self.parallel_runner is not None:
                    self.parallel_runner.callback_basic_info(info)
            elif status == JXL_DEC_COLOR_ENCODING:
                icc = self._get_icc_profile()
            elif status == JXL_DEC_JPEG_RECONSTRUCTION:
                jpeg = np.zeros(self.init_jpeg_buffer, dtype=np.uint8)
                check_dec_status(L.JxlDecoderSetJPEGBuffer(self._dec, jpeg.ctypes.data, len(jpeg)))
            elif status == JXL_DEC_JPEG_NEED_MORE_OUTPUT:
                need = L.JxlDecoderReleaseJPEGBuffer(self._dec)
                jpeg = np.concatenate([jpeg, np.zeros(need, dtype=np.uint8)])
                check_dec_status(L.JxlDecoderSetJPEGBuffer(self._dec, jpeg.ctypes.data, len(jpeg)))
            elif status == JXL_DEC_NEED_IMAGE_OUT_BUFFER:
                pixels = self._output(info, data_type, fmt)
            elif status in (JXL_DEC_FULL_IMAGE, JXL_DEC_FRAME, JXL_DEC_FRAME_PROGRESSION):
                continue
            elif status == JXL_DEC_SUCCESS:
                if jpeg is not None:
                    remaining = L.JxlDecoderReleaseJPEGBuffer(self._dec)
                    jpeg = jpeg[: len(jpeg) - remaining]
                L.JxlDecoderReset(self._dec)
                meta = Metadata(info.xsize, info.ysize, info.intensity_target, info.min_nits, info.orientation, info.num_color_channels,
                                info.alpha_bits > 0, info.intrinsic_xsize, info.intrinsic_ysize, icc)
                return meta, fmt, pixels, jpeg
            elif status == JXL_DEC_NEED_PREVIEW_OUT_BUFFER:
                raise NotImplementedFeature("preview image output")
            elif status == JXL_DEC_BOX_NEED_MORE_OUTPUT:
                raise NotImplementedFeature("box output")
            elif status == JXL_DEC_PREVIEW_IMAGE:
                raise NotImplementedFeature("preview image")
            elif status == JXL_DEC_BOX:
                raise NotImplementedFeature("box handling")
            elif status == JXL_DEC_BOX_COMPLETE:
                raise NotImplementedFeature("box complete")
            else:
                raise UnknownStatus(status)

    @staticmethod
    def _convert(raw: np.ndarray, fmt: JxlPixelFormat) -> np.ndarray:
        """PixelType::convert (common.rs:59-124): endian-aware reinterpretation of the byte buffer."""
        dt = {JXL_TYPE_UINT8: "u1", JXL_TYPE_UINT16: "u2", JXL_TYPE_FLOAT: "f4", JXL_TYPE_FLOAT16: "f2"}[fmt.data_type]
        order = ">" if fmt.endianness == JXL_BIG_ENDIAN else "<"
        n = len(raw) // np.dtype(dt).itemsize
        return raw[: n * np.dtype(dt).itemsize].view(np.dtype(order + dt)).astype(np.dtype(dt))

    def decode(self, data: bytes):
        """decode.rs:440-455 — returns (Metadata, pixels) with the sample type inferred from the header."""
        meta, fmt, pixels, _ = self._decode_internal(data, None, self.icc_profile, False)
        return meta, self._convert(pixels, fmt)

    def decode_with(self, data: bytes, dtype):
        """decode.rs:461-484 — decode_with::<T>; dtype in {uint8, uint16, float32, float16}."""
        name = np.dtype(dtype).name
        if name not in _PIXEL_TYPES:
            raise UnsupportedBitWidth(name)
        meta, fmt, pixels, _ = self._decode_internal(data, _PIXEL_TYPES[name][0], self.icc_profile, False)
        return meta, self._convert(pixels, fmt)

    # ---- image.rs:32-132, the `image` crate integration (trait ToDynamic): the decoded buffer as an image object, None when the combination
    # of sample type and channel count has no DynamicImage variant.  The stand-in for DynamicImage here is a (height, width, channels) numpy
    # array tagged with the variant's name.
    _DYNAMIC = {("float32", 3): "ImageRgb32F", ("float32", 4): "ImageRgba32F", ("uint8", 1): "ImageLuma8", ("uint8", 2): "ImageLumaA8",
                ("uint8", 3): "ImageRgb8", ("uint8", 4): "ImageRgba8", ("uint16", 1): "ImageLuma16", ("uint16", 2): "ImageLumaA16",
                ("uint16", 3): "ImageRgb16", ("uint16", 4): "ImageRgba16"}

    def _to_image(self, meta, fmt, pixels):
        arr = self._convert(pixels, fmt)
        variant = self._DYNAMIC.get((arr.dtype.name, fmt.num_channels))
        if variant is None or arr.size != meta.width * meta.height * fmt.num_channels:     # (ImageBuffer::from_raw: the buffer must hold the image exactly)
            return None
        return DynamicImage(variant, arr.reshape(meta.height, meta.width, fmt.num_channels))

    def decode_to_image(self, data: bytes):
        """image.rs:53-66 — decode with the sample type the header asks for; Optional[DynamicImage]."""
        meta, fmt, pixels, _ = self._decode_internal(data, None, False, False)
        return self._to_image(meta, fmt, pixels)

    def decode_to_image_with(self, data: bytes, dtype):
        """image.rs:68-86 — decode_to_image_with::<T>."""
        name = np.dtype(dtype).name
        if name not in _PIXEL_TYPES:
            raise UnsupportedBitWidth(name)
        meta, fmt, pixels, _ = self._decode_internal(data, _PIXEL_TYPES[name][0], False, False)
        return self._to_image(meta, fmt, pixels)

    def reconstruct(self, data: bytes):
        """decode.rs:493-514 — returns (Metadata, ('jpeg', bytes) | ('pixels', ndarray))."""
        meta, fmt, pixels, jpeg = self._decode_internal(data, None, self.icc_profile, True)
        if jpeg is not None and len(jpeg):
            return meta, ("jpeg", jpeg.tobytes())
        return meta, ("pixels", self._convert(pixels, fmt))


class DynamicImage:
    """Stand-in for image::DynamicImage (image.rs:88-132): `variant` names the enum variant, `pixels` is (height, width, channels)."""

    def __init__(self, variant: str, pixels: np.ndarray):
        self.variant, self.pixels = variant, pixels

    def to_rgba16(self) -> np.ndarray:
        """DynamicImage::to_rgba16 as the reference's test uses it (image.rs:169): grey is replicated, alpha defaults to opaque, 8-bit samples
        scale by 257, float samples by 65535 (clamped)."""
        p = self.pixels
        if p.dtype == np.uint8:
            p = p.astype(np.uint16) * 257
        elif p.dtype == np.float32:
            p = np.rint(np.clip(p, 0.0, 1.0) * 65535.0).astype(np.uint16)
        c = p.shape[2]
        rgb = np.repeat(p[:, :, :1], 3, axis=2) if c <= 2 else p[:, :, :3]
        alpha = p[:, :, c - 1:c] if c in (2, 4) else np.full(p.shape[:2] + (1,), 65535, np.uint16)
        return np.concatenate([rgb, alpha], axis=2).astype(np.uint16)


def decoder_builder(**options) -> JxlDecoder:
    """jpegxl-rs/src/decode.rs:535 — `decoder_builder().pixel_format(..).build()` becomes keyword arguments."""
    return JxlDecoder(**options)


def _layout(planar, plane_stride, scale, bias):
    """-> JxlHipOutputLayout, or None for interleaved samples without scale / bias (the calls without a layout).  scale / bias: up to four values, one per channel
    slot (missing ones 1 / 0); giving either asks for affine output."""
    if not planar and scale is None and bias is None:
        if plane_stride:
            raise ValueError("plane_stride needs planar=True")
        return None
    lay = JxlHipOutputLayout(1 if planar else 0, int(plane_stride), 0 if scale is None and bias is None else 1)
    for dst, src, default in ((lay.scale, scale, 1.0), (lay.bias, bias, 0.0)):
        vals = [] if src is None else [float(v) for v in np.atleast_1d(src)]
        if len(vals) > 4:
            raise ValueError("scale / bias take at most four values, one per channel slot")
        for c in range(4):
            dst[c] = vals[c] if c < len(vals) else default
    return lay


def _resize(resize, crop):
    """-> JxlHipOutputResize, or None for an output of the image's own size.  resize: (width, height) of the output; crop: (x0, y0, width, height) of the decoded picture
    that is resampled into it (needs resize)."""
    if resize is None:
        if crop is not None:
            raise ValueError("crop needs resize=(width, height)")
        return None
    w, h = (int(v) for v in resize)
    x0, y0, cw, ch = (0, 0, 0, 0) if crop is None else (int(v) for v in crop)
    if min(w, h, x0, y0, cw, ch) < 0 or max(w, h, x0, y0, cw, ch) >= 1 << 32:
        raise ValueError("resize / crop values must fit 32 unsigned bits")
    return JxlHipOutputResize(w, h, x0, y0, cw, ch)


_FILTERS = {"bilinear": 0, "bicubic": 1}


def _filter_id(filter):
    """"bilinear" (the antialiased triangle filter) / "bicubic" (antialiased cubic convolution, a = -0.5), or the number include/jxl_hip.h gives them"""
    if filter is None:
        return 0
    if isinstance(filter, str):
        if filter not in _FILTERS:
            raise ValueError(f"filter must be one of {sorted(_FILTERS)}, not {filter!r}")
        return _FILTERS[filter]
    return int(filter)


def _resample(resize, crop, filter, mirror):
    """-> JxlHipOutputResample: _resize() with the filter and the mirror (both need resize)"""
    if resize is None:
        raise ValueError("crop, filter and mirror need resize=(width, height)")
    rs = _resize(resize, crop)
    f = _filter_id(filter)
    if not 0 <= f < 1 << 32:
        raise ValueError("filter must fit 32 unsigned bits")
    return JxlHipOutputResample(rs.xsize, rs.ysize, rs.crop_x0, rs.crop_y0, rs.crop_xsize, rs.crop_ysize, f, 1 if mirror else 0)


def _jpeg_scaled(jpeg_scale, downscale, rs):
    """libjpeg's scaled decodes (include/jxl_hip.h JxlHipBatchSetOutputJpegScaled): refuses the combination with downscale; the resize of such an output always travels
    as a JxlHipOutputResample (filter 0, no mirror: the ...Resized call, byte for byte)"""
    if int(downscale) != 1:
        raise GenericError("unsupported: jpeg_scale %d together with downscale %d (one of the two scaled decodes)" % (int(jpeg_scale), int(downscale)))
    if isinstance(rs, JxlHipOutputResize):
        rs = JxlHipOutputResample(rs.xsize, rs.ysize, rs.crop_x0, rs.crop_y0, rs.crop_xsize, rs.crop_ysize, 0, 0)
    return rs


JXL_HIP_RESAMPLE_U8 = 1


def _resize_u8(downscale, rs):
    """the integer resample (include/jxl_hip.h JxlHipBatchSetOutputJpegResampled): refuses what the C calls have no argument for, a downscale and a missing target"""
    if int(downscale) != 1:
        raise GenericError("unsupported: integer resample together with downscale %d (the 1:8 decode is not a libjpeg-exact one)" % int(downscale))
    if rs is None:
        raise GenericError("unsupported: integer resample without a target size (resize_u8 needs resize=(width, height))")


def _planes(extra_planes, plane_scale, plane_bias, planes_offset, planes_stride=0):
    """-> JxlHipOutputPlanes (which keeps its arrays referenced), or None without extra_planes.  extra_planes: extra-channel indices, one plane each (they may repeat);
    plane_scale / plane_bias: one value per plane (float16 / float32 output); planes_offset / planes_stride: where the first plane starts in the destination and the
    bytes from one plane to the next, 0 = the defaults (include/jxl_hip.h JxlHipOutputPlanes)."""
    if extra_planes is None:
        if plane_scale is not None or plane_bias is not None or planes_offset or planes_stride:
            raise ValueError("plane_scale, plane_bias, planes_offset and planes_stride need extra_planes=[...]")
        return None
    idx = [int(k) for k in extra_planes]
    if any(k < 0 or k >= 1 << 32 for k in idx):
        raise ValueError("extra_planes holds extra-channel indices (unsigned 32-bit)")
    m = len(idx)
    p = JxlHipOutputPlanes()
    p.num_planes = m
    p._idx = (C.c_uint32 * max(1, m))(*idx)
    p.extra_index = C.cast(p._idx, C.POINTER(C.c_uint32))
    p.offset, p.plane_stride = int(planes_offset), int(planes_stride)
    for name, src in (("scale", plane_scale), ("bias", plane_bias)):
        if src is None:
            continue
        vals = [float(v) for v in np.atleast_1d(src)]
        if len(vals) != m:
            raise ValueError(f"plane_{name} needs one value per requested plane ({m}), not {len(vals)}")
        arr = (C.c_float * max(1, m))(*vals)
        setattr(p, "_" + name, arr)
        setattr(p, name, C.cast(arr, C.POINTER(C.c_float)))
    return p


# output_color= by name: white point, primaries, transfer function (JxlColorEncoding's enums)
_NAMED_COLORS = {"srgb": (1, 1, 13), "linear_srgb": (1, 1, 8), "display_p3": (1, 11, 13), "rec2020_pq": (1, 9, 16), "rec2020_hlg": (1, 9, 18)}


def color_encoding(color) -> JxlColorEncoding:
    """-> JxlColorEncoding of `color`: one of "srgb", "linear_srgb", "display_p3", "rec2020_pq", "rec2020_hlg", a JxlColorEncoding, or a dict with the enums
    white_point (1 D65 / 2 custom / 10 E / 11 DCI), primaries (1 sRGB / 2 custom / 9 BT.2100 / 11 P3), tf (1 Rec.709 / 8 linear / 13 sRGB / 16 PQ / 17 DCI / 18 HLG),
    gamma (!= 0 replaces tf), color_space (0 RGB, 1 grey), rendering_intent, and for the custom enums white_xy / red_xy / green_xy / blue_xy.  white_xy or the three
    primaries given without their enum select the custom one."""
    if isinstance(color, JxlColorEncoding):
        return color
    if isinstance(color, str):
        if color not in _NAMED_COLORS:
            raise ValueError("output_color: %r is none of %s" % (color, ", ".join(sorted(_NAMED_COLORS))))
        color = dict(zip(("white_point", "primaries", "tf"), _NAMED_COLORS[color]))
    d = dict(color)
    e = JxlColorEncoding()
    e.color_space = int(d.pop("color_space", 0))
    white_xy, prim = d.pop("white_xy", None), [d.pop(k, None) for k in ("red_xy", "green_xy", "blue_xy")]
    if any(v is not None for v in prim) and not all(v is not None for v in prim):
        raise ValueError("output_color: red_xy, green_xy and blue_xy come together")
    e.white_point = int(d.pop("white_point", 2 if white_xy is not None else 1))
    e.primaries = int(d.pop("primaries", 2 if prim[0] is not None else 1))
    if white_xy is not None:
        e.white_point_xy[0], e.white_point_xy[1] = float(white_xy[0]), float(white_xy[1])
    for name, v in zip(("primaries_red_xy", "primaries_green_xy", "primaries_blue_xy"), prim):
        if v is not None:
            getattr(e, name)[0], getattr(e, name)[1] = float(v[0]), float(v[1])
    gamma = float(d.pop("gamma", 0.0))
    e.transfer_function, e.gamma = (65535, gamma) if gamma != 0.0 else (int(d.pop("tf", 13)), 0.0)
    d.pop("tf", None)
    e.rendering_intent = int(d.pop("rendering_intent", 1))
    if d:
        raise ValueError("output_color: unknown keys %s" % sorted(d))
    return e


def _color(output_color, convert_non_xyb):
    """-> JxlHipOutputColor, or None without output_color"""
    if output_color is None:
        if convert_non_xyb:
            raise ValueError("convert_non_xyb needs output_color=")
        return None
    return JxlHipOutputColor(color_encoding(output_color), 1 if convert_non_xyb else 0)


def color_conversion_matrix(from_color, to_color) -> np.ndarray:
    """The 3x3 float64 matrix that takes linear light of `from_color` to linear light of `to_color` (each as for color_encoding): through XYZ D50 with linear Bradford
    adaptation, the rule of output_color= (include/jxl_hip.h JxlHipColorConversionMatrix).  Host only."""
    a, b = color_encoding(from_color), color_encoding(to_color)
    m = (C.c_double * 9)()
    if libjxl().JxlHipColorConversionMatrix(C.byref(a), C.byref(b), C.byref(m)) != 0:
        raise GenericError(last_error())
    return np.array(list(m), dtype=np.float64).reshape(3, 3)


def _per_image(value, n, is_one):
    """one value for the job, or a sequence of n per-image values -> (list of n, whether it was a sequence)"""
    if value is None or isinstance(value, (str, bytes)) or not hasattr(value, "__iter__"):
        return [value] * n, False
    vals = list(value)                      # (any iterable, a generator included)
    if is_one(vals):
        return [tuple(vals)] * n, False
    if len(vals) != n:
        raise ValueError(f"a per-image sequence needs {n} entries, not {len(vals)}")
    return vals, True


def _byref(s):
    return None if s is None else C.byref(s)


# ---- batch extension (include/jxl_hip.h, JxlHipBatch*) -------------------------------------------------------------------
class BatchDecoder:
    """Device-resident decode of a batch of independent images: inputs and outputs stay in HBM."""

    def __init__(self, device: int = 0):
        L = libjxl()
        self._h = L.JxlHipBatchCreate(device)
        if not self._h:
            raise CannotCreateDecoder(last_error())
        self._n = 0
        self._fmt = []
        self._scale = []
        self._jpeg_scale = []
        self._layouts = []
        self._resizes = []
        self._planes = []

    def __del__(self):
        if getattr(self, "_h", None):
            libjxl().JxlHipBatchDestroy(self._h)
            self._h = None

    def _chk(self, status):
        if status != JXL_DEC_SUCCESS:
            raise GenericError(last_error())

    def _set_output(self, i, fmt, device_ptr, downscale, layout=None, resize=None, jpeg_scale=1, resize_u8=False, planes=None, color=None):
        L = libjxl()
        if resize_u8:
            _resize_u8(downscale, resize)
            resize = _jpeg_scaled(jpeg_scale, downscale, resize)
            self._chk(L.JxlHipBatchSetOutputJpegResampled(self._h, i, C.byref(fmt), device_ptr, int(jpeg_scale), _byref(layout), _byref(resize), JXL_HIP_RESAMPLE_U8))
        elif jpeg_scale != 1:
            resize = _jpeg_scaled(jpeg_scale, downscale, resize)
            self._chk(L.JxlHipBatchSetOutputJpegScaled(self._h, i, C.byref(fmt), device_ptr, int(jpeg_scale), _byref(layout), _byref(resize)))
        elif isinstance(resize, JxlHipOutputResample):
            self._chk(L.JxlHipBatchSetOutputResampled(self._h, i, C.byref(fmt), device_ptr, int(downscale), _byref(layout), C.byref(resize)))
        elif resize is not None:
            self._chk(L.JxlHipBatchSetOutputResized(self._h, i, C.byref(fmt), device_ptr, int(downscale), _byref(layout), C.byref(resize)))
        elif layout is not None:
            self._chk(L.JxlHipBatchSetOutputLayout(self._h, i, C.byref(fmt), device_ptr, int(downscale), C.byref(layout)))
        elif downscale == 1:
            self._chk(L.JxlHipBatchSetOutput(self._h, i, C.byref(fmt), device_ptr))
        else:
            self._chk(L.JxlHipBatchSetOutputScaled(self._h, i, C.byref(fmt), device_ptr, int(downscale)))
        if planes is not None:
            self._chk(L.JxlHipBatchSetOutputPlanes(self._h, i, C.byref(planes)))
        if color is not None:
            self._chk(L.JxlHipBatchSetOutputColor(self._h, i, C.byref(color)))
        self._planes.append(planes)
        self._fmt.append(fmt)
        self._scale.append(int(downscale))
        self._jpeg_scale.append(int(jpeg_scale))
        self._layouts.append(layout)
        self._resizes.append(resize)

    def add(self, data: bytes, dtype="uint8", num_channels=0, endianness=Endianness.Native, align=0, device_ptr=None, downscale=1,
            planar=False, plane_stride=0, scale=None, bias=None, resize=None, crop=None, filter=None, mirror=False, jpeg_scale=1, resize_u8=False,
            extra_planes=None, plane_scale=None, plane_bias=None, planes_offset=0, planes_stride=0, output_color=None, convert_non_xyb=False) -> int:
        """downscale=8: the 1:8 decode (include/jxl_hip.h JxlHipBatchSetOutputScaled) — output(i) is the ceil(w / 8) x ceil(h / 8) picture; `data` may end behind
        the LF part of its frame.
        planar=True: one plane per channel, [C, H, W] with rows `align`ed and planes plane_stride bytes apart (0 = tight); scale / bias (up to four values, one per
        channel slot, float16 / float32 output): samples are stored as v * scale[c] + bias[c] (include/jxl_hip.h JxlHipOutputLayout).
        resize=(w, h): the output is w x h pixels, the decoded picture — oriented, at `downscale` — resampled with the antialiased triangle filter (torch's
        interpolate(mode="bilinear", antialias=True)); crop=(x0, y0, w, h): only that rectangle of the picture, as if cropped first (include/jxl_hip.h JxlHipOutputResize).
        filter="bilinear" (that triangle filter) | "bicubic" (antialiased cubic convolution, a = -0.5: torch's mode="bicubic", antialias=True); mirror=True: the resampled
        picture is stored with its columns reversed (include/jxl_hip.h JxlHipOutputResample).  Both need resize; a call without them is the ...Resized call as before.
        jpeg_scale=2 | 4 | 8: libjpeg's scaled decode of a JPEG transcode (include/jxl_hip.h JxlHipBatchSetOutputJpegScaled) — the ceil(w / s) x ceil(h / s) picture
        PIL's draft() gives for the original file, sample for sample, as the source of everything above (a crop is in the scaled picture).  Only decode_jpeg_pixels()
        writes such an output (decode() + finish() fail the image); not together with downscale.  jpeg_scale=8 of a grey, 4:4:4 or 4:2:2 image is decoded from
        the DC terms alone (jpeg_dc_only(i)): `data` may then end anywhere behind the LF part of its frame (lf_part_size(data)); a prefix of any other image
        fails the next prepare() with "truncated".
        resize_u8=True (needs resize, and an image decode_jpeg_pixels() takes): the resample runs in Pillow's 8-bit arithmetic over the u8 picture libjpeg gives
        (include/jxl_hip.h JxlHipBatchSetOutputJpegResampled) — the u8 output is np.asarray(Image.open(file).crop(box).resize(size, BILINEAR | BICUBIC)) byte for
        byte, every other type and layout follows from it, and the intermediates are u8.  Only decode_jpeg_pixels() writes such an output; not together with downscale.
        extra_planes=[k, ...]: extra channel k of the image — as it is: depth, masks, spectral bands — as a plane of one sample per pixel behind the colour output of the
        same destination, all planes from the one decode (include/jxl_hip.h JxlHipOutputPlanes).  The planes take dtype, endianness and align of the colour output and
        follow its geometry (orientation, resize, crop, filter, mirror); with planar=True colour and planes form one [C + m, H, W] block.  plane_scale / plane_bias: one
        value per plane (float output); planes_offset / planes_stride: where the first plane starts and the bytes from plane to plane, 0 = the defaults —
        planes_layout(i) tells, and out_size(i) / output(i) cover the whole destination.  An index the image does not have, downscale=8 and libjpeg-exact outputs
        are refused: "unsupported: extra planes ...".
        output_color="srgb" | "linear_srgb" | "display_p3" | "rec2020_pq" | "rec2020_hlg" | a dict (color_encoding()): the colour encoding the pixels come out in, whatever
        the image's header names (include/jxl_hip.h JxlHipOutputColor) — an XYB image exactly as if its header named that encoding, at its own intensity target; an image
        that is not XYB keeps its samples unless convert_non_xyb=True, which converts it (transfer function, primaries, transfer function) in the frame tail.  Composes with
        downscale=8, layouts, resize and extra_planes; libjpeg-exact outputs refuse it: "unsupported: output colour ..."."""
        layout = _layout(planar, plane_stride, scale, bias)
        rs = _resize(resize, crop) if filter is None and not mirror else _resample(resize, crop, filter, mirror)
        L = libjxl()
        buf = np.frombuffer(data, dtype=np.uint8)
        prefix_ok = downscale != 1 or int(jpeg_scale) == 8                  # decodes that may end behind the LF stage
        if prefix_ok:
            L.JxlHipBatchSetOption(self._h, b"allow_partial", 1)
        try:
            i = L.JxlHipBatchAddImage(self._h, buf.ctypes.data, len(data))
        finally:
            if prefix_ok:
                L.JxlHipBatchSetOption(self._h, b"allow_partial", 0)
        if i < 0:
            raise GenericError(last_error())
        fmt = JxlPixelFormat(num_channels, _PIXEL_TYPES[np.dtype(dtype).name][0], endianness, align)
        self._set_output(i, fmt, device_ptr, downscale, layout, rs, jpeg_scale, resize_u8, _planes(extra_planes, plane_scale, plane_bias, planes_offset, planes_stride),
                         _color(output_color, convert_non_xyb))
        self._n += 1
        return i

    def add_many(self, datas, dtype="uint8", num_channels=0, device_ptrs=None, threads=4, endianness=Endianness.Native, align=0, downscale=1,
                 planar=False, plane_stride=0, scale=None, bias=None, resize=None, crop=None, filter=None, mirror=False, jpeg_scale=1, resize_u8=False,
                 extra_planes=None, plane_scale=None, plane_bias=None, planes_offset=0, planes_stride=0) -> int:
        """Parses the images of `datas` (bytes objects) on `threads` host threads and appends them in order (JxlHipBatchAddImages);
        device_ptrs: optional caller-owned device destination per image.  Returns the index of the first one.  downscale, planar, plane_stride, scale, bias, resize, crop, filter, mirror, jpeg_scale, resize_u8,
        extra_planes, plane_scale, plane_bias, planes_offset, planes_stride: as for add()."""
        L = libjxl()
        layout = _layout(planar, plane_stride, scale, bias)
        rs = _resize(resize, crop) if filter is None and not mirror else _resample(resize, crop, filter, mirror)
        planes = _planes(extra_planes, plane_scale, plane_bias, planes_offset, planes_stride)
        n = len(datas)
        ptrs = (C.c_char_p * n)(*datas)
        sizes = (C.c_size_t * n)(*[len(d) for d in datas])
        prefix_ok = downscale != 1 or int(jpeg_scale) == 8
        if prefix_ok:
            L.JxlHipBatchSetOption(self._h, b"allow_partial", 1)
        try:
            first = L.JxlHipBatchAddImages(self._h, ptrs, sizes, n, int(threads))
        finally:
            if prefix_ok:
                L.JxlHipBatchSetOption(self._h, b"allow_partial", 0)
        if first < 0:
            raise GenericError(last_error())
        fmt = JxlPixelFormat(num_channels, _PIXEL_TYPES[np.dtype(dtype).name][0], endianness, align)
        for k in range(n):
            self._set_output(first + k, fmt, device_ptrs[k] if device_ptrs is not None else None, downscale, layout, rs, jpeg_scale, resize_u8, planes)
        self._n += n
        return first

    def reset(self):
        """Forgets the images, keeps the device arenas and buffer sharing (JxlHipBatchReset): fill and prepare again."""
        libjxl().JxlHipBatchReset(self._h)
        self._n = 0
        self._fmt = []
        self._scale = []
        self._jpeg_scale = []
        self._layouts = []
        self._resizes = []
        self._planes = []

    def info(self, i) -> JxlBasicInfo:
        info = JxlBasicInfo()
        self._chk(libjxl().JxlHipBatchGetBasicInfo(self._h, i, C.byref(info)))
        return info

    def planes_layout(self, i):
        """(offset, plane_stride, total) of image i's destination, in bytes: where the first extra plane starts, the bytes from one plane to the next, the size of the
        whole destination — colour output and planes (include/jxl_hip.h JxlHipBatchOutputPlanesLayout).  Without extra_planes: (total, 0, total).  Host only."""
        off, pitch, total = C.c_size_t(), C.c_size_t(), C.c_size_t()
        self._chk(libjxl().JxlHipBatchOutputPlanesLayout(self._h, int(i), C.byref(off), C.byref(pitch), C.byref(total)))
        return int(off.value), int(pitch.value), int(total.value)

    def out_size(self, i) -> int:
        if self._planes[i] is not None:
            return self.planes_layout(i)[2]
        s = C.c_size_t()
        if self._jpeg_scale[i] != 1:
            rs = _jpeg_scaled(self._jpeg_scale[i], self._scale[i], self._resizes[i])
            self._chk(libjxl().JxlHipBatchOutBufferSizeJpegScaled(self._h, i, C.byref(self._fmt[i]), self._jpeg_scale[i], _byref(self._layouts[i]), _byref(rs), C.byref(s)))
        elif isinstance(self._resizes[i], JxlHipOutputResample):
            self._chk(libjxl().JxlHipBatchOutBufferSizeResampled(self._h, i, C.byref(self._fmt[i]), self._scale[i], _byref(self._layouts[i]), C.byref(self._resizes[i]), C.byref(s)))
        elif self._resizes[i] is not None:
            self._chk(libjxl().JxlHipBatchOutBufferSizeResized(self._h, i, C.byref(self._fmt[i]), self._scale[i], _byref(self._layouts[i]), C.byref(self._resizes[i]), C.byref(s)))
        elif self._layouts[i] is not None:
            self._chk(libjxl().JxlHipBatchOutBufferSizeLayout(self._h, i, C.byref(self._fmt[i]), self._scale[i], C.byref(self._layouts[i]), C.byref(s)))
        elif self._scale[i] == 1:
            self._chk(libjxl().JxlHipBatchOutBufferSize(self._h, i, C.byref(self._fmt[i]), C.byref(s)))
        else:
            self._chk(libjxl().JxlHipBatchOutBufferSizeScaled(self._h, i, C.byref(self._fmt[i]), self._scale[i], C.byref(s)))
        return s.value

    def set_lane_stride(self, lf=64, hf=64):
        libjxl().JxlHipBatchSetLaneStride(self._h, lf, hf)

    def set_option(self, name: str, value: int):
        libjxl().JxlHipBatchSetOption(self._h, name.encode(), int(value))

    def share_buffers(self, owner: "BatchDecoder"):
        """Use `owner`'s coefficient / pixel planes (call before prepare; see include/jxl_hip.h JxlHipBatchShareBuffers)."""
        self._chk(libjxl().JxlHipBatchShareBuffers(self._h, owner._h if owner is not None else None))   # (None: planes of its own again)
        self._owner = owner   # keep it alive

    def share_coefficients(self, owner: "BatchDecoder"):
        """Use `owner`'s quantised-coefficient planes (call before prepare; include/jxl_hip.h JxlHipBatchShareCoefficients)."""
        self._chk(libjxl().JxlHipBatchShareCoefficients(self._h, owner._h if owner is not None else None))
        self._coef_owner = owner

    def prepare(self, stream=None):
        self._chk(libjxl().JxlHipBatchPrepare(self._h, stream))

    def decode(self, stream=None):
        self._chk(libjxl().JxlHipBatchDecode(self._h, stream))

    def decode_timed(self, stream=None):
        self._chk(libjxl().JxlHipBatchDecodeTimed(self._h, stream))

    def decode_part(self, part: int, stream=None, timed=False):
        """part 1 = front (LF stage), 2 = rest (HF, IDCT, filters, output) — or 3 = HF only, 4 = IDCT, filters, output; see include/jxl_hip.h."""
        self._chk(libjxl().JxlHipBatchDecodePart(self._h, stream, part, 1 if timed else 0))

    def collect_times(self):
        """-> (dict stage -> summed ms, number of timed decodes)"""
        t = JxlHipStageTimes(); runs = C.c_int()
        self._chk(libjxl().JxlHipBatchCollectTimes(self._h, C.byref(t), C.byref(runs)))
        return {n: getattr(t, n) for n, _ in JxlHipStageTimes._fields_}, runs.value

    def finish(self, stream=None):
        self._chk(libjxl().JxlHipBatchFinish(self._h, stream))

    # ---- JPEG reconstruction of the batch (include/jxl_hip.h JxlHipBatchReconstructJpegs; decode.rs:493 `reconstruct` for many files at once)
    def can_reconstruct_jpeg(self, i) -> bool:
        """True if image i is a lossless JPEG transcode whose file can be given back; otherwise last_error() says why not."""
        return bool(libjxl().JxlHipBatchCanReconstructJpeg(self._h, i))

    def reconstruct_jpegs(self, stream=None, progressive_on_device=False):
        """One run of the entropy stages for the whole batch, then the JPEG files (sequential scans are entropy-coded on the GPU; with progressive_on_device
        the scans of progressive files as well, otherwise those files are coded on the host).  An image that fails does so alone: jpeg(i) raises for it."""
        self.set_option("jpeg_device_progressive", 1 if progressive_on_device else 0)
        self._chk(libjxl().JxlHipBatchReconstructJpegs(self._h, stream))

    def jpeg(self, i) -> bytes:
        """The reconstructed file of image i; DecodeError with the image's reason if it has none."""
        L = libjxl()
        if L.JxlHipBatchJpegStatus(self._h, i) != JXL_DEC_SUCCESS:
            raise GenericError(last_error())
        n = L.JxlHipBatchJpegSize(self._h, i)
        out = np.empty(max(n, 1), dtype=np.uint8)
        self._chk(L.JxlHipBatchCopyJpeg(self._h, i, out.ctypes.data, n))
        return out[:n].tobytes()

    # ---- libjpeg-exact pixels of JPEG transcodes (include/jxl_hip.h JxlHipBatchDecodeJpegPixels)
    def can_decode_jpeg_pixels(self, i) -> bool:
        """True if decode_jpeg_pixels() takes image i (host only); otherwise last_error() says why not: "unsupported: libjpeg-exact decode of ..."."""
        return bool(libjxl().JxlHipBatchCanDecodeJpegPixels(self._h, i))

    def jpeg_dc_only(self, i) -> bool:
        """True if image i (output set: after add) will be decoded from its DC terms alone — jpeg_scale=8 of a grey, 4:4:4 or 4:2:2 transcode — i.e. if a prefix
        of lf_part_size() bytes was enough (include/jxl_hip.h JxlHipBatchJpegDcOnly); set_option("jpeg_dc_only", 0) turns the path off."""
        return bool(libjxl().JxlHipBatchJpegDcOnly(self._h, int(i)))

    def jpeg_region(self, i):
        """None, or (gx0, gy0, gx1, gy1): the rectangle of 256x256 groups — gx0 <= gx < gx1, gy0 <= gy < gy1 — that decode_jpeg_pixels() decodes of image i (output set:
        after add) under set_option("jpeg_region", 1): what the crop of its output needs (include/jxl_hip.h JxlHipBatchJpegRegion has the rule).  None: the image is
        decoded whole — no crop, DC-only, or not taken by the libjpeg-exact decode.  Host only."""
        g = (C.c_uint32 * 4)()
        return tuple(int(v) for v in g) if libjxl().JxlHipBatchJpegRegion(self._h, int(i), C.byref(g)) else None

    def decode_jpeg_pixels(self, stream=None) -> list:
        """The samples libjpeg gives for the original JPEG file of every transcode of the batch (integer IDCT, libjpeg's chroma upsampling and colour conversion), written
        like a decode(): output(i) / device_output(i) hand them out.  Returns, per image, None or the reason why that image has no pixels (it fails alone)."""
        L = libjxl()
        self._chk(L.JxlHipBatchDecodeJpegPixels(self._h, stream))
        return [None if L.JxlHipBatchJpegPixelsStatus(self._h, i) == JXL_DEC_SUCCESS else last_error() for i in range(self._n)]

    def device_output(self, i) -> int:
        return libjxl().JxlHipBatchDeviceOutput(self._h, i)

    def output(self, i, stream=None) -> np.ndarray:
        n = self.out_size(i)
        out = np.empty(n, dtype=np.uint8)
        self._chk(libjxl().JxlHipBatchCopyOutput(self._h, i, out.ctypes.data, n, stream))
        return JxlDecoder._convert(out, self._fmt[i])

    def debug_read(self, i: int, name: str, channel: int = 0, dtype=np.float32) -> np.ndarray:
        """Testing: a device buffer of image i's first frame after a decode (include/jxl_hip.h JxlHipBatchDebugRead), as a flat array."""
        L = libjxl()
        n = L.JxlHipBatchDebugRead(self._h, i, name.encode(), channel, None, 0, None)
        if n == 0:
            raise GenericError(last_error())
        out = np.empty(n // np.dtype(dtype).itemsize, dtype=dtype)
        L.JxlHipBatchDebugRead(self._h, i, name.encode(), channel, out.ctypes.data, n, None)
        return out

    def info_value(self, name: str) -> int:
        """Facts about the prepared batch by name (include/jxl_hip.h JxlHipBatchGetInfo), e.g. "lf_simt_frames"."""
        return int(libjxl().JxlHipBatchGetInfo(self._h, name.encode()))

    @property
    def total_pixels(self):
        return libjxl().JxlHipBatchTotalPixels(self._h)

    @property
    def compressed_bytes(self):
        return libjxl().JxlHipBatchCompressedBytes(self._h)

    @property
    def stage_bytes(self):
        """Algorithmic HBM bytes of one decode of the batch per stage (lf, lfpost, hf, idct, filters, out)."""
        a = (C.c_uint64 * 6)()
        libjxl().JxlHipBatchStageBytes(self._h, C.byref(a))
        return dict(zip(("lf", "lfpost", "hf", "idct", "filter", "out"), [int(v) for v in a]))

    @property
    def device_bytes(self):
        return libjxl().JxlHipBatchDeviceBytes(self._h)


def decode_lf_grouped(batches, stream=None, timed=False):
    """Piece 5 (LF decode) of several prepared BatchDecoders on one stream, as the pipeline enqueues it for jobs that are ready together: adjacent batches whose LF
    streams take the same SIMT kernel share one launch of it, every other batch gets the launches of decode_part(5) (include/jxl_hip.h JxlHipBatchDecodeLfGrouped).
    The other pieces of each batch follow through decode_part."""
    fn = libjxl().JxlHipBatchDecodeLfGrouped
    fn.restype, fn.argtypes = C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_int]
    hs = (C.c_void_p * len(batches))(*[b._h for b in batches])
    if fn(hs, len(batches), stream, 1 if timed else 0) != JXL_DEC_SUCCESS:
        raise GenericError(last_error())


def lf_part_size(data: bytes) -> int:
    """The number of leading bytes of the file that hold the LF part of its first frame: data[:n] is the shortest prefix the 1:8 decode (downscale=8) and a DC-only
    decode (jpeg_scale=8, BatchDecoder.jpeg_dc_only) accept.  From the headers and the TOC, so a prefix that holds those gives the same answer; DecodeError
    "truncated" before that.  0: the whole file is needed (one-group frames).  Host only (include/jxl_hip.h JxlHipLfPartSize)."""
    buf = np.frombuffer(data, dtype=np.uint8)
    n = C.c_size_t()
    if libjxl().JxlHipLfPartSize(buf.ctypes.data if len(data) else None, len(data), C.byref(n)) != JXL_DEC_SUCCESS:
        raise GenericError(last_error())
    return int(n.value)


def arena_pool_trim() -> int:
    """Hands every pooled device arena back to the HIP runtime (JxlHipArenaPoolTrim); returns the bytes released."""
    return int(libjxl().JxlHipArenaPoolTrim())


def image_out_size(data: bytes, dtype="uint8", num_channels=0, endianness=Endianness.Native, align=0, downscale=1, planar=False, plane_stride=0, scale=None, bias=None,
                   resize=None, crop=None, jpeg_scale=1, extra_planes=None, plane_scale=None, plane_bias=None, planes_offset=0, planes_stride=0):
    """(JxlBasicInfo, bytes of the decoded image in that format) from the headers alone — host-only (JxlHipImageOutSize).
    extra_planes, plane_scale, plane_bias, planes_offset, planes_stride: the size of the colour output with those extra-channel planes behind it, as for BatchDecoder.add
    (JxlHipImageOutSizePlanes); what the image does not take raises "unsupported: extra planes ...".
    jpeg_scale=2 | 4 | 8: the size of libjpeg's scaled decode, as for BatchDecoder.add (JxlHipImageOutSizeJpegScaled); not together with downscale.
    downscale=8: the size of the 1:8 decode (JxlHipImageOutSizeScaled); the info stays that of the full-size image.
    planar, plane_stride, scale, bias: the layout as for BatchDecoder.add (JxlHipImageOutSizeLayout); a layout the image or the sample type does not take raises.
    resize, crop: the size of the resized output, as for BatchDecoder.add (JxlHipImageOutSizeResized); a crop that leaves the image raises."""
    fmt = JxlPixelFormat(num_channels, _PIXEL_TYPES[np.dtype(dtype).name][0], endianness, align)
    info, size = JxlBasicInfo(), C.c_size_t()
    buf = np.frombuffer(data, dtype=np.uint8)
    layout = _layout(planar, plane_stride, scale, bias)
    rs = _resize(resize, crop)
    planes = _planes(extra_planes, plane_scale, plane_bias, planes_offset, planes_stride)
    if planes is not None:
        if jpeg_scale != 1:
            raise GenericError("unsupported: extra planes beside a libjpeg-exact output (jpeg_scale)")
        rsm = None if rs is None else _resample(resize, crop, None, False)
        if libjxl().JxlHipImageOutSizePlanes(buf.ctypes.data, len(data), C.byref(fmt), int(downscale), _byref(layout), _byref(rsm), C.byref(planes), C.byref(info), C.byref(size)) != JXL_DEC_SUCCESS:
            raise GenericError(last_error())
        return info, size.value
    if jpeg_scale != 1:
        rs = _jpeg_scaled(jpeg_scale, downscale, rs)
        if libjxl().JxlHipImageOutSizeJpegScaled(buf.ctypes.data, len(data), C.byref(fmt), int(jpeg_scale), _byref(layout), _byref(rs), C.byref(info), C.byref(size)) != JXL_DEC_SUCCESS:
            raise GenericError(last_error())
    elif rs is not None:
        if libjxl().JxlHipImageOutSizeResized(buf.ctypes.data, len(data), C.byref(fmt), int(downscale), _byref(layout), C.byref(rs), C.byref(info), C.byref(size)) != JXL_DEC_SUCCESS:
            raise GenericError(last_error())
    elif layout is not None:
        if libjxl().JxlHipImageOutSizeLayout(buf.ctypes.data, len(data), C.byref(fmt), int(downscale), C.byref(layout), C.byref(info), C.byref(size)) != JXL_DEC_SUCCESS:
            raise GenericError(last_error())
    elif downscale == 1:
        check_dec_status(libjxl().JxlHipImageOutSize(buf.ctypes.data, len(data), C.byref(fmt), C.byref(info), C.byref(size)))
    elif libjxl().JxlHipImageOutSizeScaled(buf.ctypes.data, len(data), C.byref(fmt), int(downscale), C.byref(info), C.byref(size)) != JXL_DEC_SUCCESS:
        raise GenericError(last_error())
    return info, size.value


class PinnedBuffer:
    """Pinned host memory (JxlHipHostAlloc) as a numpy uint8 array: destination of a pipeline's host_out copies."""

    def __init__(self, nbytes: int):
        self._p = libjxl().JxlHipHostAlloc(max(1, int(nbytes)))
        if not self._p:
            raise MemoryError(last_error())
        self.nbytes = int(nbytes)
        self.array = np.ctypeslib.as_array((C.c_uint8 * max(1, self.nbytes)).from_address(self._p))[: self.nbytes]

    @property
    def ptr(self) -> int:
        return self._p

    def __del__(self):
        if getattr(self, "_p", None):
            self.array = None
            libjxl().JxlHipHostFree(self._p)
            self._p = None


class Pipeline:
    """The streaming decode pipeline of one GPU (include/jxl_hip.h JxlHipPipeline*; csrc/pipeline.h): submit jobs of compressed images, the library overlaps
    their stages — host parse / upload, LF, HF, IDCT, filters, copies — over its own streams and threads.  submit() returns a ticket, wait(ticket) the per-image
    status once the pixels are where they were asked for."""

    def __init__(self, device: int = 0, **options):
        o = JxlHipPipelineOptions()
        o.wide_first = -1
        for k, v in options.items():
            if not hasattr(o, k):
                raise TypeError(f"unknown pipeline option {k}")
            setattr(o, k, int(v))
        self._h = libjxl().JxlHipPipelineCreate(int(device), C.byref(o))
        if not self._h:
            raise CannotCreateDecoder(last_error())
        self._keep = {}

    def close(self):
        if getattr(self, "_h", None):
            libjxl().JxlHipPipelineDestroy(self._h)
            self._h = None
            self._keep = {}

    __del__ = close

    def submit(self, datas, dtype="uint8", num_channels=0, device_ptrs=None, host_ptrs=None, capacities=None, endianness=Endianness.Native, align=0, downscale=1,
               planar=False, plane_stride=0, scale=None, bias=None, resize=None, crop=None, filter=None, mirror=False, jpeg_pixels=False, jpeg_scale=1, resize_u8=False,
               extra_planes=None, plane_scale=None, plane_bias=None, planes_offset=0, planes_stride=0, output_color=None, convert_non_xyb=False) -> int:
        """Job of len(datas) images (bytes objects).  device_ptrs / host_ptrs: one destination address per image (exactly one of the two lists); the bytes objects and
        the destinations are kept referenced until wait().  downscale=8: the job is decoded at 1:8 (JxlHipPipelineSubmitScaled).  planar, plane_stride, scale, bias:
        the layout of every image of the job, as for BatchDecoder.add (JxlHipPipelineSubmitLayout).  resize, crop: every image of the job comes out resize[0] x resize[1]
        pixels (JxlHipPipelineSubmitResized) — destinations of one size, e.g. consecutive slices of one [N, C, H, W] tensor; an image the crop leaves fails alone.
        crop, filter ("bilinear" | "bicubic") and mirror each take one value for the job or a sequence of len(datas) per-image values (a None in a crop sequence: the
        whole picture; four plain integers are always ONE crop (x0, y0, w, h) for the whole job, also when the job has four images — per-image crops are a sequence of
        4-tuples or Nones; a string or a number is one filter / mirror for the job, any other iterable is read as per-image values).  Whenever one of them is a sequence, or filter / mirror is set, the job goes out with one JxlHipOutputResample per image
        (JxlHipPipelineSubmitResampled): one target size, everything else the image's own.
        jpeg_pixels: a job of libjpeg-exact pixels (JxlHipPipelineSubmitJpegPixels; BatchDecoder.decode_jpeg_pixels as pipeline stages) with the same keywords; an image
        that decode does not take fails alone, downscale other than 1 is refused here.
        jpeg_scale=2 | 4 | 8 (with jpeg_pixels only; one scale per job): libjpeg's scaled decode, as for BatchDecoder.add (JxlHipPipelineSubmitJpegPixelsScaled) —
        destinations are sized with image_out_size(..., jpeg_scale=), crops are in the scaled picture.
        resize_u8=True (with jpeg_pixels and resize only): every image of the job is resampled in Pillow's 8-bit arithmetic, as for BatchDecoder.add
        (JxlHipPipelineSubmitJpegPixelsResampled); an image the libjpeg-exact decode does not take fails alone.
        extra_planes, plane_scale, plane_bias, planes_offset, planes_stride: extra-channel planes behind every image's colour output, as for BatchDecoder.add
        (JxlHipPipelineSubmitPlanes) — destinations and capacities are sized with image_out_size(..., extra_planes=); an image that lacks one of the channels
        fails alone; not with jpeg_pixels.
        output_color, convert_non_xyb: the colour encoding of every image of the job, as for BatchDecoder.add (JxlHipPipelineSubmitColor); an image the target is refused
        for — a grey target on a colour image, convert_non_xyb on an image whose colour is only an ICC profile — fails alone; not with jpeg_pixels."""
        color = _color(output_color, convert_non_xyb)
        if color is not None and jpeg_pixels:
            raise GenericError("unsupported: output colour of a libjpeg-exact output (a jpeg_pixels job): those are libjpeg's samples")
        planes = _planes(extra_planes, plane_scale, plane_bias, planes_offset, planes_stride)
        if planes is not None and jpeg_pixels:
            raise GenericError("unsupported: extra planes beside a libjpeg-exact output (a jpeg_pixels job)")
        if resize_u8:
            _resize_u8(downscale, resize)
            if not jpeg_pixels:
                raise GenericError("unsupported: integer resample in a job that is not a libjpeg-exact one (resize_u8 needs jpeg_pixels=True: it resamples the u8 picture libjpeg gives)")
        if jpeg_pixels and int(downscale) != 1:
            raise GenericError("unsupported: libjpeg-exact decode of an output with downscale %d (libjpeg's scaled IDCTs are other arithmetic)" % int(downscale))
        if jpeg_scale != 1 and not jpeg_pixels:
            raise GenericError("unsupported: jpeg_scale %s in a job that is not a libjpeg-exact one (jpeg_pixels=True: only that decode writes libjpeg's scaled picture)" % (jpeg_scale,))
        layout = _layout(planar, plane_stride, scale, bias)
        n = len(datas)
        crops, seq_c = _per_image(crop, n, lambda v: len(v) == 4 and all(isinstance(x, (int, np.integer)) for x in v))
        if not seq_c and crop is not None and n:
            crop = crops[0]                 # (an iterable of four integers has been read: keep the tuple)
        filters, seq_f = _per_image(filter, n, lambda v: False)
        mirrors, seq_m = _per_image(mirror, n, lambda v: False)
        each = None
        if seq_c or seq_f or seq_m or filter is not None or mirror:
            each = (JxlHipOutputResample * max(1, n))(*[_resample(resize, crops[k], filters[k], mirrors[k]) for k in range(n)])
        rs = None if each is not None else _resize(resize, crop)
        ptrs = (C.c_char_p * n)(*datas)
        sizes = (C.c_size_t * n)(*[len(d) for d in datas])
        fmt = JxlPixelFormat(num_channels, _PIXEL_TYPES[np.dtype(dtype).name][0], endianness, align)
        dev = (C.c_void_p * n)(*device_ptrs) if device_ptrs is not None else None
        host = (C.c_void_p * n)(*host_ptrs) if host_ptrs is not None else None
        caps = (C.c_size_t * n)(*capacities) if capacities is not None else None
        if jpeg_pixels:
            if each is None and resize is not None:
                each = (JxlHipOutputResample * max(1, n))(*[_resample(resize, crop, None, False) for _ in range(n)])      # (filter 0, no mirror: the ...Resized call, byte for byte)
            if resize_u8:
                t = libjxl().JxlHipPipelineSubmitJpegPixelsResampled(self._h, ptrs, sizes, n, C.byref(fmt), dev, host, caps, _byref(layout), each, int(jpeg_scale), JXL_HIP_RESAMPLE_U8)
            elif jpeg_scale != 1:
                t = libjxl().JxlHipPipelineSubmitJpegPixelsScaled(self._h, ptrs, sizes, n, C.byref(fmt), dev, host, caps, _byref(layout), each, int(jpeg_scale))
            else:
                t = libjxl().JxlHipPipelineSubmitJpegPixels(self._h, ptrs, sizes, n, C.byref(fmt), dev, host, caps, _byref(layout), each)
        elif color is not None:
            if each is None and resize is not None:
                each = (JxlHipOutputResample * max(1, n))(*[_resample(resize, crop, None, False) for _ in range(n)])
            t = libjxl().JxlHipPipelineSubmitColor(self._h, ptrs, sizes, n, C.byref(fmt), dev, host, caps, int(downscale), _byref(layout), each, _byref(planes), C.byref(color))
        elif planes is not None:
            if each is None and resize is not None:
                each = (JxlHipOutputResample * max(1, n))(*[_resample(resize, crop, None, False) for _ in range(n)])
            t = libjxl().JxlHipPipelineSubmitPlanes(self._h, ptrs, sizes, n, C.byref(fmt), dev, host, caps, int(downscale), _byref(layout), each, C.byref(planes))
        elif each is not None:
            t = libjxl().JxlHipPipelineSubmitResampled(self._h, ptrs, sizes, n, C.byref(fmt), dev, host, caps, int(downscale), _byref(layout), each)
        elif rs is not None:
            t = libjxl().JxlHipPipelineSubmitResized(self._h, ptrs, sizes, n, C.byref(fmt), dev, host, caps, int(downscale), _byref(layout), C.byref(rs))
        elif layout is not None:
            t = libjxl().JxlHipPipelineSubmitLayout(self._h, ptrs, sizes, n, C.byref(fmt), dev, host, caps, int(downscale), C.byref(layout))
        elif downscale == 1:
            t = libjxl().JxlHipPipelineSubmit(self._h, ptrs, sizes, n, C.byref(fmt), dev, host, caps)
        else:
            t = libjxl().JxlHipPipelineSubmitScaled(self._h, ptrs, sizes, n, C.byref(fmt), dev, host, caps, int(downscale))
        if t < 0:
            raise GenericError(last_error())
        self._keep[t] = (datas, ptrs, sizes, dev, host, caps, n)
        return t

    def wait(self, ticket: int, check=True):
        """-> (per-image status list, end_ms).  check: raise GenericError if an image failed."""
        n = self._keep[ticket][6] if ticket in self._keep else 0
        st = (C.c_int * max(1, n))()
        end = C.c_float()
        rc = libjxl().JxlHipPipelineWait(self._h, int(ticket), st, n, C.byref(end))
        self._keep.pop(ticket, None)
        if rc != JXL_DEC_SUCCESS and check:
            raise GenericError(last_error())
        return list(st)[:n], float(end.value)

    # ---- reconstruction jobs (include/jxl_hip.h JxlHipPipelineSubmitJpegs; BatchDecoder.reconstruct_jpegs as pipeline stages)
    def submit_jpegs(self, datas, progressive_on_device=False, host_writer=False) -> int:
        """Job of len(datas) JPEG transcodes whose original files are wanted back, byte for byte.  No format and no destinations: the files stay with the pipeline
        until wait_jpegs(ticket).  progressive_on_device / host_writer: the two switches of BatchDecoder.reconstruct_jpegs (host_writer wins).  An image that
        cannot be reconstructed fails alone; such jobs mix freely with every other kind of job."""
        n = len(datas)
        ptrs = (C.c_char_p * n)(*datas)
        sizes = (C.c_size_t * n)(*[len(d) for d in datas])
        flags = (JXL_HIP_JPEG_DEVICE_PROGRESSIVE if progressive_on_device else 0) | (JXL_HIP_JPEG_HOST_WRITER if host_writer else 0)
        t = libjxl().JxlHipPipelineSubmitJpegs(self._h, ptrs, sizes, n, flags)
        if t < 0:
            raise GenericError(last_error())
        self._keep[t] = (datas, ptrs, sizes, None, None, None, n)
        return t

    def wait_jpegs(self, ticket: int):
        """-> (files, errors, end_ms): files[i] is the reconstructed file of image i as bytes, or None; errors[i] is None, or that image's reason.  Releases the ticket."""
        L = libjxl()
        n = self._keep[ticket][6] if ticket in self._keep else 0
        st = (C.c_int * max(1, n))()
        sizes = (C.c_size_t * max(1, n))()
        end = C.c_float()
        rc = L.JxlHipPipelineWaitJpegs(self._h, int(ticket), st, sizes, n, C.byref(end))
        call_error = last_error() if rc != JXL_DEC_SUCCESS else ""
        files, errors = [None] * n, [None] * n
        try:
            for i in range(n):
                if st[i] == 0:
                    out = np.empty(max(int(sizes[i]), 1), dtype=np.uint8)
                    if L.JxlHipPipelineCopyJpeg(self._h, int(ticket), i, out.ctypes.data, int(sizes[i])) != JXL_DEC_SUCCESS:
                        raise GenericError(last_error())
                    files[i] = out[:int(sizes[i])].tobytes()
                    continue
                L.JxlHipPipelineJpegStatus(self._h, int(ticket), i)
                errors[i] = last_error()
                if "JxlHipPipelineJpegStatus: unknown ticket" in errors[i]:      # (the wait itself failed — a ticket of another kind, an unknown one: nothing was collected)
                    raise GenericError(call_error or errors[i])
        finally:
            L.JxlHipPipelineReleaseJpegs(self._h, int(ticket))
            self._keep.pop(ticket, None)
        return files, errors, float(end.value)

    def wait_all(self):
        check_dec_status(libjxl().JxlHipPipelineWaitAll(self._h))

    def reset_clock(self):
        check_dec_status(libjxl().JxlHipPipelineResetClock(self._h))

    def collect_times(self):
        t, runs = JxlHipStageTimes(), C.c_int()
        check_dec_status(libjxl().JxlHipPipelineCollectTimes(self._h, C.byref(t), C.byref(runs)))
        return {n: getattr(t, n) for n, _ in JxlHipStageTimes._fields_}, runs.value

    @property
    def stage_bytes(self):
        out = (C.c_uint64 * 6)()
        libjxl().JxlHipPipelineStageBytes(self._h, C.byref(out))
        return dict(zip(("lf", "lfpost", "hf", "idct", "filter", "out"), [int(v) for v in out]))

    def info(self, name: str) -> int:
        return int(libjxl().JxlHipPipelineGetInfo(self._h, name.encode()))

    def set_option(self, name: str, value: int):
        """Options for the jobs submitted from now on (include/jxl_hip.h JxlHipPipelineSetOption): "jpeg_region" = 1 — libjpeg-exact jobs decode only the groups the
        crops of their outputs need (BatchDecoder.jpeg_region); info("hf_groups_decoded") / info("hf_groups_total") of the job prepared last.  "lf_group_max" (1 .. 8):
        jobs that are ready together share one SIMT LF launch, at most this many; "lf_streams_effective": LF streams in use (0: sized to the hardware queues);
        info("lf_groups") / info("lf_grouped_jobs") / info("lf_group_largest") count the launches since the last reset_clock()."""
        libjxl().JxlHipPipelineSetOption(self._h, name.encode(), int(value))


# ---- lossless encoder (include/jxl_hip.h JxlHipEncoder*; jpegxl-rs/src/encode.rs for the builder's names) ---------------------------------------
class EncodeError(Exception):
    """errors.rs EncodeError"""


ENCODE_PHASES = ("upload", "tokenise", "code_build", "count_scan", "pack", "copy_back", "splice")


def _rows_are_tight(shape, strides, item):
    """whether the samples of a row follow one another (the stride of an axis of extent 1 means nothing) and the rows go forward"""
    w, c = shape[1], shape[2] if len(shape) == 3 else 1
    if len(shape) == 3 and c > 1 and strides[2] != item:
        return False
    return (w == 1 or strides[1] == c * item) and (shape[0] == 1 or strides[0] >= w * c * item)


def _describe_input(img, bits, alpha_premultiplied, keep):
    """-> JxlHipEncodeImage for a numpy array, a torch tensor or anything with __cuda_array_interface__ (H x W or H x W x C, uint8 / uint16); `keep` holds what must outlive the call"""
    cai = None
    if type(img).__module__.split(".")[0] == "torch":
        import torch
        if img.is_cuda:                         # (read directly: torch's own __cuda_array_interface__ does not cover every integer type)
            torch.cuda.synchronize(img.device)
            item = img.element_size()
            cai = {"shape": tuple(img.shape), "typestr": {torch.uint8: "|u1", getattr(torch, "uint16", None): "<u2"}.get(img.dtype, str(img.dtype)),
                   "strides": tuple(s * item for s in img.stride()), "data": (img.data_ptr(), False)}
        else:
            img = img.numpy()
    if cai is None:
        cai = getattr(img, "__cuda_array_interface__", None)
    if cai is not None:
        shape, typestr, strides, ptr, on_device = tuple(cai["shape"]), cai["typestr"], cai.get("strides"), int(cai["data"][0]), 1
    else:
        img = np.asarray(img)
        if img.ndim in (2, 3) and not _rows_are_tight(img.shape, img.strides, img.itemsize):
            img = np.ascontiguousarray(img)
        shape, typestr, strides, ptr, on_device = img.shape, img.dtype.str, img.strides, img.ctypes.data, 0
    keep.append(img)
    if typestr not in ("|u1", "<u2"):
        raise EncodeError("unsupported: samples of type %s (uint8 and little-endian uint16 are encoded)" % typestr)
    item = 1 if typestr == "|u1" else 2
    if len(shape) not in (2, 3):
        raise EncodeError("unsupported: an image of %d dimensions (H x W or H x W x C)" % len(shape))
    h, w, c = shape[0], shape[1], shape[2] if len(shape) == 3 else 1
    pitch = 0
    if strides is not None:
        if not _rows_are_tight(shape, strides, item):
            raise EncodeError("unsupported: samples that are not interleaved and contiguous within a row")
        pitch = int(strides[0]) if h > 1 else 0
    return JxlHipEncodeImage(ptr, on_device, w, h, c, int(bits) if bits is not None else 8 * item, JXL_TYPE_UINT8 if item == 1 else JXL_TYPE_UINT16, pitch, 1 if alpha_premultiplied else 0)


def encode_lossless_bound(width, height, num_channels, bits=8, dtype="uint8") -> int:
    """JxlHipEncodeLosslessBound: the worst-case codestream size; needs no GPU."""
    im = JxlHipEncodeImage(None, 0, width, height, num_channels, bits, JXL_TYPE_UINT8 if np.dtype(dtype) == np.uint8 else JXL_TYPE_UINT16, 0, 0)
    n = C.c_size_t()
    if libjxl().JxlHipEncodeLosslessBound(C.byref(im), C.byref(n)):
        raise EncodeError(last_error())
    return n.value


class LosslessEncoder:
    """One JxlHipEncoder: encode(images) runs the whole list through one set of kernel launches.  device=-1: host only (refusals and bounds)."""

    def __init__(self, device: int = 0):
        self._h = libjxl().JxlHipEncoderCreate(device)
        if not self._h:
            raise EncodeError(last_error())

    def __del__(self):
        if getattr(self, "_h", None):
            libjxl().JxlHipEncoderDestroy(self._h)
            self._h = None

    def encode(self, images, bits=None, alpha_premultiplied=False, stream=None, raise_on_error=True):
        """-> list of codestreams (bytes); with raise_on_error=False a failed image gives its EncodeError in the list instead"""
        L, keep = libjxl(), []
        per_bits, _ = _per_image(bits, len(images), lambda v: False)
        arr = (JxlHipEncodeImage * max(1, len(images)))(*[_describe_input(im, b, alpha_premultiplied, keep) for im, b in zip(images, per_bits)])
        L.JxlHipEncoderEncodeLossless(self._h, arr, len(images), stream)
        out = []
        for i in range(len(images)):
            if L.JxlHipEncoderStatus(self._h, i):
                err = EncodeError(last_error())
                if raise_on_error:
                    raise err
                out.append(err)
                continue
            buf = C.create_string_buffer(L.JxlHipEncoderSize(self._h, i))
            if L.JxlHipEncoderCopy(self._h, i, buf, len(buf)):
                raise EncodeError(last_error())
            out.append(buf.raw)
        return out

    def max_token(self, i) -> int:
        return int(libjxl().JxlHipEncoderMaxToken(self._h, i))

    def phase_times(self) -> dict:
        ms = (C.c_float * 7)()
        libjxl().JxlHipEncoderPhaseTimes(self._h, C.byref(ms))
        return dict(zip(ENCODE_PHASES, [float(v) for v in ms]))


def encode_lossless(images, bits=None, device=0) -> list:
    """Lossless JPEG XL codestreams of `images` (numpy H x W / H x W x C uint8 / uint16 arrays, torch tensors or anything with __cuda_array_interface__; 1 to 4 channels:
    grey, grey + alpha, RGB, RGBA), all through one set of GPU launches.  bits: the depth (1..16), one value or one per image; default 8 / 16 by type."""
    return LosslessEncoder(device).encode(images, bits=bits)


@dataclass
class EncoderResult:
    """encode.rs:42 EncoderResult"""
    data: bytes


class JxlEncoder:
    """encode.rs JxlEncoder, the lossless case: encoder_builder(lossless=True, has_alpha=...).encode(data, width, height)."""

    def __init__(self, has_alpha=False, lossless=None, device=0, **other):
        refused = {"speed", "quality", "jpeg_quality", "use_container", "uses_original_profile", "decoding_speed", "init_buffer_size", "color_encoding", "target_intensity",
                   "parallel_runner", "use_box", "memory_manager"}
        for k in other:
            if k not in refused:
                raise TypeError(f"unknown encoder option {k}")
            raise EncodeError(f"unsupported: encoder option {k} (the encoder writes lossless bare codestreams only)")
        if not lossless:
            raise EncodeError("unsupported: lossy encoding (build the encoder with lossless=True)")
        self.has_alpha, self.lossless, self._device = bool(has_alpha), True, device

    def encode(self, data, width, height, bits=None) -> EncoderResult:
        a = np.asarray(data)
        if a.dtype not in (np.uint8, np.uint16):
            raise EncodeError("unsupported: samples of type %s (uint8 and uint16 are encoded)" % a.dtype)
        if width <= 0 or height <= 0 or a.size % (width * height) or not 1 <= a.size // (width * height) <= 4:
            raise EncodeError("the data does not hold width x height pixels of 1 to 4 channels")
        c = a.size // (width * height)
        if (c in (2, 4)) != self.has_alpha:
            raise EncodeError("%d channels %s has_alpha" % (c, "need" if c in (2, 4) else "contradict"))
        return EncoderResult(LosslessEncoder(self._device).encode([a.reshape(height, width, c)], bits=bits)[0])

    def encode_jpeg(self, data):
        raise EncodeError("unsupported: encode_jpeg (JPEG transcoding is not written)")

    def encode_frame(self, frame, width, height):
        raise EncodeError("unsupported: encode_frame (one frame of interleaved samples through encode())")

    def multiple(self, width, height):
        raise EncodeError("unsupported: multiple frames (animation is not written)")

    def add_metadata(self, metadata, compress=False):
        raise EncodeError("unsupported: metadata boxes (the encoder writes bare codestreams)")

    def set_frame_option(self, option, value):
        raise EncodeError("unsupported: frame options (one fixed lossless stream shape)")


def encoder_builder(**options) -> JxlEncoder:
    """encode.rs:523 encoder_builder(): options are keyword arguments; everything but lossless=True and has_alpha raises EncodeError("unsupported: ...")"""
    return JxlEncoder(**options)
