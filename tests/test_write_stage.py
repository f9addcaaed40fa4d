"""GPU tests (-m gpu) that pin the WRITE STAGE: every output format derived, exactly, from the decoder's own little-endian float32 output.

Given the float the pipeline produced, the u8 / u16 / f16 value, byte order, channel subset, orientation and row padding of any other output
format follow from IEEE 754 and the API's documentation, so the reference here is numpy (expected_output below), shares no code with oracle/ and
needs no tolerance.  The input of the comparison is the product's stored-orientation, 4-channel, little-endian f32 decode of the same stream.
The comparison rests on one property of the code (kernels.hip / kernels_features.hip): for a given stream and decoder configuration the float
that reaches StoreSample (pixel_ops.h, the one sample conversion of every kernel below) / the packed stores is computed before, and independently of, the output format — the format only
selects a branch of the store.  One kernel serves every format of a stream, so no comparison here mixes two kernels; that the fused and the
stage-by-stage VarDCT kernels agree bit for bit is asserted on its own (test_fused_and_unfused_kernels_write_the_same_floats).

Write paths, the stream that reaches each here, and the host condition that routes it there:
  * FusedGabEpf1OutKernel (packed dword stores for u8 RGB / RGBA in stored orientation with width % 4 == 0 and 4-byte-aligned rows — the RGB
    form with a DPP exchange per quad —, StorePixel otherwise): streams fused_*: single XYB VarDCT frame, gaborish on, one EPF iteration, sRGB,
    no upsampling, not complex (decoder.cc PrepareTables `fused`; kernels.hip FusedEligible).
  * OutputKernel: stream epf0 (no EPF iteration, so no EPF kernel is there to write: kernels.hip EpfWritesOutput is false);
    behind UpsampleKernel: stream upsampled (upsampling 2, 203 x 139: OutPixelPtr works with img_w / img_h, not the coded size);
    its chroma-upsampling branch: stream ycbcr420 (a YCbCr frame with 2x2 subsampled chroma, FrameDev.subsampled).
  * EpfTileKernel / EpfTile12Kernel handing their last pass to ColorAndStore -> StorePixel: stream epf2 (two EPF iterations: not fusable,
    EpfWritesOutput true).
  * ModularOutputKernel: streams modular_rgba8, modular_rgba16, modular_greya8, modular_grey8, the ramps and the plain float planes — a single
    Modular frame that is not XYB, not upsampled, replaces the whole canvas and has no float extra channel (decoder.cc: `complex` stays false).
  * WriteKernel (frame tail of `complex` images, decoder.cc ParseImage / Prepare): vardct_layers and modular_layers (more than one frame),
    patches (flag 2 + a reference-only frame), unpremul (associated alpha + unpremul_alpha, Prepare sets complex), modular_grey_layers,
    sample_grey.jxl (patches), the layered float planes (two frames) and the float-alpha plane (a float extra channel).

Crafted float planes (lossless float Modular images put chosen bit patterns in front of the sample conversion): a 24-bit float plane
(1 + 7 + 16 bits) reaches every class of the half converter with both signs, a binary16 plane pins half -> f32 -> half as the identity over all
63488 patterns with an exponent field below 31, a binary32 plane carries values above 1 and the exact rounding ties of the integer outputs, a
second one +inf, NaN and the largest finite floats.
-inf is not delivered: binary32 samples of the synthesiser are limited to non-negative patterns and the narrow formats have no
infinities.  Every crafted plane asserts its own coverage (at least 32 samples per class) on the f32 decode before anything is compared."""
import ctypes as C
import struct

import numpy as np
import pytest

from conftest import fixture_bytes
import synth_lib as S
from test_gpu_parity import COLOUR_ENCODINGS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def jx(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import jpegxl_rs_amd as jx
    return jx


# ---- the reference: a numpy write stage -----------------------------------------------------------------------------------------------
DTYPES = ("uint8", "uint16", "float16", "float32")
ORIENT = {1: lambda v: v, 2: lambda v: v[:, ::-1], 3: lambda v: v[::-1, ::-1], 4: lambda v: v[::-1], 5: lambda v: v.swapaxes(0, 1),
          6: lambda v: v[::-1].swapaxes(0, 1), 7: lambda v: v[::-1, ::-1].swapaxes(0, 1), 8: lambda v: v[:, ::-1].swapaxes(0, 1)}
# (EXIF: 2 mirror horizontally, 3 rotate 180, 4 mirror vertically, 5 transpose, 6 rotate 90 clockwise — the first output row is the first stored column read
# bottom-up —, 7 anti-transpose, 8 rotate 90 counter-clockwise)


def select_samples(f32_rgba, nch, orientation, grey):
    """(H, W, nch) float32: the channels a caller who asks for nch channels gets — 4: R G B A, 3: R G B, 2: (G, A) of a colour image / (grey, A) of a grey one,
    1: G / grey — in the requested orientation."""
    lum = 0 if grey else 1
    idx = {4: [0, 1, 2, 3], 3: [0, 1, 2], 2: [lum, 3], 1: [lum]}[nch]
    return np.ascontiguousarray(ORIENT[orientation](f32_rgba[..., idx]))


def convert_samples(v, dtype, int_mul=None):
    """float32 array -> the native-endian integer view of the samples of `dtype` (u8, u16, the bits of f16 as u16, the bits of f32 as u32)"""
    v = np.ascontiguousarray(v, dtype=np.float32)
    if dtype == "float32":
        return v.view(np.uint32)
    if dtype == "float16":
        with np.errstate(over="ignore", under="ignore", invalid="ignore"):
            return v.astype(np.float16).view(np.uint16)
    mul = np.float32(int_mul if int_mul else (255 if dtype == "uint8" else 65535))
    with np.errstate(invalid="ignore"):
        q = np.rint(np.clip(v, np.float32(0), np.float32(1)).astype(np.float32) * mul)       # rint: round half to even, as NearestInt / __float2int_rn
    return np.nan_to_num(q, nan=0.0).astype(np.uint8 if dtype == "uint8" else np.uint16)


def padded_stride(row_bytes, align):
    return row_bytes if align <= 1 else (row_bytes + align - 1) // align * align


def expected_output(f32_rgba, *, dtype, nch, big_endian=False, align=0, orientation=1, int_mul=None, grey=False):
    """The exact bytes of the output format (dtype, nch, byte order, align, orientation[, integer range]) given the stored-orientation RGBA f32 decode
    (h, w, 4): a (rows, stride) uint8 array; the bytes behind a row's samples (padding) are zero here and are not to be compared."""
    q = convert_samples(select_samples(f32_rgba, nch, orientation, grey), dtype, int_mul)
    if big_endian:
        q = q.byteswap()
    rows = q.reshape(q.shape[0], -1).view(np.uint8)
    out = np.zeros((rows.shape[0], padded_stride(rows.shape[1], align)), np.uint8)
    out[:, :rows.shape[1]] = rows
    return out


def test_expected_output_helper():
    """The reference itself (no device involved): the f16 branch against struct's binary16 packing on fixed binary32 patterns, the integer branch on hand-computed
    ties, and the eight orientations of a 3 x 2 array."""
    pats = [0x00000000, 0x80000000, 0x3F800000, 0xBF800000, 0x3F801000, 0x3F803000, 0x3F802FFF, 0x3F801001, 0x3FFFF000, 0x477FE000, 0x477FEFFF, 0x477FF000, 0x47800000,
            0x7F7FFFFF, 0x7F800000, 0xFF800000, 0x38800000, 0x387FFFFF, 0x38000000, 0x33800000, 0x33000000, 0x33000001, 0x32FFFFFF, 0xB3000001, 0x33C00000, 0x00000001,
            0x3EAAAAAB, 0x3F000000, 0x3B808081, 0x42F70000]
    v = np.array(pats, np.uint32).view(np.float32)
    got = convert_samples(v, "float16")
    for p, g in zip(v, got):
        try:
            want = struct.unpack("<H", struct.pack("<e", float(p)))[0]
        except OverflowError:                                                     # struct refuses what rounds to infinity
            want = 0x7C00 | (0x8000 if p < 0 else 0)
        assert int(g) == want, (hex(int(p.view(np.uint32))), hex(int(g)), hex(want))
    assert convert_samples(np.array([np.nan], np.float32), "float16")[0] & 0x7FFF > 0x7C00
    # 0.5 x 255 = 127.5 -> 128 and 0.5 x 1023 = 511.5 -> 512 (even), 2.5 / 255 -> 2 if the product is the tie; clamping; -0
    t = np.array([0.5, -1.0, 2.0, np.inf, -np.inf, -0.0, 1.0], np.float32)
    assert convert_samples(t, "uint8").tolist() == [128, 0, 255, 255, 0, 0, 255]
    assert convert_samples(t, "uint16", 1023).tolist() == [512, 0, 1023, 1023, 0, 0, 1023]
    assert convert_samples(np.array([0.5], np.float32), "uint16").tolist() == [32768]          # 32767.5: tie to even
    a = np.arange(24, dtype=np.float32).reshape(2, 3, 4)                       # h = 2, w = 3
    outs = [select_samples(a, 4, o, False) for o in range(1, 9)]
    assert [x.shape[:2] for x in outs] == [(2, 3)] * 4 + [(3, 2)] * 4
    assert len({x.tobytes() for x in outs}) == 8
    px = lambda y, x: a[y, x, 0]
    # first output row of each orientation, spelled out: (stored row, stored column) of its samples
    assert outs[1][0, :, 0].tolist() == [px(0, 2), px(0, 1), px(0, 0)] and outs[2][0, :, 0].tolist() == [px(1, 2), px(1, 1), px(1, 0)]
    assert outs[3][0, :, 0].tolist() == [px(1, 0), px(1, 1), px(1, 2)] and outs[4][0, :, 0].tolist() == [px(0, 0), px(1, 0)]
    assert outs[5][0, :, 0].tolist() == [px(1, 0), px(0, 0)] and outs[6][0, :, 0].tolist() == [px(1, 2), px(0, 2)] and outs[7][0, :, 0].tolist() == [px(0, 2), px(1, 2)]
    assert select_samples(a, 2, 1, False)[0, 0].tolist() == [1, 3] and select_samples(a, 2, 1, True)[0, 0].tolist() == [0, 3] and select_samples(a, 1, 1, False)[0, 0].tolist() == [1]
    e = expected_output(a, dtype="uint16", nch=3, big_endian=True, align=64)
    assert e.shape == (2, 64) and e[0, :20].tolist() == [0, 0] + [0xFF] * 16 + [0, 0]          # (0, 1, 2 | 4, 5, 6 | 8 ... clamped; then padding)


# ---- the product: one decode through the C ABI, raw bytes out ------------------------------------------------------------------------------
def raw_decode(jx, data, dtype, nch, big_endian=False, align=0, keep_orientation=False, unpremul=False, depth_bits=0):
    """-> (width, height, bytes of the image-out buffer) exactly as JxlDecoder._decode_internal drives the ABI (decode_with), plus JxlDecoderSetImageOutBitDepth
    (custom depth `depth_bits`) after the buffer is set"""
    L = jx.libjxl()
    raw = np.frombuffer(data, np.uint8)
    dec = L.JxlDecoderCreate(None)
    assert dec
    try:
        assert L.JxlDecoderSubscribeEvents(dec, jx.JXL_DEC_BASIC_INFO | jx.JXL_DEC_FULL_IMAGE) == 0
        assert L.JxlDecoderSetKeepOrientation(dec, 1 if keep_orientation else 0) == 0
        assert L.JxlDecoderSetUnpremultiplyAlpha(dec, 1 if unpremul else 0) == 0
        assert L.JxlDecoderSetInput(dec, raw.ctypes.data, len(raw)) == 0
        L.JxlDecoderCloseInput(dec)
        fmt = jx.JxlPixelFormat(nch, jx._PIXEL_TYPES[dtype][0], jx.JXL_BIG_ENDIAN if big_endian else jx.JXL_LITTLE_ENDIAN, align)
        info = jx.JxlBasicInfo()
        out = None
        while True:
            st = L.JxlDecoderProcessInput(dec)
            if st == jx.JXL_DEC_BASIC_INFO:
                assert L.JxlDecoderGetBasicInfo(dec, C.byref(info)) == 0
            elif st == jx.JXL_DEC_NEED_IMAGE_OUT_BUFFER:
                size = C.c_size_t()
                assert L.JxlDecoderImageOutBufferSize(dec, C.byref(fmt), C.byref(size)) == 0, jx.last_error()
                out = np.full(size.value, 0xA5, np.uint8)
                assert L.JxlDecoderSetImageOutBuffer(dec, C.byref(fmt), out.ctypes.data, out.nbytes) == 0, jx.last_error()
                if depth_bits:
                    assert L.JxlDecoderSetImageOutBitDepth(dec, C.byref(jx.JxlBitDepth(2, depth_bits, 0))) == 0, jx.last_error()
            elif st in (jx.JXL_DEC_FULL_IMAGE, jx.JXL_DEC_FRAME):
                continue
            elif st == jx.JXL_DEC_SUCCESS:
                break
            else:
                raise AssertionError((st, jx.last_error()))
    finally:
        L.JxlDecoderDestroy(dec)
    assert out is not None
    return info.xsize, info.ysize, out


def batch_decode(jx, data, dtype, nch, big_endian=False, align=0, keep_orientation=False):
    """-> (width, height, bytes) through the batch extension (JxlHipBatch*), which — unlike JxlDecoderSetImageOutBuffer, see test_the_abi_refuses_... below — hands out one
    or two channels of a colour image; it has no un-premultiplication and no custom integer depth"""
    b = jx.BatchDecoder(0)
    b.set_option("keep_orientation", 1 if keep_orientation else 0)
    b.add(data, dtype, nch, jx.JXL_BIG_ENDIAN if big_endian else jx.JXL_LITTLE_ENDIAN, align)
    b.prepare(); b.decode(); b.finish()
    out = np.full(b.out_size(0), 0xA5, np.uint8)
    assert jx.libjxl().JxlHipBatchCopyOutput(b._h, 0, out.ctypes.data, out.nbytes, None) == 0, jx.last_error()
    info = b.info(0)
    return info.xsize, info.ysize, out


def stored_rgba_f32(jx, data, unpremul=False):
    """the input of every comparison: (h, w, 4) float32, stored orientation, little endian"""
    w, h, buf = raw_decode(jx, data, "float32", 4, keep_orientation=True, unpremul=unpremul)
    assert buf.nbytes == w * h * 16
    return buf.view("<f4").astype(np.float32).reshape(h, w, 4)


def stream_bases(jx, data, unpremul):
    """nch -> the RGBA f32 input of the comparison.  One array for every channel count, except with un-premultiplied output: the division only happens when alpha is
    handed out (4 channels), so the colour of 3-channel output comes from the 3-channel f32 decode under the same setting — the same kernel, not dividing"""
    base = stored_rgba_f32(jx, data, unpremul)
    if not unpremul:
        return {n: base for n in (1, 2, 3, 4)}
    w, h, buf = raw_decode(jx, data, "float32", 3, keep_orientation=True, unpremul=True)
    rgb = buf.view("<f4").astype(np.float32).reshape(h, w, 3)
    assert not np.array_equal(rgb, base[..., :3]) and (base[..., :3].max(axis=2) > base[..., 3]).any()        # (the division happened: some colour exceeds its alpha)
    return {3: np.dstack([rgb, base[..., 3:]]), 4: base}


def check_format(jx, data, base, *, dtype, nch, big_endian=False, align=0, orientation=1, int_mul=None, grey=False, unpremul=False, depth_bits=0, what=""):
    """One decode in the given format, byte-compared with expected_output(base).  f16 samples whose input is NaN only have to be NaN; integer samples whose input
    is NaN are not asserted."""
    want = expected_output(base, dtype=dtype, nch=nch, big_endian=big_endian, align=align, orientation=orientation, int_mul=int_mul, grey=grey)
    if nch < 3 and not grey:                                                  # the C ABI refuses fewer than three channels of a colour image; the batch extension writes G
        assert not unpremul and not depth_bits
        w, h, buf = batch_decode(jx, data, dtype, nch, big_endian, align, keep_orientation=orientation == 1)
    else:
        w, h, buf = raw_decode(jx, data, dtype, nch, big_endian, align, keep_orientation=orientation == 1, unpremul=unpremul, depth_bits=depth_bits)
    tag = (what, dtype, nch, "BE" if big_endian else "LE", align, orientation, int_mul)
    bps = np.dtype(dtype).itemsize
    rows, stride = want.shape
    assert (h, w) == ((base.shape[1], base.shape[0]) if orientation > 4 else base.shape[:2]), tag
    row_bytes = w * nch * bps
    assert stride == padded_stride(row_bytes, align) and buf.nbytes == stride * (rows - 1) + row_bytes, (tag, buf.nbytes, stride, rows, row_bytes)
    got = np.zeros((rows, stride), np.uint8)
    got.reshape(-1)[:buf.nbytes] = buf
    got, want = got[:, :row_bytes], want[:, :row_bytes]
    src = select_samples(base, nch, orientation, grey).reshape(rows, -1)
    nan = np.isnan(src)
    if nan.any() and dtype != "float32":
        order = ">" if big_endian else "<"
        g = np.ascontiguousarray(got).view(order + "u" + str(bps)).astype(np.uint32)
        wv = np.ascontiguousarray(want).view(order + "u" + str(bps)).astype(np.uint32)
        if dtype == "float16":
            assert ((g[nan] & 0x7FFF) > 0x7C00).all(), (tag, "NaN in, no NaN out")
        assert np.array_equal(g[~nan], wv[~nan]), (tag, int((g[~nan] != wv[~nan]).sum()))
        return
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        y, xb = bad[0]
        raise AssertionError((tag, "%d differing bytes, first at row %d byte %d: got %d want %d (source sample %r)" % (len(bad), y, xb, got[y, xb], want[y, xb], float(src[y, xb // bps]))))


def padding_align(row_bytes):
    return next(a for a in (64, 96, 80, 112, 144) if row_bytes % a)


# ---- 2. the format matrix over every write path ------------------------------------------------------------------------------------------------
def _alpha(w, h, lo=0):
    return (lo + np.add.outer(np.arange(h) * 3, np.arange(w) * 5) % (256 - lo)).astype(np.uint8)


def _with_features(fn, **feat):
    S.set_features(**feat)
    try:
        return fn()
    finally:
        S.set_features()


def _modular_image(seed, w, h, c, bits):
    rng = np.random.default_rng(seed)
    base = S.synthetic_image(seed, max(w, 8), max(h, 8)).astype(np.int64)[:h, :w]
    full = (1 << bits) - 1
    img = np.stack([base[..., i % 3] * full // 255 for i in range(c)], -1)
    img = np.clip(img + rng.integers(-3, 4, img.shape) * (full // 255), 0, full)
    img[0, :4] = 0; img[1, :4] = full                                       # both ends of the range
    return img.astype(np.int32)


def _vardct_layers():
    big, small = S.synthetic_image(6, 200, 136), S.synthetic_image(9, 64, 48)
    return S.encode_vardct_frame(big, S.frame(is_last=0, save_as_reference=1), seed=3, strategy_mix=2) + \
        S.encode_vardct_frame(small, S.frame(emit=1, have_crop=1, crop_x0=100, crop_y0=60, canvas_w=200, canvas_h=136, blend_mode=1, blend_source=1), seed=4)


def _modular_layers():
    img, small = _modular_image(5, 203, 139, 4, 8), _modular_image(9, 64, 48, 4, 8)
    return S.encode_modular_frame(img, S.frame(is_last=0, save_as_reference=2), bits=8) + \
        S.encode_modular_frame(small, S.frame(emit=1, have_crop=1, crop_x0=10, crop_y0=20, canvas_w=203, canvas_h=139, blend_mode=2, blend_source=2), bits=8)


def _patches():
    ref_a, main = S.synthetic_image(50, 64, 48), S.synthetic_image(51, 200, 136)
    hdr = dict(frame_type=2, is_last=0, save_before_ct=1, have_crop=1, canvas_w=200, canvas_h=136)
    ra = S.encode_vardct_frame(ref_a, S.frame(save_as_reference=1, **hdr), seed=3)
    patches = [(1, 4, 6, 20, 16, [(10, 12, [(1, 0, 0)]), (100, 50, [(2, 0, 0)]), (150, 100, [(3, 0, 1)]), (180, 120, [(2, 0, 0)])])]
    return ra + _with_features(lambda: S.encode_vardct_frame(main, S.frame(emit=1), seed=4), patches=patches)


def _modular_grey_layers():
    img, small = _modular_image(7, 139, 203, 1, 8), _modular_image(8, 48, 64, 1, 8)
    return S.encode_modular_frame(img, S.frame(is_last=0, save_as_reference=1), bits=8) + \
        S.encode_modular_frame(small, S.frame(emit=1, have_crop=1, crop_x0=30, crop_y0=40, canvas_w=139, canvas_h=203, blend_mode=1, blend_source=1), bits=8)


# name -> (builder, grey, unpremul_alpha); sizes: non-square everywhere, odd where the path allows, 520 wide = three groups
STREAMS = {
    "fused_rgb_w4": (lambda: S.encode_vardct(S.synthetic_image(1, 200, 136), seed=3, strategy_mix=2, epf_iters=1, gab=1), False, False),
    "fused_rgba_w4": (lambda: S.encode_vardct(S.synthetic_image(2, 200, 136), seed=3, strategy_mix=2, epf_iters=1, gab=1, alpha=_alpha(200, 136)), False, False),
    "fused_rgb_odd": (lambda: S.encode_vardct(S.synthetic_image(3, 203, 139), seed=4, strategy_mix=1, epf_iters=1, gab=1), False, False),
    "fused_rgba_odd": (lambda: S.encode_vardct(S.synthetic_image(4, 67, 41), seed=5, epf_iters=1, gab=1, alpha=_alpha(67, 41)), False, False),
    "fused_rgb_three_groups": (lambda: S.encode_vardct(S.synthetic_image(5, 520, 72), seed=6, strategy_mix=2, epf_iters=1, gab=1), False, False),
    "epf0": (lambda: S.encode_vardct(S.synthetic_image(6, 200, 136), seed=3, strategy_mix=2, epf_iters=0, gab=1), False, False),
    "epf2": (lambda: S.encode_vardct(S.synthetic_image(7, 77, 61), seed=4, epf_iters=2, gab=1, alpha=_alpha(77, 61)), False, False),
    "upsampled": (lambda: S.encode_vardct(S.synthetic_image(8, 203, 139), seed=4, strategy_mix=2, epf_iters=2, gab=1, upsampling=2, alpha=_alpha(203, 139)), False, False),
    "ycbcr420": (lambda: S.encode_ycbcr(S.synthetic_image(9, 203, 139), "420", seed=2), False, False),
    "modular_rgba8": (lambda: S.encode_modular(_modular_image(10, 203, 139, 4, 8), 8, True, 0), False, False),
    "modular_rgba16": (lambda: S.encode_modular(_modular_image(11, 77, 61, 4, 16), 16, False, 0), False, False),
    "modular_greya8": (lambda: S.encode_modular(_modular_image(12, 139, 77, 2, 8), 8, False, 0), True, False),
    "modular_grey8": (lambda: S.encode_modular(_modular_image(13, 77, 139, 1, 8), 8, False, 0), True, False),
    "vardct_layers": (_vardct_layers, False, False),
    "modular_layers": (_modular_layers, False, False),
    "patches": (_patches, False, False),
    "unpremul": (lambda: S.encode_vardct_frame(S.synthetic_image(5, 200, 136), S.frame(alpha_premultiplied=1), seed=3, alpha=_alpha(200, 136, 64)), False, True),
    "modular_grey_layers": (_modular_grey_layers, True, False),
    "sample_grey": (lambda: fixture_bytes("sample_grey.jxl"), True, False),
}
WRITE_KERNEL_STREAMS = ("vardct_layers", "modular_layers", "patches", "unpremul", "modular_grey_layers")


def build_stream(name, orientation=1):
    fn, grey, unpremul = STREAMS[name]
    S.set_orientation(orientation)
    try:
        return fn(), grey, unpremul
    finally:
        S.set_orientation()


@pytest.mark.parametrize("name", sorted(STREAMS))
def test_format_matrix(jx, name):
    """{u8, u16, f16, f32} x {little, big endian} x {1, 2, 3, 4 channels} x {align 0, an align that pads}: 64 decodes of the stream, each byte for byte the numpy
    write stage applied to the stream's own RGBA f32 decode."""
    data, grey, unpremul = build_stream(name)
    bases = stream_bases(jx, data, unpremul)
    assert np.isfinite(bases[4]).all() and bases[4][..., :3].std() > 0.01
    h, w = bases[4].shape[:2]
    for dtype in DTYPES:
        for nch in ((3, 4) if unpremul else (1, 2, 3, 4)):                       # (un-premultiplied output exists behind the C ABI only, and that has no 1- / 2-channel colour output)
            row_bytes = w * nch * np.dtype(dtype).itemsize
            for align in (0, padding_align(row_bytes)):
                for big in (False, True):
                    check_format(jx, data, bases[nch], dtype=dtype, nch=nch, big_endian=big, align=align, grey=grey, unpremul=unpremul, what=name)


@pytest.mark.parametrize("name", sorted(n for n in STREAMS if n != "sample_grey"))
def test_orientation_through_every_write_path(jx, name):
    """Orientations 6 and 7 (all of 2..8 on the plain VarDCT stream and on one frame-tail stream) of a non-square image through each write path: u16 big endian and
    f16, 3 and 4 channels, plus u8 RGB with padded rows; the oriented output is the stored-orientation f32 decode of the same stream, re-oriented by numpy."""
    every = name in ("fused_rgb_w4", "modular_layers")
    for o in (range(2, 9) if every else (6, 7)):
        data, grey, unpremul = build_stream(name, o)
        bases = stream_bases(jx, data, unpremul)
        base = bases[4]
        assert base.shape[0] != base.shape[1]
        ow = base.shape[0] if o > 4 else base.shape[1]
        for dtype, big in (("uint16", True), ("float16", False)) + ((("uint8", False), ("float32", True)) if every else ()):
            for nch in (3, 4):
                check_format(jx, data, bases[nch], dtype=dtype, nch=nch, big_endian=big, orientation=o, grey=grey, unpremul=unpremul, what=name)
        check_format(jx, data, bases[3], dtype="uint8", nch=3, align=padding_align(ow * 3), orientation=o, grey=grey, unpremul=unpremul, what=name)
        if not unpremul:
            check_format(jx, data, base, dtype="float16", nch=2, big_endian=True, orientation=o, grey=grey, what=name)


def test_the_abi_refuses_one_and_two_channels_of_a_colour_image(jx):
    """JxlDecoderImageOutBufferSize / SetImageOutBuffer fail for num_channels 1 and 2 unless the image is grey (as libjxl does): why the matrix takes those formats of
    colour images through the batch extension"""
    data, _, _ = build_stream("fused_rgba_odd")
    for nch in (1, 2):
        with pytest.raises(AssertionError, match="too low for colour output"):
            raw_decode(jx, data, "uint8", nch)


def test_fused_and_unfused_kernels_write_the_same_floats(jx):
    """FusedGabEpf1OutKernel against the stage-by-stage kernels (force_unfused_filters): the f32 output of the same stream, bit for bit — and every integer / half
    format of the stage-by-stage path derived from its own f32 output (the matrix of OutputKernel's siblings under that option)."""
    data = S.encode_vardct(S.synthetic_image(1, 200, 136), seed=3, strategy_mix=2, epf_iters=1, gab=1, alpha=_alpha(200, 136))

    def batch(dtype, nch, unfused, big=False):
        b = jx.BatchDecoder(0)
        b.add(data, dtype, nch, jx.JXL_BIG_ENDIAN if big else jx.JXL_LITTLE_ENDIAN)
        b.set_option("force_unfused_filters", 1 if unfused else 0)
        b.prepare(); b.decode(); b.finish()
        return b.output(0)                                                    # (values, whatever the byte order was)
    fused, unfused = batch("float32", 4, False), batch("float32", 4, True)
    assert np.array_equal(fused.view(np.uint32), unfused.view(np.uint32)), int((fused.view(np.uint32) != unfused.view(np.uint32)).sum())
    base = unfused.reshape(136, 200, 4)
    for dtype in ("uint8", "uint16", "float16"):
        for nch in (1, 2, 3, 4):
            for big in (False, True):
                got = batch(dtype, nch, True, big)
                want = convert_samples(select_samples(base, nch, 1, False), dtype)
                assert np.array_equal(got.view(want.dtype).reshape(want.shape), want), (dtype, nch, big)


@pytest.mark.parametrize("name", ["fused_rgb_w4", "modular_rgba16", "vardct_layers"])
def test_image_out_bit_depth(jx, name):
    """JxlDecoderSetImageOutBitDepth with a custom depth: samples are round-half-even(clamp(v) x (2^bits - 1)) — on a VarDCT stream, a Modular stream and a
    frame-tail stream, for 3 and 4 channels and both byte orders."""
    data, grey, unpremul = build_stream(name)
    base = stored_rgba_f32(jx, data, unpremul)
    for dtype, bits in (("uint8", 1), ("uint8", 5), ("uint16", 1), ("uint16", 5), ("uint16", 10), ("uint16", 12), ("uint16", 16)):
        for nch, big in ((3, False), (4, True)):
            check_format(jx, data, base, dtype=dtype, nch=nch, big_endian=big, int_mul=(1 << bits) - 1, depth_bits=bits, grey=grey, what=name)


# ---- 3. the whole domain of the sample conversion ----------------------------------------------------------------------------------------------
MIN_SAMPLES = 32


def half_classes(v):
    """name -> mask over the float32 array v: the classes of a binary32 -> binary16 conversion, from the bit pattern alone (sign taken apart by the caller)"""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    a = (u & 0x7FFFFFFF).astype(np.int64)
    e = (a >> 23) - 127
    man = a & 0x7FFFFF
    finite = (a >> 23) != 255
    nrm = finite & (e >= -14) & (e <= 14)
    rem, m = man & 0x1FFF, man >> 13
    sub = finite & (e >= -24) & (e <= -15)
    d = np.where(sub, -1 - e, 14)                                              # bits dropped from the 24-bit significand
    sig = man | 0x800000
    srem, shalf, sm = sig & ((1 << d) - 1), 1 << (d - 1), sig >> d
    top = finite & (e == 15)
    return {
        "normal_exact": nrm & (rem == 0), "normal_round_down": nrm & (rem > 0) & (rem < 0x1000), "normal_round_up": nrm & (rem > 0x1000),
        "normal_tie_to_even_kept": nrm & (rem == 0x1000) & (m % 2 == 0), "normal_tie_to_even_bumped": nrm & (rem == 0x1000) & (m % 2 == 1),
        "carry_into_exponent": nrm & (m == 0x3FF) & (rem >= 0x1000),
        "top_binade_finite": top & ((m < 0x3FF) | (rem < 0x1000)), "65504_to_65520_stays_finite": top & (m == 0x3FF) & (rem < 0x1000),
        "carry_into_infinity": top & (m == 0x3FF) & (rem >= 0x1000), "beyond_half_range": finite & (e >= 16),
        "subnormal_round_down": sub & (srem < shalf), "subnormal_round_up": sub & (srem > shalf),
        "subnormal_tie_kept": sub & (srem == shalf) & (sm % 2 == 0), "subnormal_tie_bumped": sub & (srem == shalf) & (sm % 2 == 1),
        "exactly_2^-25_to_zero": finite & (e == -25) & (man == 0), "just_above_2^-25_to_2^-24": finite & (e == -25) & (man > 0),
        "below_2^-25_to_zero": finite & (a > 0) & (e < -25), "zero": a == 0,
    }


def int_tie_classes(v, mul):
    """exact ties of the integer conversion: clamp(v) x mul == k + 0.5 in float32, by the parity of k"""
    with np.errstate(invalid="ignore"):
        p = np.clip(np.ascontiguousarray(v, dtype=np.float32), np.float32(0), np.float32(1)).astype(np.float32) * np.float32(mul)
        k = np.floor(p)
        tie = (p - k) == np.float32(0.5)
    return {"tie_%d_even_k" % mul: tie & (k % 2 == 0), "tie_%d_odd_k" % mul: tie & (k % 2 == 1)}


def assert_coverage(masks, what):
    short = {n: int(m.sum()) for n, m in masks.items() if int(m.sum()) < MIN_SAMPLES}
    assert not short, (what, "classes with fewer than %d samples" % MIN_SAMPLES, short)


def float24_patterns():
    """24-bit float patterns (sign, 7 exponent bits with bias 63, 16 mantissa bits: IntToFloatSample) for every class of half_classes, both signs"""
    rng = np.random.default_rng(24)
    pat = lambda e, m16: ((np.asarray(e, np.int64) + 63) << 16) | np.asarray(m16, np.int64)
    out = []
    n = 48
    en = rng.integers(-14, 15, n)                                               # normal halves: the half keeps 10 of the 16 mantissa bits
    m10 = rng.integers(0, 1 << 10, n)
    out += [pat(en, m10 << 6), pat(en, (m10 << 6) | rng.integers(1, 32, n)), pat(en, (m10 << 6) | rng.integers(33, 64, n)),
            pat(en, ((m10 & ~1) << 6) | 32), pat(en, ((m10 | 1) << 6) | 32), pat(en, (0x3FF << 6) | rng.integers(32, 64, n)), pat(en, np.full(n, (0x3FF << 6) | 32))]
    out += [pat(np.full(n, 15), rng.integers(0, 0xFFC0, n)), pat(np.full(64, 15), 0xFFC0 | (np.arange(64) % 32)), pat(np.full(64, 15), 0xFFE0 | (np.arange(64) % 32)),
            pat(rng.integers(16, 65, n), rng.integers(0, 1 << 16, n))]
    for e in range(-24, -14):                                                   # subnormal halves: d = 6 + (-14 - e) of the 17 significand bits go
        d = -8 - e
        kept = rng.integers(0, 1 << (16 - d), 24) if d < 16 else np.zeros(24, np.int64)         # (below the leading one)
        low = rng.integers(0, 1 << (d - 1), 24)
        out += [pat(np.full(24, e), ((kept << d) | low) & 0xFFFF), pat(np.full(24, e), ((kept << d) | (1 << (d - 1)) | np.maximum(low, 1)) & 0xFFFF),
                pat(np.full(24, e), ((kept << d) | (1 << (d - 1))) & 0xFFFF)]
        if d < 16:
            out += [pat(np.full(24, e), (((kept & ~1) << d) | (1 << (d - 1))) & 0xFFFF), pat(np.full(24, e), (((kept | 1) << d) | (1 << (d - 1))) & 0xFFFF)]
    out += [pat(np.full(n, -25), np.zeros(n, np.int64)), pat(np.full(n, -25), rng.integers(1, 1 << 16, n)), pat(rng.integers(-62, -25, n), rng.integers(0, 1 << 16, n)),
            np.zeros(n, np.int64)]
    out += [pat(rng.integers(-8, 1, 4 * n), rng.integers(0, 1 << 16, 4 * n))]    # plain values around [0, 1] for the integer outputs
    p = np.concatenate(out)
    return np.concatenate([p, p | (1 << 23)])


def int_tie_values(mul, rng, count=64):
    """non-negative float32 v with f32(v) x f32(mul) exactly k + 0.5, `count` of them for even and for odd k (a search over the neighbours of (k + 0.5) / mul)"""
    ks = np.arange(0, mul, dtype=np.int64)
    guess = ((ks + 0.5) / mul).astype(np.float32).view(np.uint32).astype(np.int64)
    found = {0: [], 1: []}
    for off in (0, -1, 1, -2, 2, -3, 3):
        v = (guess + off).astype(np.uint32).view(np.float32)
        hit = (v * np.float32(mul) == (ks + 0.5).astype(np.float32)) & (v <= 1)
        for par in (0, 1):
            found[par].append(v[hit & (ks % 2 == par)])
    res = []
    for par in (0, 1):
        u = np.unique(np.concatenate(found[par]))
        assert len(u) >= MIN_SAMPLES, (mul, par, len(u))
        res.append(rng.choice(u, min(count, len(u)), replace=False))
    return np.concatenate(res)


def float32_patterns():
    """non-negative binary32 patterns up to 1.125 (beyond that the synthesiser's residuals leave 32 bits): rounding ties of x 255 / x 65535 / x 1023, values above 1,
    half ties and half subnormals, the underflow edge, plain values"""
    rng = np.random.default_rng(32)
    n = 48
    parts = [int_tie_values(m, rng) for m in (255, 65535, 1023)]
    parts.append((1 + rng.random(n) * 0.125).astype(np.float32))
    e = rng.integers(-14, 0, n) + 127
    m = rng.integers(0, 1 << 10, n)
    parts.append(((e << 23) | (m << 13) | 0x1000).astype(np.uint32).view(np.float32))                      # half ties, both parities
    parts.append(((e << 23) | (m << 13) | rng.integers(1, 0x2000, n)).astype(np.uint32).view(np.float32))
    es = rng.integers(-24, -14, n) + 127
    parts.append(((es << 23) | rng.integers(0, 1 << 23, n)).astype(np.uint32).view(np.float32))            # half subnormals
    parts.append(np.array([0x33000000] * n + [0x33000001] * n + [0x32FFFFFF] * n, np.uint32).view(np.float32))
    parts.append(rng.random(4 * n, dtype=np.float32))
    return np.concatenate(parts).view(np.uint32).astype(np.int64)


def nonfinite_patterns():
    """binary32 patterns of the top binade and beyond it, all within 2^24 of each other (which keeps the residuals small): the largest finite floats, +inf, quiet and
    signalling NaNs"""
    rng = np.random.default_rng(33)
    n = 64
    return np.concatenate([np.full(n, 0x7F800000), np.array([0x7FC00000, 0x7F800001, 0x7FFFFFFF, 0x7FA00000] * (n // 4)), rng.integers(0x7F000000, 0x7F800000, n),
                           np.full(n, 0x7F7FFFFF)]).astype(np.int64)


def float_plane(patterns, w, h, seed):
    """(h, w, 3) int32 plane that holds every pattern at least once (the list repeated and shuffled)"""
    n = h * w * 3
    assert n >= len(patterns)
    p = np.resize(patterns, n)
    np.random.default_rng(seed).shuffle(p)
    return p.reshape(h, w, 3).astype(np.int32)


def float_streams(ints, bits, exp_bits):
    """the plane as a plain image (-> ModularOutputKernel / StoreSample) and as two frames, the second a crop of the same samples blended with mode replace
    (-> WriteKernel; the composite is the plane again)"""
    h, w = ints.shape[:2]
    y0, x0, ch, cw = 5, 7, h // 2, w // 2
    S.set_float(exp_bits)
    try:
        plain = S.encode_modular(ints, bits, False, 0)
        layered = S.encode_modular_frame(ints, S.frame(is_last=0, save_as_reference=1), bits) + \
            S.encode_modular_frame(ints[y0:y0 + ch, x0:x0 + cw], S.frame(emit=1, have_crop=1, crop_x0=x0, crop_y0=y0, canvas_w=w, canvas_h=h, blend_mode=0, blend_source=1), bits)
    finally:
        S.set_float(0)
    return {"plain": plain, "layered": layered}


def float24_plane():
    return float_plane(float24_patterns(), 72, 40, 1)


def float32_plane():
    return float_plane(float32_patterns(), 56, 40, 2)


def nonfinite_plane():
    return float_plane(nonfinite_patterns(), 24, 16, 4)


def float16_plane():
    """every binary16 pattern with an exponent field below 31, both signs: 63488 patterns"""
    p = np.arange(1 << 16, dtype=np.int64)
    return float_plane(p[((p >> 10) & 31) != 31], 160, 136, 3)


def float24_coverage(colour):
    """the coverage conditions of the 24-bit plane on its f32 decode (h, w, 3): every half class with both signs, and the integer classes"""
    neg = np.signbit(colour)
    masks = {}
    for name, m in half_classes(colour).items():
        masks["+" + name], masks["-" + name] = m & ~neg, m & neg
    with np.errstate(invalid="ignore"):
        masks.update({"int_below_zero": colour < 0, "int_above_one": colour > 1, "int_minus_zero": colour.view(np.uint32) == 0x80000000,
                      "int_inside": (colour > 0) & (colour < 1)})
    return masks


def float32_coverage(colour):
    masks = {}
    for mul in (255, 65535, 1023):
        masks.update(int_tie_classes(colour, mul))
    hc = half_classes(colour)
    masks.update({"above_one": colour > 1, "half_tie_kept": hc["normal_tie_to_even_kept"], "half_tie_bumped": hc["normal_tie_to_even_bumped"],
                  "half_subnormal": hc["subnormal_round_down"] | hc["subnormal_round_up"],
                  "exactly_2^-25": hc["exactly_2^-25_to_zero"], "just_above_2^-25": hc["just_above_2^-25_to_2^-24"], "below_2^-25": hc["below_2^-25_to_zero"]})
    return masks


def nonfinite_coverage(colour):
    return {"plus_infinity": np.isposinf(colour), "nan": np.isnan(colour), "beyond_half_range": half_classes(colour)["beyond_half_range"]}


def check_all_formats_of_plane(jx, data, base, what, depths=()):
    for dtype in DTYPES:
        for nch, big in ((3, False), (4, True), (1, True), (2, False)):
            check_format(jx, data, base, dtype=dtype, nch=nch, big_endian=big, what=what)
    for dtype, bits in depths:
        check_format(jx, data, base, dtype=dtype, nch=3, int_mul=(1 << bits) - 1, depth_bits=bits, what=what)


@pytest.mark.parametrize("path", ["plain", "layered"])
def test_half_converter_on_every_class_of_input(jx, path):
    """A 24-bit float plane (1 + 7 + 16 bits) through ModularOutputKernel (plain) and WriteKernel (layered): f16 output equals astype(float16) bit for bit for normal halves
    rounding down, up and on a tie (kept / bumped), mantissa carry into the exponent and into infinity, [65504, 65520) staying finite, the subnormal range with ties,
    2^-25 exactly -> 0, just above -> 2^-24, below -> 0, zero — each with both signs —; u8 / u16 of negative, above-one and -0 samples clamp."""
    ints = float24_plane()
    data = float_streams(ints, 24, 7)[path]
    base = stored_rgba_f32(jx, data)
    # the decode is the float the 24-bit pattern names: sign, exponent - 63 + 127, mantissa << 7 (no crafted pattern is a subnormal of the 24-bit format)
    mag = ints.astype(np.int64) & 0x7FFFFF
    assert ((mag == 0) | ((mag >> 16) != 0)).all()
    want_f32 = np.where(mag == 0, 0, (((mag >> 16) - 63 + 127) << 23) | ((mag & 0xFFFF) << 7)) | ((ints.astype(np.int64) >> 23) << 31)
    assert np.array_equal(base[..., :3].view(np.uint32), want_f32.astype(np.uint32))
    assert_coverage(float24_coverage(base[..., :3]), "float24 " + path)
    check_all_formats_of_plane(jx, data, base, "float24 " + path, depths=(("uint16", 10), ("uint8", 5)))


@pytest.mark.parametrize("path", ["plain", "layered"])
def test_integer_rounding_ties_and_non_finite_samples(jx, path):
    """A binary32 plane through both write kernels: exact ties v x 255 / 65535 / 1023 == k + 0.5 (even and odd k) round to even in u8 / u16 / 10-bit output,
    values above 1 clamp; half ties, half subnormals and the underflow edge once more from binary32 input."""
    ints = float32_plane()
    data = float_streams(ints, 32, 8)[path]
    base = stored_rgba_f32(jx, data)
    assert np.array_equal(base[..., :3].view(np.uint32), ints.astype(np.uint32))          # f32 output is the file's floats, bit for bit (NaN payloads included)
    assert_coverage(float32_coverage(base[..., :3]), "float32 " + path)
    check_all_formats_of_plane(jx, data, base, "float32 " + path, depths=(("uint16", 10),))


@pytest.mark.parametrize("path", ["plain", "layered"])
def test_infinity_and_nan_samples(jx, path):
    """+inf, NaN (quiet and signalling patterns) and the largest finite floats as binary32 samples: f32 output keeps the bits, f16 gives +inf / NaN / +inf, u8 / u16
    clamp +inf to the maximum; integer outputs of NaN are not asserted.
    These streams also pin the Modular entropy stage on samples near 2^31: W + N - NW leaves 32 bits there, and the wave-wide decoder's clamped gradient once
    took the wrapped sum for the median of (N, W, W + N - NW) — the device then refused them as corrupt (ANS final state)."""
    ints = nonfinite_plane()
    data = float_streams(ints, 32, 8)[path]
    base = stored_rgba_f32(jx, data)
    assert np.array_equal(base[..., :3].view(np.uint32), ints.astype(np.uint32))
    assert_coverage(nonfinite_coverage(base[..., :3]), "non-finite " + path)
    check_all_formats_of_plane(jx, data, base, "non-finite " + path, depths=(("uint16", 10),))


@pytest.mark.parametrize("path", ["plain", "layered", "float_alpha"])
def test_half_to_float_to_half_is_the_identity(jx, path):
    """A binary16 plane with every pattern whose exponent field is below 31: f16 output is the file's halves, bit for bit (subnormals, -0), through ModularOutputKernel,
    WriteKernel and — as an RGBA image whose alpha is a half too — the float-alpha route into WriteKernel."""
    ints = float16_plane()
    if path == "float_alpha":
        ints = np.dstack([ints, np.roll(ints[..., 0], 17, axis=1)])
        S.set_float(5)
        try:
            data = S.encode_modular(ints, 16, False, 0)
        finally:
            S.set_float(0)
    else:
        data = float_streams(ints, 16, 5)[path]
    base = stored_rgba_f32(jx, data)
    nc = ints.shape[2]
    assert len(np.unique(base[..., :3].view(np.uint32))) == 63488                  # coverage: every pattern arrived as a distinct float
    want = ints.astype(np.uint16).view(np.float16).astype(np.float32)
    assert np.array_equal(base[..., :nc].view(np.uint32), want.view(np.uint32))
    w, h, buf = raw_decode(jx, data, "float16", nc)
    assert np.array_equal(buf.view("<u2").reshape(h, w, nc), ints.astype(np.uint16))
    check_all_formats_of_plane(jx, data, base, "float16 " + path)


# ---- 4. full-range ramps through ModularOutputKernel -----------------------------------------------------------------------------------------------
def test_full_range_ramps(jx):
    """A 256 x 256 16-bit image that holds every value once: u16 output is the identity.  An 8-bit image with all 256 values: u8 the identity, u16 v x 257.
    Exact by arithmetic (v / 255 x 65535 = v x 257)."""
    rng = np.random.default_rng(5)
    ramp16 = rng.permutation(1 << 16).reshape(256, 256, 1).astype(np.int32)
    img16 = np.dstack([ramp16, ramp16[::-1], ramp16[:, ::-1]])
    data = S.encode_modular(img16, 16, False, 0)
    for big in (False, True):
        w, h, buf = raw_decode(jx, data, "uint16", 3, big)
        assert np.array_equal(buf.view(">u2" if big else "<u2").reshape(256, 256, 3), img16)
    ramp8 = (rng.permutation(1 << 12) % 256).reshape(64, 64, 1).astype(np.int32)
    img8 = np.dstack([ramp8, ramp8[::-1], 255 - ramp8])
    assert len(np.unique(ramp8)) == 256
    data = S.encode_modular(img8, 8, False, 0)
    _, _, buf = raw_decode(jx, data, "uint8", 3)
    assert np.array_equal(buf.reshape(64, 64, 3), img8)
    for big in (False, True):
        _, _, buf = raw_decode(jx, data, "uint16", 3, big)
        assert np.array_equal(buf.view(">u2" if big else "<u2").reshape(64, 64, 3), img8 * 257)


# ---- 5. the fast path and the frame tail are the same function of the same samples ------------------------------------------------------------------
PATH_ENCODINGS = dict(COLOUR_ENCODINGS, default_srgb={}, linear=dict(white_point=1, primaries=1, tf=8))


@pytest.mark.parametrize("name", sorted(PATH_ENCODINGS))
def test_fast_path_and_frame_tail_write_the_same_samples(jx, name):
    """One 200 x 136 XYB frame as a single-frame image (the fast path: the last filter kernel or OutputKernel hands it to ColorAndStore -> StorePixel; the default
    sRGB frame with gaborish and one EPF pass takes FusedGabEpf1OutKernel) and as the first of two frames, the second a 64 x 48 crop that replaces its rectangle
    (the frame tail: ColorKernel, BlendColorKernel, WriteKernel).  Colour transform, transfer function and sample conversion of the two paths are one definition
    (pixel_ops.h), so outside the crop the f32 output is equal bit for bit, and so are u8 and u16 — for every transfer function, with and without the filters."""
    img = S.synthetic_image(31, 200, 136)
    x0, y0, cw, ch = 40, 30, 64, 48
    S.set_color(**PATH_ENCODINGS[name])
    try:
        pairs = []
        for filt in (dict(gab=1, epf_iters=1), dict(gab=0, epf_iters=0)):
            single = S.encode_vardct(img, seed=5, strategy_mix=2, **filt)
            layered = S.encode_vardct_frame(img, S.frame(is_last=0, save_as_reference=1), seed=5, strategy_mix=2, **filt) + \
                S.encode_vardct_frame(S.synthetic_image(9, cw, ch), S.frame(emit=1, have_crop=1, crop_x0=x0, crop_y0=y0, canvas_w=200, canvas_h=136, blend_mode=0, blend_source=1), seed=4)
            pairs.append((filt, single, layered))
    finally:
        S.set_color()
    compared = np.ones((136, 200), bool)
    compared[y0:y0 + ch, x0:x0 + cw] = False
    assert int(compared.sum()) == 200 * 136 - cw * ch                             # the whole image but the crop: nothing else is masked
    for filt, single, layered in pairs:
        for dtype, view in (("float32", "<u4"), ("uint8", "u1"), ("uint16", "<u2")):
            outs = []
            for data in (single, layered):
                w, h, buf = raw_decode(jx, data, dtype, 3)
                assert (w, h) == (200, 136)
                outs.append(buf.view(view).reshape(136, 200, 3))
            fast, tail = outs
            differing = int((fast[compared] != tail[compared]).sum())
            print(name, filt, dtype, "differing samples outside the crop:", differing)
            assert differing == 0, (name, filt, dtype, differing)
            assert not np.array_equal(fast[~compared], tail[~compared])             # (the second frame did land in its rectangle)
